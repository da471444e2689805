// Host side of the conv / GEMM launchers (gemm_sk.hip, conv_wide.hip, gemm_lds.hip, conv_narrow.hip, conv_lds.hip, conv_gemm.hip,
// conv_pair.hip, conv_pair64.hip): the A/B switches, the one routed launch, the run-time flag -> template argument dispatcher, the operand
// alignment test and the in-kernel stamp buffer.  Nothing here is device code.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"

namespace gsv {

// The steps of launch_conv_gemm (conv_gemm.hip), in the order it tries them; the last one, conv_gemm_kernel, takes everything.
// Each returns 0 = launched, 1 = not eligible (the next step is tried), < 0 = error.
int launch_gemm_sk(int dtype, const ConvArgs& a, hipStream_t s);      // gemm_sk.hip: split-K / 64 x 64 GEMM for under-filled grids
int launch_conv_wide(int dtype, const ConvArgs& a, hipStream_t s);    // conv_wide.hip: persistent 128-channel tile convolution
int launch_gemm_lds(int dtype, const ConvArgs& a, hipStream_t s);     // gemm_lds.hip: 128 x 128 LDS-tiled GEMM (taps == 1)
int launch_conv_narrow(int dtype, const ConvArgs& a, hipStream_t s);  // conv_narrow.hip: persistent 16 / 32 / 64-channel convolution
int launch_conv_lds(int dtype, const ConvArgs& a, hipStream_t s);     // conv_lds.hip: LDS-staged tile convolution (stride 1)

// Every A/B switch of these files: the environment is read once, at the first conv / GEMM launch of the process.  The defaults are
// the measured choices (the measurements stand beside the rules that use them); a switch restores the alternative for comparison
// runs (tools/conv_probe.py, tools/gemm_probe.py, tools/cfm_bench.py).  "set" = defined with any value.
inline const char* env_switch(const char* name) { return getenv(name); }
inline long long env_number(const char* name, long long unset) { const char* v = env_switch(name); return v ? atoll(v) : unset; }
inline char env_first(const char* name) { const char* v = env_switch(name); return v ? v[0] : '\0'; }
struct ConvSwitches {
  bool no_conv_lds = env_switch("GSV_NO_CONV_LDS");            // set: conv_wide, gemm_lds, conv_narrow and conv_lds are skipped
  bool trace_conv_gemm = env_switch("GSV_TRACE_CONV_GEMM");    // set: print every shape that reaches conv_gemm_kernel
  long long gemm_small_tiles = env_number("GSV_CONV_GEMM_SMALL_TILES", 64);   // conv_gemm: 64 x 64 tiles below this many 128 x 128 ones; 0 = never
  bool no_gemm_sk = env_switch("GSV_NO_GEMM_SK");              // set: skinny GEMMs go on to gemm_lds
  int sk_max_tiles = (int)env_number("GSV_SK_MAX_TILES", 160); // gemm_sk only below this many 128 x 128 tiles
  bool gemm_t64 = env_first("GSV_GEMM_T64") != '0';            // 0: K % 512 == 0 takes the streaming split-K kernel, not gemm_t64
  int t64_slab = (int)env_number("GSV_T64_SLAB", 128);         // 256: one resident gemm_t64 workgroup per CU, 256-half stages
  bool no_conv_wide = env_switch("GSV_NO_CONV_WIDE");          // set: 128-channel convs take conv_lds' one tile per workgroup
  int wide_waves = (int)env_number("GSV_WIDE_WAVES", 8);       // 4: the 4-wave geometry of conv_wide
  bool wide_prof = env_switch("GSV_WIDE_PROF");                // set: in-kernel stamps of one conv_wide tile, printed after the third launch
  int gemm_xcd = env_first("GSV_GEMM_XCD") == '0' ? 0 : env_first("GSV_GEMM_XCD") == '1' ? 1 : 2;   // 2: gemm_lds tile order 1 or 2 by shape; 1: order 1 only; 0: launch order
  int gemm_waves = (int)env_number("GSV_GEMM_WAVES", 8);       // 4: gemm_lds never takes its 8-wave form
  long long gemm_w8_max_tiles = env_number("GSV_GEMM_W8_MAX_TILES", 256);     // 8-wave gemm_lds up to this many tiles
  bool no_persist = env_switch("GSV_CONV_NO_PERSIST");         // set: no conv_narrow (16 / 32 / 64 channels go to conv_lds)
  bool no_persist64 = env_switch("GSV_CONV_NO_PERSIST64");     // set: the same for the 64-channel stage only
  int narrow_per_cu = std::max(1, (int)env_number("GSV_NARROW_PER_CU", 3));   // resident conv_narrow workgroups per CU at most
  bool narrow_prof = env_switch("GSV_NARROW_PROF");            // set: in-kernel stamps of one conv_narrow tile, printed after the third launch
  bool no_half_tile = env_switch("GSV_CONV_NO_HALF_TILE");     // set: under-filled conv_lds grids keep 256-step tiles
  bool half_always = env_switch("GSV_CONV_HALF_ALWAYS");       // set: 128-step tiles whatever the grid (experiment)
  int half_waves = (int)env_number("GSV_CONV_HALF_WAVES", 8);  // 4: the 4-wave geometry of the 128-step tiles
  int tile_waves = (int)env_number("GSV_CONV_TILE_WAVES", 8);  // 4: the 4-wave geometry of the 256-step tiles
  bool no_conv_pair = env_switch("GSV_NO_CONV_PAIR");          // set: conv_pair_eligible is false, the engines launch a pair's two convs
  bool no_conv_pair64 = env_switch("GSV_NO_CONV_PAIR64");      // set: the 64-channel stage keeps a pair's two conv_narrow launches
  int pair_per_cu = std::max(1, (int)env_number("GSV_PAIR_PER_CU", 3));       // resident conv_pair workgroups per CU at most
};
inline const ConvSwitches& conv_switches() {
  static const ConvSwitches sw{};
  return sw;
}

// The one launch of these files: raise the kernel's dynamic-LDS limit to LdsCap bytes at the first launch of this instantiation
// (0 = the kernel uses none beyond the default), record the route, launch, check.
template <auto Kern, int LdsCap, typename... Args>
int launch_routed(unsigned long long route, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  if constexpr (LdsCap > 0) {
    static bool cap_set = false;
    if (!cap_set) {
      GSV_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, LdsCap));
      cap_set = true;
    }
  }
  set_conv_route(route);
  GSV_LAUNCH(Kern, grid, block, lds, s, args...);
  return GSV_OK;
}
constexpr int LDS_CAP = 160 * 1024;   // gfx950: 160 KB of LDS per workgroup

// Run-time bools -> template arguments: with_flags(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...),
// so a launcher names its kernel once, as  kernel<..., R.value, A.value>  inside a generic lambda.  Every combination is
// instantiated; a site whose kernel does not exist for all of them dispatches the flags that are free.
template <typename F> int with_flags(F&& f) { return f(); }
template <typename F, typename... Bools> int with_flags(F&& f, bool b, Bools... rest) {
  return with_flags([&](auto... tail) { return b ? f(std::true_type{}, tail...) : f(std::false_type{}, tail...); }, rest...);
}

// both operands are fetched as 16-byte chunks of G elements
template <int G> bool operands_aligned(const ConvArgs& a) {
  return a.ldx % G == 0 && a.ldw % G == 0 && (uintptr_t)a.x % 16 == 0 && (uintptr_t)a.w % 16 == 0;
}

// In-kernel stamps of one tile (ConvArgs::prof; measurement runs, GSV_WIDE_PROF / GSV_NARROW_PROF): the buffer is allocated at the
// first launch with the switch set, and after the third launch the stamps are printed as microseconds since the tile's first.
struct TileStamps {
  unsigned long long* dev = nullptr;
  int calls = 0;
  unsigned long long* buffer(bool on) {
    if (on && !dev) { (void)hipMalloc((void**)&dev, 64 * 8); (void)hipMemset(dev, 0, 64 * 8); }
    return dev;
  }
  void report(hipStream_t s, int max_stamps, const char* fmt, ...) {
    if (!dev || ++calls != 3) return;
    (void)hipStreamSynchronize(s);
    unsigned long long hp[64];
    (void)hipMemcpy(hp, dev, sizeof(hp), hipMemcpyDeviceToHost);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    for (int i = 1; i < max_stamps && hp[i]; ++i) fprintf(stderr, " %.2f", (double)(hp[i] - hp[0]) / 100.0);
    fprintf(stderr, "\n");
  }
};

}  // namespace gsv
