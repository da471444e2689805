// gsv HIP library -- shared helpers (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>

#include "../../include/gsv.h"

namespace gsv {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

void set_error(const char* fmt, ...);

#define GSV_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      gsv::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return GSV_ERR_HIP;                                                               \
    }                                                                                   \
  } while (0)

#define GSV_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      gsv::set_error(__VA_ARGS__);             \
      return GSV_ERR_ARG;                      \
    }                                          \
  } while (0)

#define GSV_RC(e)            \
  do {                       \
    int _rc = (e);           \
    if (_rc) return _rc;     \
  } while (0)

// Host code that launches typed kernels is a template on the element type T; an entry point picks T once, from its handle or
// from a dtype argument:
//   return GSV_WITH_T(h, decode<T>(h, ...));
#define GSV_WITH_DTYPE(dt, call)                                         \
  [&]() -> int {                                                         \
    if ((dt) == GSV_F16) { using T = _Float16; return call; }            \
    using T = float;                                                     \
    return call;                                                         \
  }()
#define GSV_WITH_T(h, call) GSV_WITH_DTYPE((h)->dtype, call)

// every kernel launch of the engine files: the launch and its error check, the argument list written once
#define GSV_LAUNCH(kern, grid, block, shmem, s, ...)                    \
  do {                                                                   \
    hipLaunchKernelGGL(kern, grid, block, shmem, s, __VA_ARGS__);        \
    GSV_HIP(hipGetLastError());                                          \
  } while (0)

template <typename T> struct DT;
template <> struct DT<float> { static constexpr int id = GSV_F32; static constexpr int G = 4; };
template <> struct DT<_Float16> { static constexpr int id = GSV_F16; static constexpr int G = 8; };

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(_Float16 v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v) { return (T)v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// XCD-aware workgroup order: the dispatcher deals linear workgroup ids round-robin to the 8 XCDs (id % 8), each with its
// own 4 MB L2.  This bijection gives XCD x the CONTIGUOUS run of virtual ids [x * n/8, (x+1) * n/8), so a kernel that
// decodes (tile row, tile column) from the virtual id keeps each XCD on its own slice of the weights / heads.
__device__ __forceinline__ int xcd_virtual_id(int orig, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}
static inline size_t dt_size(int dt) { return dt == GSV_F16 ? 2 : 4; }

// ------------------------------------------------------------------------------------
// Workgroup barrier for LDS producer / consumer hand-offs.  __syncthreads() also emits `s_waitcnt vmcnt(0)`: it waits for every
// outstanding GLOBAL load and store of the wave -- in the persistent conv kernels that is the next tile's window prefetch and
// the previous tile's output stores, i.e. exactly the HBM time the persistence was meant to hide (same lesson as t2s_mega.hip).
// Only LDS traffic has to be complete here; results of global loads are waited for where they are used.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// generic channels-last implicit-GEMM conv (conv_gemm.hip)
// ------------------------------------------------------------------------------------
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_LRELU = 3, ACT_MISH = 4, ACT_CLAMP1 = 5, ACT_SILU = 6, ACT_GELU = 7,
       ACT_GELU_TANH = 8, ACT_LRELU01 = 9, ACT_LOGCLAMP = 10 /* log(max(u, 1e-5)): mel_processing.py:8-14 */,
       ACT_RELU20 = 11 /* Hardtanh(0, 20): eres2net/ERes2NetV2.py:19-21 */, ACT_LOG_EPS = 12 /* log(max(u, FLT_EPSILON)): eres2net/kaldi.py:654 */ };

// Transcendental activations live in ONE out-of-line copy per translation unit: the conv epilogues are unrolled
// 16-64x, and inlining tanhf / expf / log1pf / erff into every instance grew the conv kernels by 26 % and made the
// accumulate / residual variants 2-3x slower (instruction-cache misses), measured with rocprofv3 on MI355X.
static __device__ __noinline__ float post_act_slow(int act, float u) {
  switch (act) {
    case ACT_TANH: { const float t = __expf(-2.f * fabsf(u)); return copysignf(__fdividef(1.f - t, 1.f + t), u); }   // = fast_tanh below
    case ACT_MISH: return u * tanhf(u > 20.f ? u : log1pf(expf(u)));   // x * tanh(softplus(x))
    case ACT_SILU: return u / (1.f + expf(-u));
    case ACT_GELU: return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
    case ACT_GELU_TANH: return 0.5f * u * (1.f + tanhf(0.79788456080286536f * (u + 0.044715f * u * u * u)));
    case ACT_LOGCLAMP: return logf(fmaxf(u, 1e-5f));
    case ACT_LOG_EPS: return logf(fmaxf(u, 1.1920928955078125e-07f));
    default: return u;
  }
}

__device__ __forceinline__ float post_act_f(int act, float u) {
  if (act == ACT_NONE) return u;
  if (act == ACT_RELU) return fmaxf(u, 0.f);
  if (act == ACT_CLAMP1) return fminf(fmaxf(u, -1.f), 1.f);
  if (act == ACT_LRELU01) return u > 0.f ? u : 0.01f * u;   // nn.LeakyReLU() default slope
  if (act == ACT_RELU20) return fminf(fmaxf(u, 0.f), 20.f);
  return post_act_slow(act, u);
}

// Epilogue activation with the code fixed at compile time for the two cases that matter for speed (none: every ResBlock
// conv; tanh: conv_post over 4.1 M samples), -1 = decide per value from the run-time code.  The kernels test the run-time
// code ONCE per epilogue pass and call the matching instance (conv_wide.hip has the measurement that led here).
__device__ __forceinline__ float fast_tanh(float u) {
  const float t = __expf(-2.f * fabsf(u));
  return copysignf(__fdividef(1.f - t, 1.f + t), u);
}
template <int ACTC> __device__ __forceinline__ float post_act_c(int act, float u) {
  if (ACTC == ACT_NONE) return u;
  if (ACTC == ACT_TANH) return fast_tanh(u);
  return post_act_f(act, u);
}
#define GSV_ACT_DISPATCH(act, fn)                                         \
  do {                                                                    \
    if ((act) == ACT_NONE) fn(std::integral_constant<int, ACT_NONE>{});   \
    else if ((act) == ACT_TANH) fn(std::integral_constant<int, ACT_TANH>{}); \
    else fn(std::integral_constant<int, -1>{});                           \
  } while (0)

struct ConvArgs {
  const void* x = nullptr;   // [Z][T_in][ldx] activations, channels-last
  const void* w = nullptr;   // [Z][Cout][ldw]  weights, K index = tap*Cin + cin (cin fastest)
  const float* bias = nullptr;  // [Cout_real] fp32 or null
  const float* gate = nullptr;  // [Cout_real] fp32 or null: v = ((acc + bias) * gate + res) * scale
  void* y = nullptr;         // [Z][T_out][ldy]
  const void* res = nullptr; // residual, same dtype/shape convention as y (ldr)
  int T_in = 0, T_out = 0;   // valid input rows / output rows actually stored
  int T_virt = 0;            // number of GEMM columns computed (== T_out unless ups_u > 0)
  int Cin = 0, Cout = 0, taps = 1;
  int stride = 1, dil = 1, pad = 0;  // input row = t*stride + tap*dil - pad
  int ldx = 0, ldw = 0, ldy = 0, ldr = 0;
  int y_col0 = 0;            // column offset into y rows (for writing channel slices)
  int pre_act = ACT_NONE;    // activation applied to x at load (ACT_LRELU uses pre_slope)
  float pre_slope = 0.1f;
  int post_act = ACT_NONE;   // activation applied after bias (+res)
  float scale = 1.0f;        // v = (acc + bias + res) * scale
  int accumulate = 0;        // y += v instead of y = v
  int out_f32 = 0;           // y is fp32 regardless of T
  int res_f32 = 0;           // res is fp32 regardless of T
  int ups_u = 0, ups_pad = 0, ups_cout = 0;  // transposed-conv scatter: row = s*u + n/ups_cout - pad
  int Z = 1;
  long long xz = 0, wz = 0, yz = 0, rz = 0;  // batch strides in elements
  unsigned long long* prof = nullptr;   // conv_wide.hip measurement runs (GSV_WIDE_PROF): s_memrealtime stamps of one tile
  int bz = 0;                                // batch stride of bias / gate (grouped convs)
  int xcd_order = 0;                         // set by the launcher: 1 = decode tile ids through xcd_virtual_id
  int w_nt = 0;                              // weights are loaded non-temporal (streamed once per step: keep them out of the
                                             // Infinity Cache so that OTHER layers' weights stay resident), GEMM paths only
  int z_res = 0;                             // batched launch (Z > 1) whose residual has its own slice stride rz: takes the LDS GEMM
                                             // path (bwe.hip; other batched launches with a residual keep the generic kernel)
  // segmented decode (vits.hip gsv_vits_decode_segments): one int32 per OUTPUT row, the row's segment or -1 for a gap row.
  // A gap row is stored as 0 whatever the conv computes (bias, residual, accumulate included).  launch_conv_gemm applies it
  // in a row pass after the conv kernel (launch_seg_rows), so a masked launch takes the same instantiation and records the
  // same route as an unmasked one, and the conv kernels never read it: their code and registers are the unmasked ones.
  // Null = unmasked.  (One 8-byte field: three of them regrouped the kernel arguments and cost gemm_lds a 64-byte spill.)
  const int* row_seg = nullptr;
  // per-row gates (flow-matching sessions, cfm_session.hip): gate_rows > 0 = output row t is gated by the vector
  // gate + (t / gate_rows) * gate_ld instead of the one vector at gate (gate_rows = frames per utterance: the lookup is per
  // output row, a tile may span several utterances).  Z == 1, no transposed-conv scatter.  Only the *_GROWS instantiations of
  // gemm_sk / gemm_t64 / gemm_lds / conv_gemm read the two fields; 0 = one vector, the kernels and routes of before.
  int gate_rows = 0, gate_ld = 0;
};
// Route record (gsv_debug_last_conv_route): every launch site of launch_conv_gemm / launch_conv_pair stores which kernel
// instantiation it launched, as one 64-bit code of byte fields (include/gsv.h has the layout).  A plain store on the host:
// no formatting, allocation or synchronisation on the launch path.
enum { ROUTE_GEMM_SK = 1, ROUTE_GEMM_T64 = 2, ROUTE_CONV_WIDE = 3, ROUTE_GEMM_LDS = 4, ROUTE_CONV_LDS = 5, ROUTE_CONV_NARROW = 6,
       ROUTE_CONV_GEMM = 7, ROUTE_CONV_PAIR = 8, ROUTE_GEMM_PANEL = 9 };
enum { ROUTE_RES = 1, ROUTE_ACCU = 2, ROUTE_ALLW = 4, ROUTE_WNT = 8, ROUTE_SEG = 16, ROUTE_GROWS = 32 };
constexpr unsigned long long route_code(int family, int dtype, int p0 = 0, int p1 = 0, int p2 = 0, int p3 = 0, int p4 = 0, int flags = 0) {
  return (unsigned long long)(family & 255) | (unsigned long long)(dtype & 255) << 8 | (unsigned long long)(p0 & 255) << 16 |
         (unsigned long long)(p1 & 255) << 24 | (unsigned long long)(p2 & 255) << 32 | (unsigned long long)(p3 & 255) << 40 |
         (unsigned long long)(p4 & 255) << 48 | (unsigned long long)(flags & 255) << 56;
}
constexpr int route_flags(bool res, bool accu, bool allw = false, bool wnt = false) {
  return (res ? ROUTE_RES : 0) | (accu ? ROUTE_ACCU : 0) | (allw ? ROUTE_ALLW : 0) | (wnt ? ROUTE_WNT : 0);
}
void set_conv_route(unsigned long long code);
// the row pass of a segmented launch (ConvArgs::row_seg): gap rows of y [rows][ldy] (columns col0 .. col0 + C) to 0, and with a
// per-segment bias table tab [n][ldb], segment rows + tab[row_seg[t]] (the per-segment voice biases of gsv_vits_decode_segments)
int launch_seg_rows(int dtype, int out_f32, void* y, int ldy, int col0, int C, int rows, const int* row_seg, const float* tab, int ldb,
                    hipStream_t s);

// picks the kernel for the shape (conv_gemm.hip; the kernels it chooses from are declared in conv_launch.h)
int launch_conv_gemm(int dtype, const ConvArgs& a, hipStream_t s);
// the prefill's panel GEMM (gemm_panel.hip), called IN FRONT of the dispatcher by the prefill itself: 0 = launched, 1 = not
// eligible (go on to launch_conv_gemm), < 0 = error.  tile: 0 = the launcher's choice by shape, 1..3 = one member of the family,
// 4 = tile 3 with the two-accumulator sum of gemm_t64
bool gemm_panel_eligible(int dtype, const ConvArgs& a);
int gemm_panel_auto_tile(const ConvArgs& a, int* wgs_out);   // the launcher's tile (1..3) for the shape and its workgroup count
int launch_gemm_panel(int dtype, const ConvArgs& a, int tile, hipStream_t s);
// the same, in the form (tile and summation) that computes the bits launch_conv_gemm would compute for the descriptor; 1 = none
int launch_gemm_panel_as_dispatcher(int dtype, const ConvArgs& a, hipStream_t s);

// fused ResBlock pair of the generator's narrow stages (conv_pair.hip): y = (convs2(lrelu(convs1(lrelu(x)))) + x) * scale [+ y]
struct ConvPairArgs {
  const _Float16* x = nullptr;     // [T][ldx] fp16, channels-last
  const _Float16* w1 = nullptr;    // [C][taps * C] tap-major, dilation `dil`
  const float* b1 = nullptr;
  const _Float16* w2 = nullptr;    // [C][taps * C], dilation 1
  const float* b2 = nullptr;
  _Float16* y = nullptr;           // [T][ldy]
  int T = 0, C = 0, taps = 0, dil = 1, ldx = 0, ldy = 0;
  float scale = 1.f;
  int accumulate = 0;
};
// supported: a kernel exists for the shape (what gsv_op_conv_pair / gsv_op_conv_pair_seg accept; C = 16 / 32, and 64 unmasked).
// eligible: the generator runs the pair as that kernel (supported, and at C = 64 T >= 16 384 unless GSV_NO_CONV_PAIR64 is set).
bool conv_pair_supported(int dtype, int C, int taps, int dil, int T, bool seg);
bool conv_pair_eligible(int dtype, int C, int taps, int dil, int T, bool seg);
int launch_conv_pair(const ConvPairArgs& a, hipStream_t s);
int launch_conv_pair64(const ConvPairArgs& a, hipStream_t s);   // conv_pair64.hip: C = 64, reached through launch_conv_pair
// the pair of a segmented decode: row_seg [T] int32, -1 = gap row (ConvArgs::row_seg).  Gap rows of the intermediate and of y are
// 0, as after convs1 -> row pass -> convs2 -> row pass.  row_seg travels beside ConvPairArgs, whose layout the unmasked kernels keep.
int launch_conv_pair_seg(const ConvPairArgs& a, const int* row_seg, hipStream_t s);

// Attention route record (gsv_debug_last_attn_route): every attention launcher stores which family it launched and with how
// many 16-query tiles per workgroup (0 for the materialised path).  A plain store on the host, as set_conv_route.
enum { ATTN_ROWS = 1, ATTN_SEG = 2, ATTN_REL96 = 3, ATTN_MAT = 4 };
void set_attn_route(int family, int qt);

// fused attention, fp16, head dim 64 (attn.hip); vt_buf: heads * 64 * ceil32(T) halfs of scratch
// rope_cs != null: rotate the first 2*rope_half channels of q and k in place first (cos|sin table [T][rope_half][2])
int launch_flash_attn64_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* vt_buf, int T, int heads,
                            float scale, void* out, int ldo, hipStream_t s, const float* rope_cs = nullptr, int rope_half = 0);
// the same over `rows` utterances of T frames in the same two launches: row b's q / k / v start xz elements after row b-1's,
// its output oz elements after, its V^T scratch vtz halfs after (vtz >= heads * 64 * ceil32(T))
int launch_flash_attn64_f16_rows(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* vt_buf, int T, int heads,
                                 float scale, void* out, int ldo, hipStream_t s, const float* rope_cs, int rope_half, int rows,
                                 long long xz, long long vtz, long long oz, int qt = 0);
// qt (both launchers): 0 = query tiles per workgroup by the launcher's rule (and the GSV_FLASH_QT switch), 1 / 2 / 4 = that
// instantiation (test hooks)

// the segmented form: n_seg sequences of seg_lens[s] ([host]) rows back to back, each attending to its own keys only, in the same
// two launches; vt_buf: heads * 64 * 32 * sum ceil(seg_lens[s] / 32) halfs of scratch (may arrive uninitialised)
int launch_flash_attn64_f16_seg(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* vt_buf, int n_seg,
                                const int* seg_lens, int heads, float scale, void* out, int ldo, hipStream_t s, int qt = 0);

// enc_p self-attention with window-4 relative positions, fp16, head dim 96 (attn.hip)
int launch_flash_rel96_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* vt_buf, int T, int heads,
                           float scale, const float* rel_k, const float* rel_v, void* out, int ldo, hipStream_t s,
                           const int* kr = nullptr);   // kr: per-query key range [kr[2i], kr[2i+1]), non-decreasing (block-diagonal)

// per-row low-rank delta of the adapted DiT passes (lora.hip).  tab[s] = slot s's block of weights (engine dtype) and its
// padded rank rp; the site's A [n_proj * rp][K] starts coef_a * rp elements into the block and its B [N][rp] coef_b * rp.
// Row b (Tn frames of x [.][K] and y [.][N]) with s = slot[b * slot_stride] >= 0 gets y += gate (.) ((x A^T) B^T); max_rp =
// the largest rp among the slots of this launch (it sizes the LDS tile).
struct LoraSlot { const void* base; int rp, pad_; };
int launch_lora_delta(int dtype, const void* x, void* y, int Tn, int DB, int K, int N, int n_proj, const int* slot, int slot_stride,
                      const LoraSlot* tab, int max_rp, long long coef_a, long long coef_b, const float* gate, hipStream_t s,
                      int gate_ld = 0);   // gate_ld > 0: row b's gate vector is gate + b * gate_ld (the per-row kernels)

// elementwise / small ops (ops.hip)
int launch_layernorm(int dtype, const void* x, int x_f32, const void* res, int res_f32, const float* gamma,
                     const float* beta, void* y, int y_f32, int rows, int C, float eps, hipStream_t s,
                     const int* row_seg = nullptr);   // row_seg: gap rows (-1) are stored as 0 (ConvArgs::row_seg)
int launch_convert(const float* src, void* dst, int dtype, long long n, hipStream_t s);

}  // namespace gsv
