// Persistent narrow convolution (fp16, stride 1, C_in = 16 / 32 / 64 and C_out <= C_in: the last generator stages, 4.1 M and 2 M
// time steps of 16 / 32 channels, and the 64-channel stage before them).
// They are pure HBM streaming (131 MB per tensor, ~nothing to multiply), and one 256-step tile per workgroup made
// every tile a serial chain  load window -> LDS -> MFMA -> LDS transpose -> store  plus a reload of all 11 tap slabs:
// 184-244 us per conv against 52-79 us of HBM time.  Here a workgroup is PERSISTENT over tiles: the weights of all
// taps are staged once, and the NEXT tile's input window and epilogue operands are requested (unconditional, clamped
// addresses; zeros selected afterwards) before the current tile's MFMAs and epilogue, then written to LDS when the
// current tile is done -- the load round trip hides behind the previous tile's work.
#include "conv_launch.h"
#include "mfma_frag.h"

namespace gsv {

template <int CC, int TM, int TN, int WN, bool RES, bool ACCU>
__global__ __launch_bounds__(64 * WN) void conv_narrow_f16_kernel(ConvArgs a, int rows_win, int ntiles) {
  typedef _Float16 T;
  typedef h8 F;
  typedef h4 T4;
  constexpr int G = 8, KC = 16, CT = 32 * TM, TT = 32 * TN * WN, NT = 64 * WN;
  static_assert(TT == 256, "tiles are 256 time steps");
  constexpr int LDX = CC + G, VPR = CC / G;
  constexpr int XB = (306 * VPR + NT - 1) / NT;
  // epilogue passes: as many wave columns per pass as the fp32 tile may take of the window's LDS (the smallest window is 258
  // rows).  One column per pass meant 2 barriers per column -- 16 per tile at 8 waves; with 128-row passes it is 4.
  constexpr int WPP = CC == 16 ? 1 : 128 / (TN * 32), NP = WN / WPP;
  constexpr int LDO = CT + 4, PR = TN * 32 * WPP, IPR = CT / 4, NI = PR * IPR / NT;
  static_assert(WN % WPP == 0 && (size_t)PR * LDO * 4 <= (size_t)258 * (CC + 8) * 2, "epilogue tile must fit in the smallest window");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = (T*)smem;                                   // [rows_win][LDX]; the epilogue's fp32 [PR][LDO] tile aliases it
  T* ws = xs + (size_t)rows_win * LDX;                // [taps][CT][LDX], staged once
  float* os = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const T* __restrict__ x = (const T*)a.x;
  const T* __restrict__ w = (const T*)a.w;
  const int total = rows_win * VPR;
  const bool vec_ok = ((a.ldy & 3) == 0) && ((a.y_col0 & 3) == 0) && ((a.ldr & 3) == 0);
  const int ecg = tid % IPR, ec = 4 * ecg;
  const int env = max(0, min(4, a.Cout - ec));
  f4 ebias = (f4){0.f, 0.f, 0.f, 0.f};
  if (a.bias) for (int j = 0; j < env; ++j) ebias[j] = a.bias[ec + j];
  // ---- all taps' weights, once per workgroup
  {
    const int totw = a.taps * CT * VPR;
    for (int v = tid; v < totw; v += NT) {
      const int tap = v / (CT * VPR), rem = v - tap * (CT * VPR);
      const int row = rem / VPR, col = rem - row * VPR;
      F val = zfrag<F>();
      if (row < a.Cout) val = *(const F*)(w + (long long)row * a.ldw + (long long)tap * a.Cin + col * G);
      *(F*)(ws + ((size_t)tap * CT + row) * LDX + col * G) = val;
    }
  }
  // window of tile `tile` -> registers: clamped (always valid) addresses, zero rows outside the sequence selected after
  auto load_window = [&](int tile, F* regs) {
    const int win_start = tile * TT - a.pad;
#pragma unroll
    for (int i = 0; i < XB; ++i) {
      const int v = min(tid + i * NT, total - 1);
      const int row = v / VPR, col = v - row * VPR;
      const int ti = win_start + row;
      const F val = *(const F*)(x + (long long)min(max(ti, 0), a.T_in - 1) * a.ldx + col * G);
      regs[i] = (ti >= 0 && ti < a.T_in) ? val : zfrag<F>();
    }
  };
  auto store_window = [&](const F* regs) {
#pragma unroll
    for (int i = 0; i < XB; ++i) {
      const int v = tid + i * NT;
      if (v < total) {
        const int row = v / VPR, col = v - row * VPR;
        F val = regs[i];
        if (a.pre_act == ACT_LRELU) val = lrelu_l(val, a.pre_slope);
        else if (a.pre_act == ACT_RELU) val = relu_l(val);
        *(F*)(xs + (size_t)row * LDX + col * G) = val;
      }
    }
  };
  int tile = blockIdx.x;
  {
    F first[XB];
    load_window(min(tile, ntiles - 1), first);
    store_window(first);
  }
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int t0 = tile * TT;
    const bool pf = a.prof && blockIdx.x == 100 && tile == 100 + 3 * (int)gridDim.x && tid == 0;
    int pi = 0;
#define NSTAMP() do { if (pf) a.prof[pi++] = __builtin_amdgcn_s_memrealtime(); } while (0)
    NSTAMP();
    // ---- requests for the NEXT tile's window and THIS tile's epilogue operands go out first
    F nxt[XB];
    load_window(min(tile + (int)gridDim.x, ntiles - 1), nxt);
    T4 rv[RES ? NP * NI : 1], yv[ACCU ? NP * NI : 1];
#pragma unroll
    for (int q = 0; q < ((RES || ACCU) ? NP * NI : 0); ++q) {
      const int pass = q / NI, e = q - pass * NI;
      const int t = min(t0 + pass * PR + (tid + e * NT) / IPR, a.T_out - 1);
      const int cc = min(ec, max(a.Cout - 4, 0));          // clamped channel group: loads stay in bounds; masked by env at use
      if (RES) rv[q] = *(const T4*)((const T*)a.res + (long long)t * a.ldr + cc);
      if (ACCU) yv[q] = *(const T4*)((const T*)a.y + (long long)t * a.ldy + a.y_col0 + cc);
    }
    NSTAMP();
    f16v acc[TM][TN];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;
    for (int tap = 0; tap < a.taps; ++tap) {
      const int shift = tap * a.dil;
      const T* wb = ws + (size_t)tap * CT * LDX;
#pragma unroll
      for (int ks = 0; ks < CC / KC; ++ks) {
        const int kk = ks * KC + G * h;
        F af[TM], bf[TN];
#pragma unroll
        for (int m = 0; m < TM; ++m) af[m] = *(const F*)(wb + (size_t)(m * 32 + r) * LDX + kk);
#pragma unroll
        for (int n = 0; n < TN; ++n) bf[n] = *(const F*)(xs + (size_t)((wn * TN + n) * 32 + r + shift) * LDX + kk);
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int n = 0; n < TN; ++n) mma32l(acc[m][n], af[m], bf[n]);
      }
    }
    NSTAMP();
    // ---- epilogue through LDS (whole channels-last rows per store), one wave column per pass
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
      __syncthreads();
      NSTAMP();
      if (wn / WPP == pass) {
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int g = 0; g < 4; ++g)
              *(f4*)(os + (size_t)(((wn % WPP) * TN + n) * 32 + r) * LDO + m * 32 + 8 * g + 4 * h) =
                  (f4){acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
      }
      NSTAMP();
      __syncthreads();
      NSTAMP();
      auto items = [&](auto act_tag) {      // activation code tested once per pass, not per element
  #pragma unroll
        for (int e = 0; e < NI; ++e) {
          const int q = pass * NI + e;
          const int tl = (tid + e * NT) / IPR;
          const int t = t0 + pass * PR + tl;
          if (!(t < a.T_virt && t < a.T_out && env > 0)) continue;
          const f4 av = *(const f4*)(os + (size_t)tl * LDO + 4 * ecg);
          float v[4];
  #pragma unroll
          for (int j = 0; j < 4; ++j) {
            float u = av[j] + ebias[j];
            if (RES) u += (float)rv[q][j];
            u *= a.scale;
            u = post_act_c<decltype(act_tag)::value>(a.post_act, u);
            if (ACCU) u += (float)yv[q][j];
            v[j] = u;
          }
          if (a.out_f32) {                 // conv_post: one fp32 output channel
            float* yp = (float*)a.y + (long long)t * a.ldy + a.y_col0 + ec;
            for (int j = 0; j < env; ++j) yp[j] = v[j];
          } else {
            T* yp = (T*)a.y + (long long)t * a.ldy + a.y_col0 + ec;
            if (vec_ok && env == 4) *(T4*)yp = (T4){(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
            else for (int j = 0; j < env; ++j) yp[j] = (T)v[j];
          }
        }
      };
      GSV_ACT_DISPATCH(a.post_act, items);
    }
    NSTAMP();
    __syncthreads();                 // the fp32 tile (aliasing the window) has been read by every thread
    NSTAMP();
    store_window(nxt);
    __syncthreads();
    NSTAMP();
  }
}

template <int CC, int TM, int TN, int WN>
static int launch_narrow(const ConvArgs& a, int rows_win, hipStream_t s) {
  const int ntiles = cdiv(a.T_virt, 256);
  const size_t lds = ((size_t)rows_win + (size_t)a.taps * 32 * TM) * (CC + 8) * 2;
  // resident workgroups per CU: as many as the LDS footprint allows, capped (GSV_NARROW_PER_CU, default 3).  These stages
  // are HBM-bound and every workgroup keeps one tile's window + operands in flight, so residency = bytes in flight.
  const int per_cu = std::max(1, std::min(conv_switches().narrow_per_cu, (int)((156 * 1024) / lds)));
  const int grid = std::min(ntiles, 256 * per_cu);
  static TileStamps stamps;
  ConvArgs ap = a;
  ap.prof = stamps.buffer(conv_switches().narrow_prof);
  GSV_RC(with_flags([&](auto R, auto A) {
    return launch_routed<conv_narrow_f16_kernel<CC, TM, TN, WN, R.value, A.value>, LDS_CAP>(
        route_code(ROUTE_CONV_NARROW, GSV_F16, CC, TM, TN, WN, 0, route_flags(R.value, A.value)), dim3(grid), dim3(64 * WN), lds, s, ap, rows_win, ntiles);
  }, a.res != nullptr, a.accumulate != 0));
  stamps.report(s, 20, "[narrow prof] C %d taps %d (start | requests issued | taps done | epilogue done | barrier | window stored):", CC, a.taps);
  return GSV_OK;
}

// Which instantiation takes the launch: the kernel's channel count (64 / 32 / 16), or 0 = not eligible; *rows_win = rows of a tile's
// input window.  A plain stride-1 conv that writes T-dtype rows, one input chunk, all taps' weights resident in LDS.
static int narrow_channels(const ConvArgs& a, int* rows_win) {
  const ConvSwitches& sw = conv_switches();
  // what the tile kernel needs (conv_lds.hip launch_conv_lds): a shape it refuses goes to conv_gemm_kernel, not here
  if (a.Z != 1 || a.stride != 1 || a.Cin % 16 != 0 || a.T_virt < 256 || a.gate) return 0;   // gate: 1x1 (gemm) epilogues only
  if ((a.res && a.res_f32) || (a.accumulate && a.out_f32)) return 0;   // preloaded operands are engine-dtype tiles
  if (!operands_aligned<8>(a)) return 0;
  const int span = (a.taps - 1) * (a.dil < 0 ? -a.dil : a.dil);
  if (span > 50) return 0;                      // staging batch is sized for windows of <= 306 rows
  *rows_win = 256 + span;                       // a tile owns 256 time steps
  if (a.Cout > 64 || a.ups_u != 0 || a.dil < 1 || a.T_out < a.T_virt || a.T_in < 1) return 0;
  // residual / accumulate tiles are loaded, and fp16 rows stored, as vectors of 4 channels
  const bool vec4 = !a.out_f32 && !a.res_f32 && a.Cout % 4 == 0 && (!a.res || a.ldr % 4 == 0) && a.ldy % 4 == 0 && a.y_col0 % 4 == 0;
  if (a.Cout > 32) {
    // the 64-channel stage: all 11 tap slabs resident = 145 KB of LDS = ONE workgroup per CU; run with 8 waves (2 per SIMD,
    // 32 columns each) so one wave's MFMAs overlap another's LDS reads
    const size_t lds = ((size_t)*rows_win + (size_t)a.taps * 64) * (64 + 8) * 2;
    const bool ok = !sw.no_persist && !sw.no_persist64 && vec4 && a.T_virt >= 16384 && a.Cin == 64 && lds <= LDS_CAP;
    return ok ? 64 : 0;
  }
  const bool epi_free = !a.res && !a.accumulate;       // no vector operand loads: any Cout / fp32 output (conv_post) is fine
  const size_t lds = ((size_t)*rows_win + (size_t)a.taps * 32) * (a.Cin + 8) * 2;
  const bool ok = !sw.no_persist && (epi_free || vec4) && a.T_virt >= 4096 && (a.Cin == 16 || a.Cin == 32) && lds <= 64 * 1024;
  return ok ? a.Cin : 0;
}

// 0 = launched, 1 = not eligible, < 0 = error
int launch_conv_narrow(int dtype, const ConvArgs& a, hipStream_t s) {
  if (dtype != GSV_F16) return 1;
  int rows = 0;
  switch (narrow_channels(a, &rows)) {
    case 64: return launch_narrow<64, 2, 1, 8>(a, rows, s);
    case 32: return launch_narrow<32, 1, 2, 4>(a, rows, s);
    case 16: return launch_narrow<16, 1, 2, 4>(a, rows, s);
    default: return 1;
  }
}

}  // namespace gsv
