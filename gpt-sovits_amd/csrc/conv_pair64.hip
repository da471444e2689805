// The fused ResBlock pair of conv_pair.hip at C = 64 (the generator's 64-channel stage, 1 M time steps at the bench shape):
//
//     y = ( convs2( lrelu( convs1( lrelu(x) ) ) ) + x ) * scale  [+ y]
//
// conv_pair_f16_kernel's layout does not fit at 64 channels: every wave would hold all of convs1's fragments (352 VGPRs at 11
// taps) and convs2's slabs alone are 101 KB.  Here ONE workgroup of 8 waves owns a CU: wave = (mh, cg), mh = which 32 of the 64
// output channels, cg = which quarter of the time columns.
//   convs1's weights for the wave's 32 output channels in registers (TAPS * 4 A-fragments, 176 VGPRs at 11 taps), loaded once
//   convs2's tap slabs [TAPS][64][72] in LDS, staged once (101 KB at 11 taps), both biases behind them
//   tile = 256 output steps at <= 7 taps, 128 at 9 / 11 (Pair64Shape): window + intermediate + slabs <= 155 KB
//   window  x[t0 - h2 - h1, t0 - h2 + RY + h1) -> LDS (lrelu while staging), prefetched one tile ahead in registers
//   convs1 over RY = 288 / 160 intermediate rows: column tiles cg, cg + 4, (cg + 8) of the wave's half -> + bias -> fp16 -> lrelu
//     -> zero outside [0, T) -> LDS
//   convs2 over the tile's rows from that image -> fp32 tile through LDS (aliasing window + intermediate) -> + bias + x, * scale,
//     (+ y) -> whole channels-last rows
// Every rounding point of the two conv_narrow_f16_kernel<64, 2, 1, 8> launches is kept: same 32x32x16 MFMA, taps outer / k-steps
// inner from a zero accumulator, fp32 bias, fp16 intermediate, fp16 lrelu, the same epilogue expression.  Splitting the output
// channels over waves changes no element's summation order.  y must not overlap x: other workgroups read x rows as halo.
#include "conv_launch.h"
#include "mfma_frag.h"

namespace gsv {

namespace {

typedef _Float16 T;
typedef h8 F;
typedef h4 T4;

template <int TAPS> struct Pair64Shape {
  static constexpr int TS = TAPS <= 7 ? 256 : 128;              // output steps per tile
  static constexpr int RY = (TS + TAPS - 1 + 31) / 32 * 32;     // intermediate rows: 288 / 160
  static constexpr int RX = RY + 50;                            // window rows at most (2 * 25 of dilated halo)
  static constexpr int LDX = 64 + 8;
  static constexpr size_t LDS = (size_t)(RX + RY + TAPS * 64) * LDX * 2 + 128 * 4;
  static_assert(LDS <= LDS_CAP, "window + intermediate + convs2's slabs + biases must fit in LDS");
};

template <int TAPS, bool ACCU>
__global__ __launch_bounds__(512) void conv_pair64_f16_kernel(ConvPairArgs a, int ntiles) {
  typedef Pair64Shape<TAPS> S;
  constexpr int G = 8, KC = 16, CC = 64, KS = CC / KC, NT = 512, LDX = S::LDX, VPR = CC / G;
  constexpr int TS = S::TS, RY = S::RY, RX = S::RX, TN = TS / 128;
  constexpr int XB = (RX * VPR + NT - 1) / NT;
  constexpr int LDO = CC + 4, IPR = CC / 4, NI = TS * IPR / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = (T*)smem;                                   // [RX][LDX]; the epilogue's fp32 [TS][LDO] tile aliases it and ys
  T* ys = xs + (size_t)RX * LDX;                      // [RY][LDX] lrelu(convs1(...)) of this tile
  T* w2s = ys + (size_t)RY * LDX;                     // [TAPS][64][LDX] convs2's weights; convs1's live in registers (below)
  float* bs = (float*)(w2s + (size_t)TAPS * CC * LDX);   // b1[64] | b2[64]
  float* os = (float*)smem;
  static_assert((size_t)TS * LDO * 4 <= (size_t)(RX + RY) * LDX * 2, "epilogue tile must fit in window + intermediate image");
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: scalar loop bounds
  const int mh = wv & 1, cg = wv >> 1;
  const int r = lane & 31, h = lane >> 5;
  const T* __restrict__ x = a.x;
  const int h2 = (TAPS - 1) / 2, h1 = h2 * a.dil;
  const int rows_win = RY + 2 * h1;
  {
    const int totw = TAPS * CC * VPR;
    for (int v = tid; v < totw; v += NT) {
      const int tap = v / (CC * VPR), rem = v - tap * (CC * VPR);
      const int row = rem / VPR, col = rem - row * VPR;
      *(F*)(w2s + ((size_t)tap * CC + row) * LDX + col * G) = *(const F*)(a.w2 + (long long)row * TAPS * CC + (long long)tap * CC + col * G);
    }
    if (tid < 128) bs[tid] = tid < 64 ? a.b1[tid] : a.b2[tid - 64];
  }
  F w1r[TAPS * KS];
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      w1r[tap * KS + ks] = *(const F*)(a.w1 + (long long)(mh * 32 + r) * TAPS * CC + (long long)tap * CC + ks * KC + G * h);
  // window chunk i of this thread: row wr + 64 i, 16-byte column wc (512 threads = 64 rows of 8 chunks per batch).  Rows past
  // rows_win are loaded too (the clamped address is valid whatever the row) and dropped at the store.
  // Epilogue item q of this thread: tile row er + 32 q, channels ec .. ec + 3.
  // All four are recomputed from the thread id where they are used (fresh_tid keeps the compiler from holding them, and every
  // address built from them, in registers across the MFMA phases: at 11 taps the kernel has none to spare).
  auto fresh_tid = [&]() { int t = tid; asm volatile("" : "+v"(t)); return t; };
  auto load_window = [&](int tile, F* regs) {
    const int ft = fresh_tid(), wr = ft / VPR, wc = (ft % VPR) * G;
    const int win_start = tile * TS - h2 - h1 + wr;
#pragma unroll
    for (int i = 0; i < XB; ++i) {
      const int ti = win_start + i * (NT / VPR);
      const F val = *(const F*)(x + (long long)min(max(ti, 0), a.T - 1) * a.ldx + wc);
      regs[i] = (ti >= 0 && ti < a.T) ? val : zfrag<F>();
    }
  };
  auto store_window = [&](const F* regs) {
    const int ft = fresh_tid(), wr = ft / VPR, wc = (ft % VPR) * G;
#pragma unroll
    for (int i = 0; i < XB; ++i)
      if (wr + i * (NT / VPR) < rows_win) *(F*)(xs + (size_t)(wr + i * (NT / VPR)) * LDX + wc) = lrelu_l(regs[i], 0.1f);
  };
  int tile = blockIdx.x;
  {
    F first[XB];
    load_window(min(tile, ntiles - 1), first);
    store_window(first);
  }
  __syncthreads();
#pragma unroll 1
  for (; tile < ntiles; tile += gridDim.x) {
    const int t0 = tile * TS;
    // ---- requests for the NEXT tile's window and THIS tile's epilogue operands go out first
    F nxt[XB];
    load_window(min(tile + (int)gridDim.x, ntiles - 1), nxt);
    T4 rv[NI], yv[ACCU ? NI : 1];
    {
      const int ft = fresh_tid(), er = ft / IPR, ec = 4 * (ft % IPR);
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const int t = min(t0 + er + q * (NT / IPR), a.T - 1);
        rv[q] = *(const T4*)(x + (long long)t * a.ldx + ec);
        if (ACCU) yv[q] = *(const T4*)(a.y + (long long)t * a.ldy + ec);
      }
    }
    // ---- convs1 (dilation d) over the RY intermediate rows, this wave's 32 output channels: column tiles cg, cg + 4, (cg + 8)
#pragma unroll 1
    for (int n1 = cg; n1 < RY / 32; n1 += 4) {
      f16v acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
        const int shift = tap * a.dil;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const F bf = *(const F*)(xs + (size_t)(n1 * 32 + r + shift) * LDX + ks * KC + G * h);
          mma32l(acc, w1r[tap * KS + ks], bf);
        }
      }
      const int row = n1 * 32 + r, t = t0 - h2 + row;
      const bool inside = t >= 0 && t < a.T;             // convs2 pads its input with zeros, not with convs1 of padding
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = mh * 32 + 8 * g + 4 * h;          // accumulator rows 8 g + 4 h + j of the wave's half
        const f4 b1v = *(const f4*)(bs + c0);
        T4 v = (T4){(T)(acc[4 * g] + b1v[0]), (T)(acc[4 * g + 1] + b1v[1]), (T)(acc[4 * g + 2] + b1v[2]), (T)(acc[4 * g + 3] + b1v[3])};
        v = __builtin_elementwise_max(v, v * (T)0.1f);
        if (!inside) v = (T4){0, 0, 0, 0};
        *(T4*)(ys + (size_t)row * LDX + c0) = v;
      }
    }
    __syncthreads();                                     // the intermediate image is complete; the window is dead
    // ---- convs2 (dilation 1): this wave's 32 output channels of its quarter of the tile's columns
    f16v acc2[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc2[n][i] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap) {
      const T* wb = w2s + (size_t)tap * CC * LDX;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int kk = ks * KC + G * h;
        const F af = *(const F*)(wb + (size_t)(mh * 32 + r) * LDX + kk);
        F bf[TN];
#pragma unroll
        for (int n = 0; n < TN; ++n) bf[n] = *(const F*)(ys + (size_t)((cg * TN + n) * 32 + r + tap) * LDX + kk);
#pragma unroll
        for (int n = 0; n < TN; ++n) mma32l(acc2[n], af, bf[n]);
      }
    }
    // ---- epilogue through LDS (whole channels-last rows per store), the whole tile in one pass
    __syncthreads();                                     // every wave has read the intermediate image
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(f4*)(os + (size_t)((cg * TN + n) * 32 + r) * LDO + mh * 32 + 8 * g + 4 * h) =
            (f4){acc2[n][4 * g], acc2[n][4 * g + 1], acc2[n][4 * g + 2], acc2[n][4 * g + 3]};
    __syncthreads();
    const int ft = fresh_tid(), er = ft / IPR, ec = 4 * (ft % IPR);
    const f4 ebias = *(const f4*)(bs + 64 + ec);
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int tl = er + q * (NT / IPR);
      const int t = t0 + tl;
      if (t >= a.T) continue;
      const f4 av = *(const f4*)(os + (size_t)tl * LDO + ec);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float u = av[j] + ebias[j];
        u += (float)rv[q][j];
        u *= a.scale;
        if (ACCU) u += (float)yv[q][j];
        v[j] = u;
      }
      *(T4*)(a.y + (long long)t * a.ldy + ec) = (T4){(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
    }
    __syncthreads();                 // the fp32 tile (aliasing the window) has been read by every thread
    store_window(nxt);
    __syncthreads();
  }
}

template <int TAPS>
int launch_pair64(const ConvPairArgs& a, hipStream_t s) {
  const int ntiles = cdiv(a.T, Pair64Shape<TAPS>::TS);
  const int grid = std::min(ntiles, 256);              // one workgroup per CU: the LDS footprint allows no second
  return with_flags([&](auto A) {
    return launch_routed<conv_pair64_f16_kernel<TAPS, A.value>, LDS_CAP>(
        route_code(ROUTE_CONV_PAIR, GSV_F16, 64, TAPS, 0, 0, 0, route_flags(false, A.value)), dim3(grid), dim3(512), Pair64Shape<TAPS>::LDS, s, a, ntiles);
  }, a.accumulate != 0);
}

}  // namespace

// called by launch_conv_pair (conv_pair.hip) after its operand, shape and alignment checks
int launch_conv_pair64(const ConvPairArgs& a, hipStream_t s) {
  const _Float16 *xe = a.x + (long long)(a.T - 1) * a.ldx + 64, *ye = a.y + (long long)(a.T - 1) * a.ldy + 64;
  GSV_REQUIRE(ye <= a.x || xe <= a.y, "conv_pair: C = 64 does not run in place (y overlaps x, which other workgroups read as halo)");
  GSV_REQUIRE(a.ldy % 4 == 0 && ((uintptr_t)a.y % 8) == 0 && a.ldx >= 64 && a.ldy >= 64, "conv_pair: C = 64 stores rows as 8-byte vectors");
  switch (a.taps) {
    case 3: return launch_pair64<3>(a, s);
    case 5: return launch_pair64<5>(a, s);
    case 7: return launch_pair64<7>(a, s);
    case 9: return launch_pair64<9>(a, s);
    case 11: return launch_pair64<11>(a, s);
    default: set_error("conv_pair: no kernel for taps=%d", a.taps); return GSV_ERR_ARG;
  }
}

}  // namespace gsv
