// One ResBlock pair of the HiFi-GAN generator's narrow stages in ONE kernel (gfx950, fp16):
//
//     y = ( convs2( lrelu( convs1( lrelu(x) ) ) ) + x ) * scale  [+ y]          (reference module/models.py:262-283: ResBlock1)
//
// convs1 has dilation d, convs2 dilation 1, both k taps, C -> C channels with C = 16 or 32 (the last two generator stages at
// 2 M / 4.1 M samples: 131 MB per tensor).  As two launches a pair moves 5 tensors through HBM (x in, t out | t in, x as
// residual, y out); fused it moves 2 (x once -- the residual rows come out of L2, where the window load left them -- and y).
// Construction = conv_narrow_f16_kernel (conv_narrow.hip) twice inside one persistent 256-step tile:
//   convs1's weights in registers (A-fragments, loaded once per wave), convs2's in LDS
//   window  x[t0 - h2 - h1, t0 - h2 + 288 + h1) -> LDS (lrelu while staging), prefetched one tile ahead in registers
//   convs1 over 288 rows (9 MFMA column tiles dealt to the 4 waves) -> + bias -> fp16 -> lrelu -> zero outside [0, T)  -> LDS
//   convs2 over the tile's 256 rows from that LDS image -> fp32 tile transposed through LDS -> + bias + x, * scale, (+ y) -> rows
// Every rounding point of the two-launch path is kept (fp16 intermediate, fp16 lrelu, same tap / k order of the MFMAs): the
// result is bit-identical to it, except that with scale != 1 AND accumulate the compiler contracts the last two operations of
// the two epilogues differently (one fp16 ulp on ~0.02 % of the elements; tests/test_ops_gpu.py::test_conv_pair_matches_two_launches).
// SEG = true is the same pair inside a segmented decode (gsv_op_conv_pair_seg; gap rows of the intermediate and of y are 0).
#include "conv_launch.h"

namespace gsv {

namespace {

typedef _Float16 T;
typedef h8 F;
typedef _Float16 T4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mma32p(f16v& acc, const h8& a, const h8& b) { acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ h8 lrelu8(h8 v, float s) { h8 t = v * (_Float16)s; return __builtin_elementwise_max(v, t); }
__device__ __forceinline__ T4 lrelu4(T4 v, float s) { T4 t = v * (_Float16)s; return __builtin_elementwise_max(v, t); }

constexpr int ROWS_Y = 288;      // intermediate rows per tile (9 x 32 >= 256 + 2 * 5)
constexpr int ROWS_X = 338;      // window rows at most (288 + 2 * 5 * 5)

// SEG = the pair of a segmented decode (gsv_vits_decode_segments): row_seg holds one int32 per row, -1 = gap row.  An intermediate
// gap row goes into the LDS image as 0 and an output gap row is stored as 0, which is what the row passes after convs1 and convs2
// do on the two-launch path.  Everything SEG adds sits under `if constexpr (SEG)` and row_seg is a trailing kernel argument that
// the unmasked instantiations never read (ConvPairArgs keeps its layout): they keep the registers and scratch they had without it.
// second launch bound = waves per SIMD the register allocation must leave room for: 2 workgroups per CU at C = 32, 3 at C = 16
template <int CC, int TAPS, bool ACCU, bool SEG>
__global__ __launch_bounds__(256, CC == 32 ? 2 : 3) void conv_pair_f16_kernel(ConvPairArgs a, int ntiles, const int* __restrict__ row_seg) {
  constexpr int G = 8, KC = 16, CT = 32, WN = 4, TN = 2, NT = 256;
  constexpr int LDX = CC + G, VPR = CC / G;
  constexpr int XB = (ROWS_X * VPR + NT - 1) / NT;
  // epilogue passes of 128 (C = 16) / 256 (C = 32) rows: the fp32 tile may take the window AND the intermediate image by then
  constexpr int WPP = CC == 16 ? 2 : 4, NP = WN / WPP;
  constexpr int LDO = CT + 4, PR = TN * 32 * WPP, IPR = CT / 4, NI = PR * IPR / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = (T*)smem;                                   // [ROWS_X][LDX]; the epilogue's fp32 [PR][LDO] tile aliases it
  T* ys = xs + (size_t)ROWS_X * LDX;                  // [ROWS_Y][LDX] lrelu(convs1(...)) of this tile
  T* w2s = ys + (size_t)ROWS_Y * LDX;                 // [TAPS][CT][LDX] convs2's weights; convs1's live in registers (below)
  float* os = (float*)smem;
  static_assert(PR * LDO * 4 <= (ROWS_X + ROWS_Y) * LDX * 2, "epilogue tile must fit in window + intermediate image");
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const T* __restrict__ x = a.x;
  const int h2 = (TAPS - 1) / 2, h1 = h2 * a.dil;
  const int rows_win = ROWS_Y + 2 * h1;
  const int total = rows_win * VPR;
  const int ecg = tid % IPR, ec = 4 * ecg;
  const int env = max(0, min(4, CC - ec));
  f4 ebias = (f4){0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < env; ++j) ebias[j] = a.b2[ec + j];
  // convs1's bias for the channels this lane holds in an accumulator: rows 8 g + 4 h + j
  f4 b1v[4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = 8 * g + 4 * h + j; b1v[g][j] = c < CC ? a.b1[c] : 0.f; }
  // ---- convs2's weights into LDS, convs1's into registers (every wave multiplies all of them by its own column tiles: TAPS *
  // CC / 16 A-fragments = 44 / 88 VGPRs at 11 taps; keeping them out of LDS is what lets 2 (C = 32) to 4 (C = 16) workgroups
  // share a CU -- with both slabs in LDS the C = 32 kernel ran one workgroup per CU and was slower than two launches)
  {
    const int totw = TAPS * CT * VPR;
    for (int v = tid; v < totw; v += NT) {
      const int tap = v / (CT * VPR), rem = v - tap * (CT * VPR);
      const int row = rem / VPR, col = rem - row * VPR;
      F val = {0, 0, 0, 0, 0, 0, 0, 0};
      if (row < CC) val = *(const F*)(a.w2 + (long long)row * TAPS * CC + (long long)tap * CC + col * G);
      *(F*)(w2s + ((size_t)tap * CT + row) * LDX + col * G) = val;
    }
  }
  F w1r[TAPS * (CC / KC)];
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
    for (int ks = 0; ks < CC / KC; ++ks) {
      F val = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < CC) val = *(const F*)(a.w1 + (long long)r * TAPS * CC + (long long)tap * CC + ks * KC + G * h);
      w1r[tap * (CC / KC) + ks] = val;
    }
  auto load_window = [&](int tile, F* regs) {
    const int win_start = tile * 256 - h2 - h1;
#pragma unroll
    for (int i = 0; i < XB; ++i) {
      const int v = min(tid + i * NT, total - 1);
      const int row = v / VPR, col = v - row * VPR;
      const int ti = win_start + row;
      const F val = *(const F*)(x + (long long)min(max(ti, 0), a.T - 1) * a.ldx + col * G);
      regs[i] = (ti >= 0 && ti < a.T) ? val : (F){0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  auto store_window = [&](const F* regs) {
#pragma unroll
    for (int i = 0; i < XB; ++i) {
      const int v = tid + i * NT;
      if (v < total) {
        const int row = v / VPR, col = v - row * VPR;
        *(F*)(xs + (size_t)row * LDX + col * G) = lrelu8(regs[i], 0.1f);
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
    const int t0 = tile * 256;
    // ---- requests for the NEXT tile's window and THIS tile's epilogue operands go out first
    F nxt[XB];
    load_window(min(tile + (int)gridDim.x, ntiles - 1), nxt);
    T4 rv[NP * NI], yv[ACCU ? NP * NI : 1];
    constexpr int NS1 = (ROWS_Y / 32 + WN - 1) / WN;
    int so[SEG ? NP * NI : 1], s1[SEG ? NS1 : 1];
#pragma unroll
    for (int q = 0; q < NP * NI; ++q) {
      const int pass = q / NI, e = q - pass * NI;
      const int t = min(t0 + pass * PR + (tid + e * NT) / IPR, a.T - 1);
      const int cc = min(ec, CC - 4);
      rv[q] = *(const T4*)(x + (long long)t * a.ldx + cc);
      if (ACCU) yv[q] = *(const T4*)(a.y + (long long)t * a.ldy + cc);
      if constexpr (SEG) so[q] = row_seg[t];
    }
    if constexpr (SEG) {               // the intermediate rows of this lane's column tiles (wn, wn + 4, wn + 8)
#pragma unroll
      for (int i = 0; i < NS1; ++i) s1[i] = row_seg[min(max(t0 - h2 + (wn + i * WN) * 32 + r, 0), a.T - 1)];
    }
    // ---- convs1 (dilation d) over the 288 intermediate rows: column tiles wn, wn + 4 and, wave 0, tile 8
    for (int n1 = wn, i1 = 0; n1 < ROWS_Y / 32; n1 += WN, ++i1) {
      f16v acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
        const int shift = tap * a.dil;
#pragma unroll
        for (int ks = 0; ks < CC / KC; ++ks) {
          const int kk = ks * KC + G * h;
          const F bf = *(const F*)(xs + (size_t)(n1 * 32 + r + shift) * LDX + kk);
          mma32p(acc, w1r[tap * (CC / KC) + ks], bf);
        }
      }
      const int row = n1 * 32 + r, t = t0 - h2 + row;
      bool inside = t >= 0 && t < a.T;                   // convs2 pads its input with zeros, not with convs1 of padding
      if constexpr (SEG) inside = inside && (i1 == 0 ? s1[0] : i1 == 1 ? s1[1] : s1[2]) >= 0;   // nor with convs1 of a gap row
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 8 * g + 4 * h;
        if (c0 < CC) {
          T4 v = (T4){(T)(acc[4 * g] + b1v[g][0]), (T)(acc[4 * g + 1] + b1v[g][1]), (T)(acc[4 * g + 2] + b1v[g][2]),
                      (T)(acc[4 * g + 3] + b1v[g][3])};
          v = lrelu4(v, 0.1f);
          if (!inside) v = (T4){0, 0, 0, 0};
          *(T4*)(ys + (size_t)row * LDX + c0) = v;
        }
      }
    }
    __syncthreads();                                     // the intermediate image is complete; the window is dead
    // ---- convs2 (dilation 1) over the tile's 256 rows
    f16v acc2[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc2[n][i] = 0.f;
    for (int tap = 0; tap < TAPS; ++tap) {
      const T* wb = w2s + (size_t)tap * CT * LDX;
#pragma unroll
      for (int ks = 0; ks < CC / KC; ++ks) {
        const int kk = ks * KC + G * h;
        const F af = *(const F*)(wb + (size_t)r * LDX + kk);
        F bf[TN];
#pragma unroll
        for (int n = 0; n < TN; ++n) bf[n] = *(const F*)(ys + (size_t)((wn * TN + n) * 32 + r + tap) * LDX + kk);
#pragma unroll
        for (int n = 0; n < TN; ++n) mma32p(acc2[n], af, bf[n]);
      }
    }
    // ---- epilogue through LDS (whole channels-last rows per store), one wave column per pass
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
      __syncthreads();
      if (wn / WPP == pass) {
#pragma unroll
        for (int n = 0; n < TN; ++n)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(f4*)(os + (size_t)(((wn % WPP) * TN + n) * 32 + r) * LDO + 8 * g + 4 * h) =
                (f4){acc2[n][4 * g], acc2[n][4 * g + 1], acc2[n][4 * g + 2], acc2[n][4 * g + 3]};
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < NI; ++e) {
        const int q = pass * NI + e;
        const int tl = (tid + e * NT) / IPR;
        const int t = t0 + pass * PR + tl;
        if (!(t < a.T && env > 0)) continue;
        const f4 av = *(const f4*)(os + (size_t)tl * LDO + 4 * ecg);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float u = av[j] + ebias[j];
          u += (float)rv[q][j];
          if constexpr (SEG && ACCU) {
            // the unmasked kernel rounds `* scale + y` once to fp32 (v_pk_fma_f32) and then to fp16.  Next to the select the
            // compiler turns half of the lanes into v_fma_mixlo_f16, which rounds once, to fp16: 1 ulp apart on ~0.01 % of the
            // elements.  A map without gaps must give the unmasked pair's bits, so the fp32 value is pinned before the select.
            u = __builtin_fmaf(u, a.scale, (float)yv[q][j]);
            asm volatile("" : "+v"(u));
          } else {
            u *= a.scale;
            if (ACCU) u += (float)yv[q][j];
          }
          if constexpr (SEG) u = so[q] < 0 ? 0.f : u;
          v[j] = u;
        }
        T* yp = a.y + (long long)t * a.ldy + ec;
        if (env == 4) *(T4*)yp = (T4){(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
        else for (int j = 0; j < env; ++j) yp[j] = (T)v[j];
      }
    }
    __syncthreads();                 // the fp32 tile (aliasing the window) has been read by every thread
    store_window(nxt);
    __syncthreads();
  }
}

template <int CC, int TAPS>
int launch_pair(const ConvPairArgs& a, const int* row_seg, hipStream_t s) {
  const int ntiles = cdiv(a.T, 256);
  const size_t lds = ((size_t)ROWS_X + ROWS_Y + (size_t)TAPS * 32) * (CC + 8) * 2;
  const int per_cu = std::max(1, std::min(conv_switches().pair_per_cu, (int)((156 * 1024) / lds)));
  const int grid = std::min(ntiles, 256 * per_cu);
  return with_flags([&](auto A, auto SEG) {
    return launch_routed<conv_pair_f16_kernel<CC, TAPS, A.value, SEG.value>, LDS_CAP>(
        route_code(ROUTE_CONV_PAIR, GSV_F16, CC, TAPS, 0, 0, 0, route_flags(false, A.value) | (SEG.value ? ROUTE_SEG : 0)), dim3(grid), dim3(256), lds, s,
        a, ntiles, row_seg);
  }, a.accumulate != 0, row_seg != nullptr);
}

template <int CC>
int launch_pair_taps(const ConvPairArgs& a, const int* row_seg, hipStream_t s) {
  switch (a.taps) {
    case 3: return launch_pair<CC, 3>(a, row_seg, s);
    case 5: return launch_pair<CC, 5>(a, row_seg, s);
    case 7: return launch_pair<CC, 7>(a, row_seg, s);
    case 9: return launch_pair<CC, 9>(a, row_seg, s);
    case 11: return launch_pair<CC, 11>(a, row_seg, s);
    default: set_error("conv_pair: no kernel for taps=%d", a.taps); return GSV_ERR_ARG;
  }
}

}  // namespace

bool conv_pair_supported(int dtype, int C, int taps, int dil, int T, bool seg) {
  // taps: exactly the instantiated kernels (launch_pair_taps, launch_conv_pair64); any other count would read tap slabs past w1 / w2
  const bool inst = taps == 3 || taps == 5 || taps == 7 || taps == 9 || taps == 11;
  // C = 64 (conv_pair64.hip) has no masked instantiation: a segmented decode keeps its two convs there
  const bool chan = C == 16 || C == 32 || (C == 64 && !seg);
  return !conv_switches().no_conv_pair && dtype == GSV_F16 && chan && inst && dil >= 1 && ((taps - 1) / 2) * dil <= 25 && T >= 256;
}

bool conv_pair_eligible(int dtype, int C, int taps, int dil, int T, bool seg) {
  if (!conv_pair_supported(dtype, C, taps, dil, T, seg)) return false;
  // the 64-channel pair takes over where the persistent narrow conv does (conv_narrow.hip narrow_channels): below it the two
  // convs are conv_lds launches that fill the GPU with small tiles, and one workgroup per CU of 128 / 256-step tiles does not
  if (C == 64) return !conv_switches().no_conv_pair64 && T >= 16384;
  return true;
}

namespace {
int launch_conv_pair_any(const ConvPairArgs& a, const int* row_seg, hipStream_t s) {
  GSV_REQUIRE(a.x && a.y && a.w1 && a.w2 && a.b1 && a.b2, "conv_pair: null operand");
  GSV_REQUIRE(conv_pair_supported(GSV_F16, a.C, a.taps, a.dil, a.T, row_seg != nullptr) || conv_switches().no_conv_pair, "conv_pair: shape C=%d taps=%d dil=%d T=%d not supported",
              a.C, a.taps, a.dil, a.T);
  GSV_REQUIRE(a.ldx % 8 == 0 && a.ldy % 4 == 0 && ((uintptr_t)a.x % 16) == 0 && ((uintptr_t)a.w1 % 16) == 0 && ((uintptr_t)a.w2 % 16) == 0,
              "conv_pair: operands must be 16-byte aligned");
  if (a.C == 64) return launch_conv_pair64(a, s);
  return a.C == 16 ? launch_pair_taps<16>(a, row_seg, s) : launch_pair_taps<32>(a, row_seg, s);
}
}  // namespace

int launch_conv_pair(const ConvPairArgs& a, hipStream_t s) {
  set_conv_route(0);
  return launch_conv_pair_any(a, nullptr, s);
}

int launch_conv_pair_seg(const ConvPairArgs& a, const int* row_seg, hipStream_t s) {
  set_conv_route(0);
  GSV_REQUIRE(row_seg, "conv_pair_seg: row_seg is null (the unmasked pair is launch_conv_pair)");
  return launch_conv_pair_any(a, row_seg, s);
}

}  // namespace gsv
