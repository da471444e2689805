// LDS-tiled GEMM on MFMA (taps == 1): Y[t][n] = X[t][:] . W[n][:], the prefill projections (M = sum of prompt
// lengths, K = 512 / 2048), the 1x1 convs of enc_p and the Linear layers of the DiT and of BWE.  128 (n) x 128 (t) tile,
// BK = 64, both operands double-buffered in LDS through registers: the loads of K-chunk c+1 are in flight while
// chunk c feeds 16 MFMAs per wave, one barrier per chunk; ~74 KB of LDS -> two workgroups per CU.
#include "conv_launch.h"
#include "mfma_frag.h"

namespace gsv {

// NW = waves per workgroup: 4 (64 x 64 outputs per wave; two workgroups per CU when the grid is large enough) or 8 (64 x 32 per
// wave: for grids with fewer tiles than CUs, where a workgroup is alone on its CU and a second wave per SIMD hides its stalls)
#ifndef GSV_GEMM_W8_BK
#define GSV_GEMM_W8_BK 128
#endif
// GROWS: per-row gates (ConvArgs::gate_rows): the gate vector is looked up per OUTPUT ROW in the epilogue (a 128-row tile spans
// several utterances) instead of once per thread in the prologue; everything else, the summation order included, is the same
template <typename T, bool RES, bool WNT = false, int NW = 4, bool GROWS = false>
__global__ __launch_bounds__(NW * 64) void gemm_lds_kernel(ConvArgs a) {
  typedef typename FragL<T>::type F;
  constexpr int G = DT<T>::G, KC = 2 * G;
  // K elements per chunk: 128 B per row (64 fp16 / 32 fp32); the 8-wave fp16 form (one workgroup per CU, 139 KB of LDS) stages
  // 256-B rows: half as many iterations, barriers and load round trips per tile
  constexpr int BK = (NW == 8 && sizeof(T) == 2 ? GSV_GEMM_W8_BK : 64 * 2 / (int)sizeof(T));
  constexpr int LDX = BK + G;
  constexpr int VPR = BK / G;                        // 8 vectors per row
  constexpr int CT = 128, TT = 128, NT = NW * 64;
  constexpr int NLD = CT * VPR / NT;                 // vectors per thread per operand per chunk (4 / 2)
  constexpr int TM = 2, TN = NW == 8 ? 1 : 2, WN = NW == 8 ? 4 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* xs = (T*)smem;                                  // [2][TT][LDX]
  T* ws = xs + 2 * TT * LDX;                         // [2][CT][LDX]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;
  // XCD-aware tile order (unbatched launches): each XCD's L2 keeps a contiguous band of output-channel tiles' weights
  int bx = blockIdx.x, by = blockIdx.y;
  if (gridDim.z == 1 && a.xcd_order) {
    const int vid = xcd_virtual_id(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    if (a.xcd_order == 2) { by = vid % gridDim.y; bx = vid / gridDim.y; }      // an XCD gets all column tiles of a band of ROW tiles
    else { bx = vid % gridDim.x; by = vid / gridDim.x; }
  }
  const int t0 = bx * TT, cout0 = by * CT;
  const int z = blockIdx.z;                            // batch (attention heads): operand / output offsets
  const T* __restrict__ x = (const T*)a.x + (long long)z * a.xz;
  const T* __restrict__ w = (const T*)a.w + (long long)z * a.wz;
  const long long ybase = (long long)z * a.yz, rbase = (long long)z * a.rz;
  const int K = a.Cin;

  // epilogue operands first (see conv_lds_kernel)
  constexpr int LDO = CT + 4, PR = TN * 32, IPR = CT / 4, NI = PR * IPR / NT;
  typedef T T4 __attribute__((ext_vector_type(4)));
  const bool vec_ok = ((a.ldy & 3) == 0) && ((a.y_col0 & 3) == 0) && ((a.ldr & 3) == 0);
  const int ecg = tid % IPR, ec = cout0 + 4 * ecg;
  const int env = max(0, min(4, a.Cout - ec));
  f4 ebias = (f4){0.f, 0.f, 0.f, 0.f};
  if (a.bias) for (int j = 0; j < env; ++j) ebias[j] = a.bias[z * a.bz + ec + j];
  f4 egate = (f4){1.f, 1.f, 1.f, 1.f};
  if constexpr (!GROWS)
    if (a.gate) for (int j = 0; j < env; ++j) egate[j] = a.gate[z * a.bz + ec + j];
  T4 rv[RES ? WN * NI : 1];
  rv[0] = (T4){(T)0.f, (T)0.f, (T)0.f, (T)0.f};
  if (RES) {
#pragma unroll
    for (int q = 0; q < WN * NI; ++q) {
      rv[q] = (T4){(T)0.f, (T)0.f, (T)0.f, (T)0.f};
      const int pass = q / NI, e = q - pass * NI;
      const int t = t0 + pass * PR + (tid + e * NT) / IPR;
      if (t < a.T_virt && env > 0) {
        const T* rp = (const T*)a.res + rbase + (long long)t * a.ldr + ec;
        if (vec_ok && env == 4) rv[q] = *(const T4*)rp;
        else for (int j = 0; j < env; ++j) rv[q][j] = rp[j];
      }
    }
  }

  f16v acc[TM][TN];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;

  auto load_tiles = [&](int k0, F* xr, F* wr) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int v = tid + i * NT;
      const int row = v / VPR, col = v - row * VPR;
      const int kk = k0 + col * G;
      const int t = t0 + row, co = cout0 + row;
      xr[i] = (t < a.T_in && kk < K) ? *(const F*)(x + (long long)t * a.ldx + kk) : zfrag<F>();
      if (WNT) wr[i] = (co < a.Cout && kk < K) ? __builtin_nontemporal_load((const F*)(w + (long long)co * a.ldw + kk)) : zfrag<F>();
      else wr[i] = (co < a.Cout && kk < K) ? *(const F*)(w + (long long)co * a.ldw + kk) : zfrag<F>();
    }
  };
  auto store_tiles = [&](int buf, F* xr, const F* wr) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int v = tid + i * NT;
      const int row = v / VPR, col = v - row * VPR;
      F val = xr[i];
      if (a.pre_act == ACT_LRELU) val = lrelu_l(val, a.pre_slope);
      else if (a.pre_act == ACT_RELU) val = relu_l(val);
      *(F*)(xs + ((size_t)buf * TT + row) * LDX + col * G) = val;
      *(F*)(ws + ((size_t)buf * CT + row) * LDX + col * G) = wr[i];
    }
  };
  // Two chunks in flight (round 3, the 8-wave variant = ONE workgroup per CU): chunk c is multiplied from LDS buffer c & 1 while chunk c + 1 waits in one register set and
  // chunk c + 2 is being requested into the other.  With ONE chunk of prefetch distance an iteration (16-32 MFMAs per wave,
  // ~0.2 us) could not be shorter than a global-load round trip (1-2 us under load): the K = 512 GEMMs of the AR prefill ran 8
  // such iterations per tile, 9 x their MFMA time.  The loop is unrolled by two so that the register sets keep static names.
  const int nchunks = (K + BK - 1) / BK;
  auto compute = [&](int buf) {
    const T* xb = xs + (size_t)buf * TT * LDX;
    const T* wb = ws + (size_t)buf * CT * LDX;
#pragma unroll
    for (int ks = 0; ks < BK / KC; ++ks) {
      const int kk = ks * KC + G * h;
      F af[TM], bf[TN];
#pragma unroll
      for (int m = 0; m < TM; ++m) af[m] = *(const F*)(wb + (size_t)((wm * TM + m) * 32 + r) * LDX + kk);
#pragma unroll
      for (int n = 0; n < TN; ++n) bf[n] = *(const F*)(xb + (size_t)((wn * TN + n) * 32 + r) * LDX + kk);
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) mma32l(acc[m][n], af[m], bf[n]);
    }
  };
  if constexpr (NW == 8) {
    F xa[NLD], wa[NLD], xq[NLD], wq[NLD];
    load_tiles(0, xa, wa);
    store_tiles(0, xa, wa);
    load_tiles(BK, xa, wa);                            // chunk 1 (zeros beyond K: load_tiles tests every element)
    __syncthreads();
    for (int c = 0; c < nchunks; c += 2) {
      load_tiles((c + 2) * BK, xq, wq);
      compute(0);
      if (c + 1 >= nchunks) break;
      store_tiles(1, xa, wa);
      __syncthreads();
      load_tiles((c + 3) * BK, xa, wa);
      compute(1);
      if (c + 2 < nchunks) {
        store_tiles(0, xq, wq);
        __syncthreads();
      }
    }
  } else {
    // 4 waves: two workgroups per CU already keep two chunks in flight per CU, and the second register set would cost the second
    // workgroup (118 -> 214 VGPRs + 64 accumulators); measured: 39.3 vs 40.1 us on the prefill's QKV / FFN1 launches
    {
      F xr[NLD], wr[NLD];
      load_tiles(0, xr, wr);
      store_tiles(0, xr, wr);
    }
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      const int buf = c & 1;
      F xr[NLD], wr[NLD];
      const bool more = c + 1 < nchunks;
      if (more) load_tiles((c + 1) * BK, xr, wr);
      compute(buf);
      if (more) {
        store_tiles(buf ^ 1, xr, wr);
        __syncthreads();
      }
    }
  }

  float* os = (float*)smem;                           // [PR][LDO]
  int gb = 0, glim = 0, gcur = -1;                    // GROWS: utterance of the row at hand, first row of the next one, the one loaded
  if constexpr (GROWS) { gb = t0 / a.gate_rows; glim = (gb + 1) * a.gate_rows; }
#pragma unroll
  for (int pass = 0; pass < WN; ++pass) {
    __syncthreads();
    if (wn == pass) {
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          const int tl = n * 32 + r;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int cl = (wm * TM + m) * 32 + 8 * g + 4 * h;
            *(f4*)(os + (size_t)tl * LDO + cl) = (f4){acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]};
          }
        }
    }
    __syncthreads();
    // the activation code is tested once per pass, not per element (conv_wide.hip: ~50 scalar instructions per value otherwise)
    auto items = [&](auto act_tag) {
  #pragma unroll
      for (int e = 0; e < NI; ++e) {
        const int q = pass * NI + e;
        const int tl = (tid + e * NT) / IPR;
        const int t = t0 + pass * PR + tl;
        if (!(t < a.T_virt && env > 0)) continue;
        const f4 av = *(const f4*)(os + (size_t)tl * LDO + 4 * ecg);
        if constexpr (GROWS) {
          // the thread's items come in ascending t and its four channels are fixed: walk the utterance index forward from the
          // tile's first (one uniform division per workgroup) and reload the gate values only when the utterance changes
          while (t >= glim) { ++gb; glim += a.gate_rows; }
          if (gb != gcur) {
            gcur = gb;
            const float* gp = a.gate + (long long)gb * a.gate_ld + ec;
            for (int j = 0; j < env; ++j) egate[j] = gp[j];
          }
        }
        float v[4];
  #pragma unroll
        for (int j = 0; j < 4; ++j) {
          float u = (av[j] + ebias[j]) * egate[j];
          if (RES) u += to_f(rv[q][j]);
          u *= a.scale;
          u = post_act_c<decltype(act_tag)::value>(a.post_act, u);
          v[j] = u;
        }
        const long long yoff = ybase + (long long)t * a.ldy + a.y_col0 + ec;
        const bool vec = vec_ok && env == 4 && ((ybase & 3) == 0);
        if (a.out_f32) {
          float* yp = (float*)a.y + yoff;
          if (vec) *(f4*)yp = (f4){v[0], v[1], v[2], v[3]};
          else for (int j = 0; j < env; ++j) yp[j] = v[j];
        } else {
          T* yp = (T*)a.y + yoff;
          if (vec) *(T4*)yp = (T4){(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
          else for (int j = 0; j < env; ++j) yp[j] = (T)v[j];
        }
      }
    };
    GSV_ACT_DISPATCH(a.post_act, items);
  }
}

// 0 = launched, 1 = not eligible, < 0 = error
template <typename T> static int launch_gemm_lds_t(const ConvArgs& a, hipStream_t s) {
  constexpr int G = DT<T>::G;
  constexpr int BK = 64 * 2 / (int)sizeof(T);
  const ConvSwitches& sw = conv_switches();
  if (a.taps != 1 || a.stride != 1 || a.ups_u > 0 || a.accumulate || a.pad != 0) return 1;
  if (a.T_virt < 512 || a.Cout < 96 || a.Cin % (2 * G) != 0 || a.Cin < BK) return 1;
  if (a.Z > 1 && ((a.xz % G) || (a.wz % G) || (a.res && (!a.z_res || a.rz % G)))) return 1;   // batched: head slices must stay 16-byte aligned
  if (a.res && a.res_f32) return 1;
  if (!operands_aligned<G>(a)) return 1;
  const dim3 grid(cdiv(a.T_virt, 128), cdiv(a.Cout, 128), a.Z);
  ConvArgs b = a;
  b.xcd_order = sw.gemm_xcd ? 1 : 0;
  // Which operand an XCD's L2 should keep: every tile streams one activation panel [128][K] and one weight panel [128][K].
  // Order 1 gives an XCD a band of weight panels (all row tiles of a few column tiles); when the activations are the larger
  // operand and ALL weights fit an L2 anyway (prefill: 5760 x 2048 activations = 23.6 MB against 2 MB of weights), order 2 gives
  // it a band of row tiles with all their column tiles, so that an activation panel is fetched from memory once per XCD
  // instead of once per column tile (tools/gemm_probe.py, GSV_GEMM_XCD=1 restores order 1).
  if (sw.gemm_xcd == 2 && (long long)a.T_virt > 2LL * a.Cout && (size_t)a.Cout * a.Cin * sizeof(T) <= (size_t)3 << 20) b.xcd_order = 2;
  // 8 waves per workgroup where the grid has fewer tiles than the chip has CUs (prefill out-projection / FFN2: 180 tiles, the
  // DiT's QKV: 192, enc_p 1 x 1 convs): the workgroup is alone on its CU; GSV_GEMM_WAVES=4 restores round 2's geometry
  const bool w8 = sizeof(T) == 2 && sw.gemm_waves == 8 && (long long)grid.x * grid.y * grid.z <= sw.gemm_w8_max_tiles && a.Cin >= GSV_GEMM_W8_BK;
  // 4 waves: 73.7 KB (the epilogue tile, 33.8 KB, fits inside); 8 waves: 139 KB at 128-wide chunks
  const size_t lds = (size_t)2 * (128 + 128) * ((w8 ? GSV_GEMM_W8_BK : BK) + G) * sizeof(T);
  auto launch = [&](auto R, auto NTW, auto W8) {
    constexpr int NW = W8.value ? 8 : 4;
    return launch_routed<gemm_lds_kernel<T, R.value, NTW.value, NW>, LDS_CAP>(
        route_code(ROUTE_GEMM_LDS, DT<T>::id, NW, b.xcd_order, 0, 0, 0, route_flags(R.value, false, false, NTW.value)), grid, dim3(NW * 64), lds, s, b);
  };
  // per-row gates: the residual form only (the DiT's gated GEMMs carry one); without a residual the launch goes on to conv_gemm
  if (a.gate_rows) {
    if (!a.res || a.Z != 1) return 1;
    return with_flags([&](auto W8) {
      constexpr int NW = W8.value ? 8 : 4;
      return launch_routed<gemm_lds_kernel<T, true, false, NW, true>, LDS_CAP>(
          route_code(ROUTE_GEMM_LDS, DT<T>::id, NW, b.xcd_order, 0, 0, 0, route_flags(true, false) | ROUTE_GROWS), grid, dim3(NW * 64), lds, s, b);
    }, w8);
  }
  // the residual form has no non-temporal variant
  if (a.res) return with_flags([&](auto W8) { return launch(std::true_type{}, std::false_type{}, W8); }, w8);
  return with_flags([&](auto NTW, auto W8) { return launch(std::false_type{}, NTW, W8); }, a.w_nt != 0, w8);
}

int launch_gemm_lds(int dtype, const ConvArgs& a, hipStream_t s) {
  if (dtype == GSV_F16) return launch_gemm_lds_t<_Float16>(a, s);
  if (dtype == GSV_F32) return launch_gemm_lds_t<float>(a, s);
  return 1;
}

}  // namespace gsv
