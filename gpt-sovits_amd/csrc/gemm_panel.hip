// Panel GEMM of the AR prefill (fp16, taps == 1): Y[t][n] = X[t][:] . W[n][:] for the three epilogue forms t2s_prefill_rows passes
// (fp16 out + bias, fp16 out + bias + ReLU, fp32 out + bias + fp16 residual).  gemm_lds.hip cuts 128 x 128 tiles whatever the
// shape; at M = 5760 that is 1.05 - 1.4 rounds of 512 slots (QKV, FFN1) or 180 tiles on 256 CUs (the N = 512 layers).  Here a
// template parameter picks the tile from a small family so that each of the four shapes runs as ONE round of 240 workgroups,
// one per CU, and the K chunks of a tile arrive through a ring of LDS buffers filled by LDS-DMA, so that a workgroup alone on
// its CU keeps several chunks in flight.
//
// Bit-identity with gemm_lds_kernel: per output element the same mfma_f32_32x32x16_f16 sequence (weights as A, activations as
// B, K ascending in steps of 16, one accumulator, zero start) and the same fp32 epilogue in the same order: (acc + bias),
// + residual, * scale, activation, one rounding.  Tile shape, staging and store width move no sum.
//
// Staging: a stage is [TR activation rows | TC weight rows] x 128 B (BK = 64 halfs).  One global_load_lds_dwordx4 writes 8 whole
// rows lane-linear; the XOR swizzle sits on the SOURCE address and on the ds_read_b128 alike (slot ^ ((row >> 1) & 7): the 16
// lanes of a read group, rows r .. r + 15 at one logical slot, land on 16 distinct 16-byte bank groups).  Rows beyond M / N
// are clamped to the last valid row (never padded in memory); their outputs are not stored.  The DMA is issued from inline
// asm (M0 is written in the statement that reads it), so the compiler neither counts nor drains it: chunk c is waited for
// with a counted vmcnt that leaves the NS - 2 younger chunks in flight, then a raw s_barrier.
#include "conv_launch.h"
#include "mfma_frag.h"

namespace gsv {

namespace {

struct PanelArgs {
  const _Float16* x; const _Float16* w; const float* bias; void* y; const _Float16* res;
  int M, N, K, ldx, ldw, ldy, ldr;
  float scale;
  int relu, xcd_order, gy;
};

typedef __attribute__((address_space(3))) unsigned char lds_byte;

// LDS-DMA of 8 rows x 128 B (16 B per lane, lane i -> lds_dst + 16 i)
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// chunk hand-off: at most N younger DMA instructions stay in flight; this wave's LDS reads are complete
template <int N> __device__ __forceinline__ void wait_dma_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
}

// TB x CB = tile in 32-row blocks (t rows x n columns), WT x WN waves (t x n), NS ring stages.
// RES: fp32 out + fp16 residual; otherwise fp16 out (ReLU by a.relu).
// SUM2: the summation of gemm_t64_f16_kernel (gemm_sk.hip) instead of gemm_lds': two accumulators per element, the even k-steps of
// 16 in one and the odd ones in the other, each ascending, added once in front of the epilogue.  Up to 2048 rows the dispatcher
// launches gemm_t64 for the prefill's shapes; with this form the panel kernel computes the dispatcher's bits there as well.
template <int TB, int CB, int WT, int WN, int NS, bool RES, bool SUM2 = false>
__global__ __launch_bounds__(WT * WN * 64) void gemm_panel_kernel(PanelArgs a) {
  constexpr int NW = WT * WN, NT = NW * 64;
  constexpr int TR = TB * 32, TC = CB * 32, RT = TR + TC;
  constexpr int TM = CB / WN, TN = TB / WT;            // 32 x 32 accumulators per wave: TM (n) x TN (t)
  constexpr int L = RT / 8 / NW;                       // DMA instructions per wave per chunk
  constexpr int STAGE = RT * 128;
  static_assert(CB % WN == 0 && TB % WT == 0 && (RT / 8) % NW == 0 && TR % 8 == 0, "tile / wave geometry");
  static_assert(L * (NS - 2) <= 63, "vmcnt is a 6-bit count");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int wt = wave / WN, wn = wave % WN;
  int bx, by;
  {
    const int n = gridDim.x;
    const int vid = a.xcd_order ? xcd_virtual_id(blockIdx.x, n) : (int)blockIdx.x;
    by = vid % a.gy; bx = vid / a.gy;                  // an XCD gets all column tiles of a band of row tiles
  }
  const int t0 = bx * TR, cout0 = by * TC;
  const int K = a.K;
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_byte*)smem;

  // per-lane source of each DMA instruction (chunk 0): row group g = i * NW + wave, row = 8 g + lane / 8, 16-byte slot lane % 8
  const _Float16* src[L];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int row = (i * NW + wave) * 8 + (lane >> 3);
    const int slot = (lane & 7) ^ ((row >> 1) & 7);
    if (row < TR) src[i] = a.x + (long long)min(t0 + row, a.M - 1) * a.ldx + slot * 8;
    else src[i] = a.w + (long long)min(cout0 + row - TR, a.N - 1) * a.ldw + slot * 8;
  }
  auto issue = [&](int c, int buf) {
#pragma unroll
    for (int i = 0; i < L; ++i) glds16(src[i] + c * 64, lds0 + buf * STAGE + (i * NW + wave) * 1024);
  };

  const int nch = K / 64;
  issue(0, 0);

  // epilogue operands: requested behind the first chunk, ahead of the others (the hand-off of chunk 0 waits for them too)
  constexpr int VW = RES ? 4 : 8;                      // channels per item: one 16-byte store
  constexpr int LDO = TC + 4, PR = TN * 32, IPR = TC / VW, NI = PR * IPR / NT;
  static_assert(NT % IPR == 0 && (PR * IPR) % NT == 0, "epilogue geometry");
  static_assert(PR * LDO * 4 <= NS * STAGE, "the epilogue tile lives in the ring");
  const int ecg = tid % IPR, ec = cout0 + VW * ecg;
  const bool col_ok = ec < a.N;                        // N % 8 == 0: a column group is whole or absent
  // loaded unconditionally from clamped addresses (masked items are never stored): a conditional load would leave the compiler
  // unsure of what is pending, and it would then wait for vmcnt(0), i.e. for the previous STORE as well, ahead of every store
  const int ecl = min(ec, a.N - VW);
  float ebias[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) ebias[j] = a.bias[ecl + j];
  h4 rv[RES ? WT * NI : 1];
  if (RES) {
#pragma unroll
    for (int q = 0; q < WT * NI; ++q) {
      const int pass = q / NI, e = q - pass * NI;
      const int t = min(t0 + pass * PR + (tid + e * NT) / IPR, a.M - 1);
      rv[q] = *(const h4*)(a.res + (long long)t * a.ldr + ecl);
    }
  }
#pragma unroll
  for (int i = 1; i <= NS - 2; ++i)
    if (i < nch) issue(i, i);

  constexpr int NA = SUM2 ? 2 : 1;
  f16v acc[NA][TM][TN];
#pragma unroll
  for (int p = 0; p < NA; ++p)
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[p][m][n][i] = 0.f;

  const int sw = (r >> 1) & 7;
  int buf = 0, nbuf = NS - 1;
  for (int c = 0; c < nch; ++c) {
    if (c + NS - 2 < nch) wait_dma_barrier<L * (NS - 2)>();
    else wait_dma_barrier<0>();
    if (c + NS - 1 < nch) issue(c + NS - 1, nbuf);     // into the buffer chunk c - 1 was multiplied from
    const unsigned char* xb = smem + buf * STAGE;
    const unsigned char* wb = xb + TR * 128;
    // fragments of k-step ks + 1 are requested ahead of the MFMAs of k-step ks
    h8 af[2][TM], bf[2][TN];
    auto frags = [&](int ks, int set) {
      const int off = ((2 * ks + h) ^ sw) * 16;
#pragma unroll
      for (int m = 0; m < TM; ++m) af[set][m] = *(const h8*)(wb + ((wn * TM + m) * 32 + r) * 128 + off);
#pragma unroll
      for (int n = 0; n < TN; ++n) bf[set][n] = *(const h8*)(xb + ((wt * TN + n) * 32 + r) * 128 + off);
    };
    frags(0, 0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks < 3) frags(ks + 1, (ks + 1) & 1);
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) mma32l(acc[SUM2 ? (ks & 1) : 0][m][n], af[ks & 1][m], bf[ks & 1][n]);   // a chunk is 4 k-steps: ks & 1 is the k-step's parity
    }
    buf = buf + 1 == NS ? 0 : buf + 1;
    nbuf = nbuf + 1 == NS ? 0 : nbuf + 1;
  }

  // every DMA has landed (the last hand-off waited for vmcnt(0)); the ring becomes the epilogue tile [PR][LDO] fp32
  // The epilogue operands are touched here, outside any branch: the compiler places its one wait for them at this point and knows
  // nothing is pending afterwards (behind the masked items' branches it would otherwise wait for vmcnt(0) ahead of every store).
#pragma unroll
  for (int j = 0; j < VW; ++j) asm volatile("" : "+v"(ebias[j]));
  if (RES) {
#pragma unroll
    for (int q = 0; q < WT * NI; ++q) asm volatile("" : "+v"(rv[q]));
  }
  float* os = (float*)smem;
#pragma unroll
  for (int pass = 0; pass < WT; ++pass) {
    lds_barrier();
    if (wt == pass) {
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          const int tl = n * 32 + r;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int cl = (wn * TM + m) * 32 + 8 * g + 4 * h;
            f4 v4;
#pragma unroll
            for (int i = 0; i < 4; ++i) v4[i] = SUM2 ? acc[0][m][n][4 * g + i] + acc[NA - 1][m][n][4 * g + i] : acc[0][m][n][4 * g + i];
            *(f4*)(os + tl * LDO + cl) = v4;
          }
        }
    }
    lds_barrier();
    // the activation is tested once per pass, not per element
    auto items = [&](auto relu_tag) {
#pragma unroll
      for (int e = 0; e < NI; ++e) {
        const int tl = (tid + e * NT) / IPR;
        const int t = t0 + pass * PR + tl;
        if (!(t < a.M && col_ok)) continue;
        float v[VW];
#pragma unroll
        for (int j4 = 0; j4 < VW / 4; ++j4) {
          const f4 av = *(const f4*)(os + tl * LDO + VW * ecg + 4 * j4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float u = av[j] + ebias[4 * j4 + j];
            if (RES) u += (float)rv[RES ? pass * NI + e : 0][j];
            u *= a.scale;
            if (decltype(relu_tag)::value) u = fmaxf(u, 0.f);
            v[4 * j4 + j] = u;
          }
        }
        const long long yoff = (long long)t * a.ldy + ec;
        if constexpr (RES) {
          *(f4*)((float*)a.y + yoff) = (f4){v[0], v[1], v[2], v[3]};
        } else {
          h8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (_Float16)v[j];
          *(h8*)((_Float16*)a.y + yoff) = o;
        }
      }
    };
    if (!RES && a.relu) items(std::true_type{});
    else items(std::false_type{});
  }
}

// The family.  id = forced `tile` of gsv_op_gemm_panel; rows x cols, waves as t x n, ring stages, LDS bytes:
//   1: 192 x 256, 2 x 4, 2 stages, 112 KB  (FFN1: N = 2048 -> 30 x 8 = 240 workgroups at M = 5760)
//   2: 192 x 192, 2 x 3, 3 stages, 144 KB  (QKV: N = 1536 -> 30 x 8 = 240)
//   3:  96 x 128, 1 x 4, 5 stages, 140 KB  (out-projection, FFN2: N = 512 -> 60 x 4 = 240)
//   4:  tile 3 with gemm_t64's two-accumulator sum (SUM2; route p2 = 1): the dispatcher's bits where it launches gemm_t64
template <int TB, int CB, int WT, int WN, int NS, bool SUM2 = false> int launch_tile(const PanelArgs& a0, bool res, hipStream_t s) {
  PanelArgs a = a0;
  const int gx = cdiv(a.M, TB * 32);
  a.gy = cdiv(a.N, CB * 32);
  const dim3 grid(gx * a.gy), block(WT * WN * 64);
  const size_t lds = (size_t)NS * (TB + CB) * 32 * 128;
  static_assert((size_t)NS * (TB + CB) * 32 * 128 <= LDS_CAP, "LDS budget");
  if (res)
    return launch_routed<gemm_panel_kernel<TB, CB, WT, WN, NS, true, SUM2>, LDS_CAP>(
        route_code(ROUTE_GEMM_PANEL, GSV_F16, TB, CB, SUM2 ? 1 : 0, 0, 0, route_flags(true, false)), grid, block, lds, s, a);
  return launch_routed<gemm_panel_kernel<TB, CB, WT, WN, NS, false, SUM2>, LDS_CAP>(
      route_code(ROUTE_GEMM_PANEL, GSV_F16, TB, CB, SUM2 ? 1 : 0, 0, 0, route_flags(false, false)), grid, block, lds, s, a);
}

}  // namespace

bool gemm_panel_eligible(int dtype, const ConvArgs& a) {
  if (dtype != GSV_F16) return false;
  if (!a.x || !a.w || !a.y || !a.bias) return false;    // all three forms carry a bias
  if (a.taps != 1 || a.stride != 1 || a.pad != 0 || a.ups_u > 0 || a.Z > 1 || a.row_seg) return false;
  if (a.gate || a.accumulate || a.pre_act != ACT_NONE || a.y_col0 != 0) return false;
  if (a.T_in < 1 || a.T_out != a.T_in || a.T_virt != a.T_in) return false;
  if (a.Cin < 64 || a.Cin % 64 != 0 || a.Cout < 8 || a.Cout % 8 != 0) return false;
  if (!operands_aligned<8>(a) || a.ldx < a.Cin || a.ldw < a.Cin || a.ldy < a.Cout) return false;
  if ((uintptr_t)a.y % 16 != 0) return false;
  if (a.res) {
    // fp32 out + bias + fp16 residual, no activation
    if (!a.out_f32 || a.res_f32 || a.post_act != ACT_NONE) return false;
    if (a.ldy % 4 != 0 || a.ldr % 4 != 0 || a.ldr < a.Cout || (uintptr_t)a.res % 8 != 0) return false;
  } else {
    // fp16 out + bias (+ ReLU)
    if (a.out_f32 || (a.post_act != ACT_NONE && a.post_act != ACT_RELU)) return false;
    if (a.ldy % 8 != 0) return false;
  }
  return true;
}

// The launcher's choice: the tile with the least rounds x tile area on 256 CUs (one workgroup per CU), the larger tile on a tie
// (fewer workgroups stage the same operands).  Where that choice needs more than one round anyway, the count of rounds says little
// (workgroups of later rounds start as CUs fall free) and the larger tiles' higher MFMA density decides: the largest tile that
// still gives every CU a workgroup.  At M = 5760 this is 192 x 192 for QKV, 192 x 256 for FFN1 and 96 x 128 for the N = 512
// layers, 240 workgroups each; at M = 23040 192 x 256 throughout (profiles/prefill_panel_probe.txt has the sweep).
int gemm_panel_auto_tile(const ConvArgs& a, int* wgs_out) {
  static const int rows[3] = {192, 192, 96}, cols[3] = {256, 192, 128};
  long long wgs[3];
  int best = -1;
  long long best_cost = 0;
  for (int i = 0; i < 3; ++i) {                        // largest tile first: a tie keeps the larger one
    wgs[i] = (long long)cdiv(a.T_in, rows[i]) * cdiv(a.Cout, cols[i]);
    const long long cost = (wgs[i] + 255) / 256 * rows[i] * cols[i];
    if (best < 0 || cost < best_cost) { best = i; best_cost = cost; }
  }
  if (wgs[best] > 256)
    for (int i = 0; i < best; ++i)
      if (wgs[i] >= 256) { best = i; break; }
  if (wgs_out) *wgs_out = (int)std::min<long long>(wgs[best], 1 << 30);
  return best + 1;
}

// Which summation launch_conv_gemm's kernel for this (eligible) descriptor performs: 0 = gemm_lds' (one accumulator), 1 = gemm_t64's
// (two), -1 = another one the panel kernel has no form of (gemm_sk's four-way split, conv_lds, conv_gemm).  It restates the
// eligibility tests of launch_gemm_sk and launch_gemm_lds, which stay as they are; tests/test_t2s_prefill_gemm_gpu.py fails if
// the two part ways.
int gemm_panel_dispatcher_sum(const ConvArgs& a) {
  const ConvSwitches& sw = conv_switches();
  const long long tiles128 = (long long)cdiv(a.T_virt, 128) * cdiv(a.Cout, 128);
  if (!sw.no_gemm_sk && a.Cin >= 256 && a.Cout >= 64 && tiles128 < sw.sk_max_tiles && a.T_virt <= 2048)
    return sw.gemm_t64 && a.Cin % 512 == 0 ? 1 : -1;
  if (!sw.no_conv_lds && a.T_virt >= 512 && a.Cout >= 96) return 0;
  return -1;
}

// 0 = launched, 1 = not eligible (the caller goes on to launch_conv_gemm), < 0 = error.  tile: 0 = by shape, 1..3 = forced, 4 = tile 3
// with gemm_t64's sum
int launch_gemm_panel(int dtype, const ConvArgs& c, int tile, hipStream_t s) {
  if (!gemm_panel_eligible(dtype, c) || tile < 0 || tile > 4) return 1;
  PanelArgs a;
  a.x = (const _Float16*)c.x; a.w = (const _Float16*)c.w; a.bias = c.bias; a.y = c.y; a.res = (const _Float16*)c.res;
  a.M = c.T_in; a.N = c.Cout; a.K = c.Cin; a.ldx = c.ldx; a.ldw = c.ldw; a.ldy = c.ldy; a.ldr = c.ldr;
  a.scale = c.scale; a.relu = c.post_act == ACT_RELU;
  a.xcd_order = conv_switches().gemm_xcd ? 1 : 0;
  a.gy = 0;
  if (tile == 0) tile = gemm_panel_auto_tile(c, nullptr);
  if (tile == 1) return launch_tile<6, 8, 2, 4, 2>(a, c.res != nullptr, s);
  if (tile == 2) return launch_tile<6, 6, 2, 3, 3>(a, c.res != nullptr, s);
  if (tile == 4) return launch_tile<3, 4, 1, 4, 5, true>(a, c.res != nullptr, s);
  return launch_tile<3, 4, 1, 4, 5>(a, c.res != nullptr, s);
}

// The panel kernel in the form that computes what launch_conv_gemm would compute for the descriptor, bit for bit; 1 = there is none
int launch_gemm_panel_as_dispatcher(int dtype, const ConvArgs& c, hipStream_t s) {
  if (!gemm_panel_eligible(dtype, c)) return 1;
  const int sum = gemm_panel_dispatcher_sum(c);
  if (sum < 0) return 1;
  return launch_gemm_panel(dtype, c, sum == 1 ? 4 : 0, s);
}

}  // namespace gsv
