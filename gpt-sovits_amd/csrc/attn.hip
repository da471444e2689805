// Fused softmax attention for the DiT blocks (H14, reference f5_tts/model/modules.py:397-457, F.scaled_dot_product_attention
// without a mask), fp16, head dim 64, gfx950.
//
// The problem is small (T ~ 1000 frames, 16 heads: 3.6 GFLOP per block) and the materialised path (scores GEMM ->
// softmax -> V transpose -> PV GEMM) spends 4 launches and a 56 MB fp32 score round trip on it, so the work is cut
// for LATENCY, not for tile reuse: one workgroup per (16 query rows, head) = 944 workgroups at T = 934, the key range
// dealt in 32-key chunks to the workgroup's 4 waves (3.7 waves per SIMD hide each other's load latency), every wave
// running an online softmax over its chunks, and one LDS combine at the end.
//
// MFMA operand trick (no LDS transpose of P): scores are computed TRANSPOSED, S^T = K Q^T with mfma_f32_16x16x32_f16
// (A = 16 keys x 32 d, B = Q^T), so a lane holds, for its query q = lane & 15, MFMA rows {4g..4g+3} of two 16-row score
// tiles (g = lane >> 4).  The K rows are loaded PERMUTED (row 4g'+i of tile a = key 8g'+i, of tile b = key 8g'+4+i), so
// those 8 values are the 8 consecutive keys 8g..8g+7 of the 32-key chunk, and they ARE a valid B operand (k-slot (g, j))
// of the second product O^T = V^T P^T whose A operand is then ONE aligned 16-byte load per d-tile from the
// pre-transposed V (vt_kernel below): fragment loads are what these kernels are bound by.  The running max / sum / rescale factors of query q then live in the lanes that
// hold O^T[.][q]: no cross-lane traffic except two xor-shuffles per reduction.
#include <stdlib.h>

#include "engine.h"

// order fence for the software pipelines: the empty asm stops IR-level sinking / hoisting of the loads across it, the
// sched_barrier stops the machine scheduler
#define GSV_PIN() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

namespace gsv {

__device__ __forceinline__ f4 mma16(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// Vt[head][d][key] = V[key][head*64 + d], keys zero padded to ldv (a multiple of 32).  The extra grid plane z == heads
// applies the DiT's rotary embedding in place to the first 2*rope_half channels of q and k (x_transformers'
// apply_rotary_pos_emb on the un-split projections, modules.py:420-427): same launch, one kernel less per block.
// Several utterances (rows of a batch) in one launch: blockIdx.z = row * planes + plane, planes = heads (+ 1 with rotary);
// row b's q / k / v start xz elements after row b-1's and its V^T buffer vtz elements after.
__global__ __launch_bounds__(256) void vt_kernel(const _Float16* __restrict__ v, int ld, int T, int ldv, _Float16* __restrict__ vt,
                                                 int heads, _Float16* __restrict__ q, int ldq, _Float16* __restrict__ k, int ldk,
                                                 const float* __restrict__ rope_cs, int rope_half, int planes, long long xz,
                                                 long long vtz) {
  const int row = blockIdx.z / planes, plane = blockIdx.z - row * planes;
  v += row * xz; q += row * xz; k += row * xz; vt += row * vtz;
  if (plane == heads) {
    const int n = T * rope_half * 2;
    const int stride = gridDim.x * gridDim.y * 256;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
      const int which = i / (T * rope_half);
      const int rr = i - which * T * rope_half;
      const int t = rr / rope_half, p = rr - t * rope_half;
      _Float16* x = (which ? k + (long long)t * ldk : q + (long long)t * ldq) + 2 * p;
      const float c = rope_cs[((long long)t * rope_half + p) * 2], sn = rope_cs[((long long)t * rope_half + p) * 2 + 1];
      const float a = (float)x[0], b = (float)x[1];
      x[0] = (_Float16)(a * c - b * sn);
      x[1] = (_Float16)(b * c + a * sn);
    }
    return;
  }
  __shared__ _Float16 tile[32][34];
  const int head = plane, j0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i;
    tile[i][tx] = j < T ? v[(long long)j * ld + head * 64 + c0 + tx] : (_Float16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + tx;
    if (j < ldv) vt[((long long)head * 64 + c0 + i) * ldv + j] = tile[tx][i];
  }
}

// QT = 16-query tiles per workgroup.  Every K / V^T fragment a wave loads feeds QT score tiles and QT output tiles:
// fragment-shaped global loads cost ~120 clocks of the CU's texture-address path each (measured),
// and with QT = 1 those loads, not MFMA or latency, set the kernel's time.
// The body both launch shapes share: q / k / out point at the first row of the sequence (a row of the batch, or a segment of a
// packed pass), vt at the first V^T column of that sequence (head 0), T is the sequence's own length.
template <int QT>
__device__ __forceinline__ void flash_attn64_tile(const _Float16* __restrict__ q, int ldq, const _Float16* __restrict__ k, int ldk,
                                                  const _Float16* __restrict__ vt, int ldv, int T, float scale,
                                                  _Float16* __restrict__ out, int ldo, int head, int q0) {
  constexpr int LDO = 68, BQ = 16 * QT;
  extern __shared__ float smem[];
  float* Os = smem;                                  // [4][BQ][LDO]
  float* Ms = smem + 4 * BQ * LDO;                   // [4][BQ]
  float* Ls = Ms + 4 * BQ;                           // [4][BQ]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  h8 qf0[QT], qf1[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const _Float16* qp = q + (long long)min(q0 + 16 * t + r, T - 1) * ldq + head * 64 + g * 8;
    qf0[t] = *(const h8*)qp;
    qf1[t] = *(const h8*)(qp + 32);
  }
  const _Float16* kh = k + head * 64 + g * 8;
  const _Float16* vh = vt + (long long)head * 64 * ldv + (long long)r * ldv + 8 * g;
  const int kra = 8 * (r >> 2) + (r & 3);           // MFMA row r of score tile a <-> key offset (tile b: + 4): see header
  f4 o[QT][4];
  float m[QT], l[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[t][d] = (f4){0.f, 0.f, 0.f, 0.f};
  }
  const int nchunks = (T + 31) >> 5;
  // Two operand sets, used alternately by a loop unrolled by two: with ONE set the prefetched registers have to be
  // copied into the loop-carried ones at the back edge, and that copy waits for vmcnt(0) -- the prefetch then hides
  // nothing (seen in the ISA: vmcnt(12) ... vmcnt(0) inside one trip).
  struct KV { h8 ka0, ka1, kb0, kb1; h8 v[4]; };
  const int lastc = nchunks - 1;
  auto fetch = [&](KV& f, int c) {
    const int key0 = c << 5;
    const _Float16* pa = kh + (long long)min(key0 + kra, T - 1) * ldk;
    const _Float16* pb = kh + (long long)min(key0 + kra + 4, T - 1) * ldk;
    f.ka0 = *(const h8*)pa; f.ka1 = *(const h8*)(pa + 32); f.kb0 = *(const h8*)pb; f.kb1 = *(const h8*)(pb + 32);
#pragma unroll
    for (int d = 0; d < 4; ++d) f.v[d] = *(const h8*)(vh + (long long)(d * 16) * ldv + key0);
  };
  auto process = [&](const KV& f, int c, bool valid) {
    const int key0 = c << 5;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      f4 sa = (f4){0.f, 0.f, 0.f, 0.f}, sb = sa;
      sa = mma16(f.ka0, qf0[t], sa); sa = mma16(f.ka1, qf1[t], sa);
      sb = mma16(f.kb0, qf0[t], sb); sb = mma16(f.kb1, qf1[t], sb);
      float p[8];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {                  // lane (q = r, g) holds the 8 CONSECUTIVE keys key0 + 8g .. + 7
        p[i] = (valid && key0 + 8 * g + i < T) ? sa[i] * scale : -INFINITY;
        p[4 + i] = (valid && key0 + 8 * g + 4 + i < T) ? sb[i] * scale : -INFINITY;
        mx = fmaxf(mx, fmaxf(p[i], p[4 + i]));
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m[t], mx);           // finite: the first chunk of a trip is always valid and has a valid key
      const float alpha = __expf(m[t] - mnew);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { p[i] = __expf(p[i] - mnew); ps += p[i]; }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l[t] = l[t] * alpha + ps;
      m[t] = mnew;
      const h8 pf = (h8){(_Float16)p[0], (_Float16)p[1], (_Float16)p[2], (_Float16)p[3], (_Float16)p[4], (_Float16)p[5], (_Float16)p[6], (_Float16)p[7]};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        o[t][d] *= alpha;
        o[t][d] = mma16(f.v[d], pf, o[t][d]);       // O^T[d*16 + 4g + i][q = 16t + r]
      }
    }
  };
  KV fA, fB;
  fetch(fA, min(wave, lastc));                    // loads are unconditional (index clamped): see gemm_sk.hip
  for (int c = wave; c < nchunks; c += 8) {
    fetch(fB, min(c + 4, lastc));
    GSV_PIN();
    process(fA, c, true);
    GSV_PIN();
    fetch(fA, min(c + 8, lastc));
    GSV_PIN();
    process(fB, c + 4, c + 4 < nchunks);         // unconditional (fully masked past the end): a conditional block lets
                                                 // the compiler sink fB's loads into it, behind process(fA)
    GSV_PIN();
  }
  // ---- combine the 4 waves' partial (m, l, O)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
#pragma unroll
    for (int d = 0; d < 4; ++d) *(f4*)&Os[((size_t)wave * BQ + 16 * t + r) * LDO + d * 16 + 4 * g] = o[t][d];
    if (g == 0) { Ms[wave * BQ + 16 * t + r] = m[t]; Ls[wave * BQ + 16 * t + r] = l[t]; }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qq = 16 * t + (threadIdx.x >> 4), d4 = (threadIdx.x & 15) * 4;
    const float mt = fmaxf(fmaxf(Ms[qq], Ms[BQ + qq]), fmaxf(Ms[2 * BQ + qq], Ms[3 * BQ + qq]));
    float den = 0.f;
    f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float e = __expf(Ms[w * BQ + qq] - mt); // exp(-inf) = 0 for a wave that saw no chunk
      den += e * Ls[w * BQ + qq];
      acc += *(const f4*)&Os[((size_t)w * BQ + qq) * LDO + d4] * e;
    }
    if (q0 + qq < T) {
      const float inv = 1.f / den;
      *(h4*)(out + (long long)(q0 + qq) * ldo + head * 64 + d4) =
          (h4){(_Float16)(acc[0] * inv), (_Float16)(acc[1] * inv), (_Float16)(acc[2] * inv), (_Float16)(acc[3] * inv)};
    }
  }
}

// Several utterances in one launch: gridDim.y = rows * heads.  Row b's q / k start xz elements after row b-1's, its V^T vtz
// and its output oz elements after.
template <int QT>
__global__ __launch_bounds__(256) void flash_attn64_f16_kernel(const _Float16* __restrict__ q, int ldq, const _Float16* __restrict__ k,
                                                               int ldk, const _Float16* __restrict__ vt, int ldv, int T, float scale,
                                                               _Float16* __restrict__ out, int ldo, int heads, long long xz,
                                                               long long vtz, long long oz) {
  // (row, head) pairs are dealt to XCDs in contiguous runs (2 heads per XCD at 16 heads and one row, 2 * rows with more):
  // all query tiles of a pair run on one XCD, so its K / V^T stay in one L2.  The pair is the slow index of the virtual id,
  // so an XCD works through its pairs one after the other and holds only the few in flight.
  const int vid = xcd_virtual_id(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int pair = vid / gridDim.x, q0 = (vid % gridDim.x) * (16 * QT);
  const int row = pair / heads, head = pair - row * heads;
  flash_attn64_tile<QT>(q + row * xz, ldq, k + row * xz, ldk, vt + row * vtz, ldv, T, scale, out + row * oz, ldo, head, q0);
}

template <int QT>
static int launch_flash_qt(const void* q, int ldq, const void* k, int ldk, const void* vt_buf, int ldv, int T, int heads, float scale,
                           void* out, int ldo, hipStream_t s, int rows, long long xz, long long vtz, long long oz) {
  const size_t lds = ((size_t)4 * 16 * QT * 68 + 8 * 16 * QT) * 4;
  static bool attr = false;
  if (!attr) {
    GSV_HIP(hipFuncSetAttribute((const void*)flash_attn64_f16_kernel<QT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL(flash_attn64_f16_kernel<QT>, dim3(cdiv(T, 16 * QT), rows * heads), dim3(256), lds, s, (const _Float16*)q, ldq,
                     (const _Float16*)k, ldk, (const _Float16*)vt_buf, ldv, T, scale, (_Float16*)out, ldo, heads, xz, vtz, oz);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

// ---------------------------------------------------------------------------------------
// Segmented (variable-length) form: n_seg sequences back to back in one [sum T][ld] matrix (the packed BERT pass,
// gsv/feature_extractor/bert.py), query i of segment s attends to the keys of segment s only.  The segment takes the place of
// the row above: a query tile never spans two segments (tiles are counted per segment, so every segment ends in a partial
// tile), and a workgroup finds its segment in the table by the tile prefix.  Table, one int4 per segment:
//   x = first row of the segment in the packed matrix      y = its length T_s
//   z = its first V^T column, 32 * sum_{s' < s} ceil(T_s' / 32): every segment starts on a 32-key boundary, so the aligned
//       16-byte V^T loads of the tile body stay aligned and a chunk never reads another segment's columns
//   w = query tiles of the segments before it
// The last segment whose prefix is <= x (binary search; wave-uniform, so the loads are scalar).
__device__ __forceinline__ int4 seg_find(const int4* __restrict__ tab, int n_seg, int x, bool by_tile) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const int4 e = tab[mid];
    if ((by_tile ? e.w : e.z) <= x) lo = mid; else hi = mid - 1;
  }
  return tab[lo];
}

// Vt[head][d][z_s + j] = V[x_s + j][head * 64 + d] for j < T_s and 0 for T_s <= j < 32 * ceil(T_s / 32): the padding columns are
// WRITTEN, the scratch buffer arrives uninitialised and a masked probability of 0 times a NaN left there is NaN.
// grid: (ldv / 32 key chunks, 2 halves of the head's 64 channels, heads); a 32-column chunk lies in one segment.
__global__ __launch_bounds__(256) void vt_seg_kernel(const _Float16* __restrict__ v, int ld, const int4* __restrict__ tab, int n_seg,
                                                     int ldv, _Float16* __restrict__ vt) {
  __shared__ _Float16 tile[32][34];
  const int head = blockIdx.z, j0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int4 sg = seg_find(tab, n_seg, j0, false);
  const int k0 = j0 - sg.z;                         // first key of this chunk inside its segment
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = k0 + i;
    tile[i][tx] = j < sg.y ? v[(long long)(sg.x + j) * ld + head * 64 + c0 + tx] : (_Float16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) vt[((long long)head * 64 + c0 + i) * ldv + j0 + tx] = tile[tx][i];
}

// grid: (query tiles of all segments, heads).  A head's tiles are a contiguous run of virtual ids, as a (row, head) pair's above.
template <int QT>
__global__ __launch_bounds__(256) void flash_attn64_seg_f16_kernel(const _Float16* __restrict__ q, int ldq, const _Float16* __restrict__ k,
                                                                   int ldk, const _Float16* __restrict__ vt, int ldv,
                                                                   const int4* __restrict__ tab, int n_seg, float scale,
                                                                   _Float16* __restrict__ out, int ldo) {
  const int vid = xcd_virtual_id(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int head = vid / gridDim.x, tile = vid % gridDim.x;
  const int4 sg = seg_find(tab, n_seg, tile, true);
  flash_attn64_tile<QT>(q + (long long)sg.x * ldq, ldq, k + (long long)sg.x * ldk, ldk, vt + sg.z, ldv, sg.y, scale,
                        out + (long long)sg.x * ldo, ldo, head, (tile - sg.w) * (16 * QT));
}

template <int QT>
static int launch_flash_seg_qt(const void* q, int ldq, const void* k, int ldk, const void* vt_buf, int ldv, const int4* tab, int n_seg,
                               int tiles, int heads, float scale, void* out, int ldo, hipStream_t s) {
  const size_t lds = ((size_t)4 * 16 * QT * 68 + 8 * 16 * QT) * 4;
  static bool attr = false;
  if (!attr) {
    GSV_HIP(hipFuncSetAttribute((const void*)flash_attn64_seg_f16_kernel<QT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  GSV_LAUNCH(flash_attn64_seg_f16_kernel<QT>, dim3(tiles, heads), dim3(256), lds, s, (const _Float16*)q, ldq, (const _Float16*)k, ldk,
             (const _Float16*)vt_buf, ldv, tab, n_seg, scale, (_Float16*)out, ldo);
  return GSV_OK;
}

// ---------------------------------------------------------------------------------------
// enc_p self-attention with window-4 relative positions (H10, reference module/attentions.py:227-258), fp16, head dim 96:
// the same transposed-score construction; the relative-key bias b[i][r] = (q_i / sqrt(d)) . rel_k[r] is added to the
// scores of the 9 keys |j - i| <= 4 (only the 2-3 chunks that straddle the diagonal take that path), their biased LOGITS
// are parked in LDS (logits need no online rescaling), and the epilogue turns them into the band probabilities that
// weight rel_v (attentions.py:253-256).  Replaces scores GEMM -> softmax_rows -> V transpose -> PV GEMM -> relv_add and
// their 2 x T^2 x 6 bytes of HBM round trips (T = 6400 folded frames at the benchmark shape).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt96_kernel(const _Float16* __restrict__ v, int ld, int T, int ldv, _Float16* __restrict__ vt) {
  __shared__ _Float16 tile[32][34];
  const int head = blockIdx.z, j0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i;
    tile[i][tx] = j < T ? v[(long long)j * ld + head * 96 + c0 + tx] : (_Float16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + tx;
    if (j < ldv) vt[((long long)head * 96 + c0 + i) * ldv + j] = tile[tx][i];
  }
}

template <int QT>
__global__ __launch_bounds__(256) void flash_rel96_f16_kernel(const _Float16* __restrict__ q, int ldq, const _Float16* __restrict__ k,
                                                              int ldk, const _Float16* __restrict__ vt, int ldv, int T, float scale,
                                                              const float* __restrict__ rel_k, const float* __restrict__ rel_v,
                                                              _Float16* __restrict__ out, int ldo, const int* __restrict__ kr) {
  constexpr int D = 96, KS = 3, DT = 6, W = 4, NB = 9, LDO = 100, BQ = 16 * QT;
  extern __shared__ float smem[];
  float* Os = smem;                                  // [4][BQ][LDO]
  float* Ms = Os + 4 * BQ * LDO;                     // [4][BQ]
  float* Ls = Ms + 4 * BQ;                           // [4][BQ]
  float* Bias = Ls + 4 * BQ;                         // [BQ][NB]   relative-key bias per query
  float* Sb = Bias + BQ * NB;                        // [BQ][NB]   biased logits of the band keys (-inf outside [0, T))
  const int vid = xcd_virtual_id(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int head = vid / gridDim.x, q0 = (vid % gridDim.x) * BQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  h8 qf[QT][KS];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const _Float16* qp = q + (long long)min(q0 + 16 * t + r, T - 1) * ldq + head * D + g * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[t][ks] = *(const h8*)(qp + 32 * ks);
  }
  // relative-key bias: wave w computes the tiles t = w, w + 4, ...; each lane dots its 24 channels, the 4 lanes of a query sum
  for (int i = threadIdx.x; i < BQ * NB; i += 256) Sb[i] = -INFINITY;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    if ((t & 3) != wave) continue;
#pragma unroll
    for (int rr = 0; rr < NB; ++rr) {
      float sdot = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) sdot += (float)qf[t][ks][e] * rel_k[rr * D + ks * 32 + g * 8 + e];
      sdot += __shfl_xor(sdot, 16, 64);
      sdot += __shfl_xor(sdot, 32, 64);
      if (g == 0) Bias[(16 * t + r) * NB + rr] = sdot * scale;
    }
  }
  __syncthreads();
  const _Float16* kh = k + head * D + g * 8;
  const _Float16* vh = vt + (long long)head * D * ldv + (long long)r * ldv + 8 * g;
  const int kra = 8 * (r >> 2) + (r & 3);
  f4 o[QT][DT];
  float m[QT], l[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
    for (int d = 0; d < DT; ++d) o[t][d] = (f4){0.f, 0.f, 0.f, 0.f};
  }
  // segmented decode (kr != null): query row i sees keys [kr[2i], kr[2i+1]) only.  The host builds non-decreasing ranges, so the
  // workgroup's keys are [lo of its first row, hi of its last row) and the chunks outside it are skipped, not masked.
  int klo[QT], khi[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qi = min(q0 + 16 * t + r, T - 1);
    klo[t] = kr ? kr[2 * qi] : 0;
    khi[t] = kr ? kr[2 * qi + 1] : T;
  }
  const int c0 = kr ? kr[2 * q0] >> 5 : 0;
  const int nchunks = kr ? (kr[2 * min(q0 + BQ - 1, T - 1) + 1] + 31) >> 5 : (T + 31) >> 5, lastc = nchunks - 1;
  struct KV { h8 ka[KS], kb[KS]; h8 v[DT]; };
  auto fetch = [&](KV& f, int c) {
    const int key0 = c << 5;
    const _Float16* pa = kh + (long long)min(key0 + kra, T - 1) * ldk;
    const _Float16* pb = kh + (long long)min(key0 + kra + 4, T - 1) * ldk;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { f.ka[ks] = *(const h8*)(pa + 32 * ks); f.kb[ks] = *(const h8*)(pb + 32 * ks); }
#pragma unroll
    for (int d = 0; d < DT; ++d) f.v[d] = *(const h8*)(vh + (long long)(d * 16) * ldv + key0);
  };
  auto process = [&](const KV& f, int c, bool valid) {
    const int key0 = c << 5;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      f4 sa = (f4){0.f, 0.f, 0.f, 0.f}, sb = sa;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { sa = mma16(f.ka[ks], qf[t][ks], sa); sb = mma16(f.kb[ks], qf[t][ks], sb); }
      float p[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ja = key0 + 8 * g + i, jb = ja + 4;
        p[i] = (valid && ja >= klo[t] && ja < khi[t]) ? sa[i] * scale : -INFINITY;
        p[4 + i] = (valid && jb >= klo[t] && jb < khi[t]) ? sb[i] * scale : -INFINITY;
      }
      const int qt0 = q0 + 16 * t;
      if (valid && key0 + 31 >= qt0 - W && key0 <= qt0 + 15 + W) {      // wave-uniform: this chunk touches the diagonal band
        const int qi = qt0 + r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int j = key0 + 8 * g + i;
          const int rp = j - qi + W;
          if (rp >= 0 && rp < NB && j >= klo[t] && j < khi[t] && qi < T) {
            p[i] += Bias[(16 * t + r) * NB + rp];
            Sb[(16 * t + r) * NB + rp] = p[i];
          }
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 8; ++i) mx = fmaxf(mx, p[i]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // a segmented row may meet a chunk with none of its keys before any of them: keep exp(-inf - -inf) out of m / l / o
      const float mnew = fmaxf(m[t], mx), msafe = mnew == -INFINITY ? 0.f : mnew;
      const float alpha = __expf(m[t] - msafe);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { p[i] = __expf(p[i] - msafe); ps += p[i]; }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l[t] = l[t] * alpha + ps;
      m[t] = mnew;
      const h8 pf = (h8){(_Float16)p[0], (_Float16)p[1], (_Float16)p[2], (_Float16)p[3], (_Float16)p[4], (_Float16)p[5], (_Float16)p[6], (_Float16)p[7]};
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        o[t][d] *= alpha;
        o[t][d] = mma16(f.v[d], pf, o[t][d]);
      }
    }
  };
  KV fA, fB;
  fetch(fA, min(c0 + wave, lastc));
  for (int c = c0 + wave; c < nchunks; c += 8) {
    fetch(fB, min(c + 4, lastc));
    GSV_PIN();
    process(fA, c, true);
    GSV_PIN();
    fetch(fA, min(c + 8, lastc));
    GSV_PIN();
    process(fB, c + 4, c + 4 < nchunks);
    GSV_PIN();
  }
#pragma unroll
  for (int t = 0; t < QT; ++t) {
#pragma unroll
    for (int d = 0; d < DT; ++d) *(f4*)&Os[((size_t)wave * BQ + 16 * t + r) * LDO + d * 16 + 4 * g] = o[t][d];
    if (g == 0) { Ms[wave * BQ + 16 * t + r] = m[t]; Ls[wave * BQ + 16 * t + r] = l[t]; }
  }
  __syncthreads();
  for (int it = threadIdx.x; it < BQ * (D / 4); it += 256) {
    const int qq = it / (D / 4), d4 = (it % (D / 4)) * 4;
    if (q0 + qq >= T) continue;
    const float mt = fmaxf(fmaxf(Ms[qq], Ms[BQ + qq]), fmaxf(Ms[2 * BQ + qq], Ms[3 * BQ + qq]));
    float den = 0.f;
    f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float e = __expf(Ms[w * BQ + qq] - mt);
      den += e * Ls[w * BQ + qq];
      acc += *(const f4*)&Os[((size_t)w * BQ + qq) * LDO + d4] * e;
    }
#pragma unroll
    for (int rr = 0; rr < NB; ++rr) {
      const float pw = __expf(Sb[qq * NB + rr] - mt);                   // band probability * den; exp(-inf) = 0 outside [0, T)
      const f4 rv = *(const f4*)(rel_v + rr * D + d4);
      acc += rv * pw;
    }
    const float inv = 1.f / den;
    *(h4*)(out + (long long)(q0 + qq) * ldo + head * D + d4) =
        (h4){(_Float16)(acc[0] * inv), (_Float16)(acc[1] * inv), (_Float16)(acc[2] * inv), (_Float16)(acc[3] * inv)};
  }
}

// self-attention with relative positions (window 4), fp16, head dim 96; vt_buf: heads * 96 * ceil32(T) halfs of scratch
int launch_flash_rel96_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldvv, void* vt_buf, int T, int heads,
                           float scale, const float* rel_k, const float* rel_v, void* out, int ldo, hipStream_t s, const int* kr) {
  GSV_REQUIRE(T >= 1 && heads >= 1 && rel_k && rel_v, "flash_rel96: bad argument");
  GSV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldo % 4 == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)out % 8) == 0 &&
              ((uintptr_t)rel_v % 16) == 0, "flash_rel96: operands must be 16-byte aligned with leading dims multiple of 8");
  const int ldv = (T + 31) / 32 * 32;
  hipLaunchKernelGGL(vt96_kernel, dim3(ldv / 32, 3, heads), dim3(256), 0, s, (const _Float16*)v, ldvv, T, ldv, (_Float16*)vt_buf);
  constexpr int QT = 2;
  set_attn_route(ATTN_REL96, QT);
  const size_t lds = ((size_t)4 * 16 * QT * 100 + 8 * 16 * QT + 2 * 16 * QT * 9) * 4;
  static bool attr = false;
  if (!attr) {
    GSV_HIP(hipFuncSetAttribute((const void*)flash_rel96_f16_kernel<QT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL(flash_rel96_f16_kernel<QT>, dim3(cdiv(T, 16 * QT), heads), dim3(256), lds, s, (const _Float16*)q, ldq,
                     (const _Float16*)k, ldk, (const _Float16*)vt_buf, ldv, T, scale, rel_k, rel_v, (_Float16*)out, ldo, kr);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

// `rows` utterances of T frames in two launches.  q / k: [T][ld] with head h at columns h*64..; v likewise; row b of q, k and v
// starts xz elements after row b-1, of out oz elements after; vt_buf: rows * vtz halfs of scratch, vtz >= heads * 64 * ceil32(T)
int launch_flash_attn64_f16_rows(const void* q, int ldq, const void* k, int ldk, const void* v, int ldvv, void* vt_buf, int T, int heads,
                                 float scale, void* out, int ldo, hipStream_t s, const float* rope_cs, int rope_half, int rows,
                                 long long xz, long long vtz, long long oz, int qt_arg) {
  GSV_REQUIRE(T >= 1 && heads >= 1 && rows >= 1, "flash_attn: empty problem");
  GSV_REQUIRE(qt_arg == 0 || qt_arg == 1 || qt_arg == 2 || qt_arg == 4, "flash_attn: qt %d is not 0 (by shape), 1, 2 or 4", qt_arg);
  GSV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldo % 4 == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)out % 8) == 0,
              "flash_attn: operands must be 16-byte aligned with leading dims multiple of 8");
  const int ldv = (T + 31) / 32 * 32;
  const int planes = heads + (rope_cs ? 1 : 0);
  GSV_REQUIRE(rows == 1 || (xz % 8 == 0 && vtz % 8 == 0 && oz % 4 == 0 && vtz >= (long long)heads * 64 * ldv),
              "flash_attn: row strides must keep every row 16-byte aligned and its V^T buffer apart");
  GSV_REQUIRE((long long)rows * planes <= 65535 && (long long)rows * heads <= 65535, "flash_attn: %d rows x %d heads exceed the grid", rows, heads);
  hipLaunchKernelGGL(vt_kernel, dim3(ldv / 32, 2, rows * planes), dim3(256), 0, s, (const _Float16*)v, ldvv, T, ldv, (_Float16*)vt_buf, heads,
                     (_Float16*)const_cast<void*>(q), ldq, (_Float16*)const_cast<void*>(k), ldk, rope_cs, rope_half, planes, xz, vtz);
  static const int qt_env = getenv("GSV_FLASH_QT") ? atoi(getenv("GSV_FLASH_QT")) : 0;     // A/B switch
  // more query tiles per workgroup = fewer K / V fragment loads per query, but fewer workgroups: keep >= ~1 per CU.  Chosen
  // from ONE row's size whatever `rows` is, so that a row computes the same bits alone and in a batch.
  // qt_arg (test hooks): one instantiation, whatever the rule and the switch say
  int qt = qt_arg ? qt_arg : qt_env ? qt_env : ((long long)cdiv(T, 64) * heads >= 200 ? 4 : ((long long)cdiv(T, 32) * heads >= 200 ? 2 : 1));
  set_attn_route(ATTN_ROWS, qt >= 4 ? 4 : qt >= 2 ? 2 : 1);
  if (qt >= 4) return launch_flash_qt<4>(q, ldq, k, ldk, vt_buf, ldv, T, heads, scale, out, ldo, s, rows, xz, vtz, oz);
  if (qt >= 2) return launch_flash_qt<2>(q, ldq, k, ldk, vt_buf, ldv, T, heads, scale, out, ldo, s, rows, xz, vtz, oz);
  return launch_flash_qt<1>(q, ldq, k, ldk, vt_buf, ldv, T, heads, scale, out, ldo, s, rows, xz, vtz, oz);
}

int launch_flash_attn64_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldvv, void* vt_buf, int T, int heads,
                            float scale, void* out, int ldo, hipStream_t s, const float* rope_cs, int rope_half) {
  return launch_flash_attn64_f16_rows(q, ldq, k, ldk, v, ldvv, vt_buf, T, heads, scale, out, ldo, s, rope_cs, rope_half, 1, 0, 0, 0);
}

// n_seg sequences of seg_lens[s] rows back to back in q / k / v / out, two launches for all of them (vt_seg_kernel, then the
// segmented kernel); vt_buf: heads * 64 * 32 * sum ceil(T_s / 32) halfs of scratch.  The segment table goes to the device through
// the library context's staging slots (engine.h): one small async copy on `s`, none when `s` already carries the same table.
int launch_flash_attn64_f16_seg(const void* q, int ldq, const void* k, int ldk, const void* v, int ldvv, void* vt_buf, int n_seg,
                                const int* seg_lens, int heads, float scale, void* out, int ldo, hipStream_t s, int qt_arg) {
  GSV_REQUIRE(q && k && v && vt_buf && out && seg_lens, "flash_attn_seg: null argument");
  GSV_REQUIRE(qt_arg == 0 || qt_arg == 1 || qt_arg == 2 || qt_arg == 4, "flash_attn_seg: qt %d is not 0 (by shape), 1, 2 or 4", qt_arg);
  GSV_REQUIRE(n_seg >= 1 && heads >= 1 && heads <= 65535, "flash_attn_seg: %d segments, %d heads", n_seg, heads);
  GSV_REQUIRE(n_seg <= gsveng::kSegTableMax, "flash_attn_seg: %d segments exceed the table's %d", n_seg, gsveng::kSegTableMax);
  GSV_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldo % 4 == 0 && ((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)out % 8) == 0 &&
              ((uintptr_t)vt_buf % 16) == 0, "flash_attn_seg: operands must be 16-byte aligned with leading dims multiple of 8");
  long long rows = 0, t32 = 0, t64 = 0;
  for (int i = 0; i < n_seg; ++i) {
    GSV_REQUIRE(seg_lens[i] >= 1, "flash_attn_seg: segment %d has length %d", i, seg_lens[i]);
    rows += seg_lens[i]; t32 += cdiv(seg_lens[i], 32); t64 += cdiv(seg_lens[i], 64);
  }
  GSV_REQUIRE(rows + 32LL * n_seg <= 0x7fffffffLL, "flash_attn_seg: %lld rows exceed the index range", rows);
  static const int qt_env = getenv("GSV_FLASH_QT") ? atoi(getenv("GSV_FLASH_QT")) : 0;     // A/B switch, as for the rows
  // the row kernel's rule on the packed problem: keep >= ~1 workgroup per CU.  Tiles are counted per segment, so the counts are sums.
  const int qt = qt_arg ? qt_arg : qt_env ? (qt_env >= 4 ? 4 : qt_env >= 2 ? 2 : 1) : (t64 * heads >= 200 ? 4 : (t32 * heads >= 200 ? 2 : 1));
  gsveng::SegTable tb;                              // holds the library context until it goes out of scope
  GSV_RC(gsveng::seg_table_begin(&tb));
  long long row0 = 0, col0 = 0, tile0 = 0;
  for (int i = 0; i < n_seg; ++i) {
    tb.image[4 * i] = (int)row0; tb.image[4 * i + 1] = seg_lens[i]; tb.image[4 * i + 2] = (int)col0; tb.image[4 * i + 3] = (int)tile0;
    row0 += seg_lens[i]; col0 += 32 * cdiv(seg_lens[i], 32); tile0 += cdiv(seg_lens[i], 16 * qt);
  }
  const int ldv = (int)col0, tiles = (int)tile0;
  // both grids (x = tiles or chunks, <= rows) and the virtual workgroup id tiles * heads have to fit an int
  GSV_REQUIRE(tile0 * heads <= 0x7fffffffLL, "flash_attn_seg: %lld query tiles x %d heads exceed the grid", tile0, heads);
  GSV_RC(gsveng::seg_table_upload(&tb, n_seg, s));
  const int4* tab = (const int4*)tb.dev;
  GSV_LAUNCH(vt_seg_kernel, dim3(ldv / 32, 2, heads), dim3(256), 0, s, (const _Float16*)v, ldvv, tab, n_seg, ldv, (_Float16*)vt_buf);
  set_attn_route(ATTN_SEG, qt);
  int rc;
  if (qt == 4) rc = launch_flash_seg_qt<4>(q, ldq, k, ldk, vt_buf, ldv, tab, n_seg, tiles, heads, scale, out, ldo, s);
  else if (qt == 2) rc = launch_flash_seg_qt<2>(q, ldq, k, ldk, vt_buf, ldv, tab, n_seg, tiles, heads, scale, out, ldo, s);
  else rc = launch_flash_seg_qt<1>(q, ldq, k, ldk, vt_buf, ldv, tab, n_seg, tiles, heads, scale, out, ldo, s);
  GSV_RC(rc);
  return gsveng::seg_table_end(&tb, s);
}

}  // namespace gsv
