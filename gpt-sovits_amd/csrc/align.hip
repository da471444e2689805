// Monotonic alignment of a text-to-frame attention (gsv_op_align*, gsv_vits_set_align): the head-averaged log-probabilities of
// q k^T over rectangles ("spans") of the two operands, and VITS' maximum_path (Viterbi over monotonic paths) on them.
//
// A call carries n spans in a device table.  Span i's workspace region starts at the sum of the regions in front of it
// (align_span_words): nf * nl fp32 log-probabilities, rounded up to 4 words, then the decision bits of the search where they do
// not fit the LDS.  Every kernel derives the offset from the table itself, so the host needs no copy of a device table and a
// span computes the same bits whatever else the call holds.
#include "align.h"

#include <math.h>

#include <algorithm>
#include <cmath>

#include "mfma_frag.h"

namespace gsv {

// bits per lane and row of the search: P = ceil(nl / 64) phonemes per lane, in a field of 1, 4 or 16 bits
__host__ __device__ inline int align_field(int nl) {
  const int P = (nl + 63) / 64;
  return P <= 1 ? 1 : P <= 4 ? 4 : 16;
}
__host__ __device__ inline bool align_searched(int nf, int nl) { return nf >= 1 && nl >= 1 && nf >= nl && nl <= ALIGN_MAX_PHONES; }
// decision words (uint32) of a span: 64-row blocks of 2 W words per lane
__host__ __device__ inline long long align_dec_words(int nf, int nl) {
  return (long long)((nf + 63) / 64) * 2 * align_field(nl) * 64;
}
__host__ __device__ inline bool align_dec_in_lds(int nf, int nl) { return align_dec_words(nf, nl) <= ALIGN_LDS_WORDS; }
__host__ __device__ inline long long align_lp_words(int nf, int nl) { return ((long long)nf * nl + 3) & ~3LL; }
__host__ __device__ inline long long align_span_words_hd(int nf, int nl) {
  if (!align_searched(nf, nl)) return 0;
  return align_lp_words(nf, nl) + (align_dec_in_lds(nf, nl) ? 0 : align_dec_words(nf, nl));
}
long long align_span_words(int nf, int nl) { return align_span_words_hd(nf, nl); }

// word offset of span `i`'s region: every thread of the block calls it (one barrier pair), all get the sum
template <int NT> __device__ long long align_span_offset(const gsv_align_span_t* __restrict__ tab, int i, long long* sh) {
  long long a = 0;
  for (int k = threadIdx.x; k < i; k += NT) a += align_span_words_hd(tab[k].nf, tab[k].nl);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (NT == 64) return a;
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  long long t = 0;
  for (int w = 0; w < NT / 64; ++w) t += sh[w];
  __syncthreads();
  return t;
}

// ---------------------------------------------------------------------------------------
// log-probabilities.  grid = (ALIGN_LP_BLOCKS, n), block = 256: block (b, i) takes the 32-frame tiles b, b + 8, ... of span i; in a
// tile, wave w takes the 32-phoneme chunks w, w + 4, ...  One (tile, chunk, head) is a 32 x 32 MFMA accumulator over head_dim:
// the lane holds one phoneme column and 16 frame rows of it.  Three passes recompute the scores (the flops are nothing): the
// per-head row maximum, the per-head row sum of expf(s - max), and the emit.
// ---------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ f16v align_scores(const T* __restrict__ qrow, const T* __restrict__ krow, int hd, int hh) {
  constexpr int G = DT<T>::G;
  typedef typename FragL<T>::type F;
  f16v acc = zfrag<f16v>();
  for (int kk = hh * G; kk < hd; kk += 2 * G) {
    const F a = *reinterpret_cast<const F*>(qrow + kk), b = *reinterpret_cast<const F*>(krow + kk);
    mma32l(acc, a, b);
  }
  return acc;
}
__device__ __forceinline__ int align_acc_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

template <typename T>
__global__ __launch_bounds__(256) void align_logp_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k, int ldk, int heads,
                                                         int hd, float scale, const gsv_align_span_t* __restrict__ tab,
                                                         float* __restrict__ ws, long long ws_words) {
  __shared__ long long sh_off[4];
  __shared__ float red[4][ALIGN_MAX_HEADS][32];   // per wave partial maxima, then partial sums
  __shared__ float row_m[ALIGN_MAX_HEADS][32], row_s[ALIGN_MAX_HEADS][32];
  const int si = blockIdx.y;
  const long long off = align_span_offset<256>(tab, si, sh_off);
  const gsv_align_span_t sp = tab[si];
  const int nf = sp.nf, nl = sp.nl;
  if (!align_searched(nf, nl) || off + align_span_words_hd(nf, nl) > ws_words) return;   // the path kernel takes the fallback
  float* __restrict__ lp = ws + off;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  const int n_chunk = (nl + 31) / 32, n_tile = (nf + 31) / 32;
  const float inv_h = 1.f / (float)heads;
  for (int tile = blockIdx.x; tile < n_tile; tile += ALIGN_LP_BLOCKS) {
    const int t0 = tile * 32;
    // rows past the span read its last row (in bounds); what they compute is dropped
    const T* __restrict__ qrow = q + (size_t)(sp.f0 + min(t0 + r, nf - 1)) * ldq;
    for (int pass = 0; pass < 2; ++pass) {
      for (int h = 0; h < heads; ++h) {
        float part[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) part[i] = pass == 0 ? -INFINITY : 0.f;
        for (int c = wave; c < n_chunk; c += 4) {
          const int j = c * 32 + r;
          const T* __restrict__ krow = k + (size_t)(sp.l0 + min(j, nl - 1)) * ldk;
          const f16v acc = align_scores<T>(qrow + h * hd, krow + h * hd, hd, hh);
          if (j < nl) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const float s = acc[i] * scale;
              if (pass == 0) part[i] = fmaxf(part[i], s);
              else part[i] += expf(s - row_m[h][align_acc_row(i, hh)]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float v = part[i];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) {
            const float u = __shfl_xor(v, o, 64);
            v = pass == 0 ? fmaxf(v, u) : v + u;
          }
          if (r == 0) red[wave][h][align_acc_row(i, hh)] = v;
        }
      }
      __syncthreads();
      for (int e = threadIdx.x; e < heads * 32; e += 256) {
        const int h = e >> 5, row = e & 31;
        if (pass == 0) row_m[h][row] = fmaxf(fmaxf(red[0][h][row], red[1][h][row]), fmaxf(red[2][h][row], red[3][h][row]));
        else row_s[h][row] = (red[0][h][row] + red[1][h][row]) + (red[2][h][row] + red[3][h][row]);
      }
      __syncthreads();
    }
    for (int c = wave; c < n_chunk; c += 4) {
      const int j = c * 32 + r;
      const T* __restrict__ krow = k + (size_t)(sp.l0 + min(j, nl - 1)) * ldk;
      float p[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) p[i] = 0.f;
      for (int h = 0; h < heads; ++h) {
        const f16v acc = align_scores<T>(qrow + h * hd, krow + h * hd, hd, hh);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = align_acc_row(i, hh);
          p[i] += expf(acc[i] * scale - row_m[h][row]) / row_s[h][row];
        }
      }
      if (j < nl) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = t0 + align_acc_row(i, hh);
          if (t < nf) lp[(size_t)t * nl + j] = logf(fmaxf(1e-30f, p[i] * inv_h));
        }
      }
    }
    __syncthreads();   // row_m / row_s are rewritten by the next tile
  }
}

// ---------------------------------------------------------------------------------------
// search and backtrack.  grid = n, block = 64: one wave per span, no barrier.  Lane l owns phonemes l P .. l P + P - 1 and keeps
// their V in fp64: one IEEE add and one compare per cell, so the path is exactly optimal for the fp32 lp it reads and a float64
// mirror is bit-equal.  Decision bit (t, j) = "came from j - 1" = V[t-1][j] < V[t-1][j-1] (a tie stays).  A lane packs its W-bit
// row fields into uint32 words over 32 / W rows before it stores them; a 64-row block is 2 W words per lane, word u of block b
// at [(b * 2 W + u) * 64 + lane], so the backtrack loads a block in one access per lane and walks its 64 rows in registers,
// reading the owner lane's word with v_readlane (the walker's position is wave-uniform).
// ---------------------------------------------------------------------------------------
template <int W>
__device__ void align_path_span(const float* __restrict__ lp, int nf, int nl, uint32_t* __restrict__ gdec, uint32_t* sdec, bool in_lds,
                                int32_t* __restrict__ ends, float* __restrict__ score, int lane) {
  constexpr int R = 32 / W, D = W == 16 ? 2 : 4;   // rows per word; rows loaded ahead
  const int P = (nl + 63) / 64, j0 = lane * P;
  double V[W];
  float x[D][W];
  auto load_row = [&](int t, float* dst) {
#pragma unroll
    for (int p = 0; p < W; ++p) dst[p] = (t < nf && p < P && j0 + p < nl) ? lp[(size_t)t * nl + j0 + p] : 0.f;
  };
  load_row(0, x[0]);
#pragma unroll
  for (int p = 0; p < W; ++p) V[p] = (j0 + p == 0) ? (double)x[0][p] : -INFINITY;
#pragma unroll
  for (int d = 0; d < D; ++d) load_row(1 + d, x[d]);
  uint32_t word = 0;
  for (int tb = 1; tb < nf; tb += D) {
    float xn[D][W];
#pragma unroll
    for (int d = 0; d < D; ++d) load_row(tb + D + d, xn[d]);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = tb + d;
      if (t < nf) {
        double last = V[0];
#pragma unroll
        for (int p = 1; p < W; ++p) if (p == P - 1) last = V[p];
        double left = __shfl_up(last, 1, 64);
        if (lane == 0) left = -INFINITY;
        uint32_t bits = 0;
#pragma unroll
        for (int p = W - 1; p >= 0; --p) {
          if (p < P) {
            const double l = p > 0 ? V[p - 1] : left;
            const bool take = V[p] < l;
            V[p] = (double)x[d][p] + (take ? l : V[p]);
            bits |= (uint32_t)take << p;
          }
        }
        word |= bits << ((t % R) * W);
        if (t % R == R - 1 || t == nf - 1) {
          const int idx = ((t >> 6) * 2 * W + (t & 63) / R) * 64 + lane;
          if (in_lds) sdec[idx] = word; else gdec[idx] = word;
          word = 0;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int p = 0; p < W; ++p) x[d][p] = xn[d][p];
  }
  // V[nf-1][nl-1] lives in lane (nl-1) / P, slot (nl-1) % P
  int jl = (nl - 1) / P, jp = (nl - 1) - jl * P, j = nl - 1;
  {
    double fin = V[0];
#pragma unroll
    for (int p = 1; p < W; ++p) if (p == jp) fin = V[p];
    if (lane == jl) *score = (float)(fin / (double)nf);
  }
  if (lane == 0) ends[j] = nf;
  for (int b = (nf - 1) >> 6; b >= 0; --b) {
    uint32_t wv[2 * W];
#pragma unroll
    for (int u = 0; u < 2 * W; ++u) {
      const int idx = (b * 2 * W + u) * 64 + lane;
      wv[u] = (b * 64 + u * R < nf) ? (in_lds ? sdec[idx] : gdec[idx]) : 0u;
    }
#pragma unroll
    for (int r = 63; r >= 0; --r) {
      const int t = b * 64 + r;
      if (t < nf && t > 0 && j > 0) {
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)wv[r / R], __builtin_amdgcn_readfirstlane(jl));
        if (j == t || ((v >> ((r % R) * W + jp)) & 1u)) {
          if (lane == 0) ends[j - 1] = t;
          --j;
          if (jp == 0) { --jl; jp = P - 1; } else --jp;
        }
      }
    }
  }
}

__global__ __launch_bounds__(64) void align_path_kernel(const gsv_align_span_t* __restrict__ tab, float* __restrict__ ws,
                                                        long long ws_words, int32_t* __restrict__ ends, float* __restrict__ score) {
  __shared__ uint32_t sdec[ALIGN_LDS_WORDS];
  const int si = blockIdx.x, lane = threadIdx.x;
  const long long off = align_span_offset<64>(tab, si, nullptr);
  const gsv_align_span_t sp = tab[si];
  const int nf = sp.nf, nl = sp.nl;
  if (nf <= 0 || nl <= 0) {
    if (lane == 0) score[si] = -INFINITY;
    return;
  }
  int32_t* __restrict__ e = ends + sp.out0;
  if (!align_searched(nf, nl) || off + align_span_words_hd(nf, nl) > ws_words) {   // the AR stopped early, or too many phonemes
    for (int j = lane; j < nl; j += 64) e[j] = (int32_t)(((long long)(j + 1) * nf) / nl);
    if (lane == 0) score[si] = -INFINITY;
    return;
  }
  const float* lp = ws + off;
  uint32_t* gdec = reinterpret_cast<uint32_t*>(ws + off + align_lp_words(nf, nl));
  const bool in_lds = align_dec_in_lds(nf, nl);
  switch (align_field(nl)) {
    case 1: align_path_span<1>(lp, nf, nl, gdec, sdec, in_lds, e, score + si, lane); break;
    case 4: align_path_span<4>(lp, nf, nl, gdec, sdec, in_lds, e, score + si, lane); break;
    default: align_path_span<16>(lp, nf, nl, gdec, sdec, in_lds, e, score + si, lane); break;
  }
}

int launch_align_logp(int dtype, const void* q, int ldq, const void* k, int ldk, int heads, int head_dim, float scale,
                      const gsv_align_span_t* tab, int n, void* ws, long long ws_bytes, hipStream_t s) {
  GSV_REQUIRE(q && k && tab && ws && n >= 1 && n <= ALIGN_MAX_SPANS, "align_logp: null argument or bad span count %d", n);
  const int G = dtype == GSV_F16 ? 8 : 4;
  GSV_REQUIRE(heads >= 1 && heads <= ALIGN_MAX_HEADS && head_dim >= 2 * G && head_dim % (2 * G) == 0 && head_dim <= 1024,
              "align_logp: %d heads of %d", heads, head_dim);
  GSV_REQUIRE(ldq >= heads * head_dim && ldk >= heads * head_dim && ldq % G == 0 && ldk % G == 0 && (uintptr_t)q % 16 == 0 &&
                  (uintptr_t)k % 16 == 0 && (uintptr_t)ws % 16 == 0,
              "align_logp: rows must be 16-byte aligned (ldq %d, ldk %d)", ldq, ldk);
  GSV_REQUIRE(scale > 0.f && std::isfinite(scale), "align_logp: scale must be positive");
  return GSV_WITH_DTYPE(dtype, ([&]() -> int {
    GSV_LAUNCH(align_logp_kernel<T>, dim3(ALIGN_LP_BLOCKS, n), dim3(256), 0, s, (const T*)q, ldq, (const T*)k, ldk, heads, head_dim, scale,
               tab, (float*)ws, ws_bytes / 4);
    return GSV_OK;
  }()));
}

int launch_align_path(const gsv_align_span_t* tab, int n, void* ws, long long ws_bytes, int32_t* ends, float* score, hipStream_t s) {
  GSV_REQUIRE(tab && ws && ends && score && n >= 1 && n <= ALIGN_MAX_SPANS, "align_path: null argument or bad span count %d", n);
  GSV_REQUIRE((uintptr_t)ws % 16 == 0, "align_path: workspace must be 16-byte aligned");
  GSV_LAUNCH(align_path_kernel, dim3(n), dim3(64), 0, s, tab, (float*)ws, ws_bytes / 4, ends, score);
  return GSV_OK;
}

}  // namespace gsv

using namespace gsv;

long long gsv_op_align_workspace(int n_spans, const gsv_align_span_t* spans, int64_t* offsets) {
  if (n_spans < 0 || n_spans > ALIGN_MAX_SPANS || (n_spans && !spans)) {
    set_error("op_align_workspace: bad span table (%d spans)", n_spans);
    return GSV_ERR_ARG;
  }
  long long w = 0;
  for (int i = 0; i < n_spans; ++i) {
    if (offsets) offsets[i] = w * 4;
    w += align_span_words(spans[i].nf, spans[i].nl);
  }
  return std::max(w * 4, 16LL);
}

int gsv_op_align_logp(const void* q, int ldq, const void* k, int ldk, int dtype, int heads, int head_dim, float scale,
                      const gsv_align_span_t* spans, int n_spans, void* workspace, long long workspace_bytes, gsv_stream_t stream) {
  return launch_align_logp(dtype, q, ldq, k, ldk, heads, head_dim, scale, spans, n_spans, workspace, workspace_bytes, (hipStream_t)stream);
}

int gsv_op_align_path(const gsv_align_span_t* spans, int n_spans, void* workspace, long long workspace_bytes, int32_t* ends, float* score,
                      gsv_stream_t stream) {
  return launch_align_path(spans, n_spans, workspace, workspace_bytes, ends, score, (hipStream_t)stream);
}

int gsv_op_align(const void* q, int ldq, const void* k, int ldk, int dtype, int heads, int head_dim, float scale,
                 const gsv_align_span_t* spans, int n_spans, void* workspace, long long workspace_bytes, int32_t* ends, float* score,
                 gsv_stream_t stream) {
  GSV_RC(launch_align_logp(dtype, q, ldq, k, ldk, heads, head_dim, scale, spans, n_spans, workspace, workspace_bytes, (hipStream_t)stream));
  return launch_align_path(spans, n_spans, workspace, workspace_bytes, ends, score, (hipStream_t)stream);
}
