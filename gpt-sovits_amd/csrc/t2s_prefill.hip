// AR decoder prefill (H2 + H3): embeds the packed [text | prompt] rows of every utterance, runs the layers over all of them
// at once (GEMMs through launch_conv_gemm, attention on MFMA for fp16), fills the head-major K/V arena and leaves each row's
// last position in the decode buffer, from where gsv_t2s_decode (t2s.hip) samples step 0.
#include <stdlib.h>
#include <type_traits>
#include <vector>

#include "t2s_engine.h"

namespace gsv {

// x[row] = E_text[id] + bert_proj(bert)[row] + alpha_t * pe[pos]     (H2; t2s_model.py:612-617)
// or       E_audio[tok] + alpha_a * pe[pos]                            (t2s_model.py:636-640)
// rows are packed per utterance: [x_0 .. x_{X-1}, y_0 .. y_{P_b-1}]; row b's prompt is prompts[poff[b] .. + P_b)
template <typename T>
__global__ void embed_prefill_kernel(const int* __restrict__ phones, const int* __restrict__ prompts,
                                     const int* __restrict__ row_off, const int* __restrict__ ph_off,
                                     const int* __restrict__ x_len, const float* __restrict__ e_text,
                                     const float* __restrict__ e_audio, const float* __restrict__ bertp,  // [sumX][d] or null
                                     const float* __restrict__ bert_bias, const float* __restrict__ pe, float alpha_t,
                                     float alpha_a, const int* __restrict__ plen, const int* __restrict__ poff, int d,
                                     T* __restrict__ x) {
  const int b = blockIdx.y;
  const int i = blockIdx.x;  // position within the row's sequence
  const int X = x_len[b], P = plen[b];
  if (i >= X + P) return;
  T* out = x + (long long)(row_off[b] + i) * d;
  if (i < X) {
    const int id = phones[ph_off[b] + i];
    const float* e = e_text + (long long)id * d;
    const float* bp = bertp ? bertp + (long long)(ph_off[b] + i) * d : nullptr;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
      float v = e[c] + (bp ? bp[c] : bert_bias[c]);
      out[c] = (T)(v + alpha_t * pe[(long long)i * d + c]);
    }
  } else {
    const int tok = prompts[poff[b] + (i - X)];
    const float* e = e_audio + (long long)tok * d;
    for (int c = threadIdx.x; c < d; c += blockDim.x) out[c] = (T)(e[c] + alpha_a * pe[(long long)(i - X) * d + c]);
  }
}

// scatter the prefill K/V (columns d..3d of qkv) into the head-major cache
template <typename T>
__global__ void kv_scatter_kernel(const T* __restrict__ qkv, const int* __restrict__ row_off, const int* __restrict__ x_len,
                                  const int* __restrict__ plen, int d, int H, int smax, T* __restrict__ kc, T* __restrict__ vc) {
  const int b = blockIdx.y, i = blockIdx.x;
  if (i >= x_len[b] + plen[b]) return;
  const int hd = d / H;
  const T* src = qkv + (long long)(row_off[b] + i) * 3 * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) {
    const int h = c / hd, e = c - h * hd;
    const long long o = (((long long)b * H + h) * smax + i) * hd + e;
    kc[o] = src[d + c];
    vc[o] = src[2 * d + c];
  }
}

// Prefill attention (H3): one thread per query, keys streamed with a block-uniform address.
// Mask (t2s_model.py:655-683): text rows see the text keys; audio rows see all text + causal audio.
template <typename T, int HD>
__global__ void prefill_attn_kernel(const T* __restrict__ qkv, const T* __restrict__ kc, const T* __restrict__ vc,
                                    const int* __restrict__ row_off, const int* __restrict__ x_len, const int* __restrict__ plen,
                                    int d, int H, int smax, T* __restrict__ out) {
  const int b = blockIdx.z, h = blockIdx.y;
  const int X = x_len[b], S = X + plen[b];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int q0 = blockIdx.x * blockDim.x;
  if (q0 >= S) return;
  const bool valid = i < S;
  const int nk = valid ? (i < X ? X : i + 1) : 0;
  // block-uniform upper bound of the key loop
  const int qlast = min(q0 + (int)blockDim.x, S) - 1;
  const int nk_max = (qlast < X) ? X : qlast + 1;
  float q[HD], acc[HD];
  const T* qp = qkv + (long long)(row_off[b] + (valid ? i : 0)) * 3 * d + h * HD;
  const float scale = rsqrtf((float)HD);
#pragma unroll
  for (int e = 0; e < HD; ++e) { q[e] = to_f(qp[e]) * scale; acc[e] = 0.f; }
  float m = -INFINITY, l = 0.f;
  const T* kb = kc + ((long long)b * H + h) * smax * HD;
  const T* vb = vc + ((long long)b * H + h) * smax * HD;
  for (int j = 0; j < nk_max; ++j) {
    const T* kr = kb + (long long)j * HD;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < HD; ++e) s += q[e] * to_f(kr[e]);
    if (j < nk) {
      const float mn = fmaxf(m, s);
      const float corr = expf(m - mn);
      const float p = expf(s - mn);
      const T* vr = vb + (long long)j * HD;
      l = l * corr + p;
#pragma unroll
      for (int e = 0; e < HD; ++e) acc[e] = acc[e] * corr + p * to_f(vr[e]);
      m = mn;
    }
  }
  if (valid) {
    T* o = out + (long long)(row_off[b] + i) * d + h * HD;
    const float inv = 1.f / l;
#pragma unroll
    for (int e = 0; e < HD; ++e) o[e] = (T)(acc[e] * inv);
  }
}

// ---------------------------------------------------------------------------------------
// Prefill attention on MFMA (fp16, head dim 32), same construction as the DiT kernel (attn.hip): transposed scores
// S^T = K Q^T (one 16x16x32 MFMA per 16 keys x 16 queries: k = head dim), the probabilities a lane holds are the B
// operand of O^T = V^T P^T, keys dealt in 32-key chunks to the 4 waves with online softmax, LDS combine.  K comes
// straight from the head-major cache (a 16-key fragment is 1 KB contiguous), V^T from a per-prefill scratch.
// Mask (t2s_model.py:655-683): text queries see the text keys; audio queries see all text + causal audio.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prefill_vt_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ row_off,
                                                         const int* __restrict__ x_len, const int* __restrict__ plen, int d,
                                                         int H, int spad, _Float16* __restrict__ vt) {
  __shared__ _Float16 tile[32][34];
  const int b = blockIdx.z, h = blockIdx.y, j0 = blockIdx.x * 32;
  const int S = x_len[b] + plen[b];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i;
    tile[i][tx] = j < S ? qkv[(long long)(row_off[b] + j) * 3 * d + 2 * d + h * 32 + tx] : (_Float16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) vt[(((long long)b * H + h) * 32 + i) * spad + j0 + tx] = tile[tx][i];
}

// The same V^T tiles plus the head-major K/V cache rows of those 32 positions: one launch per layer instead of
// kv_scatter_kernel + prefill_vt_kernel (a 32 x 32 tile of one head is 2 KB contiguous in either cache).
__global__ __launch_bounds__(256) void prefill_kvt_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ row_off,
                                                          const int* __restrict__ x_len, const int* __restrict__ plen, int d,
                                                          int H, int smax, int spad, _Float16* __restrict__ kc,
                                                          _Float16* __restrict__ vc, _Float16* __restrict__ vt) {
  __shared__ _Float16 tile[32][34];
  const int b = blockIdx.z, h = blockIdx.y, j0 = blockIdx.x * 32;
  const int S = x_len[b] + plen[b];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i;
    _Float16 v = (_Float16)0.f;
    if (j < S) {
      const _Float16* src = qkv + (long long)(row_off[b] + j) * 3 * d + h * 32 + tx;
      const long long o = (((long long)b * H + h) * smax + j) * 32 + tx;
      v = src[2 * d];
      kc[o] = src[d];
      vc[o] = v;
    }
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) vt[(((long long)b * H + h) * 32 + i) * spad + j0 + tx] = tile[tx][i];
}

template <int QT>
__global__ __launch_bounds__(256) void prefill_flash32_f16_kernel(const _Float16* __restrict__ qkv, const _Float16* __restrict__ kc,
                                                                   const _Float16* __restrict__ vt, const int* __restrict__ row_off,
                                                                   const int* __restrict__ x_len, const int* __restrict__ plen, int d,
                                                                   int H, int smax, int spad, _Float16* __restrict__ out) {
  constexpr int BQ = 16 * QT, LDO = 36;
  __shared__ float Os[4][BQ][LDO];
  __shared__ float Ms[4][BQ], Ls[4][BQ];
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * BQ;
  const int X = x_len[b], S = X + plen[b];
  if (q0 >= S) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const float scale = rsqrtf(32.f);
  h8 qf[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t)
    qf[t] = *(const h8*)(qkv + (long long)(row_off[b] + min(q0 + 16 * t + r, S - 1)) * 3 * d + h * 32 + g * 8);
  const _Float16* kb = kc + ((long long)b * H + h) * smax * 32 + g * 8;
  const _Float16* vb = vt + (((long long)b * H + h) * 32 + r) * spad + 8 * g;
  const int kra = 8 * (r >> 2) + (r & 3);           // permuted K rows: the lane's 8 scores are 8 consecutive keys (attn.hip)
  f4 o[QT][2];
  float m[QT], l[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) { m[t] = -INFINITY; l[t] = 0.f; o[t][0] = (f4){0.f, 0.f, 0.f, 0.f}; o[t][1] = o[t][0]; }
  const int qlast = min(q0 + BQ, S) - 1;
  const int nk = qlast < X ? X : qlast + 1;          // workgroup-uniform bound of the key range
  const int nchunks = (nk + 31) >> 5, lastc = nchunks - 1;
  struct KV { h8 ka, kb2; h8 v[2]; };
  auto fetch = [&](KV& f, int c) {
    const int key0 = c << 5;
    f.ka = *(const h8*)(kb + (long long)min(key0 + kra, S - 1) * 32);
    f.kb2 = *(const h8*)(kb + (long long)min(key0 + kra + 4, S - 1) * 32);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) f.v[dt] = *(const h8*)(vb + (long long)(dt * 16) * spad + key0);
  };
  auto process = [&](const KV& f, int c, bool valid) {
    const int key0 = c << 5;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int qi = q0 + 16 * t + r;
      const int lim = qi < X ? X : qi + 1;           // keys [0, lim) are visible to query qi
      f4 sa = (f4){0.f, 0.f, 0.f, 0.f}, sb = sa;
      sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.ka, qf[t], sa, 0, 0, 0);
      sb = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.kb2, qf[t], sb, 0, 0, 0);
      float p[8];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[i] = (valid && key0 + 8 * g + i < lim) ? sa[i] * scale : -INFINITY;
        p[4 + i] = (valid && key0 + 8 * g + 4 + i < lim) ? sb[i] * scale : -INFINITY;
        mx = fmaxf(mx, fmaxf(p[i], p[4 + i]));
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m[t], mx);
      const float ms = mnew == -INFINITY ? 0.f : mnew;   // a causal query may see none of this wave's keys yet
      const float alpha = __expf(m[t] - ms);
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { p[i] = __expf(p[i] - ms); ps += p[i]; }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l[t] = l[t] * alpha + ps;
      m[t] = mnew;
      const h8 pf = (h8){(_Float16)p[0], (_Float16)p[1], (_Float16)p[2], (_Float16)p[3], (_Float16)p[4], (_Float16)p[5], (_Float16)p[6], (_Float16)p[7]};
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        o[t][dt] *= alpha;
        o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.v[dt], pf, o[t][dt], 0, 0, 0);
      }
    }
  };
#define GSV_PIN2() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
  KV fA, fB;
  fetch(fA, min(wave, lastc));
  for (int c = wave; c < nchunks; c += 8) {
    fetch(fB, min(c + 4, lastc));
    GSV_PIN2();
    process(fA, c, true);
    GSV_PIN2();
    fetch(fA, min(c + 8, lastc));
    GSV_PIN2();
    process(fB, c + 4, c + 4 < nchunks);
    GSV_PIN2();
  }
#undef GSV_PIN2
#pragma unroll
  for (int t = 0; t < QT; ++t) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) *(f4*)&Os[wave][16 * t + r][dt * 16 + 4 * g] = o[t][dt];
    if (g == 0) { Ms[wave][16 * t + r] = m[t]; Ls[wave][16 * t + r] = l[t]; }
  }
  __syncthreads();
  for (int it = threadIdx.x; it < BQ * 8; it += 256) {
    const int qq = it >> 3, d4 = (it & 7) * 4;
    if (q0 + qq >= S) continue;
    const float mt = fmaxf(fmaxf(Ms[0][qq], Ms[1][qq]), fmaxf(Ms[2][qq], Ms[3][qq]));   // finite: key 0 is visible to every query
    float den = 0.f;
    f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float e = __expf(Ms[w][qq] - mt);
      den += e * Ls[w][qq];
      acc += *(const f4*)&Os[w][qq][d4] * e;
    }
    const float inv = 1.f / den;
    *(h4*)(out + (long long)(row_off[b] + q0 + qq) * d + h * 32 + d4) =
        (h4){(_Float16)(acc[0] * inv), (_Float16)(acc[1] * inv), (_Float16)(acc[2] * inv), (_Float16)(acc[3] * inv)};
  }
}

// gather each row's last prefill position of the fp32 pre-LN2 stream into the decode buffer
__global__ void gather_last_kernel(const float* __restrict__ y2, const int* __restrict__ row_off,
                                   const int* __restrict__ x_len, const int* __restrict__ plen, int d, float* __restrict__ ybuf) {
  const int b = blockIdx.x;
  const float* src = y2 + (long long)(row_off[b] + x_len[b] + plen[b] - 1) * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) ybuf[(long long)b * d + c] = src[c];
}

// each row's prompt into the head of its token history (the repetition penalty's window): ytok[b][0 .. P_b)
__global__ void prompt_copy_kernel(const int* __restrict__ prompts, const int* __restrict__ plen, const int* __restrict__ poff,
                                   int ycap, int* __restrict__ ytok) {
  const int b = blockIdx.x, P = plen[b];
  for (int t = threadIdx.x; t < P; t += blockDim.x) ytok[(long long)b * ycap + t] = prompts[poff[b] + t];
}

}  // namespace gsv

using namespace gsv;
using namespace gsveng;

namespace {

int grow_prefill(gsv_t2s* h, size_t rows) {
  if (rows <= h->pf_rows) return GSV_OK;
  const size_t d = h->cfg.dim, ff = h->cfg.ffn_dim, es = esz(h);
  rows = (rows + 255) & ~(size_t)255;
  // old buffers stay registered in allocs and are released at destroy; growth is rare
  GSV_RC(dalloc(h, &h->pf_x, rows * d * es));
  GSV_RC(dalloc(h, &h->pf_qkv, rows * 3 * d * es));
  GSV_RC(dalloc(h, &h->pf_attn, rows * d * es));
  GSV_RC(dalloc(h, &h->pf_h, rows * ff * es));
  GSV_RC(dalloc(h, (void**)&h->pf_y, rows * d * 4));
  GSV_RC(dalloc(h, (void**)&h->pf_bert, rows * d * 4));
  GSV_RC(dalloc(h, &h->pf_bert_t, rows * (size_t)h->cfg.bert_dim * es));
  h->pf_rows = rows;
  return GSV_OK;
}

// y [rows][N] = x [rows][K] W^T + bias: the one GEMM form of the prefill (callers add the output type, residual, ReLU)
ConvArgs linear(const void* x, const void* w, const float* bias, void* y, int rows, int K, int N) {
  ConvArgs g;
  g.x = x; g.w = w; g.bias = bias; g.y = y;
  g.T_in = rows; g.T_out = rows; g.T_virt = rows; g.Cin = K; g.Cout = N; g.ldx = K; g.ldw = K; g.ldy = N;
  return g;
}

// A/B switches, read once per process
bool scalar_prefill_attn() { static const bool v = getenv("GSV_SCALAR_PREFILL_ATTN") != nullptr; return v; }      // thread-per-query VALU kernel
bool no_prefill_panel() { static const bool v = getenv("GSV_NO_PREFILL_PANEL") != nullptr; return v; }           // the four per-layer GEMMs stay on the dispatcher
bool prefill_split_scatter() { static const bool v = getenv("GSV_PREFILL_SPLIT_SCATTER") != nullptr; return v; }  // K/V scatter and V^T as two launches

// The four per-layer GEMMs: the panel kernel (gemm_panel.hip) in front of the dispatcher, the way the generator calls conv_pair.
// launch_gemm_panel_as_dispatcher picks the form of the kernel that computes the dispatcher's bits for the shape (gemm_lds' single sum,
// or gemm_t64's two accumulators where the dispatcher launches that one: up to 2048 rows) and declines where it has none, so the
// mode is a speed choice only, at every row count.
// PANEL_MIN_ROWS (mode 2): below it the dispatcher's skinny kernels (gemm_sk / gemm_t64) and under-filled gemm_lds grids serve and
// single-utterance latency stays what it is; tools/gemm_probe.py --panel has the sweep (profiles/prefill_panel_probe.txt).
// One (shape, M range) above the threshold stays on the dispatcher: where gemm_lds still fits ONE round of its
// 8-wave form (<= 256 tiles of 128 x 128) while the panel kernel's tiling needs a second round -- QKV at M = 2049 .. 2560,
// measured 12.3 us against 14.5 us at M = 2160.
constexpr int PANEL_MIN_ROWS = 2049;
bool panel_pays(const ConvArgs& g) {
  if (g.T_in < PANEL_MIN_ROWS) return false;
  int wgs = 0;
  gemm_panel_auto_tile(g, &wgs);
  const long long tiles128 = (long long)((g.T_in + 127) / 128) * ((g.Cout + 127) / 128);
  return !(tiles128 <= 256 && wgs > 256);
}
int prefill_gemm(gsv_t2s* h, const ConvArgs& g, hipStream_t s) {
  const int mode = no_prefill_panel() ? 0 : h->prefill_gemm;
  if (mode == 1 || (mode == 2 && panel_pays(g))) {
    const int rc = launch_gemm_panel_as_dispatcher(h->dtype, g, s);
    if (rc != 1) return rc;
  }
  return launch_conv_gemm(h->dtype, g, s);
}

// One layer's K/V fill and attention without the engine handle: what prefill_attention (the engine) and gsv_op_prefill_attn
// (the test hook) both launch through.  row_off / x_len / plen are device arrays of B ints, vt the V^T scratch of
// B * H * 32 * ceil32(maxS) halfs (fp16 flash routes only), kc / vc one layer's head-major cache [B][H][smax][32].
struct PrefillAttnArgs {
  const void* qkv = nullptr;
  void *kc = nullptr, *vc = nullptr, *vt = nullptr, *out = nullptr;
  const int *row_off = nullptr, *x_len = nullptr, *plen = nullptr;
  int B = 0, H = 0, d = 0, smax = 0, maxS = 0;
  bool scalar = false;          // thread-per-query VALU kernel instead of the MFMA flash kernel
  bool split_scatter = false;   // K/V scatter and V^T as two launches
};

// By one of three routes: fp16 with head dim 32 runs the MFMA flash kernel behind prefill_kvt_kernel (scatter + V^T in one
// launch) or, with split_scatter, behind kv_scatter + prefill_vt; fp32 and `scalar` take kv_scatter + the scalar kernel.
template <typename T>
int launch_prefill_attention(const PrefillAttnArgs& a, hipStream_t s) {
  const int d = a.d, H = a.H, B = a.B, smax = a.smax, maxS = a.maxS;
  const T* qkv = (const T*)a.qkv;
  T* kc = (T*)a.kc;
  T* vc = (T*)a.vc;
  T* out = (T*)a.out;
  const int *row_off = a.row_off, *x_len = a.x_len, *plen = a.plen;
  const bool mfma = std::is_same<T, _Float16>::value && d / H == 32 && !a.scalar;
  const bool fused_kvt = mfma && !a.split_scatter;
  if (!fused_kvt) GSV_LAUNCH(kv_scatter_kernel<T>, dim3(maxS, B), dim3(128), 0, s, qkv, row_off, x_len, plen, d, H, smax, kc, vc);
  if constexpr (std::is_same<T, _Float16>::value) {
    if (mfma) {
      const int spad = (maxS + 31) / 32 * 32;
      _Float16* vt = (_Float16*)a.vt;
      if (fused_kvt)
        GSV_LAUNCH(prefill_kvt_kernel, dim3(spad / 32, H, B), dim3(256), 0, s, qkv, row_off, x_len, plen, d, H, smax, spad, kc, vc, vt);
      else
        GSV_LAUNCH(prefill_vt_kernel, dim3(spad / 32, H, B), dim3(256), 0, s, qkv, row_off, x_len, plen, d, H, spad, vt);
      GSV_LAUNCH(prefill_flash32_f16_kernel<4>, dim3(cdiv(maxS, 64), H, B), dim3(256), 0, s, qkv, (const _Float16*)kc,
                 (const _Float16*)vt, row_off, x_len, plen, d, H, smax, spad, out);
      return GSV_OK;
    }
  }
  GSV_LAUNCH((prefill_attn_kernel<T, 32>), dim3(cdiv(maxS, 64), H, B), dim3(64), 0, s, qkv, (const T*)kc, (const T*)vc, row_off,
             x_len, plen, d, H, smax, out);
  return GSV_OK;
}

// the engine's layer li: pf_qkv -> pf_attn and r's arena, routes from GSV_SCALAR_PREFILL_ATTN / GSV_PREFILL_SPLIT_SCATTER
template <typename T>
int prefill_attention(gsv_t2s* h, const RowState& r, int li, int maxS, hipStream_t s) {
  PrefillAttnArgs a;
  a.qkv = h->pf_qkv; a.kc = kv_ptr(h, r, li, 0); a.vc = kv_ptr(h, r, li, 1); a.vt = h->pf_vt; a.out = h->pf_attn;
  a.row_off = h->d_row_off; a.x_len = h->d_x_len; a.plen = r.plen;
  a.B = r.B; a.H = h->cfg.n_head; a.d = h->cfg.dim; a.smax = r.max_seq; a.maxS = maxS;
  a.scalar = scalar_prefill_attn(); a.split_scatter = prefill_split_scatter();
  return launch_prefill_attention<T>(a, s);
}

// gsv_op_prefill_attn: the row table of t2s_prefill_rows, scratch of its own, one launch_prefill_attention, wait, free
template <typename T>
int op_prefill_attn(PrefillAttnArgs a, const int32_t* x_len, const int32_t* p_len, hipStream_t s) {
  const int B = a.B;
  std::vector<int> tab(3 * (size_t)B);   // [row_off | x_len | plen]
  int M = 0, maxS = 0;
  for (int b = 0; b < B; ++b) {
    const int S = x_len[b] + p_len[b];
    tab[b] = M; tab[B + b] = x_len[b]; tab[2 * (size_t)B + b] = p_len[b];
    M += S;
    maxS = S > maxS ? S : maxS;
  }
  a.maxS = maxS;
  int* d_tab = nullptr;
  void* vt = nullptr;
  int rc = GSV_OK;
  if (hipMalloc((void**)&d_tab, tab.size() * 4) != hipSuccess) rc = GSV_ERR_HIP;
  if (!rc && std::is_same<T, _Float16>::value && !a.scalar &&
      hipMalloc(&vt, (size_t)B * a.H * 32 * ((maxS + 31) / 32 * 32) * 2) != hipSuccess)
    rc = GSV_ERR_HIP;
  if (!rc && hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = GSV_ERR_HIP;
  if (rc) set_error("op_prefill_attn: scratch allocation or upload failed");
  if (!rc) {
    a.row_off = d_tab; a.x_len = d_tab + B; a.plen = d_tab + 2 * (size_t)B; a.vt = vt;
    rc = launch_prefill_attention<T>(a, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) { set_error("op_prefill_attn: a kernel failed"); rc = GSV_ERR_HIP; }
  }
  (void)hipFree(vt);
  (void)hipFree(d_tab);
  return rc;
}

// Prefill of B rows with prompts of P_b = plen[b] tokens, packed back to back in `prompts` (device) from poff[b] on.
// The uniform entry (every P_b = P, poff[b] = b P) and the ragged one share this body: the kernels read P_b per row either
// way, so a uniform batch computes exactly what it computed when P was a kernel argument.  The rows land in r: the handle's own
// or, for an admission, a session's staging rows.
template <typename T>
int t2s_prefill_rows(gsv_t2s* h, RowState& r, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                     const int32_t* prompts, const int* plen, const int* poff, hipStream_t s) {
  const auto& c = h->cfg;
  const int d = c.dim, H = c.n_head;
  std::vector<int> row_off(B), ph_off(B), kvl(B);
  int M = 0, SX = 0, maxS = 0, maxP = 0;
  for (int b = 0; b < B; ++b) {
    GSV_REQUIRE(phone_lens[b] >= 1, "t2s_prefill: empty phoneme sequence in row %d", b);
    row_off[b] = M; ph_off[b] = SX;
    const int P = plen[b];
    const int S = phone_lens[b] + P;
    GSV_REQUIRE(S + 2 <= r.max_seq, "t2s_prefill: row %d needs %d positions, max_seq is %d", b, S + 2, r.max_seq);
    GSV_REQUIRE(phone_lens[b] <= h->pe_rows, "t2s_prefill: sequence exceeds the position table");
    GSV_REQUIRE(P <= h->pe_rows, "t2s_prefill: row %d's prompt of %d tokens exceeds the position table (%d rows)", b, P, h->pe_rows);
    GSV_REQUIRE(P + 1 <= h->ycap, "t2s_prefill: row %d's prompt of %d tokens exceeds the token history (%d)", b, P, h->ycap);
    kvl[b] = S; M += S; SX += phone_lens[b];
    maxS = S > maxS ? S : maxS;
    maxP = P > maxP ? P : maxP;
  }
  GSV_RC(grow_prefill(h, M));
  if (h->dtype == GSV_F16) {
    const size_t need_vt = (size_t)B * H * 32 * ((maxS + 31) / 32 * 32) * 2;
    if (need_vt > h->pf_vt_cap) { GSV_RC(dalloc(h, &h->pf_vt, need_vt + need_vt / 4)); h->pf_vt_cap = need_vt + need_vt / 4; }
  }
  r.B = B; r.P = maxP;
  r.kv0 = kvl; r.pl.assign(plen, plen + B);
  GSV_HIP(hipMemcpyAsync(h->d_x_len, phone_lens, B * 4, hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemcpyAsync(h->d_row_off, row_off.data(), B * 4, hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemcpyAsync(h->d_ph_off, ph_off.data(), B * 4, hipMemcpyHostToDevice, s));
  const int* d_plen = r.plen;
  const int* d_poff = r.plen + r.mb;
  std::vector<int> pl(2 * (size_t)r.mb, 0);
  for (int b = 0; b < B; ++b) { pl[b] = plen[b]; pl[r.mb + b] = poff[b]; }
  GSV_HIP(hipMemcpyAsync(r.plen, pl.data(), pl.size() * 4, hipMemcpyHostToDevice, s));
  {
    // row state [kv_len | active | step | n_active] is one block: one upload
    const size_t mb = (size_t)r.mb;
    std::vector<int> st(r.state_ints(), 0);
    for (int b = 0; b < B; ++b) { st[b] = kvl[b]; st[mb + b] = 1; }
    st[3 * mb] = B;
    GSV_HIP(hipMemcpyAsync(r.state, st.data(), st.size() * 4, hipMemcpyHostToDevice, s));
    GSV_HIP(hipStreamSynchronize(s));
  }
  if (maxP > 0) GSV_LAUNCH(prompt_copy_kernel, dim3(B), dim3(64), 0, s, prompts, d_plen, d_poff, h->ycap, r.ytok);
  GSV_HIP(hipStreamSynchronize(s));  // host vectors above go out of scope

  const float* bertp = nullptr;
  if (bert) {
    GSV_RC(launch_convert(bert, h->pf_bert_t, h->dtype, (long long)SX * c.bert_dim, s));
    ConvArgs g = linear(h->pf_bert_t, h->bert_w, h->bert_b, h->pf_bert, SX, c.bert_dim, d);
    g.out_f32 = 1;
    GSV_RC(launch_conv_gemm(h->dtype, g, s));
    bertp = h->pf_bert;
  }
  GSV_LAUNCH(embed_prefill_kernel<T>, dim3(maxS, B), dim3(128), 0, s, phones, prompts, h->d_row_off, h->d_ph_off, h->d_x_len,
             h->e_text, h->e_audio, bertp, h->bert_b, h->pe, h->alpha_t, h->alpha_a, d_plen, d_poff, d, (T*)h->pf_x);

  for (int li = 0; li < c.n_layer; ++li) {
    const LayerW& L = h->layers[li];
    GSV_RC(prefill_gemm(h, linear(h->pf_x, L.qkv_w, L.qkv_b, h->pf_qkv, M, d, 3 * d), s));
    GSV_RC(prefill_attention<T>(h, r, li, maxS, s));
    // y1 = attn Wo^T + bo + x  (fp32) ; x1 = LN1(y1)
    ConvArgs o = linear(h->pf_attn, L.out_w, L.out_b, h->pf_y, M, d, d);
    o.out_f32 = 1; o.res = h->pf_x; o.ldr = d;
    GSV_RC(prefill_gemm(h, o, s));
    GSV_RC(launch_layernorm(h->dtype, h->pf_y, 1, nullptr, 0, L.n1w, L.n1b, h->pf_x, 0, M, d, 1e-5f, s));
    // y2 = relu(x1 W1^T + b1) W2^T + b2 + x1  (fp32) ; x = LN2(y2) for the next layer (the decode step applies the last one)
    ConvArgs f1 = linear(h->pf_x, L.w1, L.b1, h->pf_h, M, d, c.ffn_dim);
    f1.post_act = ACT_RELU;
    GSV_RC(prefill_gemm(h, f1, s));
    ConvArgs f2 = linear(h->pf_h, L.w2, L.b2, h->pf_y, M, c.ffn_dim, d);
    f2.out_f32 = 1; f2.res = h->pf_x; f2.ldr = d;
    GSV_RC(prefill_gemm(h, f2, s));
    if (li + 1 < c.n_layer)
      GSV_RC(launch_layernorm(h->dtype, h->pf_y, 1, nullptr, 0, L.n2w, L.n2b, h->pf_x, 0, M, d, 1e-5f, s));
  }
  GSV_LAUNCH(gather_last_kernel, dim3(B), dim3(128), 0, s, h->pf_y, h->d_row_off, h->d_x_len, d_plen, d, r.ybuf);
  return GSV_OK;
}

}  // namespace

int t2s_prefill_into(gsv_t2s* h, RowState& r, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                     const int32_t* prompts_packed, const int32_t* prompt_lens, hipStream_t s) {
  std::vector<int> poff(B);
  int o = 0;
  for (int b = 0; b < B; ++b) { poff[b] = o; o += prompt_lens[b]; }
  return GSV_WITH_T(h, t2s_prefill_rows<T>(h, r, phones, phone_lens, B, bert, prompts_packed, prompt_lens, poff.data(), s));
}

extern "C" {

int gsv_t2s_prefill(gsv_t2s_t* h, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                    const int32_t* prompts, int P, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "t2s_prefill: handle not finalized");
  GSV_T2S_NO_SESSION(h, "t2s_prefill");
  GSV_REQUIRE(phones && phone_lens && (prompts || P == 0), "t2s_prefill: null argument");
  GSV_REQUIRE(B >= 1 && B <= h->max_batch, "t2s_prefill: batch %d exceeds max_batch %d", B, h->max_batch);
  GSV_REQUIRE(P >= 0, "t2s_prefill: negative prompt length %d", P);   // P == 0: prompt-free decode (t2s_model.py:849-856)
  std::vector<int> plen(B, P), poff(B);
  for (int b = 0; b < B; ++b) poff[b] = b * P;
  return GSV_WITH_T(h, t2s_prefill_rows<T>(h, h->rows, phones, phone_lens, B, bert, prompts, plen.data(), poff.data(), (hipStream_t)stream));
}

int gsv_t2s_prefill_ragged(gsv_t2s_t* h, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                           const int32_t* prompts_packed, const int32_t* prompt_lens, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "t2s_prefill_ragged: handle not finalized");
  GSV_T2S_NO_SESSION(h, "t2s_prefill_ragged");
  // Row limits pending for the decode that follows (gsv_t2s_set_row_limits): a row may then be prompt-free, its EOS horizon is
  // its own.  The kernels read P_b per row and never touch `prompts` for a row with P_b = 0: embed_prefill_kernel reads it at
  // i >= X only, prompt_copy_kernel loops over t < P_b (and is not launched when every row is prompt-free), gather_last_kernel
  // reads position X + P_b - 1 >= 0, and the attention kernels treat such a row as text only -- what the uniform P = 0 entry runs.
  const bool limits = !h->row_limits_next.empty();
  GSV_REQUIRE(phones && phone_lens && prompt_lens, "t2s_prefill_ragged: null argument");
  GSV_REQUIRE(B >= 1 && B <= h->max_batch, "t2s_prefill_ragged: batch %d exceeds max_batch %d", B, h->max_batch);
  if (limits && (int)h->row_limits_next.size() != B) {
    set_error("t2s_prefill_ragged: gsv_t2s_set_row_limits gave %d rows for a batch of %d rows", (int)h->row_limits_next.size(), B);
    h->row_limits_next.clear();
    return GSV_ERR_ARG;
  }
  std::vector<int> poff(B);
  int o = 0;
  for (int b = 0; b < B; ++b) {
    // without limits prompt-free rows keep the uniform entry (P = 0 there also masks EOS for 11 steps: t2s_model.py:849-856)
    GSV_REQUIRE(prompt_lens[b] >= (limits ? 0 : 1), "t2s_prefill_ragged: row %d has prompt length %d (must be >= 1)", b,
                prompt_lens[b]);
    poff[b] = o; o += prompt_lens[b];
  }
  GSV_REQUIRE(prompts_packed || (limits && o == 0), "t2s_prefill_ragged: null argument");
  return GSV_WITH_T(h, t2s_prefill_rows<T>(h, h->rows, phones, phone_lens, B, bert, prompts_packed, prompt_lens, poff.data(), (hipStream_t)stream));
}

int gsv_op_prefill_attn(const void* qkv, const int32_t* x_len, const int32_t* p_len, int B, int H, int d, int smax, int dtype,
                        int route, void* kc, void* vc, void* out, gsv_stream_t stream) {
  GSV_REQUIRE(qkv && x_len && p_len && kc && vc && out, "op_prefill_attn: null pointer");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_prefill_attn: bad dtype %d", dtype);
  GSV_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && smax >= 1, "op_prefill_attn: bad shape B=%d H=%d smax=%d", B, H, smax);
  GSV_REQUIRE(d == 32 * H, "op_prefill_attn: d = %d is not 32 * H (H = %d): the kernels are built for head dim 32", d, H);
  GSV_REQUIRE(route >= 0 && route <= 3, "op_prefill_attn: unknown route %d", route);
  GSV_REQUIRE(dtype == GSV_F16 || route == 0 || route == 3, "op_prefill_attn: route %d (MFMA flash) is fp16 only", route);
  long long M = 0;
  for (int b = 0; b < B; ++b) {
    GSV_REQUIRE(x_len[b] >= 1, "op_prefill_attn: empty phoneme sequence in row %d", b);
    GSV_REQUIRE(p_len[b] >= 0, "op_prefill_attn: negative prompt length %d in row %d", p_len[b], b);
    GSV_REQUIRE((long long)x_len[b] + p_len[b] + 2 <= smax, "op_prefill_attn: row %d needs %lld positions, smax is %d", b,
                (long long)x_len[b] + p_len[b] + 2, smax);
    M += x_len[b] + p_len[b];
  }
  GSV_REQUIRE(M <= 0x7fffffffLL, "op_prefill_attn: %lld packed rows", M);
  PrefillAttnArgs a;
  a.qkv = qkv; a.kc = kc; a.vc = vc; a.out = out;
  a.B = B; a.H = H; a.d = d; a.smax = smax;
  // route 0: the engine's own choice, its two process-wide switches included
  a.scalar = route == 3 || (route == 0 && scalar_prefill_attn());
  a.split_scatter = route == 2 || (route == 0 && prefill_split_scatter());
  return GSV_WITH_DTYPE(dtype, op_prefill_attn<T>(a, x_len, p_len, (hipStream_t)stream));
}

}  // extern "C"
