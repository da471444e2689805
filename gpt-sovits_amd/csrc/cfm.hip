// v3 / v4 flow-matching mel decoder (H14) for gfx950: CFM.inference (reference module/models.py:1027-1085)
// over the DiT estimator (reference f5_tts/model/backbones/dit.py:88-194, f5_tts/model/modules.py).
//
// Layout: one utterance at a time, every activation channels-last [frame][channel] in the engine dtype,
// the Euler state x and the velocity in fp32.  Every Linear / conv is one call of the MFMA GEMM / implicit-GEMM
// kernels (gemm_lds.hip / conv_lds.hip / conv_gemm.hip); the grouped position conv is a Z=16 batched implicit GEMM.
// Everything that depends only on the step index is hoisted out of the Euler loop: the time embeddings of all
// n steps are computed at once and pushed through every block's AdaLN-Zero modulation Linear as ONE [n][dim] x
// [dim][6 dim] GEMM per block (the reference re-reads those 22 x 6 dim x dim weights as a GEMV every step);
// the text embedding (ConvNeXt-V2 stack), the rotary table and the prompt / text columns of the input
// concatenation are built once per utterance (the reference caches the first two the same way, models.py:1046-1062).
// Gate * (W a + b) + residual is the GEMM epilogue (ConvArgs::gate), GELU / Mish too.
#include <cmath>
#include <cstddef>

#include "cfm_engine.h"

using namespace gsv;
using namespace gsveng;
using namespace gsvcfm;

namespace gsv {

// sinusoidal embedding (modules.py:152-164) of `rows` scalars: [rows][2*half] = sin | cos of 1000 * t * exp(-j * ln(1e4)/(half-1))
__global__ void cfm_sinus_kernel(const float* __restrict__ tvals, int rows, int half, float* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * half) return;
  int r = i / half, j = i - r * half;
  const float e = expf((float)j * -(logf(10000.f) / (float)(half - 1)));
  const float a = 1000.f * tvals[r] * e;
  out[(long long)r * 2 * half + j] = sinf(a);
  out[(long long)r * 2 * half + half + j] = cosf(a);
}

// out[r][c] = silu(a[r][c] + b[r][c])   (time + step-size embedding, then the SiLU of AdaLayerNormZero)
template <typename T>
__global__ void cfm_add_silu_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, T* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float u = a[i] + b[i];
  out[i] = (T)(u / (1.f + expf(-u)));
}

// fp32 -> engine dtype with a row stride on both sides
template <typename T>
__global__ void cfm_cast_rows_kernel(const float* __restrict__ src, int lds, int rows, int C, T* __restrict__ dst, int ldd, int col0) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)rows * C) return;
  int r = (int)(i / C), c = (int)(i - (long long)r * C);
  dst[(long long)r * ldd + col0 + c] = (T)src[(long long)r * lds + c];
}

// The kernels that look along time take the utterance (row of the batch) as blockIdx.y: one launch over all rows, every row
// an independent [Tn][C] slab, back to back.
//
// te0[t][c] = mu[t][c] + table[min(t, 4095)][c]   (TextEmbedding.forward, dit.py:50-72).  Rows from `mu_rows` on have no
// text: zeros before the table (drop_text, dit.py:44-48) -- the null text row of a guided pass.
template <typename T>
__global__ void cfm_text_pos_kernel(const float* __restrict__ mu, int mu_rows, const float* __restrict__ table, int Tn, int C,
                                    T* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  int t = (int)(i / C), c = (int)(i - (long long)t * C);
  const long long o = (long long)blockIdx.y * Tn * C + i;
  const float tab = table[(long long)min(t, 4095) * C + c];
  out[o] = (T)((int)blockIdx.y < mu_rows ? mu[o] + tab : tab);
}

// depthwise conv, 7 taps, zero padding 3 (ConvNeXtV2Block.dwconv, modules.py:250)
template <typename T>
__global__ void cfm_dwconv7_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int Tn, int C,
                                   T* __restrict__ y) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  int t = (int)(i / C), c = (int)(i - (long long)t * C);
  x += (long long)blockIdx.y * Tn * C;
  y += (long long)blockIdx.y * Tn * C;
  float acc = b[c];
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    int ti = t + j - 3;
    if (ti >= 0 && ti < Tn) acc += w[c * 7 + j] * to_f(x[(long long)ti * C + c]);
  }
  y[i] = (T)acc;
}

// GRN (modules.py:225-236): gx[row][c] = ||y[row][:, c]||_2 over the row's own frames
template <typename T>
__global__ void cfm_grn_norm_kernel(const T* __restrict__ y, int Tn, int C, float* __restrict__ gx) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
  y += (long long)blockIdx.y * Tn * C;
  gx += (long long)blockIdx.y * C;
  float s = 0.f;
  if (c < C)
    for (int t = part; t < Tn; t += 4) { float v = to_f(y[(long long)t * C + c]); s += v * v; }
  red[part][threadIdx.x & 63] = s;
  __syncthreads();
  if (part == 0 && c < C) gx[c] = sqrtf(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// y = gamma * (y * gx / (mean_c gx + 1e-6)) + beta + y
template <typename T>
__global__ void cfm_grn_apply_kernel(T* __restrict__ y, const float* __restrict__ gx, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, int Tn, int C) {
  __shared__ float wsum[4];
  y += (long long)blockIdx.y * Tn * C;
  gx += (long long)blockIdx.y * C;
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) s += gx[c];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  const float mean = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) / (float)C;
  const float inv = 1.f / (mean + 1e-6f);
  const long long n = (long long)Tn * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    int c = (int)(i % C);
    float v = to_f(y[i]);
    y[i] = (T)(gamma[c] * (v * (gx[c] * inv)) + beta[c] + v);
  }
}

// AdaLN-Zero modulation: y = LN(x) * (1 + scale) + shift, LN without affine, eps 1e-6 (modules.py:275-312).  One wave per
// row; the row is read ONCE into registers (three dependent passes over global memory cost 10 us per call at T = 934).
template <typename T, int NPL>   // NPL = elements per lane, C == 64 * NPL
__device__ __forceinline__ void cfm_ln_mod_row(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift, int row,
                                               int C, T* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const T* xr = x + (long long)row * C + lane * NPL;
  float v[NPL];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NPL; ++i) { v[i] = to_f(xr[i]); sum += v[i]; }
  const float mean = wave_sum(sum) / (float)C;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < NPL; ++i) { const float d = v[i] - mean; var += d * d; }
  const float rstd = rsqrtf(wave_sum(var) / (float)C + 1e-6f);
  T* yr = y + (long long)row * C + lane * NPL;
  const float* sc = scale + lane * NPL;
  const float* sh = shift + lane * NPL;
#pragma unroll
  for (int i = 0; i < NPL; ++i) yr[i] = (T)((v[i] - mean) * rstd * (1.f + sc[i]) + sh[i]);
}
template <typename T, int NPL>
__global__ __launch_bounds__(256) void cfm_ln_mod_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, int rows, int C, T* __restrict__ y) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  cfm_ln_mod_row<T, NPL>(x, scale, shift, row, C, y);
}
// the per-row form (sessions): utterance row b = row / Tn has its own scale / shift vectors, ld floats after row b - 1's
template <typename T, int NPL>
__global__ __launch_bounds__(256) void cfm_ln_mod_rows_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int rows, int C, T* __restrict__ y, int Tn, int ld) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long o = (long long)(row / Tn) * ld;
  cfm_ln_mod_row<T, NPL>(x, scale + o, shift + o, row, C, y);
}

// Tn > 0: the per-row form
template <typename T>
int launch_ln_mod(const void* x, const float* scale, const float* shift, int rows, int C, void* y, hipStream_t s, int Tn = 0, int ld = 0) {
  auto launch = [&](auto npl) -> int {
    if (Tn > 0)
      GSV_LAUNCH((cfm_ln_mod_rows_kernel<T, decltype(npl)::value>), dim3(cdiv(rows, 4)), dim3(256), 0, s, (const T*)x, scale, shift, rows, C, (T*)y,
                 Tn, ld);
    else
      GSV_LAUNCH((cfm_ln_mod_kernel<T, decltype(npl)::value>), dim3(cdiv(rows, 4)), dim3(256), 0, s, (const T*)x, scale, shift, rows, C, (T*)y);
    return GSV_OK;
  };
  switch (C / 64) {
    case 2: return launch(std::integral_constant<int, 2>{});
    case 4: return launch(std::integral_constant<int, 4>{});
    case 8: return launch(std::integral_constant<int, 8>{});
    case 16: return launch(std::integral_constant<int, 16>{});
    case 32: return launch(std::integral_constant<int, 32>{});
    default: set_error("cfm: dim %d is not one of 128, 256, 512, 1024, 2048", C); return GSV_ERR_ARG;
  }
}

// rotary embedding on the first 2*half channels of the q and k projections (x_transformers' apply_rotary_pos_emb on the
// un-split [n, heads*dim_head] tensors, modules.py:420-427): adjacent pairs, angle = t * inv_freq[pair]
template <typename T>
__global__ void cfm_rope_kernel(T* __restrict__ qkv, int ld, int kcol0, int rows, int Tn, int half, const float* __restrict__ cs) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * half * 2) return;
  const int which = i / (rows * half);
  const int rr = i - which * rows * half;
  const int row = rr / half, p = rr - row * half;
  const int t = row % Tn;                                  // rows = batch * Tn: the position restarts per utterance
  T* v = qkv + (long long)row * ld + (which ? kcol0 : 0) + 2 * p;
  const float c = cs[((long long)t * half + p) * 2], s = cs[((long long)t * half + p) * 2 + 1];
  const float a = to_f(v[0]), b = to_f(v[1]);
  v[0] = (T)(a * c - b * s);
  v[1] = (T)(b * c + a * s);
}

__global__ void cfm_rope_table_kernel(int Tn, int half, float* __restrict__ cs) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Tn * half) return;
  const int t = i / half, p = i - t * half;
  const float inv = 1.f / powf(10000.f, (float)(2 * p) / (float)(2 * half));
  const float ang = (float)t * inv;
  cs[2 * (long long)i] = cosf(ang);
  cs[2 * (long long)i + 1] = sinf(ang);
}

__device__ __forceinline__ unsigned long long cfm_mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void cfm_rows_fill_kernel(CfmRowChunk ch, int n, CfmRow* __restrict__ rw) {
  const int b = threadIdx.x;
  if (b < n) rw[b] = ch.r[b];
}

// x0[t][c] = temperature * noise (given channels-first [B][C][Tn], or a counter-based normal draw), zero on the prompt frames
__global__ void cfm_init_x_kernel(const float* __restrict__ noise, const CfmRow* __restrict__ rw, float temperature, int Tn, int C,
                                  float* __restrict__ x) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  int t = (int)(i / C), c = (int)(i - (long long)t * C);
  const int b = blockIdx.y;
  const unsigned long long seed = rw[b].seed;
  const int Tp = rw[b].Tp;
  x += (long long)b * Tn * C;
  float n;
  if (noise) n = noise[((long long)b * C + c) * Tn + t];
  else {
    unsigned long long h1 = cfm_mix64(seed ^ cfm_mix64((unsigned long long)i * 2 + 1)), h2 = cfm_mix64(seed ^ cfm_mix64((unsigned long long)i * 2 + 2));
    float u1 = ((float)(h1 >> 40) + 1.f) * (1.f / 16777217.f), u2 = (float)(h2 >> 40) * (1.f / 16777216.f);
    n = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
  }
  x[i] = t < Tp ? 0.f : n * temperature;
}

// Euler update x += d * v (frames >= Tp; prompt frames stay 0, models.py:1083-1084) and refresh the x columns of the DiT input;
// rows = batch * Tn, the prompt region restarts per utterance with that utterance's own length.
// GUIDED (models.py:1063-1084): v holds the conditioned estimate of request b in DiT row b and the unconditioned one in its
// twin, row B + b (rows = B * Tn frames of requests, so the twin of frame i is frame rows + i).  x += d * (v_pos + (v_pos -
// v_neg) * rate) in fp32, and the refreshed x goes into the x columns of BOTH rows: the two estimates of the next step see the
// same state.  The unguided form reads one estimate and never sees `rate`.
template <typename T, bool GUIDED>
__global__ void cfm_euler_kernel(float* __restrict__ x, const float* __restrict__ v, float d, float rate, int rows, int Tn,
                                 const CfmRow* __restrict__ rw, int C, T* __restrict__ xin, int ldin) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)rows * C;
  if (i >= n) return;
  int row = (int)(i / C), c = (int)(i - (long long)row * C);
  const int b = row / Tn, t = row - b * Tn;
  const int Tp = rw[b].Tp;
  float u = 0.f;
  if (t >= Tp) {
    if constexpr (GUIDED) {
      u = x[i];
      if (v) {
        const float vp = v[i], vn = v[n + i];
        u += d * (vp + (vp - vn) * rate);
      }
    } else {
      u = x[i] + (v ? d * v[i] : 0.f);
    }
  }
  x[i] = u;
  xin[(long long)row * ldin + c] = (T)u;
  if constexpr (GUIDED) xin[((long long)rows + row) * ldin + c] = (T)u;
}

// prompt mel (channels-first [C][Tp]) -> the cond columns of the DiT input, zero after the prompt; also zeroes the pad columns
template <typename T>
__global__ void cfm_cond_kernel(const CfmRow* __restrict__ rw, int Tn, int C, T* __restrict__ xin, int ldin, int col0, int pad0) {
  const int W = C + (ldin - pad0);
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * W) return;
  int t = (int)(i / W), c = (int)(i - (long long)t * W);
  const float* prompt = rw[blockIdx.y].prompt;
  const int Tp = rw[blockIdx.y].Tp;
  xin += (long long)blockIdx.y * Tn * ldin;
  if (c < C) xin[(long long)t * ldin + col0 + c] = (T)(prompt && t < Tp ? prompt[(long long)c * Tp + t] : 0.f);
  else xin[(long long)t * ldin + pad0 + (c - C)] = (T)0.f;
}

template <typename T>
__global__ void cfm_copy_cols_kernel(const T* __restrict__ src, int lds, int rows, int C, T* __restrict__ dst, int ldd, int col0) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)rows * C) return;
  int r = (int)(i / C), c = (int)(i - (long long)r * C);
  dst[(long long)r * ldd + col0 + c] = src[(long long)r * lds + c];
}

// one [Tn][C] slab into columns [col0, col0 + C) of every row blockIdx.y of dst (the null text embedding into all twins)
template <typename T>
__global__ void cfm_bcast_cols_kernel(const T* __restrict__ src, int Tn, int C, T* __restrict__ dst, int ldd, int col0) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  int t = (int)(i / C), c = (int)(i - (long long)t * C);
  dst[((long long)blockIdx.y * Tn + t) * ldd + col0 + c] = src[i];
}

// channels-last fp32 [Tn][C] -> channels-first [C][Tn]; the prompt frames are written as the zeros they are held at
__global__ void cfm_out_kernel(const float* __restrict__ x, const CfmRow* __restrict__ rw, int Tn, int C, float* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  int c = (int)(i / Tn), t = (int)(i - (long long)c * Tn);
  const long long o = (long long)blockIdx.y * Tn * C;
  out[o + i] = t < rw[blockIdx.y].Tp ? 0.f : x[o + (long long)t * C + c];
}

}  // namespace gsv

namespace gsvcfm {

// time-independent precomputation for all n steps: mods[l][i][6D] (l < depth) and mods[depth][i][2D]
template <typename T>
int modulations(gsv_cfm* c, hipStream_t s, int N, float** mods_out) {
  const auto& g = c->cfg;
  const int D = g.dim;
  const size_t es = sizeof(T);
  float *tvals, *sinus, *temb, *mods;
  void *sin_t, *mid_t, *stemb;
  GSV_RC(need(c, "cfm_tvals", (size_t)2 * N * 4, (void**)&tvals));
  GSV_RC(need(c, "cfm_sinus", (size_t)2 * N * 256 * 4, (void**)&sinus));
  GSV_RC(need(c, "cfm_sin_t", (size_t)2 * N * 256 * es, &sin_t));
  GSV_RC(need(c, "cfm_mid_t", (size_t)2 * N * D * es, &mid_t));
  GSV_RC(need(c, "cfm_temb", (size_t)2 * N * D * 4, (void**)&temb));
  GSV_RC(need(c, "cfm_stemb", (size_t)N * D * es, &stemb));
  GSV_RC(need(c, "cfm_mods", ((size_t)g.depth * 6 + 2) * N * D * 4, (void**)&mods));
  {
    std::vector<float> tv(2 * N);
    double t = 0.0;
    const double d = 1.0 / N;
    for (int i = 0; i < N; ++i) { tv[i] = (float)t; tv[N + i] = (float)d; t += d; }   // models.py:1042-1082
    GSV_HIP(hipMemcpyAsync(tvals, tv.data(), tv.size() * 4, hipMemcpyHostToDevice, s));
    GSV_HIP(hipStreamSynchronize(s));   // tv lives on this stack frame
  }
  GSV_LAUNCH(cfm_sinus_kernel, cfm_grid(2 * N * 128), dim3(256), 0, s, tvals, 2 * N, 128, sinus);
  GSV_LAUNCH(cfm_cast_rows_kernel<T>, cfm_grid(2 * N * 256), dim3(256), 0, s, sinus, 256, 2 * N, 256, (T*)sin_t, 256, 0);
  ConvOpt o1; o1.post_act = ACT_SILU;
  ConvOpt o2; o2.out_f32 = 1;
  // rows [0, N): time_embed(t_i); rows [N, 2N): d_embed(d)   (dit.py:149-153)
  GSV_RC(conv(c, s, c->t0, sin_t, 256, N, mid_t, N, o1));
  GSV_RC(conv(c, s, c->t2, mid_t, D, N, temb, N, o2));
  GSV_RC(conv(c, s, c->d0, (const T*)sin_t + (size_t)N * 256, 256, N, (T*)mid_t + (size_t)N * D, N, o1));
  GSV_RC(conv(c, s, c->d2, (const T*)mid_t + (size_t)N * D, D, N, temb + (size_t)N * D, N, o2));
  GSV_LAUNCH(cfm_add_silu_kernel<T>, cfm_grid((long long)N * D), dim3(256), 0, s, temb, temb + (size_t)N * D, (long long)N * D, (T*)stemb);
  for (int l = 0; l < g.depth; ++l)
    GSV_RC(conv(c, s, c->blocks[l].mod, stemb, D, N, mods + (size_t)l * N * 6 * D, N, o2));
  GSV_RC(conv(c, s, c->final_mod, stemb, D, N, mods + (size_t)g.depth * N * 6 * D, N, o2));
  *mods_out = mods;
  return GSV_OK;
}

// the text embedding stack (TextEmbedding.forward, dit.py:50-72): position table, then the ConvNeXt-V2 blocks
template <typename T>
int text_stack(gsv_cfm* c, hipStream_t s, const float* mu, int mu_rows, int TB, int Tn, void* ta, void* tb, void* tw, float* gx) {
  const int td = c->cfg.text_dim, RT = TB * Tn;
  GSV_LAUNCH(cfm_text_pos_kernel<T>, cfm_grid((long long)Tn * td, TB), dim3(256), 0, s, mu, mu_rows, c->pos_table, Tn, td, (T*)ta);
  for (auto& blk : c->text) {
    GSV_LAUNCH(cfm_dwconv7_kernel<T>, cfm_grid((long long)Tn * td, TB), dim3(256), 0, s, (const T*)ta, blk.dw, blk.db, Tn, td, (T*)tb);
    GSV_RC(launch_layernorm(c->dtype, tb, 0, nullptr, 0, blk.ng, blk.nb, tb, 0, RT, td, 1e-6f, s));
    ConvOpt og; og.post_act = ACT_GELU;
    GSV_RC(conv(c, s, blk.pw1, tb, td, RT, tw, RT, og));
    // GRN statistics are per utterance (norm over its own frames): gx [TB][2 td]
    GSV_LAUNCH(cfm_grn_norm_kernel<T>, dim3(cdiv(2 * td, 64), TB), dim3(256), 0, s, (const T*)tw, Tn, 2 * td, gx);
    GSV_LAUNCH(cfm_grn_apply_kernel<T>, dim3(std::min(1024, nblk((long long)Tn * 2 * td)), TB), dim3(256), 0, s, (T*)tw, gx, blk.gg, blk.gb,
               Tn, 2 * td);
    ConvOpt orr; orr.res = ta;
    GSV_RC(conv(c, s, blk.pw2, tw, 2 * td, RT, ta, RT, orr));
  }
  return GSV_OK;
}

// One DiT forward over DB packed rows of Tn frames.  LoRA adapters (max_rp > 0: some row carries a slot, max_rp the largest
// padded rank among them): two more launches per block, the low-rank delta on qkv right after the q/k/v GEMM (before rotary /
// V^T / attention read it) and on hb right after the out-projection GEMM, under the same gate.  Workgroups of rows without a
// slot return at once.  max_rp == 0: no such launch.  mods.rows: every launch that reads a modulation vector takes its per-row
// form (cfm_ln_mod_rows_kernel, the GROWS GEMM epilogues, the *_rows LoRA kernels); 0: the launches are the ones they were.
template <typename T>
int dit_forward(gsv_cfm* c, hipStream_t s, const void* xin, int DB, int Tn, const DitMods& mods, const int* row_slot, int slot_ld, int max_rp,
                const float* cs, float* v) {
  const auto& g = c->cfg;
  const int D = g.dim, inner = g.heads * g.dim_head, FF = D * g.ff_mult, ldin = c->ldin;
  const int half = g.dim_head / 2;
  const size_t es = sizeof(T);
  const int R = DB * Tn;
  void *hb, *c1, *nrm, *qkv, *ao, *ff;
  GSV_RC(need(c, "cfm_h", (size_t)R * D * es, &hb));
  GSV_RC(need(c, "cfm_c1", (size_t)R * D * es, &c1));
  GSV_RC(need(c, "cfm_nrm", (size_t)R * D * es, &nrm));
  GSV_RC(need(c, "cfm_qkv", (size_t)R * 3 * inner * es, &qkv));
  GSV_RC(need(c, "cfm_ao", (size_t)R * inner * es, &ao));
  GSV_RC(need(c, "cfm_ff", (size_t)R * FF * es, &ff));
  auto rows = [&](void* p, int b, int width) { return (void*)((char*)p + (size_t)b * Tn * width * es); };
  const float att_scale = 1.f / sqrtf((float)g.dim_head);
  const bool flash = c->dtype == GSV_F16 && g.dim_head == 64 && !c->materialized_attn;
  // Infinity-Cache partition: the block weights (16.8 MB per block at the v3 shape, 370 MB in all) are re-read every Euler
  // step and do not fit the 256 MB cache, so a plain cyclic sweep keeps evicting what the next step needs first.  The
  // first `resident` blocks are loaded with the default policy (they stay), the rest non-temporal (they stream past).
  const size_t per_block = ((size_t)D * 3 * inner + (size_t)inner * D + 2 * (size_t)D * FF) * es;
  static const int resident_mb = getenv("GSV_CFM_RESIDENT_MB") ? atoi(getenv("GSV_CFM_RESIDENT_MB")) : 150;   // scan: 1000 -> 3.03, 200 -> 2.95, 150 -> 2.94, 60 -> 2.97, 0 -> 2.99 ms per step
  const int resident = per_block ? (int)std::min<size_t>((size_t)g.depth, (size_t)resident_mb * 1024 * 1024 / per_block) : g.depth;
  void* vtb = nullptr;
  const long long vtz = (long long)g.heads * 64 * ((Tn + 31) / 32 * 32);   // one V^T buffer per utterance
  if (flash) GSV_RC(need(c, "cfm_vt", (size_t)DB * vtz * 2, &vtb));
  const long long lora_blk = 4ll * (D + inner);   // an adapter's elements per DiT block, in units of rp (CfmAdapter)
  const int pr = mods.rows ? Tn : 0;              // per-row modulations: frames per vector, 0 = one vector for all rows
  // ---- InputEmbedding (dit.py:75-84): proj(cat(x, cond, text)) then + ConvPositionEmbedding
  ConvOpt o;
  GSV_RC(conv(c, s, c->in_proj, xin, ldin, R, hb, R, o));
  for (int b = 0; b < DB; ++b) {
    ConvArgs a;
    const int cg = D / 16;
    a.x = rows(hb, b, D); a.w = c->pos1.w; a.bias = c->pos1.b; a.y = rows(c1, b, D);
    a.T_in = Tn; a.T_out = Tn; a.T_virt = Tn; a.Cin = cg; a.Cout = cg; a.taps = 31; a.pad = 15;
    a.ldx = D; a.ldw = 31 * cg; a.ldy = D; a.ldr = D; a.post_act = ACT_MISH;
    a.Z = 16; a.xz = cg; a.wz = (long long)cg * 31 * cg; a.yz = cg; a.bz = cg;
    GSV_RC(launch_conv_gemm(c->dtype, a, s));
    a.x = rows(c1, b, D); a.w = c->pos2.w; a.bias = c->pos2.b; a.y = rows(hb, b, D); a.accumulate = 1;   // h += mish(conv2(.))
    GSV_RC(launch_conv_gemm(c->dtype, a, s));
  }
  // ---- DiT blocks (modules.py:550-594)
  for (int l = 0; l < g.depth; ++l) {
    const DitBlockW& blk = c->blocks[l];
    const float* m = mods.blk + (size_t)l * mods.blk_stride;   // shift_a, scale_a, gate_a, shift_m, scale_m, gate_m
    GSV_RC(launch_ln_mod<T>(hb, m + D, m, R, D, nrm, s, pr, 6 * D));
    const int wnt = l >= resident ? 1 : 0;
    ConvOpt oq; oq.w_nt = wnt;   // rotary + V^T as this GEMM's epilogue was tried: no gain over the V^T launch
    GSV_RC(conv(c, s, blk.qkv, nrm, D, R, qkv, R, oq));
    if (max_rp)
      GSV_RC(launch_lora_delta(c->dtype, nrm, qkv, Tn, DB, D, 3 * inner, 3, row_slot, slot_ld, c->lora_tab, max_rp, l * lora_blk,
                               l * lora_blk + 3 * D, nullptr, s));
    if (flash) {   // every utterance in the same two launches (V^T + rotary, attention): the row is a grid dimension
      const _Float16* qb = (const _Float16*)qkv;
      GSV_RC(launch_flash_attn64_f16_rows(qb, 3 * inner, qb + inner, 3 * inner, qb + 2 * inner, 3 * inner, vtb, Tn, g.heads, att_scale,
                                          ao, inner, s, cs, half, DB, (long long)Tn * 3 * inner, vtz, (long long)Tn * inner));
    } else {
      GSV_LAUNCH(cfm_rope_kernel<T>, cfm_grid(R * half * 2), dim3(256), 0, s, (T*)qkv, 3 * inner, inner, R, Tn, half, cs);
      for (int b = 0; b < DB; ++b) {
        const T* qb = (const T*)rows(qkv, b, 3 * inner);
        GSV_RC(attention(c, s, qb, 3 * inner, 0, qb, 3 * inner, inner, 2 * inner, Tn, Tn, g.heads, g.dim_head, att_scale, nullptr,
                         nullptr, rows(ao, b, inner), inner));
      }
    }
    ConvOpt og; og.gate = m + 2 * D; og.res = hb; og.w_nt = wnt; og.gate_rows = pr; og.gate_ld = pr ? 6 * D : 0;
    GSV_RC(conv(c, s, blk.out, ao, inner, R, hb, R, og));
    if (max_rp)
      GSV_RC(launch_lora_delta(c->dtype, ao, hb, Tn, DB, inner, D, 1, row_slot, slot_ld, c->lora_tab, max_rp,
                               l * lora_blk + 3 * D + 3 * inner, l * lora_blk + 3 * D + 4 * inner, m + 2 * D, s, pr ? 6 * D : 0));
    GSV_RC(launch_ln_mod<T>(hb, m + 4 * D, m + 3 * D, R, D, nrm, s, pr, 6 * D));
    ConvOpt of; of.post_act = ACT_GELU_TANH; of.w_nt = wnt;
    GSV_RC(conv(c, s, blk.ff1, nrm, D, R, ff, R, of));
    ConvOpt o2; o2.gate = m + 5 * D; o2.res = hb; o2.w_nt = wnt; o2.gate_rows = pr; o2.gate_ld = pr ? 6 * D : 0;
    GSV_RC(conv(c, s, blk.ff2, ff, FF, R, hb, R, o2));
  }
  // ---- AdaLayerNormZero_Final (scale, shift) + proj_out (models.py:1080)
  GSV_RC(launch_ln_mod<T>(hb, mods.fin, mods.fin + D, R, D, nrm, s, pr, 2 * D));
  ConvOpt ov; ov.out_f32 = 1;
  GSV_RC(conv(c, s, c->proj_out, nrm, D, R, v, R, ov));
  return GSV_OK;
}

template int modulations<_Float16>(gsv_cfm*, hipStream_t, int, float**);
template int modulations<float>(gsv_cfm*, hipStream_t, int, float**);
template int text_stack<_Float16>(gsv_cfm*, hipStream_t, const float*, int, int, int, void*, void*, void*, float*);
template int text_stack<float>(gsv_cfm*, hipStream_t, const float*, int, int, int, void*, void*, void*, float*);
template int dit_forward<_Float16>(gsv_cfm*, hipStream_t, const void*, int, int, const DitMods&, const int*, int, int, const float*, float*);
template int dit_forward<float>(gsv_cfm*, hipStream_t, const void*, int, int, const DitMods&, const int*, int, int, const float*, float*);

int rows_upload(hipStream_t s, const CfmRow* host, int n, CfmRow* dev) {
  for (int b0 = 0; b0 < n; b0 += CFM_ROW_CHUNK) {
    const int m = std::min(CFM_ROW_CHUNK, n - b0);
    CfmRowChunk ch{};
    std::copy_n(host + b0, m, ch.r);
    GSV_LAUNCH(cfm_rows_fill_kernel, dim3(1), dim3(CFM_ROW_CHUNK), 0, s, ch, m, dev + b0);
  }
  return GSV_OK;
}

int rope_table(hipStream_t s, int Tn, int half, float* cs) {
  GSV_LAUNCH(cfm_rope_table_kernel, cfm_grid(Tn * half), dim3(256), 0, s, Tn, half, cs);
  return GSV_OK;
}

int init_x(hipStream_t s, const float* noise, const CfmRow* rw, float temperature, int Tn, int C, int B, float* x) {
  GSV_LAUNCH(cfm_init_x_kernel, cfm_grid((long long)Tn * C, B), dim3(256), 0, s, noise, rw, temperature, Tn, C, x);
  return GSV_OK;
}

}  // namespace gsvcfm

namespace {

// B utterances of Tn frames: mu [B][Tn][text_dim] fp32, noise [B][mel][Tn] fp32 or null -> out [B][mel][Tn] fp32; `host_rows`
// holds every utterance's own prompt ([mel][Tp_b] fp32, device), prompt length and noise key.  All row-wise work (Linear
// layers, AdaLN, rotary, Euler) runs over the B * Tn rows at once, which is what fills the chip and reads the 370 MB of
// weights once per step instead of once per chunk.  The ops that look along time (depthwise convs, GRN, fused attention)
// take the utterance as a grid dimension: one launch for all of them.  Only the two grouped position convs and the
// materialised attention (the parity path) are issued per utterance.
//
// Classifier-free guidance (cfg_rate > CFM_CFG_THRESHOLD, models.py:1063-1081): the DiT runs over 2 B rows.  Rows [0, B) are
// the requests as above; row B + b is request b's unconditioned twin -- the same x columns, zero cond columns, and the null
// text embedding (the text stack run on ONE extra row of zero text, then copied into every twin: it depends on Tn alone).
// The Euler state, the noise draw and the output stay B rows; cfm_euler_kernel<T, true> combines the two estimates.  Unguided,
// DB == B and every launch below is the one it was.
template <typename T>
int cfm_infer_batch(gsv_cfm* c, hipStream_t s, const float* mods, const float* mu, const std::vector<CfmRow>& host_rows, int Tn, int N,
                    const float* noise, float temperature, float cfg_rate, int max_rp, float* out) {
  const auto& g = c->cfg;
  const int D = g.dim, td = g.text_dim, md = g.mel_dim, ldin = c->ldin;
  const int half = g.dim_head / 2;
  const size_t es = sizeof(T);
  const bool guided = cfg_rate > CFM_CFG_THRESHOLD;
  const int B = (int)host_rows.size();        // requests: rows of x, noise and out
  const int DB = guided ? 2 * B : B;          // rows the DiT sees
  const int TB = guided ? B + 1 : B;          // rows of the text stack: the requests, then the null text row
  const int RX = B * Tn, R = DB * Tn;
  std::vector<CfmRow> with_twins;             // guided only: the requests' entries, then one per twin
  if (guided) {
    with_twins = host_rows;
    for (int b = 0; b < B; ++b) with_twins.push_back(CfmRow{nullptr, 0ull, host_rows[b].Tp, host_rows[b].slot});
  }
  const std::vector<CfmRow>& table = guided ? with_twins : host_rows;
  CfmRow* rw;
  GSV_RC(need(c, "cfm_rows", (size_t)DB * sizeof(CfmRow), (void**)&rw));
  GSV_RC(rows_upload(s, table.data(), DB, rw));
  float *x, *v, *cs, *gx;
  void *xin, *ta, *tb, *tw;
  GSV_RC(need(c, "cfm_x", (size_t)RX * md * 4, (void**)&x));
  GSV_RC(need(c, "cfm_v", (size_t)R * md * 4, (void**)&v));
  GSV_RC(need(c, "cfm_cs", (size_t)Tn * half * 2 * 4, (void**)&cs));
  GSV_RC(need(c, "cfm_gx", (size_t)TB * 2 * td * 4, (void**)&gx));
  GSV_RC(need(c, "cfm_xin", (size_t)R * ldin * es, &xin));
  GSV_RC(need(c, "cfm_ta", (size_t)R * td * es, &ta));
  GSV_RC(need(c, "cfm_tb", (size_t)R * td * es, &tb));
  GSV_RC(need(c, "cfm_tw", (size_t)R * 2 * td * es, &tw));
  auto rows = [&](void* p, int b, int width) { return (void*)((char*)p + (size_t)b * Tn * width * es); };

  // ---- per-utterance constants: text embedding (dit.py:50-72), cond columns, rotary table
  GSV_RC(text_stack<T>(c, s, mu, B, TB, Tn, ta, tb, tw, gx));
  {
    const int W = md + (ldin - (2 * md + td));
    GSV_LAUNCH(cfm_cond_kernel<T>, cfm_grid((long long)Tn * W, DB), dim3(256), 0, s, rw, Tn, md, (T*)xin, ldin, md, 2 * md + td);
    GSV_LAUNCH(cfm_copy_cols_kernel<T>, cfm_grid((long long)RX * td), dim3(256), 0, s, (const T*)ta, td, RX, td, (T*)xin, ldin, 2 * md);
    if (guided)   // text row B of ta is the null text embedding: into the text columns of the B twins
      GSV_LAUNCH(cfm_bcast_cols_kernel<T>, cfm_grid((long long)Tn * td, B), dim3(256), 0, s, (const T*)rows(ta, B, td), Tn, td,
                 (T*)rows(xin, B, ldin), ldin, 2 * md);
  }
  GSV_RC(rope_table(s, Tn, half, cs));
  GSV_RC(init_x(s, noise, rw, temperature, Tn, md, B, x));
  // x -> the x columns of the DiT input (v null: no update yet), and after every step the Euler update
  auto euler = [&](const float* vv, float dd) -> int {
    auto launch = [&](auto G) -> int {
      GSV_LAUNCH((cfm_euler_kernel<T, decltype(G)::value>), cfm_grid((long long)RX * md), dim3(256), 0, s, x, vv, dd, cfg_rate, RX, Tn, rw, md,
                 (T*)xin, ldin);
      return GSV_OK;
    };
    return guided ? launch(std::true_type{}) : launch(std::false_type{});
  };
  GSV_RC(euler(nullptr, 0.f));

  const float d = (float)(1.0 / N);
  const int* row_slot = (const int*)((const char*)rw + offsetof(CfmRow, slot));   // device: row b's slot, every slot_ld ints
  const int slot_ld = (int)(sizeof(CfmRow) / sizeof(int));
  for (int step = 0; step < N; ++step) {
    DitMods m;   // this step's vectors: block l's at mods[l][step], the final layer's at mods[depth][step]
    m.blk = mods + (size_t)step * 6 * D; m.blk_stride = (size_t)N * 6 * D;
    m.fin = mods + (size_t)g.depth * N * 6 * D + (size_t)step * 2 * D;
    GSV_RC(dit_forward<T>(c, s, xin, DB, Tn, m, row_slot, slot_ld, max_rp, cs, v));
    GSV_RC(euler(v, d));   // models.py:1082-1084
  }
  GSV_LAUNCH(cfm_out_kernel, cfm_grid((long long)Tn * md, B), dim3(256), 0, s, x, rw, Tn, md, out);
  return GSV_OK;
}

template <typename T>
int cfm_run(gsv_cfm* c, hipStream_t s, const float* mu, const std::vector<CfmRow>& rows, int Tn, int N, const float* noise,
            float temperature, float cfg_rate, int max_rp, float* out) {
  float* mods = nullptr;
  GSV_RC(modulations<T>(c, s, N, &mods));
  return cfm_infer_batch<T>(c, s, mods, mu, rows, Tn, N, noise, temperature, cfg_rate, max_rp, out);
}

// What the entry points share: the argument checks, the row table (row b: its own prompt, prompt length, noise key and
// adapter slot; `adapters` null = every row the base model), all before anything is launched, then the pass.  `who` names
// the entry point in the messages.
int cfm_entry(gsv_cfm* c, const char* who, const float* mu, const float* const* prompts, const int* Tp, const int* adapters, int B,
              int Tn, int n_steps, const float* noise, const uint64_t* seeds, float temperature, float cfg_rate, float* out,
              gsv_stream_t stream) {
  GSV_REQUIRE(c && c->finalized, "%s: handle not finalized", who);
  GSV_REQUIRE(!session_open(c), "%s: a flow-matching session is open on this handle and owns its workspace (gsv_cfm_session_end first)", who);
  GSV_REQUIRE(mu && out && Tp && B > 0 && Tn > 0 && n_steps > 0 && n_steps <= 1024, "%s: bad argument", who);
  const bool guided = cfg_rate > CFM_CFG_THRESHOLD;           // the DiT then sees every row and its unconditioned twin
  GSV_REQUIRE(B <= 65535 / (guided ? 2 : 1), "%s: %d rows%s exceed the grid's 65535", who, B, guided ? " and their unconditioned twins" : "");
  GSV_REQUIRE(noise || seeds, "%s: neither noise nor seeds given", who);
  std::vector<CfmRow> rows(B);
  int max_rp = 0;
  for (int b = 0; b < B; ++b) {
    GSV_REQUIRE(Tp[b] >= 0 && Tp[b] <= Tn && (Tp[b] == 0 || (prompts && prompts[b])),
                "%s: row %d: prompt length %d does not fit %d frames, or its prompt is null", who, b, Tp[b], Tn);
    const int slot = adapters ? adapters[b] : -1;
    GSV_REQUIRE(slot >= -1 && slot < GSV_CFM_MAX_ADAPTERS, "%s: row %d: adapter slot %d is outside [-1, %d)", who, b, slot,
                GSV_CFM_MAX_ADAPTERS);
    if (slot >= 0) {
      GSV_REQUIRE(slot < (int)c->adapters.size() && c->adapters[slot].dev, "%s: row %d: no adapter in slot %d", who, b, slot);
      max_rp = std::max(max_rp, c->adapters[slot].rp);
    }
    rows[b] = CfmRow{Tp[b] ? prompts[b] : nullptr, seeds ? (unsigned long long)seeds[b] : 0ull, Tp[b], slot};
  }
  return GSV_WITH_T(c, cfm_run<T>(c, (hipStream_t)stream, mu, rows, Tn, n_steps, noise, temperature, cfg_rate, max_rp, out));
}

}  // namespace

extern "C" {

int gsv_cfm_create(const gsv_dit_config* cfg, int dtype, gsv_cfm_t** out) {
  GSV_REQUIRE(cfg && out, "cfm_create: null argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "cfm_create: bad dtype");
  GSV_REQUIRE(cfg->dim > 0 && cfg->dim % 16 == 0 && (cfg->dim / 16) % 8 == 0, "cfm_create: dim=%d must be a multiple of 128", cfg->dim);
  GSV_REQUIRE(cfg->dim == 128 || cfg->dim == 256 || cfg->dim == 512 || cfg->dim == 1024 || cfg->dim == 2048,
              "cfm_create: dim=%d must be 128, 256, 512, 1024 or 2048 (row-in-registers LayerNorm)", cfg->dim);
  GSV_REQUIRE(cfg->dim_head % 16 == 0 && cfg->heads > 0 && cfg->depth > 0, "cfm_create: bad head configuration");
  GSV_REQUIRE(cfg->text_dim % 8 == 0 && cfg->mel_dim % 4 == 0 && cfg->ff_mult > 0 && cfg->conv_layers >= 0, "cfm_create: bad dims");
  GSV_RC(require_device());
  gsv_cfm* c = new gsv_cfm();
  c->cfg = *cfg;
  c->dtype = dtype;
  const char* e = getenv("GSV_CFM_MATERIALIZED_ATTN");
  c->materialized_attn = e && e[0] == '1';
  *out = c;
  return GSV_OK;
}

void gsv_cfm_destroy(gsv_cfm_t* c) {
  if (!c) return;
  for (auto& a : c->adapters) if (a.dev) (void)hipFree(a.dev);
  if (c->lora_tab) (void)hipFree(c->lora_tab);
  session_destroy(c);
  free_ctx(c);
  delete c;
}

int gsv_cfm_load_tensor(gsv_cfm_t* c, const char* name, const float* data, int64_t numel) {
  return stage_tensor(c, name, data, numel);
}

int gsv_cfm_finalize(gsv_cfm_t* c) {
  GSV_REQUIRE(c && !c->finalized, "cfm_finalize: bad handle");
  const auto& g = c->cfg;
  const int D = g.dim, td = g.text_dim, md = g.mel_dim, inner = g.heads * g.dim_head;
  GSV_RC(make_conv(c, "time_embed.time_mlp.0", D, 256, 1, true, &c->t0));
  GSV_RC(make_conv(c, "time_embed.time_mlp.2", D, D, 1, true, &c->t2));
  GSV_RC(make_conv(c, "d_embed.time_mlp.0", D, 256, 1, true, &c->d0));
  GSV_RC(make_conv(c, "d_embed.time_mlp.2", D, D, 1, true, &c->d2));
  c->text.resize(g.conv_layers);
  for (int i = 0; i < g.conv_layers; ++i) {
    const std::string p = "text_embed.text_blocks." + std::to_string(i) + ".";
    TextBlockW& b = c->text[i];
    GSV_RC(make_vec(c, p + "dwconv.weight", (size_t)td * 7, &b.dw));
    GSV_RC(make_vec(c, p + "dwconv.bias", td, &b.db));
    GSV_RC(make_vec(c, p + "norm.weight", td, &b.ng));
    GSV_RC(make_vec(c, p + "norm.bias", td, &b.nb));
    GSV_RC(make_conv(c, p + "pwconv1", 2 * td, td, 1, true, &b.pw1));
    GSV_RC(make_vec(c, p + "grn.gamma", (size_t)2 * td, &b.gg));
    GSV_RC(make_vec(c, p + "grn.beta", (size_t)2 * td, &b.gb));
    GSV_RC(make_conv(c, p + "pwconv2", td, 2 * td, 1, true, &b.pw2));
  }
  const int cin = 2 * md + td;
  c->ldin = (cin + 31) / 32 * 32;
  GSV_RC(make_conv_padded(c, "input_embed.proj", D, cin, c->ldin, 1, true, &c->in_proj));
  GSV_RC(make_conv(c, "input_embed.conv_pos_embed.conv1d.0", D, D / 16, 31, true, &c->pos1));
  GSV_RC(make_conv(c, "input_embed.conv_pos_embed.conv1d.2", D, D / 16, 31, true, &c->pos2));
  c->blocks.resize(g.depth);
  for (int i = 0; i < g.depth; ++i) {
    const std::string p = "transformer_blocks." + std::to_string(i) + ".";
    DitBlockW& b = c->blocks[i];
    GSV_RC(make_conv(c, p + "attn_norm.linear", 6 * D, D, 1, true, &b.mod));
    GSV_RC(make_stacked(c, {p + "attn.to_q", p + "attn.to_k", p + "attn.to_v"}, inner, D, &b.qkv));
    GSV_RC(make_conv(c, p + "attn.to_out.0", D, inner, 1, true, &b.out));
    GSV_RC(make_conv(c, p + "ff.ff.0.0", D * g.ff_mult, D, 1, true, &b.ff1));
    GSV_RC(make_conv(c, p + "ff.ff.2", D, D * g.ff_mult, 1, true, &b.ff2));
  }
  GSV_RC(make_conv(c, "norm_out.linear", 2 * D, D, 1, true, &c->final_mod));
  GSV_RC(make_conv(c, "proj_out", md, D, 1, true, &c->proj_out));
  // precompute_freqs_cis(text_dim, 4096) (modules.py:127-137): [pos][cos(pos f_j) | sin(pos f_j)]
  {
    std::vector<float> tab((size_t)4096 * td);
    const int half = td / 2;
    std::vector<float> fr(half);
    for (int j = 0; j < half; ++j) fr[j] = 1.0f / powf(10000.0f, (float)(2 * j) / (float)td);
    for (int p = 0; p < 4096; ++p)
      for (int j = 0; j < half; ++j) {
        const float a = (float)p * fr[j];
        tab[(size_t)p * td + j] = cosf(a);
        tab[(size_t)p * td + half + j] = sinf(a);
      }
    GSV_RC(up_f32(c, tab.data(), tab.size(), &c->pos_table));
  }
  c->staged.clear();
  c->finalized = true;
  return GSV_OK;
}

int gsv_cfm_inference(gsv_cfm_t* c, const float* mu, const float* prompt, int B, int T, int Tp, int n_steps, const float* noise,
                      float temperature, uint64_t seed, float* out, gsv_stream_t stream) {
  // the uniform table: row b's prompt is slab b of `prompt`, its noise key is derived from `seed`.  A call that cfm_entry
  // rejects before it reads a row (no handle, B out of range) gets an empty one.
  const int n = c && B > 0 && B <= 65535 ? B : 0;
  std::vector<const float*> prompts(n);
  std::vector<int> tps(n, Tp);
  std::vector<uint64_t> seeds(n);
  for (int b = 0; b < n; ++b) {
    prompts[b] = prompt && Tp > 0 ? prompt + (size_t)b * c->cfg.mel_dim * Tp : nullptr;
    seeds[b] = seed + 0x9E3779B97F4A7C15ull * (uint64_t)b;
  }
  return cfm_entry(c, "cfm_inference", mu, prompts.data(), tps.data(), nullptr, B, T, n_steps, noise, seeds.data(), temperature, 0.f, out, stream);
}

int gsv_cfm_inference_rows(gsv_cfm_t* c, const float* mu, const float* const* prompts, const int* Tp, int B, int T, int n_steps,
                           const float* noise, const uint64_t* seeds, float temperature, float* out, gsv_stream_t stream) {
  return cfm_entry(c, "cfm_inference_rows", mu, prompts, Tp, nullptr, B, T, n_steps, noise, seeds, temperature, 0.f, out, stream);
}

int gsv_cfm_inference_guided(gsv_cfm_t* c, const float* mu, const float* const* prompts, const int* Tp, int B, int T, int n_steps,
                             const float* noise, const uint64_t* seeds, float temperature, float cfg_rate, float* out,
                             gsv_stream_t stream) {
  GSV_REQUIRE(std::isfinite(cfg_rate), "cfm_inference_guided: cfg_rate is not finite");
  return cfm_entry(c, "cfm_inference_guided", mu, prompts, Tp, nullptr, B, T, n_steps, noise, seeds, temperature, cfg_rate, out, stream);
}

int gsv_cfm_inference_adapted(gsv_cfm_t* c, const float* mu, const float* const* prompts, const int* Tp, const int* adapters, int B,
                              int T, int n_steps, const float* noise, const uint64_t* seeds, float temperature, float cfg_rate,
                              float* out, gsv_stream_t stream) {
  GSV_REQUIRE(std::isfinite(cfg_rate), "cfm_inference_adapted: cfg_rate is not finite");
  return cfm_entry(c, "cfm_inference_adapted", mu, prompts, Tp, adapters, B, T, n_steps, noise, seeds, temperature, cfg_rate, out, stream);
}

int gsv_cfm_adapter_begin(gsv_cfm_t* c, int rank, float alpha) {
  GSV_REQUIRE(c && c->finalized, "cfm_adapter_begin: handle not finalized");
  GSV_REQUIRE(rank >= 1 && rank <= GSV_LORA_MAX_RANK, "cfm_adapter_begin: rank %d is outside [1, %d]", rank, GSV_LORA_MAX_RANK);
  GSV_REQUIRE(std::isfinite(alpha) && alpha > 0.f, "cfm_adapter_begin: lora_alpha must be positive and finite");
  GSV_REQUIRE((c->cfg.heads * c->cfg.dim_head) % 32 == 0, "cfm_adapter_begin: heads * dim_head = %d must be a multiple of 32",
              c->cfg.heads * c->cfg.dim_head);
  c->a_staged.clear();
  c->a_open = true;
  c->a_rank = rank;
  c->a_alpha = alpha;
  return GSV_OK;
}

int gsv_cfm_adapter_load_tensor(gsv_cfm_t* c, const char* name, const float* data, int64_t numel) {
  GSV_REQUIRE(c && name && data && numel > 0, "cfm_adapter_load_tensor: bad argument");
  GSV_REQUIRE(c->a_open, "cfm_adapter_load_tensor: no adapter_begin before '%s'", name);
  c->a_staged[name].assign(data, data + numel);
  return GSV_OK;
}

int gsv_cfm_adapter_finalize(gsv_cfm_t* c, int* slot_out) {
  GSV_REQUIRE(c && slot_out, "cfm_adapter_finalize: null argument");
  GSV_REQUIRE(c->a_open, "cfm_adapter_finalize: no adapter_begin");
  // whatever happens below, the staged adapter is gone afterwards; the store changes only at the very end
  std::map<std::string, std::vector<float>> staged;
  staged.swap(c->a_staged);
  c->a_open = false;
  const auto& g = c->cfg;
  const int D = g.dim, inner = g.heads * g.dim_head, r = c->a_rank, rp = (r + 15) / 16 * 16;
  const float scale = c->a_alpha / (float)r;
  GSV_REQUIRE((int)staged.size() == 8 * g.depth, "cfm_adapter_finalize: %zu tensors staged, a rank-%d adapter of this DiT has %d", staged.size(),
              r, 8 * g.depth);
  int slot = -1;
  for (size_t i = 0; i < c->adapters.size() && slot < 0; ++i)
    if (!c->adapters[i].dev) slot = (int)i;
  if (slot < 0) slot = (int)c->adapters.size();
  GSV_REQUIRE(slot < GSV_CFM_MAX_ADAPTERS, "cfm_adapter_finalize: all %d adapter slots are in use", GSV_CFM_MAX_ADAPTERS);
  const size_t per_block = (size_t)4 * (D + inner) * rp, total = per_block * g.depth;
  std::vector<float> host(total, 0.f);
  // lora_A [r][in] -> rows [row0, row0 + r) of a [.][in] matrix; lora_B [out][r] -> columns [0, r) of [out][rp], scaled
  auto put = [&](const std::string& name, bool is_b, int n_in_or_out, float* dst) -> int {
    auto it = staged.find(name);
    GSV_REQUIRE(it != staged.end(), "cfm_adapter_finalize: '%s' is missing", name.c_str());
    GSV_REQUIRE(it->second.size() == (size_t)r * n_in_or_out, "cfm_adapter_finalize: '%s' has %zu elements, expected %d x %d", name.c_str(),
                it->second.size(), is_b ? n_in_or_out : r, is_b ? r : n_in_or_out);
    const float* src = it->second.data();
    if (!is_b) std::copy(src, src + (size_t)r * n_in_or_out, dst);
    else
      for (int o = 0; o < n_in_or_out; ++o)
        for (int q = 0; q < r; ++q) dst[(size_t)o * rp + q] = scale * src[(size_t)o * r + q];
    return GSV_OK;
  };
  for (int l = 0; l < g.depth; ++l) {
    const std::string p = "transformer_blocks." + std::to_string(l) + ".attn.";
    float* blk = host.data() + (size_t)l * per_block;
    const char* qkv_names[3] = {"to_q", "to_k", "to_v"};
    for (int j = 0; j < 3; ++j) {
      GSV_RC(put(p + qkv_names[j] + ".lora_A", false, D, blk + (size_t)j * rp * D));
      GSV_RC(put(p + qkv_names[j] + ".lora_B", true, inner, blk + (size_t)3 * D * rp + (size_t)j * inner * rp));
    }
    GSV_RC(put(p + "to_out.0.lora_A", false, inner, blk + (size_t)(3 * D + 3 * inner) * rp));
    GSV_RC(put(p + "to_out.0.lora_B", true, D, blk + (size_t)(3 * D + 4 * inner) * rp));
  }
  const size_t es = dt_size(c->dtype);
  void* dev = nullptr;
  GSV_HIP(hipMalloc(&dev, total * es));
  hipError_t e;
  if (c->dtype == GSV_F32) e = hipMemcpy(dev, host.data(), total * 4, hipMemcpyHostToDevice);
  else {
    std::vector<_Float16> tmp(total);
    for (size_t i = 0; i < total; ++i) tmp[i] = (_Float16)host[i];
    e = hipMemcpy(dev, tmp.data(), total * 2, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && !c->lora_tab) {
    e = hipMalloc((void**)&c->lora_tab, sizeof(LoraSlot) * GSV_CFM_MAX_ADAPTERS);
    if (e == hipSuccess) e = hipMemset(c->lora_tab, 0, sizeof(LoraSlot) * GSV_CFM_MAX_ADAPTERS);
  }
  const LoraSlot entry{dev, rp, 0};
  if (e == hipSuccess) e = hipMemcpy(c->lora_tab + slot, &entry, sizeof(entry), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    set_error("cfm_adapter_finalize: upload failed: %s", hipGetErrorString(e));
    return GSV_ERR_HIP;
  }
  if (slot == (int)c->adapters.size()) c->adapters.emplace_back();
  c->adapters[slot] = CfmAdapter{dev, r, rp};
  *slot_out = slot;
  return GSV_OK;
}

int gsv_cfm_adapter_remove(gsv_cfm_t* c, int slot) {
  GSV_REQUIRE(c, "cfm_adapter_remove: null handle");
  GSV_REQUIRE(slot >= 0 && slot < (int)c->adapters.size() && c->adapters[slot].dev, "cfm_adapter_remove: no adapter in slot %d", slot);
  GSV_REQUIRE(!session_uses_adapter(c, slot), "cfm_adapter_remove: a live row of the open session runs with slot %d (fetch or release it first)", slot);
  GSV_HIP(hipDeviceSynchronize());   // nothing may still read the block
  (void)hipFree(c->adapters[slot].dev);
  c->adapters[slot] = CfmAdapter{};
  return GSV_OK;
}

int gsv_cfm_adapter_count(gsv_cfm_t* c) {
  GSV_REQUIRE(c, "cfm_adapter_count: null handle");
  int n = 0;
  for (const auto& a : c->adapters) n += a.dev != nullptr;
  return n;
}

}  // extern "C"
