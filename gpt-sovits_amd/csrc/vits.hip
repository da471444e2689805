// SoVITS engine (H6-H12) for gfx950: the v1/v2 waveform decoder (gsv_vits_decode, gsv_vits_decode_segments), the v3/v4
// semantic path up to the CFM features (gsv_vits_decode_encp), the reference encoder and extract_latent.  The generator's
// upsampling stages and the vocoders of the v3/v4 path are in generator.hip.
//
// Every activation is channels-last [time][channel] in the engine dtype, so every conv /
// 1x1 / Linear / attention product is one call of the MFMA implicit-GEMM kernel
// (conv_gemm.hip).  Fusions: leaky-relu applied on operand load, bias / residual / scale /
// accumulate / tanh in the epilogue (ResBlock1 adds and the MRF mean never run as separate
// passes), transposed convs as polyphase convs with a scatter epilogue, weight-norm folded
// once at load (the reference re-materialises it every forward), speaker-conditioning
// terms (cond(ge), WN cond_layer(ge)) folded into biases once per reference audio.
// gsv_vits_decode takes a single sequence (the reference, TTS.py:1266-1273, folds the batch into
// the time axis), so its x_mask terms are identically one and are dropped.  The two paths that do
// mask say so where they do: the segmented decode (several sequences on one time axis, the gap
// rows between them kept at zero by row maps) and wns1 of decode_encp (frames >= Lm zeroed).
// Host functions that launch typed kernels are templates on the element type T, picked once per
// entry point (GSV_WITH_T); every launch is written once (GSV_LAUNCH).
#include "engine.h"

#include <algorithm>
#include <utility>

#include "align.h"

namespace gsv {

// ---------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void gather_rows_kernel(const int* __restrict__ idx, const float* __restrict__ table, int C, int rep, int n,
                                   T* __restrict__ out) {
  // out[(i*rep + r)][c] = table[idx[i]][c]
  const int row = blockIdx.x;
  if (row >= n * rep) return;
  const float* src = table + (long long)idx[row / rep] * C;
  T* dst = out + (long long)row * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = (T)src[c];
}

// segmented decode: out[row][c] = table[ids[src[row]]][c], or 0 for a gap row (src[row] < 0)
template <typename T>
__global__ void gather_seg_kernel(const int* __restrict__ ids, const int* __restrict__ src, const float* __restrict__ table, int C,
                                  int rows, T* __restrict__ out) {
  const int row = blockIdx.x;
  if (row >= rows) return;
  const int i = src[row];
  T* dst = out + (long long)row * C;
  if (i < 0) { for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = (T)0.f; return; }
  const float* sp = table + (long long)ids[i] * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = (T)sp[c];
}

// per-segment bias table: out[s][:] = slots[slot_of[s]][:]
__global__ void gather_voice_kernel(const float* __restrict__ slots, const int* __restrict__ slot_of, int vs, float* __restrict__ out) {
  const int sg = blockIdx.x;
  const float* src = slots + (long long)slot_of[sg] * vs;
  for (int i = threadIdx.x; i < vs; i += blockDim.x) out[(long long)sg * vs + i] = src[i];
}

// T channels-last [T][ld] (cols col0..col0+C) -> fp32 channels-first [C][T]
template <typename TS>
__global__ void cl_to_cf_kernel(const TS* __restrict__ src, int Tn, int ld, int col0, int C, float* __restrict__ dst) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  int c = (int)(i / Tn), t = (int)(i % Tn);
  dst[i] = to_f(src[(long long)t * ld + col0 + c]);
}

// acts[t][c] = tanh(a[t][c]) * sigmoid(a[t][H + c])      (commons.py:96-103)
template <typename T>
__global__ void gate_kernel(const T* __restrict__ a, long long n, int H, T* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long t = i / H; int c = (int)(i - t * H);
  float x = to_f(a[t * 2 * H + c]), y = to_f(a[t * 2 * H + H + c]);
  out[i] = (T)(tanhf(x) * (1.f / (1.f + expf(-y))));
}

// x[t][c] += y[t][c] * sigmoid(y[t][H + c])                 (Conv1dGLU, modules.py:551-557)
template <typename T>
__global__ void glu_res_kernel(const T* __restrict__ y, long long n, int H, T* __restrict__ x) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long t = i / H; int c = (int)(i - t * H);
  float a = to_f(y[t * 2 * H + c]), b = to_f(y[t * 2 * H + H + c]);
  x[i] = (T)(to_f(x[i]) + a * (1.f / (1.f + expf(-b))));
}

template <typename T>
__global__ void flip_channels_kernel(const T* __restrict__ src, long long n, int C, T* __restrict__ dst) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long t = i / C; int c = (int)(i - t * C);
  dst[i] = src[t * C + (C - 1 - c)];
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// z_p[t][c] = m + noise * exp(logs) * scale   (models.py:1000); noise fp32 channels-first or counter RNG
// segmented decode (seg != null): a gap row is 0; segment s draws with its own seeds[s] and segment-local element index, and
// reads explicit noise [C][Fn] (segments packed without gaps) at column noff[s] + local frame -- each segment's noise is the
// one its own gsv_vits_decode would draw
template <typename T>
__global__ void zp_kernel(const float* __restrict__ stats, int F, int C, const float* __restrict__ noise, float scale,
                          unsigned long long seed, T* __restrict__ z, const int* __restrict__ seg, const int* __restrict__ start,
                          const int* __restrict__ noff, const unsigned long long* __restrict__ seeds, int Fn) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)F * C) return;
  int t = (int)(i / C), c = (int)(i - (long long)t * C);
  float m = stats[(long long)t * 2 * C + c], ls = stats[(long long)t * 2 * C + C + c];
  int tn = t, ldn = F;
  if (seg) {
    const int sg = seg[t];
    if (sg < 0) { z[i] = (T)0.f; return; }
    const int tl = t - start[sg];
    seed = seeds[sg];
    tn = noff[sg] + tl; ldn = Fn;
    i = (long long)tl * C + c;
  }
  float n;
  if (noise) n = noise[(long long)c * ldn + tn];
  else {
    unsigned long long h1 = mix64(seed ^ mix64((unsigned long long)i * 2 + 1)), h2 = mix64(seed ^ mix64((unsigned long long)i * 2 + 2));
    float u1 = ((float)(h1 >> 40) + 1.0f) * (1.0f / 16777217.0f), u2 = (float)(h2 >> 40) * (1.0f / 16777216.0f);
    n = sqrtf(-2.f * logf(u1)) * cosf(6.28318530718f * u2);
  }
  z[(long long)t * C + c] = (T)(m + n * expf(ls) * scale);
}

// out[c] (+)= mean_t x[t][c] * wgt
template <typename T>
__global__ void mean_time_kernel(const T* __restrict__ x, int Tn, int C, float wgt, int accumulate, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int t = 0; t < Tn; ++t) s += to_f(x[(long long)t * C + c]) / (float)Tn;
  out[c] = (accumulate ? out[c] : 0.f) + s * wgt;
}

// F.interpolate(mode="linear", align_corners=False) along time on channels-last rows (models.py:226-228)
template <typename T>
__global__ void interp_linear_kernel(const T* __restrict__ x, int Tin, int Tout, int C, T* __restrict__ y) {
  const int t = blockIdx.x;
  const float scale = (float)Tin / (float)Tout;
  float src = scale * ((float)t + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  const int i0 = min((int)src, Tin - 1);
  const int i1 = min(i0 + 1, Tin - 1);
  const float w1 = src - (float)i0, w0 = 1.f - w1;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    y[(long long)t * C + c] = (T)(w0 * to_f(x[(long long)i0 * C + c]) + w1 * to_f(x[(long long)i1 * C + c]));
}

// segmented decode with per-segment speeds: interp_linear_kernel per segment.  x holds the pre layout (segment s: Tin = len_in[s]
// rows from row start_in[s]), y the post layout (Tout = len_out[s] rows from row start_out[s]); seg_out names the segment of every
// post row, -1 = gap (written as zeros).  Same arithmetic as above with the segment's own Tin / Tout: the clamps of i0 / i1 keep
// every read inside the segment's pre rows.  Tin == Tout (speed 1) copies the row.
template <typename T>
__global__ void interp_linear_seg_kernel(const T* __restrict__ x, const int* __restrict__ seg_out, const int* __restrict__ start_in,
                                         const int* __restrict__ len_in, const int* __restrict__ start_out,
                                         const int* __restrict__ len_out, int rows, int C, T* __restrict__ y) {
  const int row = blockIdx.x;
  if (row >= rows) return;
  T* dst = y + (long long)row * C;
  const int sg = seg_out[row];
  if (sg < 0) { for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = (T)0.f; return; }
  const int t = row - start_out[sg], Tin = len_in[sg], Tout = len_out[sg];
  const T* xs = x + (long long)start_in[sg] * C;
  if (Tin == Tout) { for (int c = threadIdx.x; c < C; c += blockDim.x) dst[c] = xs[(long long)t * C + c]; return; }
  const float scale = (float)Tin / (float)Tout;
  float src = scale * ((float)t + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  const int i0 = min((int)src, Tin - 1);
  const int i1 = min(i0 + 1, Tin - 1);
  const float w1 = src - (float)i0, w0 = 1.f - w1;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    dst[c] = (T)(w0 * to_f(xs[(long long)i0 * C + c]) + w1 * to_f(xs[(long long)i1 * C + c]));
}

// F.interpolate(mode="nearest", scale_factor=sf) along time: src = min(floor(dst * (float)(1/sf)), Tin - 1)
template <typename T>
__global__ void interp_nearest_kernel(const T* __restrict__ x, int Tin, int Tout, int C, float scale, T* __restrict__ y) {
  const int t = blockIdx.x;
  const int src = min((int)floorf((float)t * scale), Tin - 1);
  for (int c = threadIdx.x; c < C; c += blockDim.x) y[(long long)t * C + c] = x[(long long)src * C + c];
}

// v2Pro: ge (+)= PReLU(ge_ref + sv_proj) * wgt   (module/models.py:971-975, then the mean over references)
__global__ void sv_prelu_acc_kernel(const float* __restrict__ ge_ref, const float* __restrict__ sv_proj, const float* __restrict__ a,
                                    float wgt, int accumulate, int n, float* __restrict__ ge) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = ge_ref[i] + sv_proj[i];
  const float u = (v >= 0.f ? v : a[i] * v) * wgt;
  ge[i] = accumulate ? ge[i] + u : u;
}

__global__ void vec_add_kernel(const float* a, const float* b, float* out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// nearest codeword: argmax_j -(xx - 2 x.e_j + ee_j)   (core_vq.py:172-176)
__global__ void argmax_code_kernel(const float* __restrict__ dots, const float* __restrict__ x, const float* __restrict__ ee,
                                   int D, int NB, int* __restrict__ codes) {
  const int t = blockIdx.x, lane = threadIdx.x;
  float xx = 0.f;
  for (int c = lane; c < D; c += 64) { float v = x[(long long)t * D + c]; xx += v * v; }
  xx = wave_sum(xx);
  float best = -INFINITY; int bi = 0x7fffffff;
  for (int j = lane; j < NB; j += 64) {
    float d = -(xx - 2.f * dots[(long long)t * NB + j] + ee[j]);
    if (d > best) { best = d; bi = j; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_xor(best, o, 64); int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) codes[t] = bi;
}

}  // namespace gsv

using namespace gsv;

// =======================================================================================
// model
// =======================================================================================

struct AttnLayerW { Conv qkv, o; float *rel_k = nullptr, *rel_v = nullptr; float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; Conv f1, f2; };
// modules.WN: per layer in_layers (kernel 5) and res_skip_layers (1x1); in_bias_eff = in_layers bias + cond_layer(ge) (fp32 [2H])
struct WNW { std::vector<Conv> in, res; std::vector<float*> in_bias_eff; Conv cond; };
struct FlowW { Conv pre, post; WNW wn; };

struct gsv_vits : gsveng::Ctx {
  gsv_vits() : Ctx("vits") {}
  gsv_vits_config cfg;
  bool has_ref = false;
  // weights
  Conv ssl_proj_enc, proj, c_pre, text_pre, c_post, mq, mkv, mo;
  std::vector<AttnLayerW> enc_ssl, enc_text, enc2;
  float *text_emb = nullptr, *codebook = nullptr, *code_ee = nullptr;
  Conv top_ssl_proj;
  void* codebook_t = nullptr;
  FlowW flows[4];
  Conv conv_pre, conv_post, cond;
  float* conv_pre_bias_eff = nullptr;
  GenW gen;
  // v3 / v4: bridge + wns1 (Encoder with an 8-layer WN)
  Conv bridge, w1_pre, w1_proj;
  WNW w1;
  // v2Pro: speaker-verification conditioning
  Conv sv_emb, ge_to512;
  float *prelu_w = nullptr, *ge_ref = nullptr, *sv_proj = nullptr, *ge512 = nullptr;
  void* sv_t = nullptr;
  // ref_enc
  Conv r_sp0, r_sp3, r_t0, r_t1, r_qkv, r_fc, r_out;
  float* ge = nullptr;         // fp32 [gin]
  void* ge_t = nullptr;        // T [gin]
  float* mo_bias_eff = nullptr;
  // voice slots of the segmented decode (gsv_vits_store_voice): [GSV_VITS_MAX_VOICES][voice_len] fp32, one row per slot holding
  // mo_bias_eff | conv_pre_bias_eff | the 16 WN in_bias_eff vectors (offsets voice_off_*)
  float* voices = nullptr;
  int voice_len = 0, voice_off_pre = 0, voice_off_in = 0;
  std::vector<char> voice_ok;
  gsveng::SegUpload seg;                        // maps and noise keys of the last segmented decode
  hipStream_t ref_stream = nullptr;             // stream of the last set_refer (store_voice copies on it, then records ev[3])
  gsveng::GenTap dbg_last;                      // input of the last generator stage (intact after a decode) for the debug hook
  // gsv_vits_set_align: the table pending for the next decode (consumed by it), and where its results go
  std::vector<gsv_align_seg_span_t> align_req;
  int32_t* align_ends = nullptr;
  float* align_score = nullptr;
  gsveng::SegUpload align_up;                   // host image of the device span table (maps: 6 ints per span)
  int lastF0 = 0, lastL = 0;                    // rows of m_q / m_kv of the last enc_p (debug hook)
  // last decode bookkeeping
  int lastF = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float last_total_ms = 0.f, last_gen_ms = 0.f;
};

using namespace gsveng;

namespace gsveng {

int make_encoder(gsv_vits* h, const std::string& prefix, int n_layers, std::vector<AttnLayerW>* out) {
  const auto& c = h->cfg;
  const int H = c.hidden_channels, FC = c.filter_channels, kc = H / c.n_heads;
  out->resize(n_layers);
  for (int i = 0; i < n_layers; ++i) {
    AttnLayerW& L = (*out)[i];
    const std::string a = prefix + ".attn_layers." + std::to_string(i) + ".";
    GSV_RC(make_stacked(h, {a + "conv_q", a + "conv_k", a + "conv_v"}, H, H, &L.qkv));
    GSV_RC(make_conv(h, a + "conv_o", H, H, 1, true, &L.o));
    GSV_RC(make_vec(h, a + "emb_rel_k", (size_t)9 * kc, &L.rel_k));
    GSV_RC(make_vec(h, a + "emb_rel_v", (size_t)9 * kc, &L.rel_v));
    GSV_RC(make_vec(h, prefix + ".norm_layers_1." + std::to_string(i) + ".gamma", H, &L.g1));
    GSV_RC(make_vec(h, prefix + ".norm_layers_1." + std::to_string(i) + ".beta", H, &L.b1));
    GSV_RC(make_vec(h, prefix + ".norm_layers_2." + std::to_string(i) + ".gamma", H, &L.g2));
    GSV_RC(make_vec(h, prefix + ".norm_layers_2." + std::to_string(i) + ".beta", H, &L.b2));
    const std::string f = prefix + ".ffn_layers." + std::to_string(i) + ".";
    GSV_RC(make_conv(h, f + "conv_1", FC, H, c.kernel_size, true, &L.f1));
    GSV_RC(make_conv(h, f + "conv_2", H, FC, c.kernel_size, true, &L.f2));
  }
  return GSV_OK;
}

// modules.WN(hidden H, kernel 5, dilation rate 1, NL layers, gin GIN) under `prefix`; the last layer has no residual half
static int make_wn(gsv_vits* h, const std::string& prefix, int NL, int H, int GIN, WNW* w) {
  w->in.resize(NL); w->res.resize(NL); w->in_bias_eff.resize(NL);
  for (int li = 0; li < NL; ++li) {
    GSV_RC(make_conv(h, prefix + ".in_layers." + std::to_string(li), 2 * H, H, 5, true, &w->in[li]));
    GSV_RC(make_conv(h, prefix + ".res_skip_layers." + std::to_string(li), li < NL - 1 ? 2 * H : H, H, 1, true, &w->res[li]));
    GSV_RC(dalloc(h, (void**)&w->in_bias_eff[li], (size_t)2 * H * 4));
  }
  return make_conv(h, prefix + ".cond_layer", 2 * H * NL, GIN, 1, true, &w->cond);
}

// attentions.Encoder.forward (attentions.py:64-84) on x [Tn][H] in place
// segmented decode: row_seg masks the gap rows of what the FFN convs read, kr makes the self-attention block-diagonal
int run_encoder(gsv_vits* h, hipStream_t s, std::vector<AttnLayerW>& layers, void* x, int Tn, const int* row_seg = nullptr,
                const int* kr = nullptr) {
  const auto& c = h->cfg;
  const int H = c.hidden_channels, FC = c.filter_channels, kc = H / c.n_heads;
  const size_t es = esz(h);
  void *qkv, *ao, *y, *ff;
  GSV_RC(need(h, "enc_qkv", (size_t)Tn * 3 * H * es, &qkv));
  GSV_RC(need(h, "enc_ao", (size_t)Tn * H * es, &ao));
  GSV_RC(need(h, "enc_y", (size_t)Tn * H * es, &y));
  GSV_RC(need(h, "enc_ff", (size_t)Tn * FC * es, &ff));
  for (auto& L : layers) {
    ConvOpt o;
    GSV_RC(conv(h, s, L.qkv, x, H, Tn, qkv, Tn, o));
    GSV_RC(attention(h, s, qkv, 3 * H, 0, qkv, 3 * H, H, 2 * H, Tn, Tn, c.n_heads, kc, 1.f / sqrtf((float)kc), L.rel_k, L.rel_v, ao, H, kr));
    GSV_RC(conv(h, s, L.o, ao, H, Tn, y, Tn, o));
    GSV_RC(launch_layernorm(h->dtype, x, 0, y, 0, L.g1, L.b1, x, 0, Tn, H, 1e-5f, s, row_seg));
    ConvOpt o1; o1.post_act = ACT_RELU; o1.row_seg = row_seg;
    GSV_RC(conv(h, s, L.f1, x, H, Tn, ff, Tn, o1));
    GSV_RC(conv(h, s, L.f2, ff, FC, Tn, y, Tn, o));
    GSV_RC(launch_layernorm(h->dtype, x, 0, y, 0, L.g2, L.b2, x, 0, Tn, H, 1e-5f, s, row_seg));
  }
  return GSV_OK;
}

// ---------------------------------------------------------------------------------------
// segmented decode (gsv_vits_decode_segments): n independent sequences back to back on one time axis, G zero "gap" rows
// between neighbours at the frame rate (G * prod(rates[:i]) after upsampling stage i) and G between their phones
// ---------------------------------------------------------------------------------------
// the gap, in frames: at every resolution it covers the reach of each conv reading that resolution, so a conv of a segment row
// reads zeros (its isolated zero padding) wherever it would reach past the segment's edge, and never the neighbour's rows
int seg_gap(const gsv_vits_config& c) {
  int g = 1;
  g = std::max(g, conv_reach(c.kernel_size, 1));   // encoder FFN convs (frame and text axes)
  g = std::max(g, conv_reach(5, 1));               // flow WN in_layers (kernel 5, dilation rate 1)
  GenW shape;
  gen_shape(c, &shape);
  return std::max(g, gen_gap(shape));              // conv_pre, ups, ResBlocks, conv_post: the rule the vocoders share (generator.hip)
}

struct SegLayout {
  int n = 0, G = 0, F = 0, L = 0, Fn = 0;        // frames / phones with gaps; Fn = frames without gaps
  std::vector<int> f0, l0, c0, p0, fn0, nf;      // per segment: first frame / phone row, first packed code / phone, packed frame,
};                                               // frames

// speeds == null: the pre layout, 2 T_s frames per segment (codebook gather, enc_ssl, MRTE, enc2).  With speeds: the post layout,
// F_s frames per segment as the speed interpolation of gsv_vits_decode leaves them (proj onwards); same gap, same phone axis.
int seg_layout(const gsv_vits_config& c, int n, const int* code_lens, const int* phone_lens, const double* speeds, SegLayout* o) {
  GSV_REQUIRE(n >= 1 && n <= 4096 && code_lens && phone_lens, "vits segments: bad segment count %d", n);
  o->n = n; o->G = seg_gap(c);
  o->f0.resize(n); o->l0.resize(n); o->c0.resize(n); o->p0.resize(n); o->fn0.resize(n); o->nf.resize(n);
  long long f = 0, l = 0, cc = 0, pp = 0, fn = 0;
  for (int i = 0; i < n; ++i) {
    GSV_REQUIRE(code_lens[i] >= 1 && phone_lens[i] >= 1, "vits segments: segment %d is empty (%d codes, %d phones)", i, code_lens[i],
                phone_lens[i]);
    GSV_REQUIRE(code_lens[i] < (1 << 23), "vits segments: too long");
    long long fs = 2LL * code_lens[i];
    if (speeds && speeds[i] != 1.0) {
      GSV_REQUIRE(std::isfinite(speeds[i]) && speeds[i] > 0.0, "vits segments: speed of segment %d must be finite and positive", i);
      const double q = (double)fs / speeds[i];
      GSV_REQUIRE(q < (double)(1 << 24), "vits segments: too long");
      fs = (long long)(int)q + 1;
    }
    if (i) { f += o->G; l += o->G; }
    o->f0[i] = (int)f; o->l0[i] = (int)l; o->c0[i] = (int)cc; o->p0[i] = (int)pp; o->fn0[i] = (int)fn; o->nf[i] = (int)fs;
    f += fs; l += phone_lens[i]; cc += code_lens[i]; pp += phone_lens[i]; fn += fs;
    GSV_REQUIRE(f < (1LL << 24) && l < (1LL << 24), "vits segments: too long");
  }
  o->F = (int)f; o->L = (int)l; o->Fn = (int)fn;
  return GSV_OK;
}

// device side of one segmented decode
struct SegRun {
  const SegLayout *lay = nullptr, *post = nullptr;       // pre layout (up to enc2), post layout (after the speed interpolation,
                                                         // proj onwards); post == lay when no segment changes its frame count
  const int *seg_f = nullptr, *seg_l = nullptr;          // segment id per pre frame row / phone row, -1 = gap
  const int* seg_p = nullptr;                            // segment id per post frame row (== seg_f when post == lay)
  const int *kr_f = nullptr, *kr_l = nullptr, *kr_x = nullptr;   // key ranges: frame and text self-attention, MRTE (phones)
  const int *src_code = nullptr, *src_phone = nullptr;   // packed code / phone index per row, -1 = gap
  const int *start = nullptr, *noff = nullptr;           // per segment: first post frame row, first packed noise column
  const int *start_pre = nullptr, *len_pre = nullptr, *len_post = nullptr;   // per segment: first pre row, pre / post frames
  const unsigned long long* seeds = nullptr;
  std::vector<int*> seg_up;                              // segment id per row after each upsampling stage
  const float* bias = nullptr;                           // per-segment voice rows [n][voice_len]
};

// A conv whose bias carries the speaker conditioning, x [F][c.cin] -> y [F][c.cout].  Plain decode: the handle's folded bias.
// Segmented decode: the vector at `voff` of a voice row -- one segment takes its row as the bias; with several, the conv runs
// without bias and a row pass over y adds each segment's own row and zeroes the gap rows (so y must feed nothing in between);
// seg_f is the row map of the layout x is in (sr->seg_f or sr->seg_p).
static int conv_voice(gsv_vits* h, hipStream_t s, const Conv& c, const void* x, int F, void* y, ConvOpt o, const float* handle_bias,
                      const SegRun* sr, size_t voff, const int* seg_f) {
  const float* vrow = sr ? sr->bias + voff : nullptr;
  o.bias_override = sr ? vrow : handle_bias;
  o.no_bias = seg_f != nullptr;
  GSV_RC(conv(h, s, c, x, c.cin, F, y, F, o));
  if (seg_f) GSV_RC(launch_seg_rows(h->dtype, 0, y, c.cout, 0, c.cout, F, seg_f, vrow, h->voice_len, s));
  return GSV_OK;
}

// The pending alignment table (gsv_vits_set_align) in the rows of this pass: span r of segment g covers frames
// f0[g] + 2 code0 .. + 2 n_codes of m_q and phones l0[g] + phone0 .. + n_phones of m_kv (the layout's gap rows included in f0 / l0),
// and writes ends[sum of the n_phones in front of it ..].  Checked before anything is launched; the table is consumed either way.
static int align_prepare(gsv_vits* h, int Tc, int L, const SegRun* sr, std::vector<gsv_align_seg_span_t>* req) {
  req->swap(h->align_req);
  h->align_req.clear();
  const int n = (int)req->size();
  if (!n) return GSV_OK;
  const int nseg = sr ? sr->lay->n : 1;
  GSV_RC(seg_upload_begin(&h->align_up));   // the previous table's upload is done before its host image is rewritten
  std::vector<int>& img = h->align_up.maps;
  img.assign((size_t)n * 6, 0);
  std::vector<std::pair<long long, int>> order(n);
  int out0 = 0;
  for (int r = 0; r < n; ++r) {
    const gsv_align_seg_span_t& a = (*req)[r];
    GSV_REQUIRE(a.segment >= 0 && a.segment < nseg, "vits align: span %d names segment %d of %d", r, a.segment, nseg);
    const int g = a.segment;
    const int codes = sr ? sr->lay->nf[g] / 2 : Tc;
    const int phones = !sr ? L : (g + 1 < nseg ? sr->lay->l0[g + 1] - sr->lay->G : sr->lay->L) - sr->lay->l0[g];
    GSV_REQUIRE(a.code0 >= 0 && a.n_codes >= 0 && a.code0 <= codes && a.n_codes <= codes - a.code0,
                "vits align: span %d covers codes [%d, +%d) of a segment of %d", r, a.code0, a.n_codes, codes);
    GSV_REQUIRE(a.phone0 >= 0 && a.n_phones >= 0 && a.phone0 <= phones && a.n_phones <= phones - a.phone0,
                "vits align: span %d covers phones [%d, +%d) of a segment of %d", r, a.phone0, a.n_phones, phones);
    int* d = &img[(size_t)r * 6];
    d[0] = (sr ? sr->lay->f0[g] : 0) + 2 * a.code0; d[1] = 2 * a.n_codes;
    d[2] = (sr ? sr->lay->l0[g] : 0) + a.phone0;   d[3] = a.n_phones;
    d[4] = out0;
    out0 += a.n_phones;
    order[r] = {(long long)d[2], r};
  }
  std::sort(order.begin(), order.end());
  long long end = -1;   // the furthest end of the non-empty spans so far, and the span that reaches it
  int last = -1;
  for (int i = 0; i < n; ++i) {
    const int b = order[i].second, l0 = img[(size_t)b * 6 + 2], nl = img[(size_t)b * 6 + 3];
    if (nl == 0) continue;             // an empty span holds no phoneme
    GSV_REQUIRE(l0 >= end, "vits align: spans %d and %d overlap in phonemes", last, b);
    end = (long long)l0 + nl;
    last = b;
  }
  return GSV_OK;
}

// the two alignment launches on m_q [F0][MH] / m_kv [L][2 MH] (keys = the first MH columns), read in place
static int align_run(gsv_vits* h, hipStream_t s, int n, const void* q, const void* kv, int MH) {
  const gsv_align_span_t* img = reinterpret_cast<const gsv_align_span_t*>(h->align_up.maps.data());
  const long long bytes = gsv_op_align_workspace(n, img, nullptr);
  GSV_REQUIRE(bytes > 0, "vits align: bad span table");
  void *tab, *ws;
  GSV_RC(need(h, "align_tab", (size_t)n * sizeof(gsv_align_span_t), &tab));
  GSV_RC(need(h, "align_ws", (size_t)bytes, &ws));
  GSV_HIP(hipMemcpyAsync(tab, img, (size_t)n * sizeof(gsv_align_span_t), hipMemcpyHostToDevice, s));
  GSV_HIP(hipEventRecord(h->align_up.ev, s));
  GSV_RC(launch_align_logp(h->dtype, q, MH, kv, 2 * MH, 4, MH / 4, 1.f / sqrtf((float)(MH / 4)), (const gsv_align_span_t*)tab, n, ws, bytes, s));
  return launch_align_path((const gsv_align_span_t*)tab, n, ws, bytes, h->align_ends, h->align_score, s);
}

// quantizer.decode + nearest x2 (H8) and TextEncoder.forward up to (and including) the speed interpolation (H10, reference
// module/models.py:199-231): returns the hidden sequence y [F][hidden] (what `enc_p` returns as its first value)
// sr != null: segmented, Tc / L / speed are ignored for the padded totals of sr->lay (in) and sr->post (out)
template <typename T>
int run_enc_p(gsv_vits* h, hipStream_t s, const int32_t* codes, int Tc, const int32_t* phones, int L, double speed, void** y_out,
              int* F_out, const SegRun* sr = nullptr) {
  const auto& c = h->cfg;
  const size_t es = esz(h);
  const int H = c.hidden_channels, SSL = c.ssl_dim, MH = 512;
  if (sr) L = sr->lay->L;
  const int F0 = sr ? sr->lay->F : 2 * Tc;
  const int F = sr ? sr->post->F : speed == 1.0 ? F0 : (int)((double)F0 / speed) + 1;   // frames after the speed interpolation
  std::vector<gsv_align_seg_span_t> align;
  GSV_RC(align_prepare(h, Tc, L, sr, &align));
  h->lastF0 = F0; h->lastL = L;
  // ---- H8: codebook gather + nearest x2
  void *q768, *y, *tx;
  GSV_RC(need(h, "q768", (size_t)F0 * SSL * es, &q768));
  GSV_RC(need(h, "enc_x", (size_t)F0 * H * es, &y));
  GSV_RC(need(h, "enc_tx", (size_t)L * H * es, &tx));
  if (sr) GSV_LAUNCH(gather_seg_kernel<T>, dim3(F0), dim3(128), 0, s, codes, sr->src_code, h->codebook, SSL, F0, (T*)q768);
  else GSV_LAUNCH(gather_rows_kernel<T>, dim3(F0), dim3(128), 0, s, codes, h->codebook, SSL, 2, Tc, (T*)q768);
  // ---- H10: enc_p
  const int *seg_f = sr ? sr->seg_f : nullptr, *kr_f = sr ? sr->kr_f : nullptr;
  ConvOpt o;
  GSV_RC(conv(h, s, h->ssl_proj_enc, q768, SSL, F0, y, F0, o));
  GSV_RC(run_encoder(h, s, h->enc_ssl, y, F0, seg_f, kr_f));
  if (sr) GSV_LAUNCH(gather_seg_kernel<T>, dim3(L), dim3(128), 0, s, phones, sr->src_phone, h->text_emb, H, L, (T*)tx);
  else GSV_LAUNCH(gather_rows_kernel<T>, dim3(L), dim3(128), 0, s, phones, h->text_emb, H, 1, L, (T*)tx);
  GSV_RC(run_encoder(h, s, h->enc_text, tx, L, sr ? sr->seg_l : nullptr, sr ? sr->kr_l : nullptr));
  {  // MRTE (mrte_model.py:25-44)
    void *s512, *t512, *q512, *kv512, *o512, *x512;
    GSV_RC(need(h, "m_s", (size_t)F0 * MH * es, &s512));
    GSV_RC(need(h, "m_t", (size_t)L * MH * es, &t512));
    GSV_RC(need(h, "m_q", (size_t)F0 * MH * es, &q512));
    GSV_RC(need(h, "m_kv", (size_t)L * 2 * MH * es, &kv512));
    GSV_RC(need(h, "m_o", (size_t)F0 * MH * es, &o512));
    GSV_RC(need(h, "m_x", (size_t)F0 * MH * es, &x512));
    GSV_RC(conv(h, s, h->c_pre, y, H, F0, s512, F0, o));
    GSV_RC(conv(h, s, h->text_pre, tx, H, L, t512, L, o));
    GSV_RC(conv(h, s, h->mq, s512, MH, F0, q512, F0, o));
    GSV_RC(conv(h, s, h->mkv, t512, MH, L, kv512, L, o));
    GSV_RC(attention(h, s, q512, MH, 0, kv512, 2 * MH, 0, MH, F0, L, 4, MH / 4, 1.f / sqrtf((float)(MH / 4)), nullptr, nullptr, o512, MH,
                     sr ? sr->kr_x : nullptr));
    if (!align.empty()) GSV_RC(align_run(h, s, (int)align.size(), q512, kv512, MH));
    ConvOpt om; om.res = s512; om.ldr = MH;
    GSV_RC(conv_voice(h, s, h->mo, o512, F0, x512, om, h->mo_bias_eff, sr, 0, seg_f));
    GSV_RC(conv(h, s, h->c_post, x512, MH, F0, y, F0, o));
  }
  GSV_RC(run_encoder(h, s, h->enc2, y, F0, seg_f, kr_f));
  if (seg_f ? sr->post != sr->lay : F != F0) {      // one segment (maps nulled) is the plain sequence
    void* yi;
    GSV_RC(need(h, "enc_x_speed", (size_t)F * H * es, &yi));
    if (seg_f)
      GSV_LAUNCH(interp_linear_seg_kernel<T>, dim3(F), dim3(64), 0, s, (const T*)y, sr->seg_p, sr->start_pre, sr->len_pre, sr->start,
                 sr->len_post, F, H, (T*)yi);
    else GSV_LAUNCH(interp_linear_kernel<T>, dim3(F), dim3(64), 0, s, (const T*)y, F0, F, H, (T*)yi);
    y = yi;
  }
  *y_out = y;
  *F_out = F;
  return GSV_OK;
}

// in_bias_eff[li] = in_layers[li].bias + cond_layer(ge)[li]: the WN's conditioning term is constant per reference audio
static int fold_wn_cond(gsv_vits* h, hipStream_t s, WNW& w, float* tmp) {
  ConvOpt o; o.out_f32 = 1;
  GSV_RC(conv(h, s, w.cond, h->ge_t, w.cond.cin, 1, tmp, 1, o));
  for (size_t li = 0; li < w.in.size(); ++li) {
    const int n = w.in[li].cout;
    GSV_LAUNCH(vec_add_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, tmp + li * n, w.in[li].b, w.in_bias_eff[li], n);
  }
  return GSV_OK;
}

// ref_enc (modules.MelStyleEncoder) over every reference -> ge, then everything ge conditions folded into biases
template <typename T>
static int set_refer_impl(gsv_vits* h, const float* const* specs, const int* frames, int bins, const float* const* sv_embs, int n_refs,
                          gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "vits_set_refer: handle not finalized");
  GSV_REQUIRE(specs && frames && n_refs >= 1, "vits_set_refer: no reference spectrogram");
  GSV_REQUIRE(bins >= h->cfg.ref_bins, "vits_set_refer: spectrogram has %d bins, need >= %d", bins, h->cfg.ref_bins);
  hipStream_t s = (hipStream_t)stream;
  h->ref_stream = s;
  const auto& c = h->cfg;
  const size_t es = esz(h);
  const int RB = c.ref_bins, RH = 128, GIN = c.gin_channels;
  for (int r = 0; r < n_refs; ++r) {
    const int Tr = frames[r];
    GSV_REQUIRE(Tr >= 1 && specs[r], "vits_set_refer: empty reference %d", r);
    void *x0, *a, *b, *y2, *qkv, *ao;
    GSV_RC(need(h, "ref_x0", (size_t)Tr * RB * es, &x0));
    GSV_RC(need(h, "ref_a", (size_t)Tr * RH * es, &a));
    GSV_RC(need(h, "ref_b", (size_t)Tr * RH * es, &b));
    GSV_RC(need(h, "ref_y2", (size_t)Tr * 2 * RH * es, &y2));
    GSV_RC(need(h, "ref_qkv", (size_t)Tr * 3 * RH * es, &qkv));
    GSV_RC(need(h, "ref_ao", (size_t)Tr * GIN * es, &ao));
    GSV_RC(cf_to_cl(h, s, specs[r], Tr, RB, x0));
    ConvOpt om; om.post_act = ACT_MISH;
    GSV_RC(conv(h, s, h->r_sp0, x0, RB, Tr, a, Tr, om));
    GSV_RC(conv(h, s, h->r_sp3, a, RH, Tr, b, Tr, om));
    ConvOpt o;
    for (int t = 0; t < 2; ++t) {
      GSV_RC(conv(h, s, t == 0 ? h->r_t0 : h->r_t1, b, RH, Tr, y2, Tr, o));
      GSV_LAUNCH(glu_res_kernel<T>, dim3(nblk((long long)Tr * RH)), dim3(256), 0, s, (const T*)y2, (long long)Tr * RH, RH, (T*)b);
    }
    GSV_RC(conv(h, s, h->r_qkv, b, RH, Tr, qkv, Tr, o));
    // 2 heads x 64, temperature sqrt(d_model) (modules.py:610)
    GSV_RC(attention(h, s, qkv, 3 * RH, 0, qkv, 3 * RH, RH, 2 * RH, Tr, Tr, 2, RH / 2, 1.f / sqrtf((float)RH), nullptr, nullptr, a, RH));
    ConvOpt orr; orr.res = b; orr.ldr = RH;
    GSV_RC(conv(h, s, h->r_fc, a, RH, Tr, y2, Tr, orr));          // fc(attn) + residual -> y2 [Tr][RH]
    GSV_RC(conv(h, s, h->r_out, y2, RH, Tr, ao, Tr, o));            // [Tr][GIN]
    if (!sv_embs) {
      GSV_LAUNCH(mean_time_kernel<T>, dim3(cdiv(GIN, 64)), dim3(64), 0, s, (const T*)ao, Tr, GIN, 1.f / n_refs, r > 0, h->ge);
    } else {
      GSV_LAUNCH(mean_time_kernel<T>, dim3(cdiv(GIN, 64)), dim3(64), 0, s, (const T*)ao, Tr, GIN, 1.f, 0, h->ge_ref);
      GSV_RC(launch_convert(sv_embs[r], h->sv_t, h->dtype, 20480, s));
      ConvOpt osv; osv.out_f32 = 1;
      GSV_RC(conv(h, s, h->sv_emb, h->sv_t, 20480, 1, h->sv_proj, 1, osv));
      GSV_LAUNCH(sv_prelu_acc_kernel, dim3(cdiv(GIN, 256)), dim3(256), 0, s, (const float*)h->ge_ref, (const float*)h->sv_proj,
                 (const float*)h->prelu_w, 1.f / n_refs, r > 0, GIN, h->ge);
    }
  }
  GSV_RC(launch_convert(h->ge, h->ge_t, h->dtype, GIN, s));
  // fold conditioning into biases: conv_pre + cond(ge); MRTE conv_o bias + ge; WN in_layers + cond_layer(ge)
  float* tmp;
  GSV_RC(need(h, "cond_tmp", (size_t)2048 * 4 * 4, (void**)&tmp));
  {
    ConvOpt o; o.out_f32 = 1;
    if (c.v2pro) {     // the MRTE adds ge_to512(ge) (models.py:997)
      GSV_RC(conv(h, s, h->ge_to512, h->ge_t, GIN, 1, h->ge512, 1, o));
      GSV_LAUNCH(vec_add_kernel, dim3(cdiv(512, 256)), dim3(256), 0, s, h->ge512, h->mo.b, h->mo_bias_eff, 512);
    } else {
      GSV_LAUNCH(vec_add_kernel, dim3(cdiv(GIN, 256)), dim3(256), 0, s, h->ge, h->mo.b, h->mo_bias_eff, GIN);
    }
    if (c.flavor != 0) {
      GSV_RC(fold_wn_cond(h, s, h->w1, tmp));
    } else {
      GSV_RC(conv(h, s, h->cond, h->ge_t, GIN, 1, tmp, 1, o));
      GSV_LAUNCH(vec_add_kernel, dim3(cdiv(h->conv_pre.cout, 256)), dim3(256), 0, s, tmp, h->conv_pre.b, h->conv_pre_bias_eff, h->conv_pre.cout);
      for (int fi = 0; fi < 4; ++fi) GSV_RC(fold_wn_cond(h, s, h->flows[fi].wn, tmp));
    }
  }
  h->has_ref = true;
  return GSV_OK;
}

}  // namespace gsveng

extern "C" {

int gsv_vits_create(const gsv_vits_config* cfg, int dtype, gsv_vits_t** out) {
  GSV_REQUIRE(cfg && out, "vits_create: null argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "vits_create: bad dtype");
  GSV_REQUIRE(cfg->flavor >= 0 && cfg->flavor <= 2, "vits_create: flavor must be 0 (v1/v2), 1 (v3) or 2 (v4)");
  GSV_REQUIRE(cfg->flavor != 0 || (cfg->n_ups >= 1 && cfg->n_ups <= 8 && cfg->n_resblocks >= 1 && cfg->n_resblocks <= 4), "vits_create: bad generator shape");
  GSV_REQUIRE(cfg->hidden_channels % cfg->n_heads == 0 && (cfg->hidden_channels / cfg->n_heads) % 8 == 0, "vits_create: head dim must be a multiple of 8");
  GSV_REQUIRE(cfg->inter_channels % 16 == 0, "vits_create: inter_channels must be a multiple of 16");
  GSV_RC(require_device());
  gsv_vits* h = new gsv_vits();
  h->cfg = *cfg;
  h->dtype = dtype;
  *out = h;
  return GSV_OK;
}

void gsv_vits_destroy(gsv_vits_t* h) {
  if (!h) return;
  free_ctx(h);
  for (auto e : h->ev) if (e) (void)hipEventDestroy(e);
  delete h;
}

int gsv_vits_load_tensor(gsv_vits_t* h, const char* name, const float* data, int64_t numel) {
  return stage_tensor(h, name, data, numel);
}

int gsv_vits_finalize(gsv_vits_t* h) {
  GSV_REQUIRE(h && !h->finalized, "vits_finalize: bad handle");
  const auto& c = h->cfg;
  const int H = c.hidden_channels, IC = c.inter_channels, GIN = c.gin_channels, SSL = c.ssl_dim;
  const int MH = 512;  // MRTE hidden (mrte_model.py:13)
  GSV_REQUIRE(GIN == MH || c.v2pro, "vits: gin_channels must equal the MRTE width 512 (mrte_model.py:36 adds ge to it)");
  // enc_p
  GSV_RC(make_conv(h, "enc_p.ssl_proj", H, SSL, 1, true, &h->ssl_proj_enc));
  GSV_RC(make_encoder(h, "enc_p.encoder_ssl", c.n_layers / 2, &h->enc_ssl));
  GSV_RC(make_encoder(h, "enc_p.encoder_text", c.n_layers, &h->enc_text));
  GSV_RC(make_encoder(h, "enc_p.encoder2", c.n_layers / 2, &h->enc2));
  GSV_RC(make_vec(h, "enc_p.text_embedding.weight", (size_t)c.n_symbols * H, &h->text_emb));
  GSV_RC(make_conv(h, "enc_p.mrte.c_pre", MH, H, 1, true, &h->c_pre));
  GSV_RC(make_conv(h, "enc_p.mrte.text_pre", MH, H, 1, true, &h->text_pre));
  GSV_RC(make_conv(h, "enc_p.mrte.c_post", H, MH, 1, true, &h->c_post));
  GSV_RC(make_conv(h, "enc_p.mrte.cross_attention.conv_q", MH, MH, 1, true, &h->mq));
  GSV_RC(make_stacked(h, {"enc_p.mrte.cross_attention.conv_k", "enc_p.mrte.cross_attention.conv_v"}, MH, MH, &h->mkv));
  GSV_RC(make_conv(h, "enc_p.mrte.cross_attention.conv_o", MH, MH, 1, true, &h->mo));
  GSV_RC(make_conv(h, "enc_p.proj", 2 * IC, H, 1, true, &h->proj));
  // codebook + top-level ssl_proj
  {
    std::vector<float> e;
    if (!fetch(h, "quantizer.vq.layers.0._codebook.embed", (size_t)c.n_bins * SSL, c.n_bins, e)) return GSV_ERR_ARG;
    GSV_RC(up_f32(h, e.data(), e.size(), &h->codebook));
    GSV_RC(up_t(h, e, &h->codebook_t));
    std::vector<float> ee(c.n_bins);
    for (int j = 0; j < c.n_bins; ++j) {
      float s = 0.f;   // fp32 sum of squares in index order, like embed.pow(2).sum(0)
      for (int k = 0; k < SSL; ++k) s += e[(size_t)j * SSL + k] * e[(size_t)j * SSL + k];
      ee[j] = s;
    }
    GSV_RC(up_f32(h, ee.data(), ee.size(), &h->code_ee));
    GSV_RC(make_conv(h, "ssl_proj", SSL, SSL, 2, true, &h->top_ssl_proj));
  }
  if (c.flavor == 0) {
    // flow
    for (int fi = 0; fi < 4; ++fi) {
      FlowW& f = h->flows[fi];
      const std::string p = "flow.flows." + std::to_string(2 * fi);
      GSV_RC(make_conv(h, p + ".pre", H, IC / 2, 1, true, &f.pre));
      GSV_RC(make_conv(h, p + ".post", IC / 2, H, 1, true, &f.post));
      GSV_RC(make_wn(h, p + ".enc", 4, H, GIN, &f.wn));
    }
    // generator
    const int UIC = c.upsample_initial_channel;
    GSV_RC(make_conv(h, "dec.conv_pre", UIC, IC, 7, true, &h->conv_pre));
    GSV_RC(make_conv(h, "dec.cond", UIC, GIN, 1, true, &h->cond));
    GSV_RC(dalloc(h, (void**)&h->conv_pre_bias_eff, (size_t)UIC * 4));
    gen_shape(c, &h->gen);
    GSV_RC(load_generator(h, "dec.", false, &h->gen));
    GSV_RC(make_conv(h, "dec.conv_post", 1, UIC >> c.n_ups, 7, false, &h->conv_post));
  } else {
    // v3 / v4 (SynthesizerTrnV3, module/models.py:1203-1206): bridge + wns1 = Encoder(512, 512, 512, 5, 1, 8, gin)
    const int W = 512, NL = 8;
    GSV_REQUIRE(IC == H, "vits: v3/v4 need inter_channels == hidden_channels (bridge = Conv1d(inter, 512) on the hidden sequence)");
    GSV_RC(make_conv(h, "bridge.0", W, IC, 1, true, &h->bridge));
    GSV_RC(make_conv(h, "wns1.pre", W, W, 1, true, &h->w1_pre));
    GSV_RC(make_conv(h, "wns1.proj", W, W, 1, true, &h->w1_proj));
    GSV_RC(make_wn(h, "wns1.enc", NL, W, GIN, &h->w1));
  }
  // ref_enc
  const int RH = 128;
  GSV_RC(make_conv(h, "ref_enc.spectral.0.fc", RH, c.ref_bins, 1, true, &h->r_sp0));
  GSV_RC(make_conv(h, "ref_enc.spectral.3.fc", RH, RH, 1, true, &h->r_sp3));
  GSV_RC(make_conv(h, "ref_enc.temporal.0.conv1.conv", 2 * RH, RH, 5, true, &h->r_t0));
  GSV_RC(make_conv(h, "ref_enc.temporal.1.conv1.conv", 2 * RH, RH, 5, true, &h->r_t1));
  GSV_RC(make_stacked(h, {"ref_enc.slf_attn.w_qs", "ref_enc.slf_attn.w_ks", "ref_enc.slf_attn.w_vs"}, RH, RH, &h->r_qkv));
  GSV_RC(make_conv(h, "ref_enc.slf_attn.fc", RH, RH, 1, true, &h->r_fc));
  GSV_RC(make_conv(h, "ref_enc.fc.fc", GIN, RH, 1, true, &h->r_out));
  GSV_RC(dalloc(h, (void**)&h->ge, (size_t)GIN * 4));
  GSV_RC(dalloc(h, &h->ge_t, (size_t)GIN * esz(h)));
  GSV_RC(dalloc(h, (void**)&h->mo_bias_eff, (size_t)MH * 4));
  if (c.v2pro) {
    GSV_RC(make_conv(h, "sv_emb", GIN, 20480, 1, true, &h->sv_emb));
    GSV_RC(make_conv(h, "ge_to512", MH, GIN, 1, true, &h->ge_to512));
    GSV_RC(make_vec(h, "prelu.weight", GIN, &h->prelu_w));
    GSV_RC(dalloc(h, (void**)&h->ge_ref, (size_t)GIN * 4));
    GSV_RC(dalloc(h, (void**)&h->sv_proj, (size_t)GIN * 4));
    GSV_RC(dalloc(h, (void**)&h->ge512, (size_t)MH * 4));
    GSV_RC(dalloc(h, &h->sv_t, (size_t)20480 * esz(h)));
  }
  for (auto& e : h->ev) GSV_HIP(hipEventCreate(&e));
  h->staged.clear();
  h->finalized = true;
  return GSV_OK;
}

int gsv_vits_set_refer(gsv_vits_t* h, const float* const* specs, const int* frames, int bins, int n_refs, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "vits_set_refer: handle not finalized");
  GSV_REQUIRE(!h->cfg.v2pro, "vits_set_refer: a v2Pro model needs gsv_vits_set_refer_sv (one sv embedding per reference)");
  return GSV_WITH_T(h, set_refer_impl<T>(h, specs, frames, bins, nullptr, n_refs, stream));
}

int gsv_vits_set_refer_sv(gsv_vits_t* h, const float* const* specs, const int* frames, int bins, const float* const* sv_embs,
                          int n_refs, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "vits_set_refer_sv: handle not finalized");
  GSV_REQUIRE(h->cfg.v2pro && sv_embs, "vits_set_refer_sv: not a v2Pro model, or no sv embeddings");
  for (int r = 0; r < n_refs; ++r) GSV_REQUIRE(sv_embs[r], "vits_set_refer_sv: missing sv embedding %d", r);
  return GSV_WITH_T(h, set_refer_impl<T>(h, specs, frames, bins, sv_embs, n_refs, stream));
}

}  // extern "C"

namespace gsveng {
// modules.WN.forward (modules.py:  in -> gate -> res/skip) on hb [F][H]: hb accumulates the residual halves, wout [F][H] the skip
// halves; xin [F][2H] and acts [F][H] are scratch.  The two ways rows are masked, and where the in-layer bias comes from:
//   sr != null (segmented flow, post layout): voice-row biases at voff + li * 2H (conv_voice), sr->seg_p keeps the gap rows of hb zero;
//   Lm < F (wns1, models.py:1252-1258): rows >= Lm of hb are zeroed after each residual add.
template <typename T>
static int run_wn(gsv_vits* h, hipStream_t s, const WNW& w, int F, void* hb, void* xin, void* acts, void* wout, const SegRun* sr,
                  size_t voff, int Lm) {
  const int NL = (int)w.in.size(), H = w.in[0].cin;
  const int* seg_f = sr ? sr->seg_p : nullptr;
  for (int li = 0; li < NL; ++li) {
    GSV_RC(conv_voice(h, s, w.in[li], hb, F, xin, ConvOpt(), w.in_bias_eff[li], sr, voff + (size_t)li * 2 * H, seg_f));   // xin feeds only the gate
    GSV_LAUNCH(gate_kernel<T>, dim3(nblk((long long)F * H)), dim3(256), 0, s, (const T*)xin, (long long)F * H, H, (T*)acts);
    if (li < NL - 1) {
      ConvOpt ores; ores.cout = H; ores.w_row0 = 0; ores.accumulate = 1; ores.row_seg = seg_f;   // h += rs[:H]
      GSV_RC(conv(h, s, w.res[li], acts, H, F, hb, F, ores));
      if (Lm < F) GSV_HIP(hipMemsetAsync((T*)hb + (size_t)Lm * H, 0, (size_t)(F - Lm) * H * sizeof(T), s));
      ConvOpt osk; osk.cout = H; osk.w_row0 = H; osk.accumulate = li > 0;       // out (+)= rs[H:]
      GSV_RC(conv(h, s, w.res[li], acts, H, F, wout, F, osk));
    } else {
      ConvOpt osk; osk.accumulate = li > 0;
      GSV_RC(conv(h, s, w.res[li], acts, H, F, wout, F, osk));
    }
  }
  return GSV_OK;
}

// the v1/v2 decode: enc_p -> proj -> z_p -> flow reverse -> generator; sr != null: segmented (gap rows masked, per-segment voice
// biases and noise keys, the gaps dropped from the waveform); everything after run_enc_p is in the post layout
template <typename T>
static int decode_wav(gsv_vits* h, hipStream_t s, const int32_t* codes, int Tc, const int32_t* phones, int L, double speed,
                      const float* noise, float noise_scale, uint64_t seed, float* wav, const SegRun* sr) {
  const auto& c = h->cfg;
  void* y = nullptr;
  int F = 0;
  GSV_RC(run_enc_p<T>(h, s, codes, Tc, phones, L, speed, &y, &F, sr));
  const size_t es = sizeof(T);
  const int H = c.hidden_channels, IC = c.inter_channels;
  const int* seg_f = sr ? sr->seg_p : nullptr;
  float* stats;
  GSV_RC(need(h, "stats", (size_t)F * 2 * IC * 4, (void**)&stats));
  { ConvOpt of; of.out_f32 = 1; GSV_RC(conv(h, s, h->proj, y, H, F, stats, F, of)); }
  // ---- z_p, H11: flow reverse
  void *z, *zf, *hb, *xin, *acts, *wout;
  GSV_RC(need(h, "z", (size_t)F * IC * es, &z));
  GSV_RC(need(h, "zf", (size_t)F * IC * es, &zf));
  GSV_RC(need(h, "wn_h", (size_t)F * H * es, &hb));
  GSV_RC(need(h, "wn_xin", (size_t)F * 2 * H * es, &xin));
  GSV_RC(need(h, "wn_acts", (size_t)F * H * es, &acts));
  GSV_RC(need(h, "wn_out", (size_t)F * H * es, &wout));
  GSV_LAUNCH(zp_kernel<T>, dim3(nblk((long long)F * IC)), dim3(256), 0, s, stats, F, IC, noise, noise_scale, (unsigned long long)seed, (T*)z,
             seg_f, sr ? sr->start : nullptr, sr ? sr->noff : nullptr, sr ? sr->seeds : nullptr, sr ? sr->post->Fn : 0);
  const int half = IC / 2;
  for (int fi = 3; fi >= 0; --fi) {
    FlowW& f = h->flows[fi];
    GSV_LAUNCH(flip_channels_kernel<T>, dim3(nblk((long long)F * IC)), dim3(256), 0, s, (const T*)z, (long long)F * IC, IC, (T*)zf);
    std::swap(z, zf);
    ConvOpt om; om.row_seg = seg_f;                  // what the WN in_layers (kernel 5) read: gap rows stay 0
    GSV_RC(conv(h, s, f.pre, z, IC, F, hb, F, om));  // x0 = channels [0, half)
    GSV_RC(run_wn<T>(h, s, f.wn, F, hb, xin, acts, wout, sr, h->voice_off_in + (size_t)fi * 4 * 2 * H, F));
    ConvOpt op; op.scale = -1.f; op.accumulate = 1; op.ldy = IC; op.y_col0 = half; op.row_seg = seg_f;  // x1 -= post(h)
    GSV_RC(conv(h, s, f.post, wout, H, F, z, F, op));
  }
  h->lastF = F;
  // keep a stable pointer to the final z for the debug hook
  {
    void* zkeep;
    GSV_RC(need(h, "z_keep", (size_t)F * IC * es, &zkeep));
    GSV_HIP(hipMemcpyAsync(zkeep, z, (size_t)F * IC * es, hipMemcpyDeviceToDevice, s));
  }
  GSV_HIP(hipEventRecord(h->ev[1], s));
  // ---- H12: generator
  void* gb[5];
  GSV_RC(gen_buffers(h, h->gen, "g", F, gb));
  void* cur = gb[3];
  GSV_RC(conv_voice(h, s, h->conv_pre, z, F, cur, ConvOpt(), h->conv_pre_bias_eff, sr, h->voice_off_pre, seg_f));
  int Tn = F;
  GSV_RC(run_generator_stages(h, s, h->gen, gb, &cur, &Tn, seg_f ? sr->seg_up.data() : nullptr, nullptr, &h->dbg_last));
  float* wout_p = wav;                 // segmented: the padded waveform, then the gaps are dropped into wav
  if (seg_f) GSV_RC(need(h, "wav_pad", (size_t)Tn * 4, (void**)&wout_p));
  { ConvOpt op; op.pre_act = ACT_LRELU; op.pre_slope = 0.01f; op.post_act = ACT_TANH; op.out_f32 = 1;
    GSV_RC(conv(h, s, h->conv_post, cur, h->conv_post.cin, Tn, wout_p, Tn, op)); }
  if (seg_f) {
    const int up = Tn / F;
    GSV_RC(launch_compact_wav(s, wout_p, seg_f, up, (long long)sr->post->G * up, (long long)Tn, wav));
  }
  GSV_HIP(hipEventRecord(h->ev[2], s));
  return GSV_OK;
}

// the v3/v4 semantic path (SynthesizerTrnV3.decode_encp, module/models.py:1234-1262): enc_p -> bridge -> nearest upsampling ->
// wns1 -> fea [512][F] fp32 channels-first
template <typename T>
static int decode_encp(gsv_vits* h, hipStream_t s, const int32_t* codes, int Tc, const int32_t* phones, int L, double speed, float* fea) {
  const auto& c = h->cfg;
  const size_t es = sizeof(T);
  const int H = c.hidden_channels, W = 512;
  void* y = nullptr;
  int Fs = 0;
  GSV_RC(run_enc_p<T>(h, s, codes, Tc, phones, L, speed, &y, &Fs));
  const double sf = c.flavor == 1 ? 1.875 : 2.0;
  const int F = (int)floor((double)Fs * sf);
  // wns1's mask length (models.py:1252-1258): frames >= Lm are zeroed at every masked point of Encoder / WN
  const double per = c.flavor == 1 ? 3.875 : 4.0;
  const int sizee = (speed == 1.0) ? (int)((double)Tc * per) : (int)((double)Tc * per / speed) + 1;
  const int Lm = std::min(sizee, F);
  void *br, *up, *hb, *xin, *acts, *wout, *st;
  GSV_RC(need(h, "e_br", (size_t)Fs * W * es, &br));
  GSV_RC(need(h, "e_up", (size_t)F * W * es, &up));
  GSV_RC(need(h, "e_h", (size_t)F * W * es, &hb));
  GSV_RC(need(h, "e_xin", (size_t)F * 2 * W * es, &xin));
  GSV_RC(need(h, "e_acts", (size_t)F * W * es, &acts));
  GSV_RC(need(h, "e_out", (size_t)F * W * es, &wout));
  GSV_RC(need(h, "e_st", (size_t)F * W * es, &st));
  auto mask_tail = [&](void* p) -> int {
    if (Lm < F) GSV_HIP(hipMemsetAsync((char*)p + (size_t)Lm * W * es, 0, (size_t)(F - Lm) * W * es, s));
    return GSV_OK;
  };
  { ConvOpt ob; ob.post_act = ACT_LRELU01; GSV_RC(conv(h, s, h->bridge, y, H, Fs, br, Fs, ob)); }   // bridge: 1x1 + LeakyReLU(0.01)
  GSV_LAUNCH(interp_nearest_kernel<T>, dim3(F), dim3(128), 0, s, (const T*)br, Fs, F, W, (float)(1.0 / sf), (T*)up);
  ConvOpt o;
  GSV_RC(conv(h, s, h->w1_pre, up, W, F, hb, F, o));
  GSV_RC(mask_tail(hb));
  GSV_RC(run_wn<T>(h, s, h->w1, F, hb, xin, acts, wout, nullptr, 0, Lm));
  GSV_RC(mask_tail(wout));
  GSV_RC(conv(h, s, h->w1_proj, wout, W, F, st, F, o));
  GSV_RC(mask_tail(st));
  GSV_LAUNCH(cl_to_cf_kernel<T>, dim3(nblk((long long)F * W)), dim3(256), 0, s, (const T*)st, F, W, 0, W, fea);
  return GSV_OK;
}

// gsv_vits_extract_latent: top-level ssl_proj (kernel 2, stride 2) -> nearest codeword of the first quantizer layer
template <typename T>
static int extract_latent(gsv_vits* h, hipStream_t s, const float* ssl, int T50, int32_t* codes) {
  const auto& c = h->cfg;
  const int SSL = c.ssl_dim, T25 = (T50 - 2) / 2 + 1;
  void* x; float *p, *dots;
  GSV_RC(need(h, "xl_x", (size_t)T50 * SSL * sizeof(T), &x));
  GSV_RC(need(h, "xl_p", (size_t)T25 * SSL * 4, (void**)&p));
  GSV_RC(need(h, "xl_d", (size_t)T25 * c.n_bins * 4, (void**)&dots));
  GSV_RC(cf_to_cl(h, s, ssl, T50, SSL, x));
  ConvOpt o; o.stride = 2; o.pad = 0; o.out_f32 = 1;
  GSV_RC(conv(h, s, h->top_ssl_proj, x, SSL, T50, p, T25, o));
  // x . E^T in the engine dtype operands (fp32 engine: exact-f32 MFMA)
  void* pt;
  GSV_RC(need(h, "xl_pt", (size_t)T25 * SSL * sizeof(T), &pt));
  GSV_RC(launch_convert(p, pt, h->dtype, (long long)T25 * SSL, s));
  ConvArgs a;
  a.x = pt; a.w = h->codebook_t; a.y = dots; a.out_f32 = 1;
  a.T_in = T25; a.T_out = T25; a.T_virt = T25; a.Cin = SSL; a.Cout = c.n_bins; a.ldx = SSL; a.ldw = SSL; a.ldy = c.n_bins;
  GSV_RC(launch_conv_gemm(h->dtype, a, s));
  GSV_LAUNCH(argmax_code_kernel, dim3(T25), dim3(64), 0, s, dots, p, h->code_ee, SSL, c.n_bins, codes);
  return GSV_OK;
}

// gsv_vits_debug_tensor: T channels-last [Tn][ld] -> out fp32 channels-first [C][Tn]
template <typename T>
static int debug_cl_to_cf(hipStream_t s, const void* src, int Tn, int C, float* out) {
  GSV_LAUNCH(cl_to_cf_kernel<T>, dim3(nblk((long long)Tn * C)), dim3(256), 0, s, (const T*)src, Tn, C, 0, C, out);
  return GSV_OK;
}
}  // namespace gsveng

extern "C" {

int gsv_vits_decode(gsv_vits_t* h, const int32_t* codes, int Tc, const int32_t* phones, int L, const float* noise,
                    float noise_scale, double speed, uint64_t seed, float* wav, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "vits_decode: handle not finalized");
  GSV_REQUIRE(h->has_ref, "vits_decode: call gsv_vits_set_refer first");
  GSV_REQUIRE(codes && phones && wav && Tc >= 1 && L >= 1, "vits_decode: empty input (T=%d, L=%d)", Tc, L);
  hipStream_t s = (hipStream_t)stream;
  GSV_REQUIRE(speed > 0.0, "vits_decode: speed must be positive");
  GSV_REQUIRE(h->cfg.flavor == 0, "vits_decode: this handle is a v3/v4 model (use gsv_vits_decode_encp + gsv_cfm_inference + a vocoder)");
  GSV_HIP(hipEventRecord(h->ev[0], s));
  return GSV_WITH_T(h, decode_wav<T>(h, s, codes, Tc, phones, L, speed, noise, noise_scale, seed, wav, nullptr));
}

int gsv_vits_segment_gap(const gsv_vits_config* cfg) {
  if (!cfg || cfg->n_ups < 1 || cfg->n_ups > 8 || cfg->n_resblocks < 1 || cfg->n_resblocks > 4) return -1;
  return seg_gap(*cfg);
}

int gsv_vits_segment_map(const gsv_vits_config* cfg, int n, const int* code_lens, const int* phone_lens, int level, int32_t* seg,
                         int64_t cap, int64_t* rows) {
  return gsv_vits_segment_map_speed(cfg, n, code_lens, phone_lens, nullptr, level, seg, cap, rows);
}

int gsv_vits_segment_map_speed(const gsv_vits_config* cfg, int n, const int* code_lens, const int* phone_lens, const double* speeds,
                               int level, int32_t* seg, int64_t cap, int64_t* rows) {
  GSV_REQUIRE(cfg && rows && cfg->n_ups >= 1 && cfg->n_ups <= 8, "vits_segment_map: bad argument");
  GSV_REQUIRE(level >= -1 && level <= cfg->n_ups, "vits_segment_map: level %d outside [-1, %d]", level, cfg->n_ups);
  SegLayout lay;
  GSV_RC(seg_layout(*cfg, n, code_lens, phone_lens, speeds, &lay));
  long long up = 1;
  for (int i = 0; i < level; ++i) up *= cfg->up_rates[i];
  const long long nr = level < 0 ? lay.L : (long long)lay.F * up;
  *rows = nr;
  if (!seg) return GSV_OK;
  GSV_REQUIRE(cap >= nr, "vits_segment_map: buffer holds %lld rows, need %lld", (long long)cap, nr);
  for (long long t = 0; t < nr; ++t) seg[t] = -1;
  for (int i = 0; i < n; ++i) {
    const long long a = level < 0 ? lay.l0[i] : lay.f0[i] * up, len = level < 0 ? phone_lens[i] : lay.nf[i] * up;
    for (long long t = a; t < a + len; ++t) seg[t] = i;
  }
  return GSV_OK;
}

int gsv_vits_store_voice(gsv_vits_t* h, int slot) {
  GSV_REQUIRE(h && h->finalized, "vits_store_voice: handle not finalized");
  GSV_REQUIRE(h->cfg.flavor == 0, "vits_store_voice: voice slots serve the v1/v2 segmented decode only");
  GSV_REQUIRE(h->has_ref, "vits_store_voice: call gsv_vits_set_refer first");
  GSV_REQUIRE(slot >= 0 && slot < GSV_VITS_MAX_VOICES, "vits_store_voice: slot %d outside [0, %d)", slot, GSV_VITS_MAX_VOICES);
  const auto& c = h->cfg;
  const int H2 = 2 * c.hidden_channels, UIC = c.upsample_initial_channel;
  if (!h->voices) {
    h->voice_off_pre = 512;
    h->voice_off_in = (512 + UIC + 3) / 4 * 4;
    h->voice_len = h->voice_off_in + 16 * H2;
    GSV_RC(dalloc(h, (void**)&h->voices, (size_t)GSV_VITS_MAX_VOICES * h->voice_len * 4));
    h->voice_ok.assign(GSV_VITS_MAX_VOICES, 0);
  }
  // stream-ordered after the set_refer that wrote the conditioning; decode_segments waits for ev[3]
  hipStream_t s = h->ref_stream;
  float* row = h->voices + (size_t)slot * h->voice_len;
  GSV_HIP(hipMemcpyAsync(row, h->mo_bias_eff, 512 * 4, hipMemcpyDeviceToDevice, s));
  GSV_HIP(hipMemcpyAsync(row + h->voice_off_pre, h->conv_pre_bias_eff, (size_t)UIC * 4, hipMemcpyDeviceToDevice, s));
  for (int fi = 0; fi < 4; ++fi)
    for (int li = 0; li < 4; ++li)
      GSV_HIP(hipMemcpyAsync(row + h->voice_off_in + (size_t)(fi * 4 + li) * H2, h->flows[fi].wn.in_bias_eff[li], (size_t)H2 * 4,
                             hipMemcpyDeviceToDevice, s));
  GSV_HIP(hipEventRecord(h->ev[3], s));
  h->voice_ok[slot] = 1;
  return GSV_OK;
}

int gsv_vits_decode_segments(gsv_vits_t* h, int n, const int32_t* codes, const int* code_lens, const int32_t* phones,
                             const int* phone_lens, const int* voice_slots, const uint64_t* seeds, const float* noise, float noise_scale,
                             float* wav, gsv_stream_t stream) {
  return gsv_vits_decode_segments_speed(h, n, codes, code_lens, phones, phone_lens, voice_slots, seeds, nullptr, noise, noise_scale, wav,
                                        stream);
}

int gsv_vits_decode_segments_speed(gsv_vits_t* h, int n, const int32_t* codes, const int* code_lens, const int32_t* phones,
                                   const int* phone_lens, const int* voice_slots, const uint64_t* seeds, const double* speeds,
                                   const float* noise, float noise_scale, float* wav, gsv_stream_t stream) {
  GSV_REQUIRE(h, "vits_decode_segments: null handle");
  GSV_REQUIRE(h->cfg.flavor == 0, "vits_decode_segments: this handle is a v3/v4 model (segmented decode covers v1/v2 only)");
  GSV_REQUIRE(h->finalized, "vits_decode_segments: handle not finalized");
  GSV_REQUIRE(codes && phones && wav && code_lens && phone_lens && voice_slots && seeds && n >= 1, "vits_decode_segments: null argument");
  for (int i = 0; i < n; ++i)
    GSV_REQUIRE(voice_slots[i] >= 0 && voice_slots[i] < GSV_VITS_MAX_VOICES && h->voice_ok.size() && h->voice_ok[voice_slots[i]],
                "vits_decode_segments: segment %d names voice slot %d, which holds no voice (gsv_vits_store_voice)", i, voice_slots[i]);
  SegLayout lay, post;
  GSV_RC(seg_layout(h->cfg, n, code_lens, phone_lens, nullptr, &lay));
  GSV_RC(seg_layout(h->cfg, n, code_lens, phone_lens, speeds, &post));
  const bool interp = post.nf != lay.nf;     // some segment changes its frame count: the post layout is a second one
  hipStream_t s = (hipStream_t)stream;
  const int F = lay.F, L = lay.L, Fp = post.F;
  // host image of every map, one upload: seg_f | seg_l | kr_f | kr_l | kr_x | src_code | src_phone | start | noff | slot, and with
  // a second layout: | seg_p | start_pre | len_pre | len_post
  GSV_RC(seg_upload_begin(&h->seg));         // the previous call's upload (any stream) is done before its host image is rewritten
  GSV_HIP(hipStreamWaitEvent(s, h->ev[3], 0));   // the voice slots are stored
  std::vector<int>& m = h->seg.maps;
  const size_t o_sf = 0, o_sl = o_sf + F, o_kf = o_sl + L, o_kl = o_kf + 2 * (size_t)F, o_kx = o_kl + 2 * (size_t)L,
               o_sc = o_kx + 2 * (size_t)F, o_sp = o_sc + F, o_st = o_sp + L, o_no = o_st + n, o_vs = o_no + n,
               o_pf = o_vs + n, o_ps = o_pf + (interp ? Fp : 0), o_pi = o_ps + (interp ? n : 0), o_po = o_pi + (interp ? n : 0),
               total = o_po + (interp ? n : 0);
  m.assign(total, -1);
  for (int t = 0; t < F; ++t) { m[o_kf + 2 * t] = t; m[o_kf + 2 * t + 1] = t + 1; m[o_kx + 2 * t] = 0; m[o_kx + 2 * t + 1] = 0; }
  for (int t = 0; t < L; ++t) { m[o_kl + 2 * t] = t; m[o_kl + 2 * t + 1] = t + 1; }
  for (int i = 0; i < n; ++i) {
    const int f0 = lay.f0[i], nf = 2 * code_lens[i], l0 = lay.l0[i], nl = phone_lens[i];
    for (int t = f0; t < f0 + nf; ++t) {
      m[o_sf + t] = i;
      m[o_kf + 2 * t] = f0; m[o_kf + 2 * t + 1] = f0 + nf;
      m[o_kx + 2 * t] = l0; m[o_kx + 2 * t + 1] = l0 + nl;
      m[o_sc + t] = lay.c0[i] + (t - f0) / 2;          // nearest x2 of the codes
    }
    for (int t = l0; t < l0 + nl; ++t) {
      m[o_sl + t] = i;
      m[o_kl + 2 * t] = l0; m[o_kl + 2 * t + 1] = l0 + nl;
      m[o_sp + t] = lay.p0[i] + (t - l0);
    }
    m[o_st + i] = post.f0[i]; m[o_no + i] = post.fn0[i]; m[o_vs + i] = voice_slots[i];
    if (interp) {
      for (int t = post.f0[i]; t < post.f0[i] + post.nf[i]; ++t) m[o_pf + t] = i;
      m[o_ps + i] = f0; m[o_pi + i] = nf; m[o_po + i] = post.nf[i];
    }
  }
  h->seg.seeds.assign(seeds, seeds + n);
  int* dm;
  unsigned long long* dseed;
  float* vb;
  GSV_RC(need(h, "seg_maps", total * 4, (void**)&dm));
  GSV_RC(need(h, "seg_seeds", (size_t)n * 8, (void**)&dseed));
  GSV_RC(need(h, "seg_voices", (size_t)n * h->voice_len * 4, (void**)&vb));
  GSV_HIP(hipMemcpyAsync(dm, m.data(), total * 4, hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemcpyAsync(dseed, h->seg.seeds.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
  GSV_HIP(hipEventRecord(h->seg.ev, s));
  GSV_LAUNCH(gather_voice_kernel, dim3(n), dim3(256), 0, s, (const float*)h->voices, (const int*)(dm + o_vs), h->voice_len, vb);
  SegRun sr;
  sr.lay = &lay; sr.post = interp ? &post : &lay;
  sr.seg_f = dm + o_sf; sr.seg_l = dm + o_sl; sr.kr_f = dm + o_kf; sr.kr_l = dm + o_kl; sr.kr_x = dm + o_kx;
  sr.src_code = dm + o_sc; sr.src_phone = dm + o_sp; sr.start = dm + o_st; sr.noff = dm + o_no; sr.seeds = dseed; sr.bias = vb;
  sr.seg_p = interp ? dm + o_pf : sr.seg_f;
  if (interp) { sr.start_pre = dm + o_ps; sr.len_pre = dm + o_pi; sr.len_post = dm + o_po; }
  if (n == 1) {     // one segment is laid out exactly as gsv_vits_decode: no gaps, nothing to mask, its voice row as the bias
    sr.seg_f = sr.seg_l = sr.seg_p = sr.kr_f = sr.kr_l = sr.kr_x = nullptr;
  }
  long long up = 1;
  for (int i = 0; i < h->cfg.n_ups && n > 1; ++i) {
    up *= h->cfg.up_rates[i];
    const std::string nm = "seg_up" + std::to_string(i);
    int* su;
    GSV_RC(need(h, nm.c_str(), (size_t)Fp * up * 4, (void**)&su));
    GSV_RC(launch_expand_seg(s, sr.seg_p, (int)up, (long long)Fp * up, su));
    sr.seg_up.push_back(su);
  }
  GSV_HIP(hipEventRecord(h->ev[0], s));
  return GSV_WITH_T(h, decode_wav<T>(h, s, codes, 0, phones, L, 1.0, noise, noise_scale, seeds[0], wav, &sr));
}

int gsv_vits_encp_frames(gsv_vits_t* h, int T, double speed) {
  if (!h || T < 1 || !(speed > 0.0)) return -1;
  const int F0 = 2 * T;
  const int Fs = (speed == 1.0) ? F0 : (int)((double)F0 / speed) + 1;
  const double sf = h->cfg.flavor == 1 ? 1.875 : 2.0;
  return (int)floor((double)Fs * sf);
}

int gsv_vits_decode_encp(gsv_vits_t* h, const int32_t* codes, int Tc, const int32_t* phones, int L, double speed, float* fea,
                         gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "vits_decode_encp: handle not finalized");
  GSV_REQUIRE(h->cfg.flavor != 0, "vits_decode_encp: this handle is a v1/v2 model (use gsv_vits_decode)");
  GSV_REQUIRE(h->has_ref, "vits_decode_encp: call gsv_vits_set_refer first");
  GSV_REQUIRE(codes && phones && fea && Tc >= 1 && L >= 1, "vits_decode_encp: empty input (T=%d, L=%d)", Tc, L);
  GSV_REQUIRE(speed > 0.0, "vits_decode_encp: speed must be positive");
  return GSV_WITH_T(h, decode_encp<T>(h, (hipStream_t)stream, codes, Tc, phones, L, speed, fea));
}

int gsv_vits_set_align(gsv_vits_t* h, const gsv_align_seg_span_t* spans, int n, int32_t* ends, float* score) {
  GSV_REQUIRE(h && h->finalized, "vits_set_align: handle not finalized");
  h->align_req.clear();
  if (!spans || n == 0) return GSV_OK;
  GSV_REQUIRE(n > 0 && n <= ALIGN_MAX_SPANS && ends && score, "vits_set_align: %d spans, or no place for the results", n);
  h->align_req.assign(spans, spans + n);
  h->align_ends = ends;
  h->align_score = score;
  return GSV_OK;
}

int gsv_vits_last_timing(gsv_vits_t* h, float* total_ms, float* generator_ms) {
  GSV_REQUIRE(h && h->finalized && h->lastF > 0, "vits_last_timing: no decode yet");
  GSV_HIP(hipEventSynchronize(h->ev[2]));
  float a = 0.f, b = 0.f;
  GSV_HIP(hipEventElapsedTime(&a, h->ev[0], h->ev[2]));
  GSV_HIP(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  if (total_ms) *total_ms = a;
  if (generator_ms) *generator_ms = b;
  return GSV_OK;
}

int gsv_vits_extract_latent(gsv_vits_t* h, const float* ssl, int T50, int32_t* codes, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized && ssl && codes, "vits_extract_latent: bad argument");
  GSV_REQUIRE(T50 >= 2, "vits_extract_latent: need at least 2 ssl frames (got %d)", T50);
  return GSV_WITH_T(h, extract_latent<T>(h, (hipStream_t)stream, ssl, T50, codes));
}

int gsv_vits_debug_tensor(gsv_vits_t* h, const char* name, float* out, int64_t cap, int64_t* numel, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized && name && out && numel, "vits_debug_tensor: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const auto& c = h->cfg;
  const std::string n(name);
  const int F = h->lastF, IC = c.inter_channels;
  if (n == "ge") {
    GSV_REQUIRE(cap >= c.gin_channels, "vits_debug_tensor: buffer too small");
    GSV_HIP(hipMemcpyAsync(out, h->ge, (size_t)c.gin_channels * 4, hipMemcpyDeviceToDevice, s));
    *numel = c.gin_channels;
    return GSV_OK;
  }
  if (n == "m_q" || n == "m_kv") {   // the MRTE attention's operands of the last enc_p: [512][F0] / [1024][L]
    const int rows = n == "m_q" ? h->lastF0 : h->lastL, C = n == "m_q" ? 512 : 1024;
    GSV_REQUIRE(rows > 0, "vits_debug_tensor: no decode yet");
    GSV_REQUIRE(cap >= (int64_t)rows * C, "vits_debug_tensor: buffer too small");
    *numel = (int64_t)rows * C;
    return GSV_WITH_T(h, debug_cl_to_cf<T>(s, h->bufs[n].p, rows, C, out));
  }
  GSV_REQUIRE(F > 0, "vits_debug_tensor: no decode yet");
  if (n == "gen_last_in") {        // input of the last generator stage, [C][T] (segmented decode: its gap rows are 0)
    const GenTap& tap = h->dbg_last;
    const long long ne = (long long)tap.T * tap.C;
    GSV_REQUIRE(tap.in && cap >= ne, "vits_debug_tensor: buffer too small");
    *numel = ne;
    return GSV_WITH_T(h, debug_cl_to_cf<T>(s, tap.in, tap.T, tap.C, out));
  }
  GSV_REQUIRE(cap >= (int64_t)F * IC, "vits_debug_tensor: buffer too small");
  *numel = (int64_t)F * IC;
  if (n == "m_p" || n == "logs_p") {
    const float* st = (const float*)h->bufs["stats"].p;
    GSV_LAUNCH(cl_to_cf_kernel<float>, dim3(nblk((long long)F * IC)), dim3(256), 0, s, st, F, 2 * IC, n == "m_p" ? 0 : IC, IC, out);
    return GSV_OK;
  }
  if (n == "z") return GSV_WITH_T(h, debug_cl_to_cf<T>(s, h->bufs["z_keep"].p, F, IC, out));
  set_error("vits_debug_tensor: unknown tensor '%s' (ge, m_p, logs_p, z, gen_last_in, m_q, m_kv)", name);
  return GSV_ERR_ARG;
}

}  // extern "C"
