// AP-BWE audio super-resolution (24 kHz -> 48 kHz) for gfx950: the reference's tools/audio_sr.py::AP_BWE.__call__ --
// torchaudio.functional.resample, amp_pha_stft (AP_BWE_main/datasets1/dataset.py:9-27), APNet_BWE_Model.forward
// (AP_BWE_main/models/model.py:76-147) and amp_pha_istft (dataset.py:30-37).
//
// Layout: one waveform at a time; the spectra and the model activations are channels-last [frame][channel]; the two branches
// (magnitude z = 0, phase z = 1) sit back to back as [2][T][C] so that every GEMM of the model is ONE Z = 2 batched launch
// (same shapes, different weights).  The resampler, both DFTs, LayerNorm statistics, log / exp / phase run in fp32 in both
// modes; only the GEMM operands and the activations between blocks follow the handle dtype.
//
//   bwe_frame_kernel      polyphase resampler + center=True reflect padding + framing -> DFT operand [T][n_fft] fp32
//   (DFT GEMM)            frames x windowed basis -> re | im [T][2 bins] fp32                       (conv_gemm, fp32)
//   bwe_logamp_kernel     log(hypot + 1e-4), atan2 -> the conv_pre operand [2][T][bins_pad]
//   (conv_pre)            Conv1d(bins -> C, k 7) of both branches, Z = 2, then LayerNorm           (conv_gemm, ops.hip)
//   per layer:
//     bwe_mix_kernel      x_mag += x_pha; x_pha += x_mag; residuals; depthwise k-7 conv; LayerNorm -> GEMM operand
//     (pwconv1)           Linear C -> 3C + exact GELU, Z = 2                                          (conv_gemm)
//     (pwconv2)           Linear 3C -> C, gamma as the epilogue gate, residual as the epilogue res, Z = 2
//   post head: LayerNorm, linear_post_mag (+ log_amp residual), linear_post_pha_r | _i (one stacked GEMM)
//   bwe_spec_kernel       exp(mag) (r, i) / hypot(r, i) -> spectrum [T][2 bins (pad 4)] fp32 (+ the atan2 debug tap)
//   (iDFT GEMM)           spectrum x inverse basis (irfft / n_fft, window) -> frames [T][n_fft] fp32
//   bwe_ola_kernel        overlap-add as a gather, divided by the squared-window envelope, n_fft / 2 trimmed
#include <algorithm>
#include <numeric>

#include "engine.h"

using namespace gsv;
using namespace gsveng;

namespace gsv {

// torchaudio.functional.resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) fused with torch.stft's center=True
// reflect padding and framing: frame[t][k] = y[reflect(t * hop + k - n_fft / 2)], y[m q + p] = sum_l K[p][l] x[m o + l - width]
// (the stride-o conv over the zero-padded input, phases interleaved).  The thread holding k in [n_fft / 2, n_fft / 2 + hop) of
// frame t also stores y[t * hop + k - n_fft / 2] unreflected: every resampled sample exactly once (the `resampled` debug tap).
template <typename TI>
__global__ __launch_bounds__(256) void bwe_frame_kernel(const TI* __restrict__ x, int n_in, const float* __restrict__ ktab, int o, int q,
                                                        int width, int L, int n_new, int nfft, int hop, int Tn, float* __restrict__ frames,
                                                        float* __restrict__ resampled) {
  const int k = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (k >= nfft || t >= Tn) return;
  const int half = nfft / 2;
  const int i0 = t * hop + k - half;
  int i = i0 < 0 ? -i0 : i0;
  if (i >= n_new) i = 2 * n_new - 2 - i;
  const int m = i / q, p = i - m * q;
  const float* kp = ktab + (long long)p * L;
  const long long base = (long long)m * o - width;
  float acc = 0.f;
  for (int l = 0; l < L; ++l) {
    const long long j = base + l;
    if (j >= 0 && j < n_in) acc += kp[l] * to_f(x[j]);
  }
  frames[(long long)t * nfft + k] = acc;
  if (k >= half && k < half + hop && i0 < n_new) resampled[i0] = acc;
}

// amp_pha_stft's epilogue: log(|X| + 1e-4) with |X| = hypot(re, im) (no epsilon inside the root), angle = atan2(im, re) with 0
// for an all-zero bin (torch.angle of +0); writes the fp32 log-amplitude (residual of mag_wb, debug tap), the fp32 phase
// (debug tap) and both branches' conv_pre operand [2][T][bp] in the engine dtype, zero beyond `bins`
template <typename T>
__global__ void bwe_logamp_kernel(const float* __restrict__ ri, int Tn, int bins, int bp, float* __restrict__ la, float* __restrict__ pha,
                                  T* __restrict__ op) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * bp) return;
  const int t = (int)(i / bp), k = (int)(i - (long long)t * bp);
  float a = 0.f, ph = 0.f;
  if (k < bins) {
    const float re = ri[(long long)t * 2 * bins + k], im = ri[(long long)t * 2 * bins + bins + k];
    a = logf(hypotf(re, im) + 1e-4f);
    ph = (re == 0.f && im == 0.f) ? 0.f : atan2f(im, re);
    la[(long long)t * bins + k] = a;
    pha[(long long)t * bins + k] = ph;
  }
  op[i] = (T)a;
  op[(long long)Tn * bp + i] = (T)ph;
}

// One layer's front half for both branches (model.py:130-133 and ConvNeXtBlock.forward up to the norm, :53-60):
// r_mag = x_mag + x_pha, r_pha = x_pha + r_mag (the residuals, stored), then per branch the depthwise k-7 conv (zero padding 3)
// and LayerNorm over C (eps 1e-6, fp32 statistics) -> the pwconv1 operand.  One workgroup per TT frames: the TT + 6 rows of
// both mixed branches are built once in LDS (fp32), then one wave per (branch, frame) row holds C = 64 * NPL values in registers.
template <typename T, int NPL>
__global__ __launch_bounds__(256) void bwe_mix_kernel(const T* __restrict__ x, int Tn, int TT, const float* __restrict__ dww,
                                                      const float* __restrict__ dwb, const float* __restrict__ lng, const float* __restrict__ lnb,
                                                      T* __restrict__ res, T* __restrict__ out) {
  constexpr int C = 64 * NPL;
  extern __shared__ float sm[];                 // [2][TT + 6][C]
  const int t0 = blockIdx.x * TT, R = TT + 6;
  const long long zs = (long long)Tn * C;
  float* sm_p = sm + (size_t)R * C;
  for (int i = threadIdx.x; i < R * C; i += 256) {
    const int r = i / C, c = i - r * C, t = t0 - 3 + r;
    float rm = 0.f, rp = 0.f;
    if (t >= 0 && t < Tn) {
      const long long o = (long long)t * C + c;
      const float xm = to_f(x[o]), xp = to_f(x[zs + o]);
      const T m = (T)(xm + xp);
      const T p = (T)(xp + to_f(m));
      rm = to_f(m);
      rp = to_f(p);
      if (r >= 3 && r < 3 + TT) { res[o] = m; res[zs + o] = p; }
    }
    sm[i] = rm;
    sm_p[i] = rp;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = wave; row < 2 * TT; row += 4) {
    const int b = row / TT, r = row - b * TT, t = t0 + r;
    if (t >= Tn) continue;
    const float* s = sm + (size_t)b * R * C + (size_t)r * C;
    float v[NPL];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int c = i * 64 + lane;
      const float* w = dww + ((size_t)b * C + c) * 7;
      float acc = dwb[b * C + c];
#pragma unroll
      for (int j = 0; j < 7; ++j) acc += w[j] * s[(size_t)j * C + c];
      v[i] = acc;
      sum += acc;
    }
    const float mean = wave_sum(sum) / (float)C;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { const float d = v[i] - mean; var += d * d; }
    const float rstd = rsqrtf(wave_sum(var) / (float)C + 1e-6f);
    T* y = out + b * zs + (long long)t * C;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int c = i * 64 + lane;
      y[c] = (T)((v[i] - mean) * rstd * lng[b * C + c] + lnb[b * C + c]);
    }
  }
}

// Post head to the inverse-DFT operand (model.py:139-147 + amp_pha_istft): spec = exp(mag_wb) (r, i) / hypot(r, i), which is
// exp(mag_wb) (cos, sin)(atan2(i, r)) without the three transcendentals; (cos, sin) of the atan2 itself where hypot is 0
// (atan2(+-0, +-0)).  Columns [bins, 2 bins) hold the imaginary parts, [2 bins, ld) are zero.  pha_wb = atan2 (debug tap).
__global__ void bwe_spec_kernel(const float* __restrict__ mag, const float* __restrict__ rim, int Tn, int bins, int ld,
                                float* __restrict__ phawb, float* __restrict__ spec) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * ld) return;
  const int t = (int)(i / ld), k = (int)(i - (long long)t * ld);
  float* sp = spec + (long long)t * ld;
  if (k < bins) {
    const float r = rim[(long long)t * 2 * bins + k], im = rim[(long long)t * 2 * bins + bins + k];
    const float ph = atan2f(im, r);
    phawb[(long long)t * bins + k] = ph;
    const float h = hypotf(r, im);
    float cs, sn;
    if (h > 0.f) { cs = r / h; sn = im / h; }
    else { cs = cosf(ph); sn = sinf(ph); }
    const float a = expf(mag[(long long)t * bins + k]);
    sp[k] = a * cs;
    sp[bins + k] = a * sn;
  } else if (k >= 2 * bins) {
    sp[k] = 0.f;
  }
}

// torch.istft(center=True, no length) after the per-frame irfft * window: out[j] = sum_t frames[t][m - t hop] / sum_t w[m - t hop]^2
// with m = j + n_fft / 2, over the frames t covering m -- a gather, no atomics, deterministic
__global__ void bwe_ola_kernel(const float* __restrict__ fr, const float* __restrict__ win, int Tn, int nfft, int hop, int L,
                               float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= L) return;
  const int m = j + nfft / 2;
  const int t_hi = min(m / hop, Tn - 1);
  const int t_lo = m - nfft + 1 <= 0 ? 0 : (m - nfft + hop) / hop;
  float s = 0.f, e = 0.f;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int k = m - t * hop;
    s += fr[(long long)t * nfft + k];
    e += win[k] * win[k];
  }
  out[j] = s / e;
}

// debug taps: channels-last [T][C] fp32 -> channels-first [C][T] (the reference's [1, bins, T] layout)
__global__ void bwe_to_cf_kernel(const float* __restrict__ x, int Tn, int C, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  const int c = (int)(i / Tn), t = (int)(i - (long long)c * Tn);
  out[i] = x[(long long)t * C + c];
}

}  // namespace gsv

namespace {

struct ResampleTab { float* k = nullptr; int o = 1, q = 1, width = 0, L = 1; };

// torchaudio's _get_sinc_resample_kernel (sinc_interp_hann), evaluated with the same float32 operation order it uses for an
// fp32 waveform; orig == new is the identity (resample returns the waveform unchanged)
std::vector<float> sinc_kernel(int orig, int nw, int* o_out, int* q_out, int* width_out) {
  if (orig == nw) { *o_out = *q_out = 1; *width_out = 0; return {1.f}; }
  const int g = std::gcd(orig, nw);
  const int o = orig / g, q = nw / g;
  const double base = std::min(o, q) * 0.99;
  const int width = (int)ceil(6.0 * o / base);
  const int L = 2 * width + o;
  const float fb = (float)base, fpi = (float)M_PI, fscale = (float)(base / o);
  std::vector<float> k((size_t)q * L);
  for (int p = 0; p < q; ++p)
    for (int l = 0; l < L; ++l) {
      const float idx = (float)(l - width) / (float)o;
      float t = (float)(-p) / (float)q + idx;
      t *= fb;
      t = std::min(6.f, std::max(-6.f, t));
      float wv = cosf(t * fpi / 6.f / 2.f);
      wv = wv * wv;
      t *= fpi;
      const float s = t == 0.f ? 1.f : sinf(t) / t;
      k[(size_t)p * L + l] = s * (wv * fscale);
    }
  *o_out = o; *q_out = q; *width_out = width;
  return k;
}

}  // namespace

struct gsv_bwe : gsveng::Ctx {
  gsv_bwe() : Ctx("bwe") {}
  gsv_bwe_config cfg;
  int bins = 0, bp = 0, lds = 0;     // n_fft / 2 + 1, conv_pre operand width (16-aligned), spectrum row (4-aligned)
  float *fwd = nullptr, *inv = nullptr, *win = nullptr;   // fp32 [2 bins][n_fft], [n_fft][lds], [n_fft]
  void *pre_w = nullptr, *pw1 = nullptr, *pw2 = nullptr;   // [2][C][7 bp], [L][2][3C][C], [L][2][C][3C] (engine dtype)
  float *pre_b = nullptr, *pre_g = nullptr, *pre_beta = nullptr;
  float *dw_w = nullptr, *dw_b = nullptr, *ln_g = nullptr, *ln_b = nullptr, *pw1_b = nullptr, *pw2_b = nullptr, *gamma = nullptr;
  float *post_g = nullptr, *post_beta = nullptr;
  Conv post_mag, post_pha;
  std::map<int, ResampleTab> rtabs;
  // last forward (debug taps)
  int lastT = 0, lastN = 0;
  float *t_res = nullptr, *t_la = nullptr, *t_pha = nullptr, *t_mag = nullptr, *t_phawb = nullptr;
};

#define BWE_LAUNCH(kern, n, ...)                                                                         \
  do {                                                                                                   \
    hipLaunchKernelGGL(kern, dim3(nblk((long long)(n))), dim3(256), 0, s, __VA_ARGS__);                 \
    GSV_HIP(hipGetLastError());                                                                          \
  } while (0)

namespace {

int bwe_resample_tab(gsv_bwe* b, int orig, ResampleTab** out) {
  auto it = b->rtabs.find(orig);
  if (it == b->rtabs.end()) {
    ResampleTab r;
    std::vector<float> k = sinc_kernel(orig, b->cfg.hr_sampling_rate, &r.o, &r.q, &r.width);
    r.L = 2 * r.width + r.o;
    if (orig == b->cfg.hr_sampling_rate) r.L = 1;
    GSV_RC(up_f32(b, k.data(), k.size(), &r.k));
    it = b->rtabs.emplace(orig, r).first;
  }
  *out = &it->second;
  return GSV_OK;
}

// one Z = 2 batched 1x1 GEMM over both branches: y[z] = epilogue(x[z] [T][K] x w[z] [N][K]^T)
int branch_gemm(gsv_bwe* b, hipStream_t s, const void* x, int K, const void* w, const float* bias, int N, int Tn, void* y, int act,
                const float* gate, const void* res) {
  ConvArgs a;
  a.x = x; a.w = w; a.y = y; a.bias = bias; a.gate = gate; a.res = res;
  a.T_in = a.T_out = a.T_virt = Tn; a.Cin = K; a.Cout = N; a.taps = 1; a.pad = 0;
  a.ldx = K; a.ldw = K; a.ldy = N; a.ldr = N; a.post_act = act;
  a.Z = 2; a.xz = (long long)Tn * K; a.wz = (long long)N * K; a.yz = (long long)Tn * N; a.rz = a.yz; a.bz = N;
  a.z_res = res ? 1 : 0;
  return launch_conv_gemm(b->dtype, a, s);
}

template <typename T>
int launch_mix(const void* x, int Tn, int C, const float* dww, const float* dwb, const float* g, const float* be, void* res, void* out,
               hipStream_t s) {
  const int TT = C <= 512 ? 8 : 4;
  const size_t lds = (size_t)2 * (TT + 6) * C * 4;
  const dim3 grid(cdiv(Tn, TT)), block(256);
#define BWE_MIX(NPL)                                                                                                          \
  do {                                                                                                                        \
    static bool attr = false;                                                                                                 \
    if (!attr) {                                                                                                              \
      GSV_HIP(hipFuncSetAttribute((const void*)bwe_mix_kernel<T, NPL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      attr = true;                                                                                                            \
    }                                                                                                                         \
    hipLaunchKernelGGL((bwe_mix_kernel<T, NPL>), grid, block, lds, s, (const T*)x, Tn, TT, dww, dwb, g, be, (T*)res, (T*)out);  \
  } while (0)
  switch (C / 64) {
    case 1: BWE_MIX(1); break;
    case 2: BWE_MIX(2); break;
    case 4: BWE_MIX(4); break;
    case 8: BWE_MIX(8); break;
    case 12: BWE_MIX(12); break;
    case 16: BWE_MIX(16); break;
    default: set_error("bwe: ConvNeXt_channels %d is not one of 64, 128, 256, 512, 768, 1024", C); return GSV_ERR_ARG;
  }
#undef BWE_MIX
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

template <typename T, typename TI>
int bwe_forward_t(gsv_bwe* b, hipStream_t s, const TI* wav, int n, const ResampleTab& rt, int n_new, float* out) {
  const auto& g = b->cfg;
  const int F = g.n_fft, hop = g.hop_size, C = g.channels, B = b->bins, bp = b->bp, ld = b->lds;
  const int Tn = 1 + n_new / hop, L = hop * (n_new / hop);
  const size_t es = sizeof(T);
  float *res, *frames, *ri, *la, *pha, *mag, *phawb, *spec;
  void *x0, *xb, *rb, *ab, *hb;
  GSV_RC(need(b, "bwe_res", (size_t)n_new * 4, (void**)&res));
  GSV_RC(need(b, "bwe_frames", (size_t)Tn * F * 4, (void**)&frames));
  GSV_RC(need(b, "bwe_ri", (size_t)Tn * 2 * B * 4, (void**)&ri));
  GSV_RC(need(b, "bwe_la", (size_t)Tn * B * 4, (void**)&la));
  GSV_RC(need(b, "bwe_pha", (size_t)Tn * B * 4, (void**)&pha));
  GSV_RC(need(b, "bwe_mag", (size_t)Tn * B * 4, (void**)&mag));
  GSV_RC(need(b, "bwe_phawb", (size_t)Tn * B * 4, (void**)&phawb));
  GSV_RC(need(b, "bwe_spec", (size_t)Tn * ld * 4, (void**)&spec));
  GSV_RC(need(b, "bwe_x0", (size_t)2 * Tn * bp * es, &x0));
  GSV_RC(need(b, "bwe_x", (size_t)2 * Tn * C * es, &xb));
  GSV_RC(need(b, "bwe_r", (size_t)2 * Tn * C * es, &rb));
  GSV_RC(need(b, "bwe_a", (size_t)2 * Tn * C * es, &ab));
  GSV_RC(need(b, "bwe_h", (size_t)2 * Tn * 3 * C * es, &hb));

  // ---- resample + STFT (audio_sr.py:47-48, dataset.py:9-27)
  hipLaunchKernelGGL(bwe_frame_kernel<TI>, dim3(cdiv(F, 256), Tn), dim3(256), 0, s, wav, n, rt.k, rt.o, rt.q, rt.width, rt.L, n_new, F,
                     hop, Tn, frames, res);
  GSV_HIP(hipGetLastError());
  {
    ConvArgs a;
    a.x = frames; a.w = b->fwd; a.y = ri; a.T_in = a.T_out = a.T_virt = Tn; a.Cin = F; a.Cout = 2 * B; a.taps = 1;
    a.ldx = F; a.ldw = F; a.ldy = 2 * B; a.out_f32 = 1;
    GSV_RC(launch_conv_gemm(GSV_F32, a, s));
  }
  BWE_LAUNCH(bwe_logamp_kernel<T>, (long long)Tn * bp, ri, Tn, B, bp, la, pha, (T*)x0);

  // ---- conv_pre + norm_pre of both branches (model.py:123-126)
  {
    ConvArgs a;
    a.x = x0; a.w = b->pre_w; a.y = xb; a.bias = b->pre_b;
    a.T_in = a.T_out = a.T_virt = Tn; a.Cin = bp; a.Cout = C; a.taps = 7; a.pad = 3;
    a.ldx = bp; a.ldw = 7 * bp; a.ldy = C; a.ldr = C;
    a.Z = 2; a.xz = (long long)Tn * bp; a.wz = (long long)C * 7 * bp; a.yz = (long long)Tn * C; a.bz = C;
    GSV_RC(launch_conv_gemm(b->dtype, a, s));
  }
  for (int z = 0; z < 2; ++z) {
    void* p = (char*)xb + (size_t)z * Tn * C * es;
    GSV_RC(launch_layernorm(b->dtype, p, 0, nullptr, 0, b->pre_g + z * C, b->pre_beta + z * C, p, 0, Tn, C, 1e-6f, s));
  }

  // ---- ConvNeXt layers (model.py:129-133)
  for (int l = 0; l < g.layers; ++l) {
    const size_t o2 = (size_t)l * 2 * C;
    GSV_RC(launch_mix<T>(xb, Tn, C, b->dw_w + o2 * 7, b->dw_b + o2, b->ln_g + o2, b->ln_b + o2, rb, ab, s));
    const size_t wsz = (size_t)2 * 3 * C * C * es;
    GSV_RC(branch_gemm(b, s, ab, C, (char*)b->pw1 + l * wsz, b->pw1_b + (size_t)l * 2 * 3 * C, 3 * C, Tn, hb, ACT_GELU, nullptr, nullptr));
    GSV_RC(branch_gemm(b, s, hb, 3 * C, (char*)b->pw2 + l * wsz, b->pw2_b + o2, C, Tn, xb, ACT_NONE, b->gamma + o2, rb));
  }

  // ---- post head (model.py:135-141)
  for (int z = 0; z < 2; ++z) {
    const size_t off = (size_t)z * Tn * C * es;
    GSV_RC(launch_layernorm(b->dtype, (char*)xb + off, 0, nullptr, 0, b->post_g + z * C, b->post_beta + z * C, (char*)ab + off, 0, Tn, C,
                            1e-6f, s));
  }
  {
    ConvOpt om; om.out_f32 = 1; om.res = la; om.res_f32 = 1; om.ldr = B;
    GSV_RC(conv(b, s, b->post_mag, ab, C, Tn, mag, Tn, om));
    ConvOpt op; op.out_f32 = 1;
    GSV_RC(conv(b, s, b->post_pha, (char*)ab + (size_t)Tn * C * es, C, Tn, ri, Tn, op));
  }
  BWE_LAUNCH(bwe_spec_kernel, (long long)Tn * ld, mag, ri, Tn, B, ld, phawb, spec);

  // ---- iSTFT (dataset.py:30-37)
  {
    ConvArgs a;
    a.x = spec; a.w = b->inv; a.y = frames; a.T_in = a.T_out = a.T_virt = Tn; a.Cin = ld; a.Cout = F; a.taps = 1;
    a.ldx = ld; a.ldw = ld; a.ldy = F; a.out_f32 = 1;
    GSV_RC(launch_conv_gemm(GSV_F32, a, s));
  }
  if (L > 0) BWE_LAUNCH(bwe_ola_kernel, L, frames, b->win, Tn, F, hop, L, out);
  b->lastT = Tn; b->lastN = n_new;
  b->t_res = res; b->t_la = la; b->t_pha = pha; b->t_mag = mag; b->t_phawb = phawb;
  return GSV_OK;
}

// appends the staged tensor to dst
int fetch_into(Ctx* h, const std::string& name, size_t n, std::vector<float>& dst) {
  std::vector<float> v;
  if (!fetch(h, name, n, (int)n, v)) return GSV_ERR_ARG;
  dst.insert(dst.end(), v.begin(), v.end());
  return GSV_OK;
}

}  // namespace

extern "C" {

int gsv_bwe_create(const gsv_bwe_config* cfg, int dtype, gsv_bwe_t** out) {
  GSV_REQUIRE(cfg && out, "bwe_create: null argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "bwe_create: bad dtype");
  GSV_REQUIRE(cfg->n_fft >= 16 && cfg->n_fft % 8 == 0, "bwe_create: n_fft=%d must be a multiple of 8", cfg->n_fft);
  GSV_REQUIRE(cfg->win_size > 0 && cfg->win_size <= cfg->n_fft, "bwe_create: win_size=%d must be in (0, n_fft]", cfg->win_size);
  GSV_REQUIRE(cfg->hop_size > 0 && cfg->hop_size <= cfg->win_size && cfg->hop_size <= cfg->n_fft / 2,
              "bwe_create: hop_size=%d must be <= win_size and <= n_fft / 2", cfg->hop_size);
  const int C = cfg->channels;
  GSV_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512 || C == 768 || C == 1024,
              "bwe_create: ConvNeXt_channels=%d must be 64, 128, 256, 512, 768 or 1024", C);
  GSV_REQUIRE(cfg->layers >= 0 && cfg->hr_sampling_rate > 0, "bwe_create: bad layers / hr_sampling_rate");
  GSV_RC(require_device());
  gsv_bwe* b = new gsv_bwe();
  b->cfg = *cfg;
  b->dtype = dtype;
  b->bins = cfg->n_fft / 2 + 1;
  b->bp = (b->bins + 15) / 16 * 16;
  b->lds = (2 * b->bins + 3) / 4 * 4;
  *out = b;
  return GSV_OK;
}

void gsv_bwe_destroy(gsv_bwe_t* b) {
  if (!b) return;
  free_ctx(b);
  delete b;
}

int gsv_bwe_load_tensor(gsv_bwe_t* b, const char* name, const float* data, int64_t numel) {
  return stage_tensor(b, name, data, numel);
}

int gsv_bwe_finalize(gsv_bwe_t* b) {
  GSV_REQUIRE(b && !b->finalized, "bwe_finalize: bad handle");
  const auto& g = b->cfg;
  const int F = g.n_fft, C = g.channels, B = b->bins, bp = b->bp, ld = b->lds, NL = g.layers;
  // DFT bases (gsv/module/mel_processing.py::_dft_basis): forward [2 bins][n_fft], inverse [n_fft][2 bins] -> rows padded to lds
  {
    std::vector<float> fw, iv;
    GSV_RC(fetch_into(b, "dft.forward", (size_t)2 * B * F, fw));
    GSV_RC(fetch_into(b, "dft.inverse", (size_t)F * 2 * B, iv));
    // the DC and Nyquist rows of the imaginary half are exact zeros, as an FFT computes them (sin(pi n) of the float64 basis
    // is 1e-16, not 0: its sign would flip the phase of a bin with a negative real part between +pi and -pi)
    std::fill(fw.begin() + (size_t)B * F, fw.begin() + (size_t)(B + 1) * F, 0.f);
    std::fill(fw.begin() + (size_t)(2 * B - 1) * F, fw.end(), 0.f);
    GSV_RC(up_f32(b, fw.data(), fw.size(), &b->fwd));
    std::vector<float> ip((size_t)F * ld, 0.f), w(F);
    for (int r = 0; r < F; ++r) std::copy(iv.begin() + (size_t)r * 2 * B, iv.begin() + (size_t)(r + 1) * 2 * B, ip.begin() + (size_t)r * ld);
    GSV_RC(up_f32(b, ip.data(), ip.size(), &b->inv));
    for (int k = 0; k < F; ++k) w[k] = fw[k];                 // row 0 of the forward basis = the centred window (cos 0 = 1)
    GSV_RC(up_f32(b, w.data(), w.size(), &b->win));
  }
  const char* br[2] = {"mag", "pha"};
  {
    std::vector<float> pw((size_t)2 * C * 7 * bp, 0.f), pb, pg, pbeta, qg, qbeta;
    for (int z = 0; z < 2; ++z) {
      const std::string p = std::string("conv_pre_") + br[z];
      std::vector<float> w;
      if (!fetch(b, p + ".weight", (size_t)C * B * 7, C, w)) return GSV_ERR_ARG;
      for (int o = 0; o < C; ++o)
        for (int i = 0; i < B; ++i)
          for (int j = 0; j < 7; ++j) pw[(((size_t)z * C + o) * 7 + j) * bp + i] = w[((size_t)o * B + i) * 7 + j];
      GSV_RC(fetch_into(b, p + ".bias", C, pb));
      GSV_RC(fetch_into(b, std::string("norm_pre_") + br[z] + ".weight", C, pg));
      GSV_RC(fetch_into(b, std::string("norm_pre_") + br[z] + ".bias", C, pbeta));
      GSV_RC(fetch_into(b, std::string("norm_post_") + br[z] + ".weight", C, qg));
      GSV_RC(fetch_into(b, std::string("norm_post_") + br[z] + ".bias", C, qbeta));
    }
    GSV_RC(up_t(b, pw, &b->pre_w));
    GSV_RC(up_f32(b, pb.data(), pb.size(), &b->pre_b));
    GSV_RC(up_f32(b, pg.data(), pg.size(), &b->pre_g));
    GSV_RC(up_f32(b, pbeta.data(), pbeta.size(), &b->pre_beta));
    GSV_RC(up_f32(b, qg.data(), qg.size(), &b->post_g));
    GSV_RC(up_f32(b, qbeta.data(), qbeta.size(), &b->post_beta));
  }
  // ConvNeXt blocks, layer-major then branch: [L][2][...]
  {
    std::vector<float> dw, db, lg, lb, w1, b1, w2, b2, gm;
    for (int l = 0; l < NL; ++l)
      for (int z = 0; z < 2; ++z) {
        const std::string p = std::string("convnext_") + br[z] + "." + std::to_string(l) + ".";
        GSV_RC(fetch_into(b, p + "dwconv.weight", (size_t)C * 7, dw));
        GSV_RC(fetch_into(b, p + "dwconv.bias", C, db));
        GSV_RC(fetch_into(b, p + "norm.weight", C, lg));
        GSV_RC(fetch_into(b, p + "norm.bias", C, lb));
        GSV_RC(fetch_into(b, p + "pwconv1.weight", (size_t)3 * C * C, w1));
        GSV_RC(fetch_into(b, p + "pwconv1.bias", (size_t)3 * C, b1));
        GSV_RC(fetch_into(b, p + "pwconv2.weight", (size_t)3 * C * C, w2));
        GSV_RC(fetch_into(b, p + "pwconv2.bias", C, b2));
        GSV_RC(fetch_into(b, p + "gamma", C, gm));
      }
    if (NL > 0) {
      GSV_RC(up_f32(b, dw.data(), dw.size(), &b->dw_w));
      GSV_RC(up_f32(b, db.data(), db.size(), &b->dw_b));
      GSV_RC(up_f32(b, lg.data(), lg.size(), &b->ln_g));
      GSV_RC(up_f32(b, lb.data(), lb.size(), &b->ln_b));
      GSV_RC(up_t(b, w1, &b->pw1));
      GSV_RC(up_f32(b, b1.data(), b1.size(), &b->pw1_b));
      GSV_RC(up_t(b, w2, &b->pw2));
      GSV_RC(up_f32(b, b2.data(), b2.size(), &b->pw2_b));
      GSV_RC(up_f32(b, gm.data(), gm.size(), &b->gamma));
    }
  }
  GSV_RC(make_conv(b, "linear_post_mag", B, C, 1, true, &b->post_mag));
  GSV_RC(make_stacked(b, {"linear_post_pha_r", "linear_post_pha_i"}, B, C, &b->post_pha));
  b->staged.clear();
  b->finalized = true;
  return GSV_OK;
}

int gsv_bwe_out_len(gsv_bwe_t* b, int n, int orig_sr) {
  if (!b || n <= 0 || orig_sr <= 0) return -1;
  const int nw = b->cfg.hr_sampling_rate;
  long long n_new = n;
  if (orig_sr != nw) {
    const int g = std::gcd(orig_sr, nw);
    const long long o = orig_sr / g, q = nw / g;
    n_new = (q * n + o - 1) / o;
  }
  if (n_new <= b->cfg.n_fft / 2 || n_new > 0x7fffffffLL) return -1;
  return (int)(b->cfg.hop_size * (n_new / b->cfg.hop_size));
}

int gsv_bwe_forward(gsv_bwe_t* b, const void* wav, int n, int dtype, int orig_sr, float* out, gsv_stream_t stream) {
  GSV_REQUIRE(b && b->finalized, "bwe_forward: handle not finalized");
  GSV_REQUIRE(wav && out && n > 0 && orig_sr > 0, "bwe_forward: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "bwe_forward: bad input dtype");
  const int nw = b->cfg.hr_sampling_rate;
  long long n_new = n;
  if (orig_sr != nw) {
    const int g = std::gcd(orig_sr, nw);
    n_new = ((long long)(nw / g) * n + orig_sr / g - 1) / (orig_sr / g);
  }
  GSV_REQUIRE(n_new < (1LL << 30), "bwe_forward: %lld samples at %d Hz is too long", n_new, nw);
  GSV_REQUIRE(n_new > b->cfg.n_fft / 2, "bwe_forward: %lld samples at %d Hz are too short for the reflect padding of %d (torch.stft "
              "refuses them)", n_new, nw, b->cfg.n_fft / 2);
  ResampleTab* rt;
  GSV_RC(bwe_resample_tab(b, orig_sr, &rt));
  hipStream_t s = (hipStream_t)stream;
  const int nn = (int)n_new;
  if (b->dtype == GSV_F16) {
    if (dtype == GSV_F16) return bwe_forward_t<_Float16, _Float16>(b, s, (const _Float16*)wav, n, *rt, nn, out);
    return bwe_forward_t<_Float16, float>(b, s, (const float*)wav, n, *rt, nn, out);
  }
  if (dtype == GSV_F16) return bwe_forward_t<float, _Float16>(b, s, (const _Float16*)wav, n, *rt, nn, out);
  return bwe_forward_t<float, float>(b, s, (const float*)wav, n, *rt, nn, out);
}

int gsv_bwe_debug_tensor(gsv_bwe_t* b, const char* name, float* out, int64_t cap, int64_t* numel, gsv_stream_t stream) {
  GSV_REQUIRE(b && b->finalized && name && out && numel, "bwe_debug_tensor: bad argument");
  GSV_REQUIRE(b->lastT > 0, "bwe_debug_tensor: no forward yet");
  hipStream_t s = (hipStream_t)stream;
  const std::string n(name);
  const int Tn = b->lastT, B = b->bins;
  if (n == "resampled") {
    GSV_REQUIRE(cap >= b->lastN, "bwe_debug_tensor: buffer too small");
    GSV_HIP(hipMemcpyAsync(out, b->t_res, (size_t)b->lastN * 4, hipMemcpyDeviceToDevice, s));
    *numel = b->lastN;
    return GSV_OK;
  }
  const float* src = n == "log_amp" ? b->t_la : n == "pha" ? b->t_pha : n == "mag_wb" ? b->t_mag : n == "pha_wb" ? b->t_phawb : nullptr;
  GSV_REQUIRE(src, "bwe_debug_tensor: unknown tensor '%s' (resampled, log_amp, pha, mag_wb, pha_wb)", name);
  GSV_REQUIRE(cap >= (int64_t)Tn * B, "bwe_debug_tensor: buffer too small");
  BWE_LAUNCH(bwe_to_cf_kernel, (long long)Tn * B, src, Tn, B, out);
  *numel = (int64_t)Tn * B;
  return GSV_OK;
}

}  // extern "C"
