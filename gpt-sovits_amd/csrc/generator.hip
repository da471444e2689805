// HiFi-GAN generator engine for gfx950: the upsampling stages shared by the SoVITS v1/v2 decoder (H12, vits.hip runs its own
// conv_pre / conv_post around them) and the vocoders of the v3/v4 path: v4 = the HiFi-GAN `Generator` used as a mel vocoder
// (H16, reference TTS_infer_pack/TTS.py:631-648, module/models.py:407-471), v3 = BigVGAN-v2 (H15, reference
// BigVGAN/bigvgan.py:226-355 with AMPBlock1 :31-131 and anti-aliased SnakeBeta).  Channels-last activations and the conv
// kernels of the decoder: leaky-relu on operand load, ResBlock1 adds and the MRF mean in the conv epilogues; the vocoders'
// mel channels are zero-padded to a multiple of 8.
#include "engine.h"

namespace gsv {

// Anti-aliased snake / snakebeta on channels-last activations [T][C] (BigVGAN Activation1d,
// alias_free_activation/torch/act.py:25-30): 2x zero-stuffed 12-tap up-FIR -> x + sin^2(a x)/(b+1e-9)
// -> 12-tap stride-2 down-FIR, replicate padding as in aa.hip.  A workgroup owns 64 time steps x 64
// channels: rows are read/written 128 B wide (lane = channel), the 2x-rate intermediate lives in LDS.
template <typename T>
__global__ __launch_bounds__(256) void aa_act_cl_kernel(const T* __restrict__ x, T* __restrict__ y, int Tn, int C, int ld,
                                                        const float* __restrict__ alpha, const float* __restrict__ beta,
                                                        int logscale, const float* __restrict__ up12,
                                                        const float* __restrict__ dn12) {
  constexpr int TT = 64, CW = 64;
  __shared__ float xs[TT + 16][CW];
  __shared__ float as[2 * TT + 16][CW];
  __shared__ float uf[12], df[12];
  const int t0 = blockIdx.x * TT, c0 = blockIdx.y * CW;
  const int cl = threadIdx.x & 63, tq = threadIdx.x >> 6;
  const int c = c0 + cl;
  const bool cok = c < C;
  if (threadIdx.x < 12) { uf[threadIdx.x] = up12[threadIdx.x]; df[threadIdx.x] = dn12[threadIdx.x]; }
  float a = 1.f, ib = 1.f;
  if (cok) {
    a = logscale ? expf(alpha[c]) : alpha[c];
    ib = 1.f / ((logscale ? expf(beta[c]) : beta[c]) + 1e-9f);
  }
  for (int i = tq; i < TT + 16; i += 4) {
    const int t = min(max(t0 - 8 + i, 0), Tn - 1);
    xs[i][cl] = cok ? to_f(x[(long long)t * ld + c]) : 0.f;
  }
  __syncthreads();
  const int n0 = 2 * t0 - 8;
  for (int k = tq; k < 2 * TT + 16; k += 4) {
    const int n = min(max(n0 + k, 0), 2 * Tn - 1);
    const int ilo = (n + 5) >> 1;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int i = ilo + j;
      const int f = n + 15 - 2 * i;
      if (f >= 0 && f < 12) {
        const int xo = min(max(i - 5, 0), Tn - 1);
        acc += xs[xo - (t0 - 8)][cl] * uf[f];
      }
    }
    const float u = 2.f * acc;
    const float sn = sinf(u * a);
    as[k][cl] = u + ib * sn * sn;
  }
  __syncthreads();
  for (int i = tq; i < TT; i += 4) {
    const int t = t0 + i;
    if (t >= Tn || !cok) continue;
    float acc = 0.f;
#pragma unroll
    for (int f = 0; f < 12; ++f) acc += df[f] * as[2 * i + f + 3][cl];
    y[(long long)t * ld + c] = (T)acc;
  }
}

}  // namespace gsv

using namespace gsv;
using namespace gsveng;

struct gsv_vocoder {
  gsv_vits ctx;               // the allocation / staging / workspace context of the engine helpers
  gsv_vocoder_config cfg;
  int cin_pad = 0;
  Conv conv_pre, conv_post;
  GenW gen;
  bool finalized = false;
};

namespace gsveng {

// Kaiser-windowed sinc low-pass of BigVGAN's Activation1d (filter.py:30-60), cutoff 0.25, half-width 0.3, 12 taps
void kaiser_sinc12(float* out) {
  const int K = 12, half = 6;
  const double cutoff = 0.25, hw = 0.3;
  const double A = 2.285 * (half - 1) * M_PI * 4 * hw + 7.95;
  const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
  auto i0 = [](double x) { double s = 1.0, t = 1.0; for (int k = 1; k < 60; ++k) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; } return s; };
  double f[12], sum = 0.0;
  for (int n = 0; n < K; ++n) {
    const double r = 2.0 * n / (K - 1) - 1.0;
    const double win = i0(beta * sqrt(1.0 - r * r)) / i0(beta);
    const double t = (n - half) + 0.5;
    const double xx = 2 * cutoff * t;
    const double sinc = xx == 0.0 ? 1.0 : sin(M_PI * xx) / (M_PI * xx);
    f[n] = 2 * cutoff * win * sinc;
    sum += f[n];
  }
  for (int n = 0; n < K; ++n) out[n] = (float)(f[n] / sum);
}

template <typename T>
static int voc_act(gsv_vits* h, hipStream_t s, const GenW& g, const VocAct& a, const void* x, void* y, int Tn, int C) {
  GSV_LAUNCH(aa_act_cl_kernel<T>, dim3(cdiv(Tn, 64), cdiv(C, 64)), dim3(256), 0, s, (const T*)x, (T*)y, Tn, C, C, a.alpha, a.beta,
             g.snake_logscale, g.up12, g.dn12);
  return GSV_OK;
}

int load_generator(gsv_vits* h, const std::string& prefix, bool bigvgan, GenW* g) {
  auto load_act = [&](const std::string& name, int C) -> int {
    VocAct a;
    GSV_RC(make_vec(h, name + ".alpha", C, &a.alpha));
    if (h->staged.count(name + ".beta")) { GSV_RC(make_vec(h, name + ".beta", C, &a.beta)); }
    else a.beta = a.alpha;   // Snake: one parameter for both (activation1d.py:58-61)
    g->acts.push_back(a);
    return GSV_OK;
  };
  g->ups.resize(g->n_ups);
  int ch = g->uic;
  for (int i = 0; i < g->n_ups; ++i) {
    const int cin = g->uic >> i, cout = g->uic >> (i + 1);
    GSV_REQUIRE(cout % 8 == 0, "generator channel count %d must be a multiple of 8", cout);
    const std::string un = prefix + "ups." + std::to_string(i) + (bigvgan ? ".0" : "");
    GSV_RC(make_ups(h, un, cin, cout, g->up_kernels[i], g->up_rates[i], &g->ups[i]));
    ch = cout;
    for (int j = 0; j < g->n_resblocks; ++j) {
      const std::string r = prefix + "resblocks." + std::to_string(i * g->n_resblocks + j);
      for (int k = 0; k < 3; ++k) {
        Conv c1, c2;
        GSV_RC(make_conv(h, r + ".convs1." + std::to_string(k), ch, ch, g->rb_kernels[j], true, &c1));
        GSV_RC(make_conv(h, r + ".convs2." + std::to_string(k), ch, ch, g->rb_kernels[j], true, &c2));
        g->rb1.push_back(c1);
        g->rb2.push_back(c2);
      }
      if (bigvgan)
        for (int k = 0; k < 6; ++k) GSV_RC(load_act(r + ".activations." + std::to_string(k) + ".act", ch));
    }
  }
  if (bigvgan) {
    GSV_RC(load_act(prefix + "activation_post.act", ch));
    float f[12];
    kaiser_sinc12(f);
    GSV_RC(up_f32(h, f, 12, &g->up12));
    GSV_RC(up_f32(h, f, 12, &g->dn12));
  }
  return GSV_OK;
}

int gen_buffers(gsv_vits* h, const GenW& g, const char* name, int F, void** gb) {
  size_t maxel = (size_t)F * g.uic;
  long long Tn = F;
  int ch = g.uic;
  for (int i = 0; i < g.n_ups; ++i) { Tn *= g.up_rates[i]; ch >>= 1; maxel = std::max(maxel, (size_t)Tn * ch); }
  const int nb = g.acts.empty() ? 5 : 6;   // BigVGAN: one more, for the activation output
  for (int i = 0; i < nb; ++i) GSV_RC(need(h, (std::string(name) + std::to_string(i)).c_str(), maxel * esz(h), &gb[i]));
  return GSV_OK;
}

int run_generator_stages(gsv_vits* h, hipStream_t s, const GenW& g, void* const* gb, void** cur_io, int* Tn_io, int* const* seg_up) {
  const bool big = !g.acts.empty();
  void* cur = *cur_io;
  int Tn = *Tn_io, ch = g.uic, ai = 0;
  for (int i = 0; i < g.n_ups; ++i) {
    const int Tout = Tn * g.up_rates[i];
    ch >>= 1;
    void* xup = gb[0]; void* xt = gb[1]; void* R = gb[2]; void* xa = big ? gb[5] : nullptr; void* xs = (cur == gb[3]) ? gb[4] : gb[3];
    const int* seg_o = seg_up ? seg_up[i] : nullptr;   // gap rows of this stage's outputs
    h->dbg_last_in = cur; h->dbg_last_T = Tn; h->dbg_last_C = 2 * ch;
    { ConvOpt ou; ou.row_seg = seg_o;
      if (!big) { ou.pre_act = ACT_LRELU; ou.pre_slope = 0.1f; }
      GSV_RC(conv(h, s, g.ups[i], cur, ch * 2, Tn, xup, Tout, ou)); }
    for (int j = 0; j < g.n_resblocks; ++j) {
      const void* xr = xup;
      for (int k = 0; k < 3; ++k) {
        const Conv& c1 = g.rb1[(i * g.n_resblocks + j) * 3 + k];
        const Conv& c2 = g.rb2[(i * g.n_resblocks + j) * 3 + k];
        const int dil = g.rb_dilations[j][k];
        // segmented: the masked pair zeroes the gap rows of its LDS intermediate and of its output itself (conv_pair.hip, SEG);
        // GSV_NO_SEG_PAIR=1 is the A/B switch back to the two convs with their row passes
        static const bool no_seg_pair = getenv("GSV_NO_SEG_PAIR") != nullptr;
        if (!big && !(seg_o && no_seg_pair) && c1.b && c2.b && c1.taps == c2.taps && conv_pair_eligible(h->dtype, ch, c1.taps, dil, Tout, seg_o != nullptr)) {
          // narrow stages: the pair in one kernel, the intermediate tensor never leaves the CU (conv_pair.hip; 64 channels: conv_pair64.hip)
          ConvPairArgs pa;
          pa.x = (const _Float16*)xr; pa.w1 = (const _Float16*)c1.w; pa.b1 = c1.b; pa.w2 = (const _Float16*)c2.w; pa.b2 = c2.b;
          pa.T = Tout; pa.C = ch; pa.taps = c1.taps; pa.dil = dil; pa.ldx = ch; pa.ldy = ch;
          if (k < 2) { pa.y = (_Float16*)R; }
          else { pa.y = (_Float16*)xs; pa.scale = 1.f / (float)g.n_resblocks; pa.accumulate = j > 0; }
          // the pair reads x as window AND residual: it must not be overwritten in place
          if ((const void*)pa.y == xr) { pa.y = (_Float16*)xt; }
          if (seg_o) { GSV_RC(launch_conv_pair_seg(pa, seg_o, s)); }
          else { GSV_RC(launch_conv_pair(pa, s)); }
          if (k < 2) { if (pa.y == (_Float16*)xt) { std::swap(xt, R); } xr = R; }
          continue;
        }
        // convs1, then convs2 + residual, each on its activated input: leaky-relu on operand load, or BigVGAN's anti-aliased snake
        ConvOpt o1; o1.dil = dil; o1.row_seg = seg_o;
        ConvOpt o2; o2.res = xr; o2.ldr = ch; o2.row_seg = seg_o;
        const void *in1 = xr, *in2 = xt;
        if (!big) { o1.pre_act = ACT_LRELU; o1.pre_slope = 0.1f; o2.pre_act = ACT_LRELU; o2.pre_slope = 0.1f; }
        if (big) { GSV_RC(GSV_WITH_T(h, voc_act<T>(h, s, g, g.acts[ai + 2 * k], xr, xa, Tout, ch))); in1 = xa; }
        GSV_RC(conv(h, s, c1, in1, ch, Tout, xt, Tout, o1));
        if (big) { GSV_RC(GSV_WITH_T(h, voc_act<T>(h, s, g, g.acts[ai + 2 * k + 1], xt, xa, Tout, ch))); in2 = xa; }
        if (k < 2) {
          GSV_RC(conv(h, s, c2, in2, ch, Tout, R, Tout, o2));
          xr = R;
        } else {
          o2.scale = 1.f / (float)g.n_resblocks; o2.accumulate = j > 0;   // the MRF mean over the blocks
          GSV_RC(conv(h, s, c2, in2, ch, Tout, xs, Tout, o2));
        }
      }
      if (big) ai += 6;
    }
    cur = xs; Tn = Tout;
  }
  *cur_io = cur; *Tn_io = Tn;
  return GSV_OK;
}

}  // namespace gsveng

extern "C" {

int gsv_vocoder_create(const gsv_vocoder_config* cfg, int dtype, gsv_vocoder_t** out) {
  GSV_REQUIRE(cfg && out, "vocoder_create: null argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "vocoder_create: bad dtype");
  GSV_REQUIRE(cfg->n_ups >= 1 && cfg->n_ups <= 8 && cfg->n_resblocks >= 1 && cfg->n_resblocks <= 4, "vocoder_create: bad shape");
  GSV_REQUIRE(cfg->kind == 0 || cfg->kind == 1, "vocoder_create: kind must be 0 (HiFi-GAN) or 1 (BigVGAN)");
  GSV_REQUIRE((cfg->upsample_initial_channel >> cfg->n_ups) % 8 == 0, "vocoder_create: final channel count must be a multiple of 8");
  int n = 0;
  GSV_HIP(hipGetDeviceCount(&n));
  gsv_vocoder* v = new gsv_vocoder();
  v->cfg = *cfg;
  v->ctx.dtype = dtype;
  v->cin_pad = (cfg->in_channels + 7) / 8 * 8;
  *out = v;
  return GSV_OK;
}

void gsv_vocoder_destroy(gsv_vocoder_t* v) {
  if (!v) return;
  free_ctx(&v->ctx);
  delete v;
}

int gsv_vocoder_load_tensor(gsv_vocoder_t* v, const char* name, const float* data, int64_t numel) {
  GSV_REQUIRE(v && name && data && numel > 0, "vocoder_load_tensor: bad argument");
  GSV_REQUIRE(!v->finalized, "vocoder_load_tensor: handle already finalized");
  v->ctx.staged[name].assign(data, data + numel);
  return GSV_OK;
}

int gsv_vocoder_finalize(gsv_vocoder_t* v) {
  GSV_REQUIRE(v && !v->finalized, "vocoder_finalize: bad handle");
  gsv_vits* h = &v->ctx;
  const auto& c = v->cfg;
  GSV_RC(make_conv_padded(h, "conv_pre", c.upsample_initial_channel, c.in_channels, v->cin_pad, 7, true, &v->conv_pre));
  gen_shape(c, &v->gen);
  v->gen.snake_logscale = c.snake_logscale;
  GSV_RC(load_generator(h, "", c.kind == 1, &v->gen));
  GSV_RC(make_conv(h, "conv_post", 1, c.upsample_initial_channel >> c.n_ups, 7, c.bias_at_final != 0, &v->conv_post));
  h->staged.clear();
  h->finalized = true;
  v->finalized = true;
  return GSV_OK;
}

int gsv_vocoder_forward(gsv_vocoder_t* v, const float* mel, int F, float* wav, gsv_stream_t stream) {
  GSV_REQUIRE(v && v->finalized, "vocoder_forward: handle not finalized");
  GSV_REQUIRE(mel && wav && F >= 1, "vocoder_forward: empty input");
  hipStream_t s = (hipStream_t)stream;
  gsv_vits* h = &v->ctx;
  const auto& c = v->cfg;
  const size_t es = esz(h);
  const bool big = c.kind == 1;
  void* xin;
  GSV_RC(need(h, "voc_in", (size_t)F * v->cin_pad * es, &xin));
  GSV_HIP(hipMemsetAsync(xin, 0, (size_t)F * v->cin_pad * es, s));
  GSV_RC(cf_to_cl(h, s, mel, F, c.in_channels, xin, v->cin_pad));
  void* gb[6];
  GSV_RC(gen_buffers(h, v->gen, "v", F, gb));
  void* cur = gb[3];
  { ConvOpt o; GSV_RC(conv(h, s, v->conv_pre, xin, v->cin_pad, F, cur, F, o)); }
  int Tn = F;
  const int ch = c.upsample_initial_channel >> c.n_ups;
  GSV_RC(run_generator_stages(h, s, v->gen, gb, &cur, &Tn));
  ConvOpt op; op.out_f32 = 1;
  const void* pin = cur;
  if (big) { GSV_RC(GSV_WITH_T(h, voc_act<T>(h, s, v->gen, v->gen.acts.back(), cur, gb[5], Tn, ch))); pin = gb[5]; }
  else { op.pre_act = ACT_LRELU; op.pre_slope = 0.01f; }
  op.post_act = c.tanh_at_final ? ACT_TANH : ACT_CLAMP1;
  GSV_RC(conv(h, s, v->conv_post, pin, ch, Tn, wav, Tn, op));
  return GSV_OK;
}

}  // extern "C"
