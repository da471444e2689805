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
// SEG = the activation of a segmented pass (gsv_vocoder_forward_segments): row_seg holds one int32 per row, -1 = gap row, and
// segment s covers rows [seg_start[s], seg_start[s] + seg_len[s]).  Both replicate paddings stop at the row's own segment: the
// up-FIR clamps its x index to the segment's rows [a, b - 1], the down-FIR clamps its 2x-rate index to [2a, 2b - 1], so the
// intermediate is only ever computed at positions inside a segment (where it belongs to that segment alone) and the taps of an
// output row reach it through the clamp.  Gap rows of x are staged but never named by a clamped index; gap rows of y are stored
// as 0.  The clamps move an index towards the row it serves, so the staged halos of the plain kernel hold every row they can
// name, however many segments a tile holds.  Everything SEG adds sits under `if constexpr (SEG)`; the three maps are trailing
// kernel arguments the plain instantiations never read.
template <typename T, bool SEG = false>
__global__ __launch_bounds__(256) void aa_act_cl_kernel(const T* __restrict__ x, T* __restrict__ y, int Tn, int C, int ld,
                                                        const float* __restrict__ alpha, const float* __restrict__ beta,
                                                        int logscale, const float* __restrict__ up12,
                                                        const float* __restrict__ dn12, const int* __restrict__ row_seg,
                                                        const int* __restrict__ seg_start, const int* __restrict__ seg_len) {
  constexpr int TT = 64, CW = 64;
  __shared__ float xs[TT + 16][CW];
  __shared__ float as[2 * TT + 16][CW];
  __shared__ float uf[12], df[12];
  __shared__ int sa[SEG ? TT + 16 : 1], sl[SEG ? TT + 16 : 1];   // SEG: first and last row of the staged row's segment, -1 = none
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
  if constexpr (SEG) {
    if (threadIdx.x < TT + 16) {
      const int r = t0 - 8 + (int)threadIdx.x;
      int fa = -1, fl = -1;
      if (r >= 0 && r < Tn) {
        const int sg = row_seg[r];
        if (sg >= 0) { fa = seg_start[sg]; fl = fa + seg_len[sg] - 1; }
      }
      sa[threadIdx.x] = fa; sl[threadIdx.x] = fl;
    }
  }
  for (int i = tq; i < TT + 16; i += 4) {
    const int t = min(max(t0 - 8 + i, 0), Tn - 1);
    xs[i][cl] = cok ? to_f(x[(long long)t * ld + c]) : 0.f;
  }
  __syncthreads();
  const int n0 = 2 * t0 - 8;
  for (int k = tq; k < 2 * TT + 16; k += 4) {
    int n, xlo = 0, xhi = Tn - 1;
    if constexpr (SEG) {
      n = n0 + k;                               // the position itself: it is read through the down-FIR's clamp
      const int ri = (n >> 1) - (t0 - 8);       // its row among the staged ones, 4 .. TT + 11
      xlo = sa[ri]; xhi = sl[ri];
      if (xlo < 0) { as[k][cl] = 0.f; continue; }   // a gap or past the ends: no clamped index names it
    } else {
      n = min(max(n0 + k, 0), 2 * Tn - 1);
    }
    const int ilo = (n + 5) >> 1;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int i = ilo + j;
      const int f = n + 15 - 2 * i;
      if (f >= 0 && f < 12) {
        const int xo = min(max(i - 5, xlo), xhi);
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
    if constexpr (SEG) {
      const int fa = sa[i + 8];
      if (fa >= 0) {
        const int lo = 2 * fa - n0, hi = 2 * sl[i + 8] + 1 - n0;
#pragma unroll
        for (int f = 0; f < 12; ++f) acc += df[f] * as[min(max(2 * i + f + 3, lo), hi)][cl];
      }
    } else {
#pragma unroll
      for (int f = 0; f < 12; ++f) acc += df[f] * as[2 * i + f + 3][cl];
    }
    y[(long long)t * ld + c] = (T)acc;
  }
}

// mel fp32 channels-first [C][Fn], the segments packed without gaps -> channels-last [F][ldd] in the gapped layout of a
// segmented pass: row t of segment row_seg[t] is packed column t - row_seg[t] * G (every gap before it is G rows); gap rows and
// the columns C .. ldd are 0
template <typename T>
__global__ void pack_mel_seg_kernel(const float* __restrict__ src, int Fn, int C, const int* __restrict__ row_seg, int G, int F,
                                    T* __restrict__ dst, int ldd) {
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  {
    const int t = t0 + tx;
    const int sg = t < F ? row_seg[t] : -1;
    const int col = sg >= 0 ? t - sg * G : -1;
    for (int i = ty; i < 32; i += 8) {
      const int c = c0 + i;
      tile[i][tx] = (c < C && col >= 0 && col < Fn) ? src[(long long)c * Fn + col] : 0.f;
    }
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (t < F && c < ldd) dst[(long long)t * ldd + c] = (T)tile[tx][i];
  }
}

}  // namespace gsv

using namespace gsv;
using namespace gsveng;

struct gsv_vocoder : gsveng::Ctx {
  gsv_vocoder() : Ctx("vocoder") {}
  gsv_vocoder_config cfg;
  int cin_pad = 0;
  Conv conv_pre, conv_post;
  GenW gen;
  SegUpload seg;              // maps of the last segmented pass
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

// the anti-aliased activation on x [Tn][C] -> y; m != null (segmented pass): replicate padding per segment, gap rows of y = 0
template <typename T>
static int launch_aa_act(hipStream_t s, const void* x, void* y, int Tn, int C, const float* alpha, const float* beta, int logscale,
                         const float* up12, const float* dn12, const SegRows* m) {
  const dim3 grid(cdiv(Tn, 64), cdiv(C, 64));
  if (m) {
    auto kern = aa_act_cl_kernel<T, true>;
    GSV_LAUNCH(kern, grid, dim3(256), 0, s, (const T*)x, (T*)y, Tn, C, C, alpha, beta, logscale, up12, dn12, m->row_seg, m->start, m->len);
  } else {
    auto kern = aa_act_cl_kernel<T, false>;
    GSV_LAUNCH(kern, grid, dim3(256), 0, s, (const T*)x, (T*)y, Tn, C, C, alpha, beta, logscale, up12, dn12, (const int*)nullptr,
               (const int*)nullptr, (const int*)nullptr);
  }
  return GSV_OK;
}

template <typename T>
static int voc_act(Ctx* h, hipStream_t s, const GenW& g, const VocAct& a, const void* x, void* y, int Tn, int C,
                   const SegRows* m = nullptr) {
  return launch_aa_act<T>(s, x, y, Tn, C, a.alpha, a.beta, g.snake_logscale, g.up12, g.dn12, m);
}

// The gap of a segmented pass, in frames, as far as a generator decides it: at every resolution it covers the one-sided input
// reach of each conv reading that resolution -- conv_pre and conv_post (7 taps), the transposed ups[i], every ResBlock conv -- so a
// conv of a segment row reads zeros (its isolated zero padding) wherever it would reach past the segment's edge, and never the
// neighbour's rows.  BigVGAN's activation adds nothing: it never reads a gap row (aa_act_cl_kernel, SEG).
int gen_gap(const GenW& c) {
  auto need_at = [](int r, long long cum) { return (int)((r + cum - 1) / cum); };
  int g = std::max(1, conv_reach(7, 1));          // conv_pre
  long long cum = 1;
  for (int i = 0; i < c.n_ups; ++i) {
    // ups[i] reads resolution `cum`: transposed conv, kernel k, stride u, padding (k - u) / 2; output row t reads input rows
    // (t + p - j) / u, j < k: ceil((k - 1 - p) / u) to the left of a segment, floor((u - 1 + p) / u) to its right
    const int u = c.up_rates[i], k = c.up_kernels[i], p = (k - u) / 2;
    g = std::max(g, need_at(std::max((k - 1 - p + u - 1) / u, (u - 1 + p) / u), cum));
    cum *= u;
    for (int j = 0; j < c.n_resblocks; ++j)        // ResBlock1 convs1 (dilated) and convs2 (dilation 1); a conv_pair counts as both
      for (int d = 0; d < 3; ++d) g = std::max(g, need_at(conv_reach(c.rb_kernels[j], c.rb_dilations[j][d]), cum));
  }
  g = std::max(g, need_at(conv_reach(7, 1), cum));   // conv_post
  return g;
}

int load_generator(Ctx* h, const std::string& prefix, bool bigvgan, GenW* g) {
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

int gen_buffers(Ctx* h, const GenW& g, const char* name, int F, void** gb) {
  size_t maxel = (size_t)F * g.uic;
  long long Tn = F;
  int ch = g.uic;
  for (int i = 0; i < g.n_ups; ++i) { Tn *= g.up_rates[i]; ch >>= 1; maxel = std::max(maxel, (size_t)Tn * ch); }
  const int nb = g.acts.empty() ? 5 : 6;   // BigVGAN: one more, for the activation output
  for (int i = 0; i < nb; ++i) GSV_RC(need(h, (std::string(name) + std::to_string(i)).c_str(), maxel * esz(h), &gb[i]));
  return GSV_OK;
}

int run_generator_stages(Ctx* h, hipStream_t s, const GenW& g, void* const* gb, void** cur_io, int* Tn_io, int* const* seg_up,
                         const SegRows* seg_act, GenTap* tap) {
  const bool big = !g.acts.empty();
  void* cur = *cur_io;
  int Tn = *Tn_io, ch = g.uic, ai = 0;
  GSV_REQUIRE(!(big && seg_up) || seg_act, "generator: a segmented BigVGAN pass needs the activation's rows");
  for (int i = 0; i < g.n_ups; ++i) {
    const int Tout = Tn * g.up_rates[i];
    ch >>= 1;
    void* xup = gb[0]; void* xt = gb[1]; void* R = gb[2]; void* xa = big ? gb[5] : nullptr; void* xs = (cur == gb[3]) ? gb[4] : gb[3];
    const int* seg_o = seg_up ? seg_up[i] : nullptr;   // gap rows of this stage's outputs
    const SegRows* seg_a = seg_o && big ? &seg_act[i] : nullptr;   // BigVGAN: the same rows with each segment's first row and count
    if (tap) *tap = GenTap{cur, Tn, 2 * ch};
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
        if (big) { GSV_RC(GSV_WITH_T(h, voc_act<T>(h, s, g, g.acts[ai + 2 * k], xr, xa, Tout, ch, seg_a))); in1 = xa; }
        GSV_RC(conv(h, s, c1, in1, ch, Tout, xt, Tout, o1));
        if (big) { GSV_RC(GSV_WITH_T(h, voc_act<T>(h, s, g, g.acts[ai + 2 * k + 1], xt, xa, Tout, ch, seg_a))); in2 = xa; }
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

// ---------------------------------------------------------------------------------------
// segmented pass: n mels back to back with G zero gap frames between neighbours
// ---------------------------------------------------------------------------------------
namespace {

struct VocLayout {
  int G = 0;
  long long F = 0, Fn = 0, up = 1;     // frames with / without gaps, samples per frame
  std::vector<int> f0;                 // first frame row of each segment
};

// checks n and frames and lays the segments out; fails before anything is launched
int voc_layout(const gsv_vocoder_config& c, int n, const int* frames, VocLayout* o) {
  GSV_REQUIRE(c.n_ups >= 1 && c.n_ups <= 8 && c.n_resblocks >= 1 && c.n_resblocks <= 4, "vocoder segments: bad config");
  GSV_REQUIRE(frames, "vocoder segments: frames is null");
  GSV_REQUIRE(n >= 1 && n <= 4096, "vocoder segments: bad segment count %d", n);
  GenW shape;
  gen_shape(c, &shape);
  o->G = gen_gap(shape);
  o->up = 1;
  for (int i = 0; i < c.n_ups; ++i) {
    GSV_REQUIRE(c.up_rates[i] >= 1, "vocoder segments: bad config");
    o->up *= c.up_rates[i];
  }
  o->f0.resize(n);
  long long f = 0, fn = 0;
  for (int i = 0; i < n; ++i) {
    GSV_REQUIRE(frames[i] >= 1, "vocoder segments: segment %d is empty (%d frames)", i, frames[i]);
    if (i) f += o->G;
    o->f0[i] = (int)f;
    f += frames[i]; fn += frames[i];
    GSV_REQUIRE(f * o->up < (1LL << 24), "vocoder segments: too long (2^24 rows or more at the output rate)");
  }
  o->F = f; o->Fn = fn;
  return GSV_OK;
}

template <typename T>
int pack_mel(hipStream_t s, const float* mel, int Fn, int C, const int* row_seg, int G, int F, void* dst, int ldd) {
  GSV_LAUNCH(pack_mel_seg_kernel<T>, dim3(cdiv(F, 32), cdiv(ldd, 32)), dim3(256), 0, s, mel, Fn, C, row_seg, G, F, (T*)dst, ldd);
  return GSV_OK;
}

// the 12 Kaiser-sinc taps on the current device for gsv_op_aa_act_cl (an engine keeps its own)
int op_filter(const float** out) {
  static float* taps[64] = {};
  int dev = 0;
  GSV_HIP(hipGetDevice(&dev));
  GSV_REQUIRE(dev >= 0 && dev < 64, "op_aa_act_cl: device %d", dev);
  if (!taps[dev]) {
    float f[12];
    kaiser_sinc12(f);
    float* p = nullptr;
    GSV_HIP(hipMalloc((void**)&p, sizeof(f)));
    GSV_HIP(hipMemcpy(p, f, sizeof(f), hipMemcpyHostToDevice));
    taps[dev] = p;
  }
  *out = taps[dev];
  return GSV_OK;
}

}  // namespace

extern "C" {

int gsv_vocoder_create(const gsv_vocoder_config* cfg, int dtype, gsv_vocoder_t** out) {
  GSV_REQUIRE(cfg && out, "vocoder_create: null argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "vocoder_create: bad dtype");
  GSV_REQUIRE(cfg->n_ups >= 1 && cfg->n_ups <= 8 && cfg->n_resblocks >= 1 && cfg->n_resblocks <= 4, "vocoder_create: bad shape");
  GSV_REQUIRE(cfg->kind == 0 || cfg->kind == 1, "vocoder_create: kind must be 0 (HiFi-GAN) or 1 (BigVGAN)");
  GSV_REQUIRE((cfg->upsample_initial_channel >> cfg->n_ups) % 8 == 0, "vocoder_create: final channel count must be a multiple of 8");
  GSV_RC(require_device());
  gsv_vocoder* v = new gsv_vocoder();
  v->cfg = *cfg;
  v->dtype = dtype;
  v->cin_pad = (cfg->in_channels + 7) / 8 * 8;
  *out = v;
  return GSV_OK;
}

void gsv_vocoder_destroy(gsv_vocoder_t* v) {
  if (!v) return;
  free_ctx(v);
  delete v;
}

int gsv_vocoder_load_tensor(gsv_vocoder_t* v, const char* name, const float* data, int64_t numel) {
  return stage_tensor(v, name, data, numel);
}

int gsv_vocoder_finalize(gsv_vocoder_t* v) {
  GSV_REQUIRE(v && !v->finalized, "vocoder_finalize: bad handle");
  const auto& c = v->cfg;
  GSV_RC(make_conv_padded(v, "conv_pre", c.upsample_initial_channel, c.in_channels, v->cin_pad, 7, true, &v->conv_pre));
  gen_shape(c, &v->gen);
  v->gen.snake_logscale = c.snake_logscale;
  GSV_RC(load_generator(v, "", c.kind == 1, &v->gen));
  GSV_RC(make_conv(v, "conv_post", 1, c.upsample_initial_channel >> c.n_ups, 7, c.bias_at_final != 0, &v->conv_post));
  v->staged.clear();
  v->finalized = true;
  return GSV_OK;
}

int gsv_vocoder_forward(gsv_vocoder_t* v, const float* mel, int F, float* wav, gsv_stream_t stream) {
  GSV_REQUIRE(v && v->finalized, "vocoder_forward: handle not finalized");
  GSV_REQUIRE(mel && wav && F >= 1, "vocoder_forward: empty input");
  hipStream_t s = (hipStream_t)stream;
  const auto& c = v->cfg;
  const size_t es = esz(v);
  const bool big = c.kind == 1;
  void* xin;
  GSV_RC(need(v, "voc_in", (size_t)F * v->cin_pad * es, &xin));
  GSV_HIP(hipMemsetAsync(xin, 0, (size_t)F * v->cin_pad * es, s));
  GSV_RC(cf_to_cl(v, s, mel, F, c.in_channels, xin, v->cin_pad));
  void* gb[6];
  GSV_RC(gen_buffers(v, v->gen, "v", F, gb));
  void* cur = gb[3];
  { ConvOpt o; GSV_RC(conv(v, s, v->conv_pre, xin, v->cin_pad, F, cur, F, o)); }
  int Tn = F;
  const int ch = c.upsample_initial_channel >> c.n_ups;
  GSV_RC(run_generator_stages(v, s, v->gen, gb, &cur, &Tn));
  ConvOpt op; op.out_f32 = 1;
  const void* pin = cur;
  if (big) { GSV_RC(GSV_WITH_T(v, voc_act<T>(v, s, v->gen, v->gen.acts.back(), cur, gb[5], Tn, ch))); pin = gb[5]; }
  else { op.pre_act = ACT_LRELU; op.pre_slope = 0.01f; }
  op.post_act = c.tanh_at_final ? ACT_TANH : ACT_CLAMP1;
  GSV_RC(conv(v, s, v->conv_post, pin, ch, Tn, wav, Tn, op));
  return GSV_OK;
}

int gsv_vocoder_segment_gap(const gsv_vocoder_config* cfg) {
  if (!cfg || cfg->n_ups < 1 || cfg->n_ups > 8 || cfg->n_resblocks < 1 || cfg->n_resblocks > 4) return -1;
  GenW shape;
  gen_shape(*cfg, &shape);
  return gen_gap(shape);
}

int gsv_vocoder_segment_map(const gsv_vocoder_config* cfg, int n, const int* frames, int level, int32_t* seg, int64_t cap) {
  GSV_REQUIRE(cfg && seg, "vocoder_segment_map: null argument");
  VocLayout lay;
  GSV_RC(voc_layout(*cfg, n, frames, &lay));
  GSV_REQUIRE(level >= 0 && level <= cfg->n_ups, "vocoder_segment_map: level %d outside [0, %d]", level, cfg->n_ups);
  long long up = 1;
  for (int i = 0; i < level; ++i) up *= cfg->up_rates[i];
  const long long nr = lay.F * up;
  GSV_REQUIRE(cap >= nr, "vocoder_segment_map: buffer holds %lld rows, need %lld", (long long)cap, nr);
  for (long long t = 0; t < nr; ++t) seg[t] = -1;
  for (int i = 0; i < n; ++i)
    for (long long t = lay.f0[i] * up; t < (lay.f0[i] + (long long)frames[i]) * up; ++t) seg[t] = i;
  return GSV_OK;
}

int gsv_vocoder_forward_segments(gsv_vocoder_t* v, const float* mel, int n, const int* frames, float* wav, gsv_stream_t stream) {
  GSV_REQUIRE(v && v->finalized, "vocoder_forward_segments: handle not finalized");
  GSV_REQUIRE(mel && wav && frames, "vocoder_forward_segments: null argument");
  VocLayout lay;
  GSV_RC(voc_layout(v->cfg, n, frames, &lay));
  if (n == 1) return gsv_vocoder_forward(v, mel, frames[0], wav, stream);   // no gap, no maps: the plain path itself
  hipStream_t s = (hipStream_t)stream;
  const auto& c = v->cfg;
  const size_t es = esz(v);
  const bool big = c.kind == 1;
  const int F = (int)lay.F, nu = c.n_ups;
  // host image of the maps, one upload: seg_f [F] | per level 1 .. n_ups: first row [n] | rows [n]
  GSV_RC(seg_upload_begin(&v->seg));         // the previous call's upload (any stream) is done before its host image is rewritten
  std::vector<int>& m = v->seg.maps;
  const size_t o_sl = (size_t)F, total = o_sl + 2 * (size_t)nu * n;
  m.assign(total, -1);
  for (int i = 0; i < n; ++i)
    for (int t = lay.f0[i]; t < lay.f0[i] + frames[i]; ++t) m[t] = i;
  {
    long long up = 1;
    for (int l = 0; l < nu; ++l) {
      up *= c.up_rates[l];
      for (int i = 0; i < n; ++i) {
        m[o_sl + (size_t)(2 * l) * n + i] = (int)(lay.f0[i] * up);
        m[o_sl + (size_t)(2 * l + 1) * n + i] = (int)(frames[i] * up);
      }
    }
  }
  int* dm;
  GSV_RC(need(v, "voc_seg_maps", total * 4, (void**)&dm));
  GSV_HIP(hipMemcpyAsync(dm, m.data(), total * 4, hipMemcpyHostToDevice, s));
  GSV_HIP(hipEventRecord(v->seg.ev, s));
  const int* seg_f = dm;
  std::vector<int*> seg_up(nu);
  std::vector<SegRows> seg_act(nu);
  {
    long long up = 1;
    for (int l = 0; l < nu; ++l) {
      up *= c.up_rates[l];
      GSV_RC(need(v, ("voc_seg_up" + std::to_string(l)).c_str(), (size_t)F * up * 4, (void**)&seg_up[l]));
      GSV_RC(launch_expand_seg(s, seg_f, (int)up, (long long)F * up, seg_up[l]));
      seg_act[l].row_seg = seg_up[l];
      seg_act[l].start = dm + o_sl + (size_t)(2 * l) * n;
      seg_act[l].len = dm + o_sl + (size_t)(2 * l + 1) * n;
    }
  }
  void* xin;
  GSV_RC(need(v, "voc_in", (size_t)F * v->cin_pad * es, &xin));
  GSV_RC(GSV_WITH_T(v, pack_mel<T>(s, mel, (int)lay.Fn, c.in_channels, seg_f, lay.G, F, xin, v->cin_pad)));
  void* gb[6];
  GSV_RC(gen_buffers(v, v->gen, "v", F, gb));
  void* cur = gb[3];
  { ConvOpt o; o.row_seg = seg_f; GSV_RC(conv(v, s, v->conv_pre, xin, v->cin_pad, F, cur, F, o)); }
  int Tn = F;
  const int ch = c.upsample_initial_channel >> c.n_ups;
  GSV_RC(run_generator_stages(v, s, v->gen, gb, &cur, &Tn, seg_up.data(), seg_act.data()));
  ConvOpt op; op.out_f32 = 1;
  const void* pin = cur;
  if (big) { GSV_RC(GSV_WITH_T(v, voc_act<T>(v, s, v->gen, v->gen.acts.back(), cur, gb[5], Tn, ch, &seg_act[nu - 1]))); pin = gb[5]; }
  else { op.pre_act = ACT_LRELU; op.pre_slope = 0.01f; }
  op.post_act = c.tanh_at_final ? ACT_TANH : ACT_CLAMP1;
  float* wpad;                         // the padded waveform, then the gaps are dropped into wav
  GSV_RC(need(v, "voc_wav_pad", (size_t)Tn * 4, (void**)&wpad));
  GSV_RC(conv(v, s, v->conv_post, pin, ch, Tn, wpad, Tn, op));
  GSV_RC(launch_compact_wav(s, wpad, seg_f, (int)lay.up, lay.G * lay.up, (long long)Tn, wav));
  return GSV_OK;
}

int gsv_op_aa_act_cl(const void* x, void* y, int Tn, int C, const float* alpha, const float* beta, int logscale, const int32_t* row_seg,
                     const int32_t* seg_start, const int32_t* seg_len, int n_seg, int dtype, gsv_stream_t stream) {
  GSV_REQUIRE(x && y && alpha && beta && Tn >= 1 && C >= 1, "op_aa_act_cl: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_aa_act_cl: bad dtype");
  GSV_REQUIRE(!row_seg || (seg_start && seg_len && n_seg >= 1), "op_aa_act_cl: a row map needs seg_start, seg_len and n_seg >= 1");
  const float* taps = nullptr;
  GSV_RC(op_filter(&taps));
  SegRows m;
  m.row_seg = row_seg; m.start = seg_start; m.len = seg_len;
  return GSV_WITH_DTYPE(dtype, launch_aa_act<T>((hipStream_t)stream, x, y, Tn, C, alpha, beta, logscale, taps, taps, row_seg ? &m : nullptr));
}

}  // extern "C"
