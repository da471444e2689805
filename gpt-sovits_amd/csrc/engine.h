// Engine context shared by the SoVITS decoder (vits.hip), the generator and vocoders (generator.hip), the flow-matching DiT
// (cfm.hip) and the AP-BWE super-sampler (bwe.hip): weight staging / upload, workspace arena, and the conv / attention /
// generator launch helpers.
#pragma once
#include <math.h>
#include <map>
#include <string>
#include <vector>

#include "common.h"

struct Conv {
  void* w = nullptr;     // T [cout][taps*cin]
  float* b = nullptr;    // fp32 [cout_real] or null
  int cin = 0, cout = 0, taps = 1;
  int ups_u = 0, ups_pad = 0, ups_cout = 0;
};

struct AttnLayerW { Conv qkv, o; float *rel_k = nullptr, *rel_v = nullptr; float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; Conv f1, f2; };
// modules.WN: per layer in_layers (kernel 5) and res_skip_layers (1x1); in_bias_eff = in_layers bias + cond_layer(ge) (fp32 [2H])
struct WNW { std::vector<Conv> in, res; std::vector<float*> in_bias_eff; Conv cond; };
struct FlowW { Conv pre, post; WNW wn; };

// HiFi-GAN / BigVGAN upsampling stages (everything between conv_pre and conv_post) with the shape they need
struct VocAct { float *alpha = nullptr, *beta = nullptr; };
struct GenW {
  int uic = 0, n_ups = 0, n_resblocks = 0;     // uic = upsample_initial_channel, halved by every stage
  int up_rates[8], up_kernels[8], rb_kernels[4], rb_dilations[4][3];
  std::vector<Conv> ups, rb1, rb2;             // rb1 / rb2 = convs1 / convs2, [stage][block][3]
  // BigVGAN only (empty / null for HiFi-GAN): anti-aliased snake parameters [stage][block][6] + activation_post, the two FIRs
  std::vector<VocAct> acts;
  int snake_logscale = 0;
  float *up12 = nullptr, *dn12 = nullptr;
};

struct Buf { void* p = nullptr; size_t cap = 0; };

struct gsv_vits {
  gsv_vits_config cfg;
  int dtype;
  bool finalized = false, has_ref = false;
  std::map<std::string, std::vector<float>> staged;
  std::vector<void*> allocs;
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
  std::vector<int> seg_host;                    // host image of the last segmented decode's maps (alive until its copy is done:
  std::vector<unsigned long long> seed_host;    // seg_ev, recorded after the upload)
  hipEvent_t seg_ev = nullptr;
  hipStream_t ref_stream = nullptr;             // stream of the last set_refer (store_voice copies on it, then records ev[3])
  const void* dbg_last_in = nullptr;            // input of the last generator stage (intact after a decode) for the debug hook
  int dbg_last_T = 0, dbg_last_C = 0;
  // workspace
  std::map<std::string, Buf> bufs;
  // last decode bookkeeping
  int lastF = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float last_total_ms = 0.f, last_gen_ms = 0.f;
};

struct ConvOpt {
  int dil = 1, pad = -1, stride = 1;
  int pre_act = gsv::ACT_NONE; float pre_slope = 0.1f;
  int post_act = gsv::ACT_NONE; float scale = 1.f; int accumulate = 0;
  int out_f32 = 0; const void* res = nullptr; int res_f32 = 0; int ldr = 0;
  int ldy = 0, y_col0 = 0;
  const float* bias_override = nullptr; bool no_bias = false;
  const float* gate = nullptr;   // per-output-channel gate: y = ((W x + b) * gate + res) * scale
  int w_nt = 0;                  // stream the weights non-temporal (ConvArgs::w_nt)
  int w_row0 = 0, cout = -1;   // use a row slice of the weight matrix
  const int* row_seg = nullptr;   // segmented decode: gap rows of the output stored as 0 (ConvArgs::row_seg)
};

namespace gsveng {

inline int nblk(long long n, int b = 256) { return (int)((n + b - 1) / b); }
inline size_t esz(const gsv_vits* h) { return gsv::dt_size(h->dtype); }

int dalloc(gsv_vits* h, void** p, size_t bytes);
int up_f32(gsv_vits* h, const float* v, size_t n, float** out);
int up_t(gsv_vits* h, const std::vector<float>& v, void** out);
// staged tensor (or a folded weight_g / weight_v pair) as an fp32 host vector
bool fetch(gsv_vits* h, const std::string& name, size_t n, int dim0, std::vector<float>& out);
int make_conv(gsv_vits* h, const std::string& name, int cout, int cin, int k, bool bias, Conv* c);
int make_conv_padded(gsv_vits* h, const std::string& name, int cout, int cin, int cin_pad, int k, bool bias, Conv* c);
int make_stacked(gsv_vits* h, const std::vector<std::string>& names, int cout_each, int cin, Conv* c);
int make_ups(gsv_vits* h, const std::string& name, int cin, int cout, int k, int u, Conv* c);
int make_vec(gsv_vits* h, const std::string& name, size_t n, float** out);
int need(gsv_vits* h, const char* name, size_t bytes, void** out);
int conv(gsv_vits* h, hipStream_t s, const Conv& c, const void* x, int ldx, int T_in, void* y, int T_out, const ConvOpt& o);
int attention(gsv_vits* h, hipStream_t s, const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0,
              int Tq, int Tk, int nh, int kc, float scale, const float* rel_k, const float* rel_v, void* out, int ldo,
              const int* kr = nullptr);   // kr: per-query key range [kr[2i], kr[2i+1]) (segmented decode)
void free_ctx(gsv_vits* h);
// fp32 channels-first [C][Tn] -> engine dtype channels-last [Tn][ldd] (first C columns; ldd = 0: C)
int cf_to_cl(gsv_vits* h, hipStream_t s, const float* src, int Tn, int C, void* dst, int ldd = 0);

// generator.hip
// copies the generator's shape out of either config struct (gsv_vits_config, gsv_vocoder_config: same field names)
template <class Cfg>
void gen_shape(const Cfg& c, GenW* g) {
  g->uic = c.upsample_initial_channel; g->n_ups = c.n_ups; g->n_resblocks = c.n_resblocks;
  for (int i = 0; i < 8; ++i) { g->up_rates[i] = c.up_rates[i]; g->up_kernels[i] = c.up_kernels[i]; }
  for (int j = 0; j < 4; ++j) { g->rb_kernels[j] = c.rb_kernels[j]; for (int d = 0; d < 3; ++d) g->rb_dilations[j][d] = c.rb_dilations[j][d]; }
}
// ups / resblocks (BigVGAN: + activations and FIRs) named `prefix`ups.N, `prefix`resblocks.N; g's shape is already set
int load_generator(gsv_vits* h, const std::string& prefix, bool bigvgan, GenW* g);
// the 5 (BigVGAN: 6) ping-pong workspaces `name`0.. of a generator fed with F frames
int gen_buffers(gsv_vits* h, const GenW& g, const char* name, int F, void** gb);
// the rows of one resolution of a segmented pass as BigVGAN's activation needs them (device pointers): row_seg [rows] int32,
// -1 = gap row; segment s covers rows [start[s], start[s] + len[s])
struct SegRows { const int* row_seg = nullptr; const int* start = nullptr; const int* len = nullptr; };
// all upsampling stages on *cur = gb[3] ([*Tn][g.uic], the conv_pre output) -> *cur [*Tn][g.uic >> g.n_ups], one of gb[3], gb[4].
// seg_up != null (segmented decode): per-stage row maps, gap rows of every stage output are 0; a BigVGAN generator also takes
// seg_act[i] = the rows of stage i's output (row_seg = seg_up[i]) for its activations
int run_generator_stages(gsv_vits* h, hipStream_t s, const GenW& g, void* const* gb, void** cur, int* Tn, int* const* seg_up = nullptr,
                         const SegRows* seg_act = nullptr);

// segmented passes (vits.hip: gsv_vits_decode_segments, generator.hip: gsv_vocoder_forward_segments): n sequences back to back on
// one time axis with G zero "gap" rows between neighbours at the frame rate, G * prod(rates[:i]) after upsampling stage i
// one-sided input reach of a conv with `taps` taps at dilation `dil` ("same" padding)
inline int conv_reach(int taps, int dil) { return (taps - 1) / 2 * dil; }
// the smallest G that covers, at every resolution, the reach of the generator's convs (conv_pre and conv_post included)
int gen_gap(const GenW& g);
// out[i] = seg[i / up], i < n: the row map of an upsampled resolution
int launch_expand_seg(hipStream_t s, const int* seg, int up, long long n, int* out);
// drop the gaps from the padded waveform src [n] (seg_f = frame-rate map, up samples per frame, gap = G * up samples) into wav
int launch_compact_wav(hipStream_t s, const float* src, const int* seg_f, int up, long long gap, long long n, float* wav);

}  // namespace gsveng
