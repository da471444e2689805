// What the five engines stand on: the context every handle derives from (gsveng::Ctx: dtype, staged tensors, device
// allocations, workspace arena) with its staging / upload / workspace / conv / attention helpers (engine.hip), and the generator
// shared by the SoVITS decoder and the vocoders (generator.hip).  gsv_vits (vits.hip), gsv_vocoder (generator.hip), gsv_cfm
// (cfm.hip), gsv_bwe (bwe.hip) and gsv_t2s (t2s_engine.h) are each a Ctx plus what their own model owns.
#pragma once
#include <math.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"

struct Conv {
  void* w = nullptr;     // T [cout][taps*cin]
  float* b = nullptr;    // fp32 [cout_real] or null
  int cin = 0, cout = 0, taps = 1;
  int ups_u = 0, ups_pad = 0, ups_cout = 0;
};

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

struct ConvOpt {
  int dil = 1, pad = -1, stride = 1;
  int pre_act = gsv::ACT_NONE; float pre_slope = 0.1f;
  int post_act = gsv::ACT_NONE; float scale = 1.f; int accumulate = 0;
  int out_f32 = 0; const void* res = nullptr; int res_f32 = 0; int ldr = 0;
  int ldy = 0, y_col0 = 0;
  const float* bias_override = nullptr; bool no_bias = false;
  const float* gate = nullptr;   // per-output-channel gate: y = ((W x + b) * gate + res) * scale
  int gate_rows = 0, gate_ld = 0;   // per-row gates: output row t takes gate + (t / gate_rows) * gate_ld (ConvArgs::gate_rows)
  int w_nt = 0;                  // stream the weights non-temporal (ConvArgs::w_nt)
  int w_row0 = 0, cout = -1;   // use a row slice of the weight matrix
  const int* row_seg = nullptr;   // segmented decode: gap rows of the output stored as 0 (ConvArgs::row_seg)
};

namespace gsveng {

inline int nblk(long long n, int b = 256) { return (int)((n + b - 1) / b); }

// The context of one engine handle.  The handles are opaque to C, so each handle struct derives from it and passes itself to the
// helpers below.  `who` prefixes the messages about the handle's tensors ("vits", "vocoder", "cfm", "bwe", "t2s").
struct Ctx {
  explicit Ctx(const char* w) : who(w) {}
  int dtype = GSV_F32;
  bool finalized = false;
  const char* who;
  std::map<std::string, std::vector<float>> staged;   // load_tensor .. finalize: fp32 host copies by name
  std::vector<void*> allocs;                          // device memory released at destroy (free_ctx)
  std::map<std::string, Buf> bufs;                    // workspace arena by name (need)
};

inline size_t esz(const Ctx* h) { return gsv::dt_size(h->dtype); }

// a usable HIP device exists: checked when a handle is created, not at its first upload
int require_device();
// gsv_*_load_tensor: stages a copy of data [numel] under `name` until finalize
int stage_tensor(Ctx* h, const char* name, const float* data, int64_t numel);

int dalloc(Ctx* h, void** p, size_t bytes);
int up_f32(Ctx* h, const float* v, size_t n, float** out);
int up_t(Ctx* h, const std::vector<float>& v, void** out);
// staged tensor (or a folded weight_g / weight_v pair) as an fp32 host vector
bool fetch(Ctx* h, const std::string& name, size_t n, int dim0, std::vector<float>& out);
// torch Conv1d weight [cout][cin][k] (+ bias) -> Conv; padded: the input channels zero-padded to cin_pad
int make_conv_padded(Ctx* h, const std::string& name, int cout, int cin, int cin_pad, int k, bool bias, Conv* c);
inline int make_conv(Ctx* h, const std::string& name, int cout, int cin, int k, bool bias, Conv* c) {
  return make_conv_padded(h, name, cout, cin, cin, k, bias, c);
}
int make_stacked(Ctx* h, const std::vector<std::string>& names, int cout_each, int cin, Conv* c);
int make_ups(Ctx* h, const std::string& name, int cin, int cout, int k, int u, Conv* c);
// a staged tensor of n elements uploaded as it is: make_vec in fp32, make_mat in the engine dtype
int make_vec(Ctx* h, const std::string& name, size_t n, float** out);
int make_mat(Ctx* h, const std::string& name, size_t n, void** out);
int need(Ctx* h, const char* name, size_t bytes, void** out);
int conv(Ctx* h, hipStream_t s, const Conv& c, const void* x, int ldx, int T_in, void* y, int T_out, const ConvOpt& o);
int attention(Ctx* h, hipStream_t s, const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0,
              int Tq, int Tk, int nh, int kc, float scale, const float* rel_k, const float* rel_v, void* out, int ldo,
              const int* kr = nullptr);   // kr: per-query key range [kr[2i], kr[2i+1]) (segmented decode)
// attention()'s choice (the GSV_MATERIALIZED_ENC_ATTN switch included) and its two routes: fused = the flash_rel96 kernel
// (fp16, kc 96, both relative tables, Tq == Tk), else the materialised path in the handle's element type
bool attention_is_fused(const Ctx* h, const void* q, int ldq, const void* kv, int ldkv, int Tq, int Tk, int kc, const float* rel_k,
                        const float* rel_v);
int attention_routed(Ctx* h, hipStream_t s, const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0,
                     int Tq, int Tk, int nh, int kc, float scale, const float* rel_k, const float* rel_v, void* out, int ldo,
                     const int* kr, bool fused);
// releases allocs and bufs: the one place that does; a destroy function adds what its own handle owns
void free_ctx(Ctx* h);
// fp32 channels-first [C][Tn] -> engine dtype channels-last [Tn][ldd] (first C columns; ldd = 0: C)
int cf_to_cl(Ctx* h, hipStream_t s, const float* src, int Tn, int C, void* dst, int ldd = 0);

// The library's own context, one per device and created at its first use: what an op entry point, which has no handle, needs
// beyond its arguments.  Today that is the segment table of gsv_op_flash_attn64_seg (attn.hip): kSegSlots slots of a page-locked
// staging buffer, a device table and an event each, all allocated when the context is created, so a call allocates nothing.
// A call fills `image` and uploads it with one async copy on its stream into the next slot; the slot's event is recorded after
// the kernels that read the table, and a slot is rewritten only when that event has passed (kSegSlots tables later, so the wait
// finds it done).  A call whose table equals the newest slot's and runs on the same stream reuses that slot without a copy: the
// 22 layers of one packed BERT pass upload their table once.  The context lives until the process ends.
constexpr int kSegTableMax = 8192, kSegSlots = 4;
struct SegSlot { int* host = nullptr; int* dev = nullptr; hipEvent_t ev = nullptr; hipStream_t stream = nullptr; int n = 0; };
struct LibCtx {
  std::mutex mu;
  SegSlot slot[kSegSlots];
  int cur = 0;
  std::vector<int> image;                             // 4 ints per segment, kSegTableMax segments
};
// a call's hold on the context: the lock is released when it goes out of scope
struct SegTable {
  std::unique_lock<std::mutex> lock;
  LibCtx* ctx = nullptr;
  int* image = nullptr;                               // [4 * kSegTableMax], filled by the caller
  const int* dev = nullptr;                           // set by seg_table_upload
};
int seg_table_begin(SegTable* t);
int seg_table_upload(SegTable* t, int n_seg, hipStream_t s);
int seg_table_end(SegTable* t, hipStream_t s);        // after the last launch that reads t->dev

// generator.hip
// copies the generator's shape out of either config struct (gsv_vits_config, gsv_vocoder_config: same field names)
template <class Cfg>
void gen_shape(const Cfg& c, GenW* g) {
  g->uic = c.upsample_initial_channel; g->n_ups = c.n_ups; g->n_resblocks = c.n_resblocks;
  for (int i = 0; i < 8; ++i) { g->up_rates[i] = c.up_rates[i]; g->up_kernels[i] = c.up_kernels[i]; }
  for (int j = 0; j < 4; ++j) { g->rb_kernels[j] = c.rb_kernels[j]; for (int d = 0; d < 3; ++d) g->rb_dilations[j][d] = c.rb_dilations[j][d]; }
}
// ups / resblocks (BigVGAN: + activations and FIRs) named `prefix`ups.N, `prefix`resblocks.N; g's shape is already set
int load_generator(Ctx* h, const std::string& prefix, bool bigvgan, GenW* g);
// the 5 (BigVGAN: 6) ping-pong workspaces `name`0.. of a generator fed with F frames
int gen_buffers(Ctx* h, const GenW& g, const char* name, int F, void** gb);
// the rows of one resolution of a segmented pass as BigVGAN's activation needs them (device pointers): row_seg [rows] int32,
// -1 = gap row; segment s covers rows [start[s], start[s] + len[s])
struct SegRows { const int* row_seg = nullptr; const int* start = nullptr; const int* len = nullptr; };
// all upsampling stages on *cur = gb[3] ([*Tn][g.uic], the conv_pre output) -> *cur [*Tn][g.uic >> g.n_ups], one of gb[3], gb[4].
// seg_up != null (segmented decode): per-stage row maps, gap rows of every stage output are 0; a BigVGAN generator also takes
// seg_act[i] = the rows of stage i's output (row_seg = seg_up[i]) for its activations
// tap != null: the input of the last stage (intact after the pass), for a debug hook
struct GenTap { const void* in = nullptr; int T = 0, C = 0; };
int run_generator_stages(Ctx* h, hipStream_t s, const GenW& g, void* const* gb, void** cur, int* Tn, int* const* seg_up = nullptr,
                         const SegRows* seg_act = nullptr, GenTap* tap = nullptr);

// segmented passes (vits.hip: gsv_vits_decode_segments, generator.hip: gsv_vocoder_forward_segments): n sequences back to back on
// one time axis with G zero "gap" rows between neighbours at the frame rate, G * prod(rates[:i]) after upsampling stage i
// upload state of a segmented pass: the host image of its maps (and noise keys), which has to stay alive until its copy is done,
// and the event recorded after the upload.  seg_upload_begin waits for the previous pass's upload (on any stream) before the
// caller rewrites the image.
struct SegUpload {
  std::vector<int> maps;
  std::vector<unsigned long long> seeds;
  hipEvent_t ev = nullptr;
  ~SegUpload() { if (ev) (void)hipEventDestroy(ev); }
};
int seg_upload_begin(SegUpload* u);
// one-sided input reach of a conv with `taps` taps at dilation `dil` ("same" padding)
inline int conv_reach(int taps, int dil) { return (taps - 1) / 2 * dil; }
// the smallest G that covers, at every resolution, the reach of the generator's convs (conv_pre and conv_post included)
int gen_gap(const GenW& g);
// out[i] = seg[i / up], i < n: the row map of an upsampled resolution
int launch_expand_seg(hipStream_t s, const int* seg, int up, long long n, int* out);
// drop the gaps from the padded waveform src [n] (seg_f = frame-rate map, up samples per frame, gap = G * up samples) into wav
int launch_compact_wav(hipStream_t s, const float* src, const int* seg_f, int up, long long gap, long long n, float* wav);

}  // namespace gsveng
