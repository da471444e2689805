// AR decoder engine state (the gsv_t2s handle) shared by t2s.hip (load / finalize, decode, debug and timing hooks) and
// t2s_prefill.hip (prefill).
#pragma once
#include "engine.h"
#include "t2s_sample.h"
#include "t2s_mega.h"

struct LayerW {
  void *qkv_w = nullptr, *out_w = nullptr, *w1 = nullptr, *w2 = nullptr;
  float *qkv_b = nullptr, *out_b = nullptr, *b1 = nullptr, *b2 = nullptr;
  float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr;
};

// A decode session (gsv_t2s_session_*): `slots` rows of the main arena that are admitted, advanced and freed one by one.  An
// admission prefills its rows in the staging copies below (rows 0 .. n - 1, the arena only as long as the admission's longest
// row) and one adopt launch moves them into their slots; see t2s_session.hip.
struct T2SSession {
  bool open = false;
  int slots = 0, budget = 0;
  bool row_sampling = false;
  gsv_sampling_params sp;
  int32_t *out_tokens = nullptr, *out_len = nullptr;         // the caller's, [slots][max_steps] and [slots]
  const int* force = nullptr; float* dump = nullptr; int* drawn = nullptr;   // gsv_t2s_set_debug's, held for the whole session
  float* logp = nullptr;                                     // gsv_t2s_set_logprobs', [slots][max_steps], likewise
  std::vector<char> live;                                    // host view of active[], refreshed by every admit / advance
  // staging: what a prefill and the step-0 tail write, sized for max_batch rows (the K/V arena grows with the admissions)
  int *st_state = nullptr, *st_plen = nullptr, *st_ytok = nullptr, *st_rng_row = nullptr, *st_out_tokens = nullptr,
      *st_out_len = nullptr, *st_slot = nullptr, *st_force = nullptr, *st_drawn = nullptr;
  unsigned long long* st_rng_seed = nullptr;
  gsv::RowSampling* st_row_sampling = nullptr;
  gsv::StepParams* st_sp = nullptr;
  float *st_ybuf = nullptr, *st_logits = nullptr, *st_dump = nullptr, *st_logp = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};                     // around the adopt launch
  float last_adopt_ms = 0.f; long long last_adopt_bytes = 0;
};

struct gsv_t2s : gsveng::Ctx {
  gsv_t2s() : Ctx("t2s") {}
  gsv_t2s_config cfg;
  int max_batch, max_seq;
  std::vector<LayerW> layers;
  void* bert_w = nullptr; float* bert_b = nullptr;
  float *e_text = nullptr, *e_audio = nullptr, *pe = nullptr;
  void* pred_w = nullptr;
  float alpha_t = 1.f, alpha_a = 1.f;
  int pe_rows = 0;
  // KV arena
  void* kv = nullptr; size_t kv_layer_stride = 0;  // elements per (layer, k|v)
  // row state
  int *d_x_len = nullptr, *d_row_off = nullptr, *d_ph_off = nullptr, *d_kv_len = nullptr, *d_active = nullptr,
      *d_step = nullptr, *d_n_active = nullptr, *d_ytok = nullptr;
  int ycap = 0;
  int* d_plen = nullptr;    // [2][max_batch]: prompt length P_b | offset of row b's prompt in the packed prompt buffer
  unsigned long long* d_rng_seed = nullptr; int* d_rng_row = nullptr;   // [max_batch] counter-RNG keys of the rows
  std::vector<unsigned long long> rng_seed_up; std::vector<int> rng_row_up;   // what the device arrays hold (skip re-uploads)
  std::vector<unsigned long long> rng_seed_next; std::vector<int> rng_row_next;   // gsv_t2s_set_row_rng: NEXT decode only
  gsv::RowSampling* d_row_sampling = nullptr;       // [max_batch] per-row sampling parameters
  std::vector<gsv_row_sampling_t> row_sampling_up;   // what the device array holds (skip re-uploads)
  std::vector<gsv_row_sampling_t> row_sampling_next; // gsv_t2s_set_row_sampling: NEXT decode only, cleared when it returns
  int* h_pinned = nullptr;
  gsv::StepParams* d_sp = nullptr;
  // decode buffers
  float *ybuf = nullptr, *xres = nullptr, *logits = nullptr;
  void *qbuf = nullptr, *abuf = nullptr, *hbuf = nullptr;
  // prefill workspace (grown on demand)
  size_t pf_rows = 0;
  void *pf_x = nullptr, *pf_qkv = nullptr, *pf_attn = nullptr, *pf_h = nullptr;
  void* pf_vt = nullptr; size_t pf_vt_cap = 0;   // V^T scratch of the MFMA prefill attention: [B][H][32][ceil32(maxS)] halfs
  float *pf_y = nullptr, *pf_bert = nullptr;
  void* pf_bert_t = nullptr;
  // current batch
  int B = 0, P = 0;         // P: the longest row's prompt (uniform prefill: every row's)
  int max_kv0 = 0;          // longest row's cached positions after prefill (host copy: bounds the decode budget)
  // persistent decode engine (t2s_mega.hip): fp16, v1/v2 shape, B <= 128; the launch-per-phase step stays as the
  // fp32 / other-shape path and behind GSV_T2S_NO_MEGA=1 for A/B
  gsv::MegaState mega;
  hipEvent_t mega_ev[2] = {nullptr, nullptr};
  float last_decode_ms = 0.f; int last_decode_steps = 0; int last_decode_mode = 0;
  bool mega_on = true;      // gsv_t2s_set_mega (A/B inside one process); GSV_T2S_NO_MEGA=1 never builds the engine
  int prefill_gemm = 2;     // gsv_t2s_set_prefill_gemm: 0 dispatcher only, 1 panel GEMM wherever eligible, 2 from PANEL_MIN_ROWS rows upwards
  const int* dbg_force = nullptr; float* dbg_dump = nullptr; int* dbg_drawn = nullptr; int dbg_stall = 0;   // gsv_t2s_set_debug / gsv_t2s_debug_stall: apply to the NEXT decode call only
  float* logp_next = nullptr;   // gsv_t2s_set_logprobs: the NEXT decode call (or the session begun next) only
  bool logp_on = false;         // the StepParams at d_sp hold a log-probability pointer: run_mega launches a LOGP kernel
  std::map<int, hipGraphExec_t> graphs;
  T2SSession ses;
};

inline void* kv_ptr(gsv_t2s* h, int layer, int which) {
  return (char*)h->kv + ((size_t)(layer * 2 + which) * h->kv_layer_stride) * gsveng::esz(h);
}

// t2s_prefill.hip: the ragged prefill of rows 0 .. B - 1 into whatever arena and row state the handle points at (an admission
// points it at the session's staging copies)
int t2s_prefill_into(gsv_t2s* h, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                     const int32_t* prompts_packed, const int32_t* prompt_lens, hipStream_t s);

// t2s_session.hip
namespace gsv {
// what the adopt launch moves for admitted row i -> slot[i]: src_* are the staging copies, dst_* the session's own
struct AdoptArgs {
  const void* src_kv = nullptr; void* dst_kv = nullptr;
  unsigned long long src_layer_stride = 0, dst_layer_stride = 0;   // elements per (layer, k|v)
  int src_smax = 0, dst_smax = 0, L = 0, H = 0, esize = 0;
  int n = 0, slots = 0, mb = 0, ycap = 0, d = 0, V = 0, src_steps = 0, dst_steps = 0;
  const int* slot = nullptr;                                       // [n] device
  const int *src_state = nullptr, *src_plen = nullptr, *src_ytok = nullptr, *src_rng_row = nullptr, *src_out_tokens = nullptr,
            *src_out_len = nullptr, *src_drawn = nullptr;
  const unsigned long long* src_rng_seed = nullptr;
  const RowSampling* src_row_sampling = nullptr;
  const float *src_ybuf = nullptr, *src_dump = nullptr, *src_logp = nullptr;
  int *dst_state = nullptr, *dst_plen = nullptr, *dst_ytok = nullptr, *dst_rng_row = nullptr, *dst_out_tokens = nullptr,
      *dst_out_len = nullptr, *dst_drawn = nullptr;
  unsigned long long* dst_rng_seed = nullptr;
  RowSampling* dst_row_sampling = nullptr;
  float *dst_ybuf = nullptr, *dst_dump = nullptr, *dst_logp = nullptr;
};
int launch_session_adopt(const AdoptArgs& a, hipStream_t s);
// ybuf[b] = e_audio[tok] + alpha_a * pe[P_b + step - 1], tok = ytok[b][P_b + step - 1], for every live row: the input embedding
// of the row's next step, which the last step of a launch does not leave behind
int launch_session_embed(const int* state, int mb, const int* plen, const int* ytok, int ycap, const float* e_audio, const float* pe,
                         float alpha_a, int d, int V, int slots, float* ybuf, hipStream_t s);
// clears the live word of slot[0 .. n - 1] (distinct, < slots) in the state block [kv_len | active | step | n_active] and takes
// the rows that were live out of n_active
int launch_session_release(int* state, int mb, const int* slot, int n, int slots, hipStream_t s);
}  // namespace gsv
