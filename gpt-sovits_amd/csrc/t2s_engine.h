// AR decoder engine state: the gsv_t2s handle, the RowState a prefill / step-0 tail / decode step works on, and the few host
// entry points the three engine files call across: t2s.hip (load / finalize, the kernels and launchers of the decode step,
// gsv_t2s_decode, debug and timing hooks), t2s_prefill.hip (prefill) and t2s_session.hip (decode sessions).
#pragma once
#include <string.h>

#include "engine.h"
#include "t2s_sample.h"
#include "t2s_mega.h"

struct LayerW {
  void *qkv_w = nullptr, *out_w = nullptr, *w1 = nullptr, *w2 = nullptr;
  float *qkv_b = nullptr, *out_b = nullptr, *b1 = nullptr, *b2 = nullptr;
  float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr;
};

// Everything a prefill, a step-0 tail and a decode step read or write for one set of rows.  The handle owns one (`rows`: the
// main arena, what gsv_t2s_decode and a session's advance run on) and a session owns a second (`staging`: where an admission
// prefills and runs step 0).  The functions that can work on either take a RowState&; nothing repoints a RowState's arrays
// after gsv_t2s_finalize (rows) / session_begin (staging) set them, except the staging K/V arena, sized per admission.
// Shared by both and left on the handle: the prefill workspace (pf_*), d_x_len / d_row_off / d_ph_off, xres / qbuf / abuf /
// hbuf, ycap and the weights.  That is safe because one stream runs one prefill or step at a time, the prefill hands over
// through ybuf alone, and the step-0 tail writes none of them: its LayerNorm GEMM reads ybuf and writes logits only.
struct RowState {
  // K/V arena [layer][k|v][row][head][max_seq][32]
  void* kv = nullptr; size_t kv_layer_stride = 0;  // elements per (layer, k|v)
  int max_seq = 0;
  // ONE block [kv_len | active | step | n_active(+pad)] of 3 * mb + 4 ints: the prefill uploads it and the persistent
  // engine's fallback saves and restores it with one copy each
  int* state = nullptr; int mb = 0;                // mb = the handle's max_batch
  size_t state_ints() const { return 3 * (size_t)mb + 4; }
  int* kv_len() const { return state; }
  int* active() const { return state + mb; }
  int* step() const { return state + 2 * mb; }
  int* n_active() const { return state + 3 * mb; }
  // per-row arrays
  int* ytok = nullptr;      // [mb][ycap] token history
  int* plen = nullptr;      // [2][mb]: prompt length P_b | offset of row b's prompt in the packed prompt buffer
  unsigned long long* rng_seed = nullptr; int* rng_row = nullptr;   // [mb] counter-RNG keys of the rows
  gsv::RowSampling* row_sampling = nullptr;        // [mb] every row's sampling values and step limits: its own, or the call's /
  gsv::RowLimits* row_limits = nullptr;            // session's scalars (decode_begin, session_begin / session_admit fill them)
  gsv::StepParams* sp = nullptr;                   // the device StepParams of these rows
  float *ybuf = nullptr, *logits = nullptr;        // [mb][dim] next step's input embedding, [mb][vocab]
  // host view of the current batch
  int B = 0, P = 0;         // P: the longest row's prompt (uniform prefill: every row's)
  std::vector<int> kv0, pl; // every row's cached positions and prompt length after prefill: bound the rows' decode budgets
};

// where a decode writes: the caller's results, the parity hooks (gsv_t2s_set_debug) and the log-probabilities
// (gsv_t2s_set_logprobs); the last four are null in production
struct RowOutputs {
  int32_t *out_tokens = nullptr, *out_len = nullptr;         // [rows][max_steps] and [rows]
  const int* force = nullptr; float* dump = nullptr; int* drawn = nullptr; float* logp = nullptr;
};

// A decode session (gsv_t2s_session_*): `slots` rows of the main arena that are admitted, advanced and freed one by one.  An
// admission prefills its rows in `staging` (rows 0 .. n - 1, the arena only as long as the admission's longest row) and one
// adopt launch moves them into their slots; see t2s_session.hip.
struct T2SSession {
  bool open = false;
  int slots = 0, budget = 0;
  bool row_sampling = false;                                 // what gsv_t2s_session_admit checks its row_sampling argument against
  gsv_sampling_params sp;
  RowOutputs out;                                            // the caller's and the hooks', held for the whole session
  std::vector<char> live;                                    // host view of active[], refreshed by every admit / advance
  RowState staging; RowOutputs staging_out;                  // sized for max_batch rows; a hook the session lacks is null here too
  int* staging_force = nullptr;                              // the buffer behind staging_out.force: an admission fills its rows
  int* st_slot = nullptr;                                    // slot upload buffer of admit / release
  hipEvent_t ev[2] = {nullptr, nullptr};                     // around the adopt launch
  float last_adopt_ms = 0.f; long long last_adopt_bytes = 0;
};

struct gsv_t2s : gsveng::Ctx {
  gsv_t2s() : Ctx("t2s") {}
  gsv_t2s_config cfg;
  int max_batch;
  std::vector<LayerW> layers;
  void* bert_w = nullptr; float* bert_b = nullptr;
  float *e_text = nullptr, *e_audio = nullptr, *pe = nullptr;
  void* pred_w = nullptr;
  float alpha_t = 1.f, alpha_a = 1.f;
  int pe_rows = 0;
  RowState rows;            // the main arena and its rows
  int *d_x_len = nullptr, *d_row_off = nullptr, *d_ph_off = nullptr;   // the prefill's row table
  int ycap = 0;
  std::vector<unsigned long long> rng_seed_up; std::vector<int> rng_row_up;   // what the device arrays hold (skip re-uploads)
  std::vector<unsigned long long> rng_seed_next; std::vector<int> rng_row_next;   // gsv_t2s_set_row_rng: NEXT decode only
  std::vector<gsv_row_sampling_t> row_sampling_up;   // what the device arrays hold (skip re-uploads)
  std::vector<gsv_row_limits_t> row_limits_up;
  std::vector<gsv_row_sampling_t> row_sampling_next; // gsv_t2s_set_row_sampling: NEXT decode only, cleared when it returns
  int* h_pinned = nullptr;
  // decode buffers
  float* xres = nullptr;
  void *qbuf = nullptr, *abuf = nullptr, *hbuf = nullptr;
  // prefill workspace (grown on demand)
  size_t pf_rows = 0;
  void *pf_x = nullptr, *pf_qkv = nullptr, *pf_attn = nullptr, *pf_h = nullptr;
  void* pf_vt = nullptr; size_t pf_vt_cap = 0;   // V^T scratch of the MFMA prefill attention: [B][H][32][ceil32(maxS)] halfs
  float *pf_y = nullptr, *pf_bert = nullptr;
  void* pf_bert_t = nullptr;
  // persistent decode engine (t2s_mega.hip): fp16, v1/v2 shape, B <= 128; the launch-per-phase step stays as the
  // fp32 / other-shape path and behind GSV_T2S_NO_MEGA=1 for A/B
  gsv::MegaState mega;
  hipEvent_t mega_ev[2] = {nullptr, nullptr};
  float last_decode_ms = 0.f; int last_decode_steps = 0; int last_decode_mode = 0;
  bool mega_on = true;      // gsv_t2s_set_mega (A/B inside one process); GSV_T2S_NO_MEGA=1 never builds the engine
  int prefill_gemm = 2;     // gsv_t2s_set_prefill_gemm: 0 dispatcher only, 1 panel GEMM wherever eligible, 2 from PANEL_MIN_ROWS rows upwards
  std::vector<gsv_row_limits_t> row_limits_next;     // gsv_t2s_set_row_limits: NEXT decode / admission only
  RowOutputs next;          // gsv_t2s_set_debug / gsv_t2s_set_logprobs: the NEXT decode call (or the session begun next) only
  int dbg_stall = 0;        // gsv_t2s_debug_stall: likewise
  bool logp_on = false;     // the StepParams at rows.sp hold a log-probability pointer: run_mega launches a LOGP kernel
  // The launch-per-phase step captured per batch size.  Graphs are captured over `rows` only: the decode step, run_mega and the
  // debug / timing hooks never run on a session's staging rows, and no pointer of `rows` changes after gsv_t2s_finalize.
  std::map<int, hipGraphExec_t> graphs;
  T2SSession ses;
};

inline void* kv_ptr(const gsv_t2s* h, const RowState& r, int layer, int which) {
  return (char*)r.kv + ((size_t)(layer * 2 + which) * r.kv_layer_stride) * gsveng::esz(h);
}

// the call's results plus the handle's next-call hooks, which are the call's alone: cleared here
inline RowOutputs take_outputs(gsv_t2s* h, int32_t* out_tokens, int32_t* out_len) {
  RowOutputs o = h->next;
  o.out_tokens = out_tokens; o.out_len = out_len;
  h->next = RowOutputs();
  h->logp_on = o.logp != nullptr;
  return o;
}

// the StepParams of a decode over the rows of r that writes to o with row pitch max_steps; whoever uploads them has filled
// r's per-row arrays for every row that can be live
inline gsv::StepParams step_params(int max_steps, const RowState& r, const RowOutputs& o) {
  gsv::StepParams p;
  memset(&p, 0, sizeof(p));
  p.max_steps = max_steps;
  p.out_tokens = o.out_tokens; p.out_len = o.out_len; p.force = o.force; p.dump = o.dump; p.drawn = o.drawn; p.logp = o.logp;
  p.plen = r.plen; p.rng_seed = r.rng_seed; p.rng_row = r.rng_row; p.row_sampling = r.row_sampling; p.row_limits = r.row_limits;
  return p;
}

// forgets what the device row tables of h->rows hold: a session writes them itself
inline void forget_row_tables(gsv_t2s* h) {
  h->rng_seed_up.clear(); h->rng_row_up.clear(); h->row_sampling_up.clear(); h->row_limits_up.clear();
}

// steps a row can run: step 0 samples from the prefill's last position, every later step appends one K/V position
inline int step_budget(int early_stop_num, int max_steps) {
  int budget = max_steps;
  if (early_stop_num >= 0 && early_stop_num + 1 < budget) budget = early_stop_num + 1;
  return budget;
}
inline int step_budget(const gsv_sampling_params& sp) { return step_budget(sp.early_stop_num, sp.max_steps); }
inline int step_budget(const gsv_row_limits_t& rl) { return step_budget(rl.early_stop_num, rl.max_steps); }

// while a decode session is open the handle's arena and row state are the session's
#define GSV_T2S_NO_SESSION(h, who)                                                                                      \
  do {                                                                                                                  \
    if ((h)->ses.open) {                                                                                                \
      gsv::set_error(who ": a decode session is open on this handle (gsv_t2s_session_end closes it)");                  \
      return GSV_ERR_STATE;                                                                                             \
    }                                                                                                                   \
  } while (0)
// its opposite; hint: " (gsv_t2s_session_begin)" where the caller could open one, else ""
#define GSV_T2S_IN_SESSION(h, who, hint)                                                                                \
  do {                                                                                                                  \
    if (!(h)->ses.open) {                                                                                               \
      gsv::set_error(who ": no decode session is open" hint);                                                           \
      return GSV_ERR_STATE;                                                                                             \
    }                                                                                                                   \
  } while (0)

// t2s_prefill.hip: the ragged prefill of rows 0 .. B - 1 into the arena and row state of r
int t2s_prefill_into(gsv_t2s* h, RowState& r, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                     const int32_t* prompts_packed, const int32_t* prompt_lens, hipStream_t s);
// t2s.hip.  Step 0 of the rows of r: logits of the last prefill position, sample, emit the first embedding
int t2s_step0_tail(gsv_t2s* h, RowState& r, hipStream_t s);
// Steps 1 .. budget - 1 of h->rows: the persistent engine if it is eligible, else (or after its fallback) the launch-per-phase
// step.  gsv_t2s_decode_info then reports mode 1 and budget - 1 steps for the engine, mode 0 and 0 steps for the launch path
// (last_decode_mode stays 0 after a fallback too); session_advance reads that mode and reports its n_steps for the launch path.
int run_chunk(gsv_t2s* h, int budget, int32_t* out_len, int* steps_run, hipStream_t s);
// the value checks of gsv_t2s_set_row_sampling, gsv_t2s_session_admit and gsv_op_sample_rows
int check_row_sampling(const char* who, const gsv_row_sampling_t* rows, int B);
// the RNG rows of gsv_t2s_set_row_rng and gsv_t2s_session_admit: the key holds 24 bits of the row (row << 40), so a row
// outside [0, 2^24) would draw the stream of another row ("The counter RNG as a contract")
int check_rng_rows(const char* who, const int32_t* rows, int B);
// the sampling values and the limits of a call with the scalars of sp: what a row that brings none of its own gets
inline gsv_row_sampling_t sampling_of(const gsv_sampling_params& sp) { return {sp.top_k, sp.top_p, sp.temperature, sp.repetition_penalty}; }
inline gsv_row_limits_t limits_of(const gsv_sampling_params& sp) { return {sp.eos_mask_steps, sp.early_stop_num, sp.max_steps, 0}; }
// gsv_t2s_set_row_limits' rows against the max_steps of the call / session that consumes them
int check_row_limits_steps(const char* who, const std::vector<gsv_row_limits_t>& rows, int max_steps);
