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
  std::map<int, hipGraphExec_t> graphs;
};

inline void* kv_ptr(gsv_t2s* h, int layer, int which) {
  return (char*)h->kv + ((size_t)(layer * 2 + which) * h->kv_layer_stride) * gsveng::esz(h);
}
