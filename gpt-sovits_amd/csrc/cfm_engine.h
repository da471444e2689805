// What cfm.hip (the one-shot flow-matching passes) and cfm_session.hip (sessions: rows with their own time, admitted and fetched
// between Euler steps) share: the handle, the row table, and the three pieces of a pass that are written once in cfm.hip --
// the modulation tables of one step count, the text embedding stack, and one DiT forward over packed rows.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "engine.h"

namespace gsv {

// what differs between the utterances of one call: the prompt mel (channels-first [C][Tp], device) and its length, and the key
// of the noise draw.  A small device array, one entry per utterance, read by the kernels below.  A guided pass appends one
// entry per unconditioned twin: prompt null (its cond columns are zeros whatever Tp says), Tp the conditioned row's.
// slot: the row's LoRA adapter (gsv_cfm_adapter_*), -1 = the base model; a twin takes its request's.
struct CfmRow {
  const float* prompt;
  unsigned long long seed;
  int Tp, slot;
};

// the table reaches the device as kernel arguments, up to CFM_ROW_CHUNK entries per launch: the runtime copies arguments at
// launch, so the host vector may go away at once and the host never waits for the stream
constexpr int CFM_ROW_CHUNK = 64;
struct CfmRowChunk { CfmRow r[CFM_ROW_CHUNK]; };

}  // namespace gsv

struct DitBlockW { Conv mod, qkv, out, ff1, ff2; };
struct TextBlockW { float *dw = nullptr, *db = nullptr, *ng = nullptr, *nb = nullptr, *gg = nullptr, *gb = nullptr; Conv pw1, pw2; };

// one stored LoRA adapter: `dev` is one block in the engine dtype, per DiT block l (rp = rank padded to 16, inner = heads *
// dim_head, everything in units of rp elements from l * 4 (D + inner)):
//   q|k|v lora_A stacked [3 rp][D] at 0, q|k|v lora_B [3 inner][rp] at 3 D, out lora_A [rp][inner] at 3 D + 3 inner,
//   out lora_B [D][rp] at 3 D + 4 inner; alpha / rank is folded into the lora_B matrices.  dev null = free slot.
struct CfmAdapter { void* dev = nullptr; int rank = 0, rp = 0; };

struct CfmSession;   // cfm_session.hip

struct gsv_cfm : gsveng::Ctx {
  gsv_cfm() : Ctx("cfm") {}
  gsv_dit_config cfg;
  int ldin = 0;
  Conv t0, t2, d0, d2, in_proj, pos1, pos2, final_mod, proj_out;
  std::vector<TextBlockW> text;
  std::vector<DitBlockW> blocks;
  float* pos_table = nullptr;   // fp32 [4096][text_dim]
  bool materialized_attn = false;   // GSV_CFM_MATERIALIZED_ATTN=1: A/B switch back to the 4-launch scores/softmax/PV path
  // LoRA adapters: the store by slot, its device image (base pointer and rp per slot, what lora.hip indexes by a row's
  // slot), and the adapter being staged between adapter_begin and adapter_finalize
  std::vector<CfmAdapter> adapters;
  gsv::LoraSlot* lora_tab = nullptr;     // device [GSV_CFM_MAX_ADAPTERS], allocated with the first adapter
  bool a_open = false;
  int a_rank = 0;
  float a_alpha = 0.f;
  std::map<std::string, std::vector<float>> a_staged;
  CfmSession* sess = nullptr;       // gsv_cfm_session_*: created by the first begin, lives with the handle
};

namespace gsvcfm {

constexpr float CFM_CFG_THRESHOLD = 1e-5f;   // guidance is active above this rate (models.py:1063)

// grid of the elementwise kernels: one thread of a 256-thread workgroup per element of n, blockIdx.y = utterance
inline dim3 cfm_grid(long long n, int B = 1) { return dim3(gsveng::nblk(n), B); }

// Where one DiT forward finds its AdaLN-Zero modulation vectors.  rows == 0: one set for all rows of the pass (the one-shot
// entries: every row is at the same step of the same step count); block l's [6D] vector is blk + l * blk_stride, the final
// layer's [2D] is fin.  rows == 1: every utterance row b has its own (a session: its own step count and step index); block l's
// is blk + l * blk_stride + b * 6D, the final layer's fin + b * 2D.
struct DitMods {
  const float* blk = nullptr;
  size_t blk_stride = 0;
  const float* fin = nullptr;
  int rows = 0;
};

// is a flow-matching session open on the handle (the one-shot entries refuse to share its workspace)
bool session_open(const gsv_cfm* c);
void session_destroy(gsv_cfm* c);
// does a live row of the open session run with LoRA slot `slot` (gsv_cfm_adapter_remove refuses it then)
bool session_uses_adapter(const gsv_cfm* c, int slot);

// time-independent precomputation for all N steps of one step count, into the workspace: mods[l][i][6D] (l < depth) and
// mods[depth][i][2D].  Synchronises the stream once (the step times are uploaded from the stack).
template <typename T> int modulations(gsv_cfm* c, hipStream_t s, int N, float** mods_out);
inline size_t mods_floats(const gsv_cfm* c, int N) { return ((size_t)c->cfg.depth * 6 + 2) * N * c->cfg.dim; }

// the text embedding stack (dit.py:50-72) over TB rows of Tn frames: rows [0, mu_rows) embed mu [mu_rows][Tn][text_dim], the
// rest are null text rows.  ta [TB][Tn][td] holds the result; tb [TB][Tn][td], tw [TB][Tn][2 td] and gx [TB][2 td] are scratch.
template <typename T> int text_stack(gsv_cfm* c, hipStream_t s, const float* mu, int mu_rows, int TB, int Tn, void* ta, void* tb, void* tw, float* gx);

// one DiT forward (dit.py:140-194) over DB packed rows of Tn frames: xin [DB * Tn][ldin] -> v [DB * Tn][mel] fp32.  cs = the
// rotary table of Tn frames; row_slot / slot_ld / max_rp: the rows' LoRA slots on the device (max_rp == 0: no adapted row).
template <typename T>
int dit_forward(gsv_cfm* c, hipStream_t s, const void* xin, int DB, int Tn, const DitMods& mods, const int* row_slot, int slot_ld, int max_rp,
                const float* cs, float* v);

// host ends of three small kernels of cfm.hip
int rows_upload(hipStream_t s, const gsv::CfmRow* host, int n, gsv::CfmRow* dev);
int rope_table(hipStream_t s, int Tn, int half, float* cs);
// x0 of B rows: temperature * noise ([B][C][Tn] given, or the counter-based draw keyed by rw[b].seed), zero on the prompt frames
int init_x(hipStream_t s, const float* noise, const gsv::CfmRow* rw, float temperature, int Tn, int C, int B, float* x);

}  // namespace gsvcfm
