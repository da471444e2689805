// AR decode sessions (gsv_t2s_session_*): their three kernels -- the adopt launch that moves freshly prefilled rows from the
// staging arena into their slots of the main arena, the launch that rebuilds the next step's input embedding of every live row
// in front of an advance, and the launch that takes rows out of the decode (a cancelled request) -- and their host side: admit
// = prefill + step 0 on the session's staging RowState, then the adopt launch; advance = the embedding rewrite, then
// run_chunk (t2s.hip) over the handle's own rows.
//
// Adopt.  An admission prefills its n rows as rows 0 .. n - 1 of a staging arena [layer][k|v][n][head][src.smax][32] (src.smax =
// the admission's longest row + 2, not max_seq) with the unchanged prefill kernels, and runs their step 0 on staging row state.
// One launch then copies, for row i and slot[i], every (layer, k|v, head) run of S_i cached positions -- S_i * 32 elements,
// contiguous on both sides -- and the row's state.  It is a pure copy: 16-byte accesses, no LDS, one workgroup per
// (row, layer, k|v, head group) run, the staging side read non-temporal (it is read once and never again).  Its traffic is
// n * S * L * 2 * d * sizeof(T) bytes read and as many written (49 152 B per cached position on the fp16 v2 decoder), which
// is what gsv_t2s_session_adopt_info reports the launch's time against.
#include <type_traits>
#include <vector>

#include "t2s_engine.h"

namespace gsv {

typedef unsigned u4v __attribute__((ext_vector_type(4)));

// One side of the adopt launch: the arena and the per-row arrays of a RowState plus where its decode writes.  drawn, dump and
// logp are null on BOTH sides when the session lacks them: the kernel tests dst's and only then reads src's.
struct AdoptView {
  void* kv; unsigned long long layer_stride;   // elements per (layer, k|v)
  int smax;                                    // positions per (row, head) of the arena
  int *state, *plen, *ytok, *rng_row, *out_tokens, *out_len, *drawn;
  unsigned long long* rng_seed;
  RowSampling* row_sampling;
  RowLimits* row_limits;
  float *ybuf, *dump, *logp;
};
// what the adopt launch moves for admitted row i -> slot[i]: src is the staging side, dst the session's own
struct AdoptArgs {
  AdoptView src, dst;
  int n, slots, mb, ycap, d, V, L, H, esize, steps;   // steps: row pitch of out_tokens / logp on both sides
  const int* slot;                                    // [n] device
};
static_assert(std::is_trivially_copyable<AdoptArgs>::value, "AdoptArgs is passed to the kernel by value");

__global__ __launch_bounds__(256) void session_adopt_kernel(AdoptArgs a, int hg /* heads per workgroup */) {
  const int tid = threadIdx.x;
  const int groups = a.H / hg, runs = a.L * 2 * groups;
  const int bid = blockIdx.x;
  if (bid < a.n * runs) {
    const int i = bid / runs, r = bid - i * runs;
    const int lw = r / groups, h0 = (r - lw * groups) * hg;
    const int slot = a.slot[i];
    const int S = min(a.src.state[i], min(a.src.smax, a.dst.smax));      // kv_len: step 0 appends nothing
    const int cpp = 32 * a.esize / 16;                                   // 16-byte chunks per cached position
    const int chunks = S * cpp;                                          // per head
    const size_t src_head = (size_t)a.src.smax * cpp, dst_head = (size_t)a.dst.smax * cpp;
    const u4v* src = (const u4v*)a.src.kv + (size_t)lw * (a.src.layer_stride / 32) * cpp + ((size_t)i * a.H + h0) * src_head;
    u4v* dst = (u4v*)a.dst.kv + (size_t)lw * (a.dst.layer_stride / 32) * cpp + ((size_t)slot * a.H + h0) * dst_head;
    const int total = hg * chunks;
    for (int t0 = tid; t0 < total; t0 += 4 * 256) {
      u4v v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * 256;
        if (t < total) {
          const int hh = t / chunks, c = t - hh * chunks;
          v[u] = __builtin_nontemporal_load(src + hh * src_head + c);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * 256;
        if (t < total) {
          const int hh = t / chunks, c = t - hh * chunks;
          dst[hh * dst_head + c] = v[u];
        }
      }
    }
    return;
  }
  // the row's state: one workgroup per admitted row
  const int i = bid - a.n * runs;
  const int slot = a.slot[i];
  const int mb = a.mb;
  const int P = a.src.plen[i], step = a.src.state[2 * mb + i];
  if (tid == 0) {
    const int act = a.src.state[mb + i];
    a.dst.plen[slot] = P;
    a.dst.state[slot] = a.src.state[i];
    a.dst.state[mb + slot] = act;
    a.dst.state[2 * mb + slot] = step;
    if (act) atomicAdd(a.dst.state + 3 * mb, 1);
    a.dst.rng_seed[slot] = a.src.rng_seed[i];
    a.dst.rng_row[slot] = a.src.rng_row[i];
    a.dst.row_sampling[slot] = a.src.row_sampling[i];
    a.dst.row_limits[slot] = a.src.row_limits[i];
    a.dst.out_len[slot] = a.src.out_len[i];
    a.dst.out_tokens[(size_t)slot * a.steps] = a.src.out_tokens[(size_t)i * a.steps];
    if (a.dst.drawn) { a.dst.drawn[2 * slot] = a.src.drawn[2 * i]; a.dst.drawn[2 * slot + 1] = a.src.drawn[2 * i + 1]; }
    if (a.dst.logp) a.dst.logp[(size_t)slot * a.steps] = a.src.logp[(size_t)i * a.steps];   // step 0's log-probability
  }
  const int hist = min(P + step, a.ycap);                                // prompt + the tokens sampled so far
  for (int t = tid; t < hist; t += 256) a.dst.ytok[(size_t)slot * a.ycap + t] = a.src.ytok[(size_t)i * a.ycap + t];
  for (int c = tid; c < a.d; c += 256) a.dst.ybuf[(size_t)slot * a.d + c] = a.src.ybuf[(size_t)i * a.d + c];
  if (a.dst.dump)                                                        // step 0's line of the [step][slots][V] dump
    for (int v = tid; v < a.V; v += 256) a.dst.dump[(size_t)slot * a.V + v] = a.src.dump[(size_t)i * a.V + v];
}

// the same fp32 expression as sample_step_kernel (t2s.hip) and MG_RUN_SAMPLER (t2s_mega.hip) write for a row that goes on
__global__ __launch_bounds__(64) void session_embed_kernel(const int* __restrict__ state, int mb, const int* __restrict__ plen,
                                                           const int* __restrict__ ytok, int ycap, const float* __restrict__ e_audio,
                                                           const float* __restrict__ pe, float alpha_a, int d, int V,
                                                           float* __restrict__ ybuf) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (!state[mb + b]) return;
  const int pos = plen[b] + state[2 * mb + b] - 1;                       // a live row has run step 0: step >= 1
  if (pos < 0 || pos >= ycap) return;
  const int tok = min(max(ytok[(long long)b * ycap + pos], 0), V - 1);
  const float* e = e_audio + (long long)tok * d;
  const float* p = pe + (long long)pos * d;
  for (int c = lane; c < d; c += 64) ybuf[(long long)b * d + c] = e[c] + alpha_a * p[c];
}

// Release: thread i clears the live word of slot[i].  The host has checked that the slots are distinct and inside the session, so
// no two threads meet on a word; n_active loses one per row that was live (a finished row has left it already).  Nothing else of
// the slot is touched: the next admission overwrites its state, and a slot that is not live is skipped by every kernel.
__global__ __launch_bounds__(64) void session_release_kernel(int* __restrict__ state, int mb, const int* __restrict__ slot, int n,
                                                             int slots) {
  for (int i = threadIdx.x; i < n; i += 64) {
    const int b = slot[i];
    if (b < 0 || b >= slots) continue;
    if (state[mb + b]) {
      state[mb + b] = 0;
      atomicSub(state + 3 * mb, 1);
    }
  }
}

}  // namespace gsv

using namespace gsv;
using namespace gsveng;

namespace {

int launch_session_adopt(const AdoptArgs& a, hipStream_t s) {
  const int hg = a.H % 4 == 0 ? 4 : 1;
  const int runs = a.L * 2 * (a.H / hg);
  GSV_LAUNCH(session_adopt_kernel, dim3(a.n * runs + a.n), dim3(256), 0, s, a, hg);
  return GSV_OK;
}

// ybuf[b] = e_audio[tok] + alpha_a * pe[P_b + step - 1], tok = ytok[b][P_b + step - 1], for every live row: the input embedding
// of the row's next step, which the last step of a launch does not leave behind
int launch_session_embed(const int* state, int mb, const int* plen, const int* ytok, int ycap, const float* e_audio, const float* pe,
                         float alpha_a, int d, int V, int slots, float* ybuf, hipStream_t s) {
  GSV_LAUNCH(session_embed_kernel, dim3(slots), dim3(64), 0, s, state, mb, plen, ytok, ycap, e_audio, pe, alpha_a, d, V, ybuf);
  return GSV_OK;
}

// clears the live word of slot[0 .. n - 1] (distinct, < slots) in the state block [kv_len | active | step | n_active] and takes
// the rows that were live out of n_active
int launch_session_release(int* state, int mb, const int* slot, int n, int slots, hipStream_t s) {
  GSV_LAUNCH(session_release_kernel, dim3(1), dim3(64), 0, s, state, mb, slot, n, slots);
  return GSV_OK;
}

// r's side of the adopt launch, with where its decode writes
AdoptView adopt_view(const RowState& r, const RowOutputs& o) {
  AdoptView v;
  v.kv = r.kv; v.layer_stride = r.kv_layer_stride; v.smax = r.max_seq;
  v.state = r.state; v.plen = r.plen; v.ytok = r.ytok; v.rng_row = r.rng_row; v.rng_seed = r.rng_seed;
  v.row_sampling = r.row_sampling; v.row_limits = r.row_limits; v.ybuf = r.ybuf;
  v.out_tokens = o.out_tokens; v.out_len = o.out_len; v.drawn = o.drawn; v.dump = o.dump; v.logp = o.logp;
  return v;
}

int session_begin(gsv_t2s* h, const gsv_sampling_params* sp, int slots, int row_sampling, int32_t* out_tokens, int32_t* out_len) {
  T2SSession& z = h->ses;
  RowState &r = h->rows, &st = z.staging;
  RowOutputs& so = z.staging_out;
  const size_t mb = (size_t)h->max_batch, d = h->cfg.dim, V = h->cfg.vocab, ms = (size_t)sp->max_steps;
  // staging copies of everything a prefill and a step-0 tail write (the staging K/V arena is sized by each admission)
  st.mb = (int)mb;
  GSV_RC(need(h, "ses_state", st.state_ints() * 4, (void**)&st.state));
  GSV_RC(need(h, "ses_plen", 2 * mb * 4, (void**)&st.plen));
  GSV_RC(need(h, "ses_ytok", mb * h->ycap * 4, (void**)&st.ytok));
  GSV_RC(need(h, "ses_rng_row", mb * 4, (void**)&st.rng_row));
  GSV_RC(need(h, "ses_rng_seed", mb * 8, (void**)&st.rng_seed));
  GSV_RC(need(h, "ses_row_sampling", mb * sizeof(RowSampling), (void**)&st.row_sampling));
  GSV_RC(need(h, "ses_row_limits", mb * sizeof(RowLimits), (void**)&st.row_limits));
  GSV_RC(need(h, "ses_sp", sizeof(StepParams), (void**)&st.sp));
  GSV_RC(need(h, "ses_out_tokens", mb * ms * 4, (void**)&so.out_tokens));
  GSV_RC(need(h, "ses_out_len", mb * 4, (void**)&so.out_len));
  GSV_RC(need(h, "ses_slot", mb * 4, (void**)&z.st_slot));
  int* drawn = nullptr;
  float *dump = nullptr, *logp = nullptr;
  GSV_RC(need(h, "ses_force", mb * ms * 4, (void**)&z.staging_force));
  GSV_RC(need(h, "ses_drawn", mb * 2 * 4, (void**)&drawn));
  GSV_RC(need(h, "ses_ybuf", mb * d * 4, (void**)&st.ybuf));
  GSV_RC(need(h, "ses_logits", mb * V * 4, (void**)&st.logits));
  GSV_RC(need(h, "ses_dump", mb * V * 4, (void**)&dump));
  GSV_RC(need(h, "ses_logp", mb * ms * 4, (void**)&logp));
  GSV_HIP(hipMemset(st.logits, 0, mb * V * 4));
  for (auto& e : z.ev) if (!e) GSV_HIP(hipEventCreate(&e));
  z.sp = *sp; z.slots = slots; z.budget = step_budget(*sp); z.row_sampling = row_sampling != 0;
  z.out = take_outputs(h, out_tokens, out_len);
  // a hook the session lacks is off in an admission's step 0 as well
  so.force = z.out.force ? z.staging_force : nullptr; so.dump = z.out.dump ? dump : nullptr;
  so.drawn = z.out.drawn ? drawn : nullptr; so.logp = z.out.logp ? logp : nullptr;
  // every slot free: active = 0, and every per-row array the kernels load for a free slot holds zeros, or the session's
  // scalars where an admission may leave them: the sampling values and limits, on the staging rows too
  GSV_HIP(hipMemset(r.state, 0, r.state_ints() * 4));
  GSV_HIP(hipMemset(r.plen, 0, 2 * mb * 4));
  GSV_HIP(hipMemset(r.rng_seed, 0, mb * 8));
  GSV_HIP(hipMemset(r.rng_row, 0, mb * 4));
  const std::vector<gsv_row_sampling_t> sampling(mb, sampling_of(z.sp));
  const std::vector<gsv_row_limits_t> limits(mb, limits_of(z.sp));
  for (const RowState* rs : {&r, &st}) {
    GSV_HIP(hipMemcpy(rs->row_sampling, sampling.data(), mb * sizeof(RowSampling), hipMemcpyHostToDevice));
    GSV_HIP(hipMemcpy(rs->row_limits, limits.data(), mb * sizeof(RowLimits), hipMemcpyHostToDevice));
  }
  GSV_HIP(hipMemset(r.ybuf, 0, mb * d * 4));
  forget_row_tables(h);   // the device arrays are the session's now
  h->rng_seed_next.clear(); h->rng_row_next.clear(); h->row_sampling_next.clear(); h->row_limits_next.clear();
  const StepParams p = step_params(z.sp.max_steps, r, z.out), ps = step_params(z.sp.max_steps, st, so);
  GSV_HIP(hipMemcpy(r.sp, &p, sizeof(p), hipMemcpyHostToDevice));
  GSV_HIP(hipMemcpy(st.sp, &ps, sizeof(ps), hipMemcpyHostToDevice));
  r.B = slots; r.P = 0;
  z.live.assign(slots, 0);
  z.last_adopt_ms = 0.f; z.last_adopt_bytes = 0;
  z.open = true;
  return GSV_OK;
}

int session_admit(gsv_t2s* h, int n, const int32_t* slot_ids, const int32_t* phones, const int32_t* phone_lens, const float* bert,
                  const int32_t* prompts_packed, const int32_t* prompt_lens, const uint64_t* rng_seeds, const int32_t* rng_rows,
                  const gsv_row_sampling_t* row_sampling, const std::vector<gsv_row_limits_t>& limits, hipStream_t s) {
  T2SSession& z = h->ses;
  RowState& st = z.staging;
  const RowOutputs& so = z.staging_out;
  const auto& c = h->cfg;
  const size_t ms = (size_t)z.sp.max_steps;
  int maxS = 0;
  long long positions = 0;
  for (int i = 0; i < n; ++i) {
    const int S = phone_lens[i] + prompt_lens[i];
    maxS = S > maxS ? S : maxS;
    positions += S;
  }
  // the staging arena: n rows of the admission's longest row + 2 positions
  st.max_seq = maxS + 2; st.kv_layer_stride = (size_t)n * c.dim * st.max_seq;
  GSV_RC(need(h, "ses_kv", (size_t)c.n_layer * 2 * st.kv_layer_stride * esz(h), &st.kv));
  GSV_HIP(hipMemcpyAsync(st.rng_seed, rng_seeds, (size_t)n * 8, hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemcpyAsync(st.rng_row, rng_rows, (size_t)n * 4, hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemcpyAsync(z.st_slot, slot_ids, (size_t)n * 4, hipMemcpyHostToDevice, s));
  // this admission's rows: their own sampling values and limits, or the session's scalars, which the adopt launch also puts
  // in the place of what the slot's last occupant had
  const std::vector<gsv_row_sampling_t> sampling = row_sampling ? std::vector<gsv_row_sampling_t>(row_sampling, row_sampling + n)
                                                                : std::vector<gsv_row_sampling_t>((size_t)n, sampling_of(z.sp));
  const std::vector<gsv_row_limits_t> mine = !limits.empty() ? limits : std::vector<gsv_row_limits_t>((size_t)n, limits_of(z.sp));
  GSV_HIP(hipMemcpyAsync(st.row_sampling, sampling.data(), (size_t)n * sizeof(RowSampling), hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemcpyAsync(st.row_limits, mine.data(), (size_t)n * sizeof(RowLimits), hipMemcpyHostToDevice, s));
  GSV_HIP(hipMemsetAsync(so.out_len, 0xFF, (size_t)n * 4, s));     // -1: not finished
  if (so.force)   // step 0 of row i is forced with its slot's entry
    for (int i = 0; i < n; ++i)
      GSV_HIP(hipMemcpyAsync(z.staging_force + (size_t)i * ms, z.out.force + (size_t)slot_ids[i] * ms, 4, hipMemcpyDeviceToDevice, s));
  GSV_RC(t2s_prefill_into(h, st, phones, phone_lens, n, bert, prompts_packed, prompt_lens, s));
  GSV_RC(t2s_step0_tail(h, st, s));   // the rows now stand where gsv_t2s_decode's rows stand after its step 0
  AdoptArgs a;
  a.src = adopt_view(st, so); a.dst = adopt_view(h->rows, z.out);
  a.n = n; a.slots = z.slots; a.mb = h->max_batch; a.ycap = h->ycap; a.d = c.dim; a.V = c.vocab; a.L = c.n_layer; a.H = c.n_head;
  a.esize = (int)esz(h); a.steps = (int)ms; a.slot = z.st_slot;
  GSV_HIP(hipEventRecord(z.ev[0], s));
  GSV_RC(launch_session_adopt(a, s));
  GSV_HIP(hipEventRecord(z.ev[1], s));
  std::vector<int> act(n);
  GSV_HIP(hipMemcpyAsync(act.data(), st.active(), (size_t)n * 4, hipMemcpyDeviceToHost, s));
  GSV_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) z.live[slot_ids[i]] = act[i] != 0;
  (void)hipEventElapsedTime(&z.last_adopt_ms, z.ev[0], z.ev[1]);
  z.last_adopt_bytes = positions * c.n_layer * 2 * c.dim * (long long)esz(h);
  return GSV_OK;
}

int session_advance(gsv_t2s* h, int n_steps, int* live_out, int* steps_out, hipStream_t s) {
  T2SSession& z = h->ses;
  const RowState& r = h->rows;
  const size_t mb = (size_t)h->max_batch;
  bool any = false;
  for (char l : z.live) any = any || l;
  h->last_decode_mode = 0; h->last_decode_ms = 0.f; h->last_decode_steps = 0;
  if (any) {
    GSV_RC(launch_session_embed(r.state, (int)mb, r.plen, r.ytok, h->ycap, h->e_audio, h->pe, h->alpha_a, h->cfg.dim, h->cfg.vocab,
                                z.slots, r.ybuf, s));
    // a chunk is a decode call whose step 0 has been run: n_steps steps are "budget" n_steps + 1
    GSV_RC(run_chunk(h, n_steps + 1, z.out.out_len, nullptr, s));
    if (h->last_decode_mode == 0) h->last_decode_steps = n_steps;   // the launch path's steps are reported here
  }
  std::vector<int> st(3 * mb);
  GSV_HIP(hipMemcpyAsync(st.data(), r.state, 3 * mb * 4, hipMemcpyDeviceToHost, s));
  GSV_HIP(hipStreamSynchronize(s));
  for (int b = 0; b < z.slots; ++b) {
    z.live[b] = st[mb + b] != 0;
    if (live_out) live_out[b] = st[mb + b] != 0;
    if (steps_out) steps_out[b] = st[2 * mb + b];
  }
  return GSV_OK;
}

// the slots are distinct and inside the session (checked by the caller): one launch on the state block, then the host mirror
int session_release(gsv_t2s* h, int n, const int32_t* slot_ids, hipStream_t s) {
  T2SSession& z = h->ses;
  GSV_HIP(hipMemcpyAsync(z.st_slot, slot_ids, (size_t)n * 4, hipMemcpyHostToDevice, s));
  GSV_RC(launch_session_release(h->rows.state, h->max_batch, z.st_slot, n, z.slots, s));
  GSV_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) z.live[slot_ids[i]] = 0;
  return GSV_OK;
}

}  // namespace

extern "C" {

int gsv_t2s_session_begin(gsv_t2s_t* h, const gsv_sampling_params* sp, int slots, int row_sampling, int32_t* out_tokens,
                          int32_t* out_len) {
  GSV_REQUIRE(h && h->finalized, "t2s_session_begin: handle not finalized");
  if (h->ses.open) {
    set_error("t2s_session_begin: a decode session is already open on this handle");
    return GSV_ERR_STATE;
  }
  GSV_REQUIRE(sp && out_tokens && out_len, "t2s_session_begin: null argument");
  GSV_REQUIRE(slots >= 1 && slots <= h->max_batch, "t2s_session_begin: %d slots, max_batch is %d", slots, h->max_batch);
  GSV_REQUIRE(sp->max_steps >= 1, "t2s_session_begin: max_steps must be >= 1");
  return session_begin(h, sp, slots, row_sampling, out_tokens, out_len);
}

int gsv_t2s_session_admit(gsv_t2s_t* h, int n, const int32_t* slot_ids, const int32_t* phones, const int32_t* phone_lens,
                          const float* bert, const int32_t* prompts_packed, const int32_t* prompt_lens, const uint64_t* rng_seeds,
                          const int32_t* rng_rows, const gsv_row_sampling_t* row_sampling, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "t2s_session_admit: handle not finalized");
  GSV_T2S_IN_SESSION(h, "t2s_session_admit", " (gsv_t2s_session_begin)");
  const T2SSession& z = h->ses;
  const int max_seq = h->rows.max_seq;
  // gsv_t2s_set_row_limits' rows are this admission's alone, whatever becomes of it
  std::vector<gsv_row_limits_t> limits;
  limits.swap(h->row_limits_next);
  const bool lim = !limits.empty();
  GSV_REQUIRE(slot_ids && phones && phone_lens && prompt_lens && rng_seeds && rng_rows, "t2s_session_admit: null argument");
  GSV_REQUIRE(n >= 1 && n <= z.slots, "t2s_session_admit: %d rows for a session of %d slots", n, z.slots);
  GSV_REQUIRE(!lim || (int)limits.size() == n, "t2s_session_admit: gsv_t2s_set_row_limits gave %d rows for an admission of %d rows",
              (int)limits.size(), n);
  if (lim) GSV_RC(check_row_limits_steps("t2s_session_admit", limits, z.sp.max_steps));
  long long packed = 0;
  for (int i = 0; i < n; ++i) packed += prompt_lens[i] > 0 ? prompt_lens[i] : 0;
  GSV_REQUIRE(prompts_packed || (lim && packed == 0), "t2s_session_admit: null argument");
  GSV_REQUIRE(!z.row_sampling || row_sampling, "t2s_session_admit: the session samples per row, row_sampling is null");
  GSV_REQUIRE(z.row_sampling || !row_sampling, "t2s_session_admit: row_sampling given, but the session was opened without it");
  if (row_sampling) GSV_RC(check_row_sampling("t2s_session_admit", row_sampling, n));
  GSV_RC(check_rng_rows("t2s_session_admit", rng_rows, n));
  // everything that can refuse the admission is checked here, before the first launch: a refused admission changes nothing
  std::vector<char> taken(z.slots, 0);
  for (int i = 0; i < n; ++i) {
    const int sl = slot_ids[i], P = prompt_lens[i];
    GSV_REQUIRE(sl >= 0 && sl < z.slots, "t2s_session_admit: row %d: slot %d outside the session's %d slots", i, sl, z.slots);
    GSV_REQUIRE(!z.live[sl], "t2s_session_admit: row %d: slot %d holds a live row", i, sl);
    GSV_REQUIRE(!taken[sl], "t2s_session_admit: slot %d is given twice", sl);
    taken[sl] = 1;
    GSV_REQUIRE(phone_lens[i] >= 1, "t2s_session_admit: empty phoneme sequence in row %d", i);
    // a prompt-free row only with limits of its own: its EOS horizon is then its own too (gsv_t2s_prefill_ragged)
    GSV_REQUIRE(P >= (lim ? 0 : 1), "t2s_session_admit: row %d has prompt length %d (must be >= 1)", i, P);
    const int budget = lim ? step_budget(limits[i]) : z.budget;
    GSV_REQUIRE((long long)phone_lens[i] + P + 2 + budget <= max_seq,
                "t2s_session_admit: row %d: %d positions + 2 + %d steps exceed the K/V arena (max_seq %d)", i, phone_lens[i] + P,
                budget, max_seq);
    GSV_REQUIRE(phone_lens[i] <= h->pe_rows && (long long)P + budget <= h->pe_rows,
                "t2s_session_admit: row %d: prompt %d + %d steps exceed the position table (%d rows)", i, P, budget, h->pe_rows);
    GSV_REQUIRE((long long)P + budget <= h->ycap, "t2s_session_admit: row %d: prompt %d + %d steps exceed the token history (%d)",
                i, P, budget, h->ycap);
  }
  return session_admit(h, n, slot_ids, phones, phone_lens, bert, prompts_packed, prompt_lens, rng_seeds, rng_rows, row_sampling, limits,
                       (hipStream_t)stream);
}

int gsv_t2s_session_advance(gsv_t2s_t* h, int n_steps, int* live_out, int* steps_out, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "t2s_session_advance: handle not finalized");
  GSV_T2S_IN_SESSION(h, "t2s_session_advance", " (gsv_t2s_session_begin)");
  GSV_REQUIRE(n_steps >= 1, "t2s_session_advance: n_steps %d must be >= 1", n_steps);
  return session_advance(h, n_steps, live_out, steps_out, (hipStream_t)stream);
}

int gsv_t2s_session_release(gsv_t2s_t* h, int n, const int32_t* slot_ids, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "t2s_session_release: handle not finalized");
  GSV_T2S_IN_SESSION(h, "t2s_session_release", " (gsv_t2s_session_begin)");
  const T2SSession& z = h->ses;
  GSV_REQUIRE(slot_ids, "t2s_session_release: null argument");
  GSV_REQUIRE(n >= 1 && n <= z.slots, "t2s_session_release: %d slots named in a session of %d slots", n, z.slots);
  std::vector<char> taken(z.slots, 0);
  for (int i = 0; i < n; ++i) {
    const int sl = slot_ids[i];
    GSV_REQUIRE(sl >= 0 && sl < z.slots, "t2s_session_release: slot %d outside the session's %d slots", sl, z.slots);
    GSV_REQUIRE(!taken[sl], "t2s_session_release: slot %d is given twice", sl);
    taken[sl] = 1;
  }
  return session_release(h, n, slot_ids, (hipStream_t)stream);
}

int gsv_t2s_session_end(gsv_t2s_t* h) {
  GSV_REQUIRE(h && h->finalized, "t2s_session_end: handle not finalized");
  GSV_T2S_IN_SESSION(h, "t2s_session_end", "");
  GSV_HIP(hipDeviceSynchronize());
  T2SSession& z = h->ses;
  z.open = false; z.live.clear();
  z.out = RowOutputs();
  h->rows.B = 0;   // the next decode needs a prefill of its own, as on a fresh handle
  forget_row_tables(h);
  h->row_limits_next.clear();
  return GSV_OK;
}

int gsv_t2s_session_state(gsv_t2s_t* h, int32_t* state) {
  GSV_REQUIRE(h && h->finalized && state, "t2s_session_state: null argument or handle not finalized");
  GSV_T2S_IN_SESSION(h, "t2s_session_state", "");
  const size_t mb = (size_t)h->max_batch, n = (size_t)h->ses.slots;
  GSV_HIP(hipDeviceSynchronize());
  for (int k = 0; k < 3; ++k) GSV_HIP(hipMemcpy(state + k * n, h->rows.state + k * mb, n * 4, hipMemcpyDeviceToHost));
  GSV_HIP(hipMemcpy(state + 3 * n, h->rows.plen, n * 4, hipMemcpyDeviceToHost));
  return GSV_OK;
}

int gsv_t2s_session_adopt_info(gsv_t2s_t* h, float* device_ms, int64_t* kv_bytes) {
  GSV_REQUIRE(h && h->finalized, "t2s_session_adopt_info: handle not finalized");
  if (device_ms) *device_ms = h->ses.last_adopt_ms;
  if (kv_bytes) *kv_bytes = h->ses.last_adopt_bytes;
  return GSV_OK;
}

}  // extern "C"
