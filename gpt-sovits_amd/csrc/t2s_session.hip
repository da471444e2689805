// Kernels of the AR decode sessions (gsv_t2s_session_*, host side in t2s.hip): the adopt launch that moves freshly prefilled rows
// from the staging arena into their slots of the main arena, the launch that rebuilds the next step's input embedding of
// every live row in front of an advance, and the launch that takes rows out of the decode (a cancelled request).
//
// Adopt.  An admission prefills its n rows as rows 0 .. n - 1 of a staging arena [layer][k|v][n][head][src_smax][32] (src_smax =
// the admission's longest row + 2, not max_seq) with the unchanged prefill kernels, and runs their step 0 on staging row state.
// One launch then copies, for row i and slot[i], every (layer, k|v, head) run of S_i cached positions -- S_i * 32 elements,
// contiguous on both sides -- and the row's state.  It is a pure copy: 16-byte accesses, no LDS, one workgroup per
// (row, layer, k|v, head group) run, the staging side read non-temporal (it is read once and never again).  Its traffic is
// n * S * L * 2 * d * sizeof(T) bytes read and as many written (49 152 B per cached position on the fp16 v2 decoder), which
// is what gsv_t2s_session_adopt_info reports the launch's time against.
#include "t2s_engine.h"

namespace gsv {

typedef unsigned u4v __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void session_adopt_kernel(AdoptArgs a, int hg /* heads per workgroup */) {
  const int tid = threadIdx.x;
  const int groups = a.H / hg, runs = a.L * 2 * groups;
  const int bid = blockIdx.x;
  if (bid < a.n * runs) {
    const int i = bid / runs, r = bid - i * runs;
    const int lw = r / groups, h0 = (r - lw * groups) * hg;
    const int slot = a.slot[i];
    const int S = min(a.src_state[i], min(a.src_smax, a.dst_smax));      // kv_len: step 0 appends nothing
    const int cpp = 32 * a.esize / 16;                                   // 16-byte chunks per cached position
    const int chunks = S * cpp;                                          // per head
    const size_t src_head = (size_t)a.src_smax * cpp, dst_head = (size_t)a.dst_smax * cpp;
    const u4v* src = (const u4v*)a.src_kv + (size_t)lw * (a.src_layer_stride / 32) * cpp + ((size_t)i * a.H + h0) * src_head;
    u4v* dst = (u4v*)a.dst_kv + (size_t)lw * (a.dst_layer_stride / 32) * cpp + ((size_t)slot * a.H + h0) * dst_head;
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
  const int P = a.src_plen[i], step = a.src_state[2 * mb + i];
  if (tid == 0) {
    const int act = a.src_state[mb + i];
    a.dst_plen[slot] = P;
    a.dst_state[slot] = a.src_state[i];
    a.dst_state[mb + slot] = act;
    a.dst_state[2 * mb + slot] = step;
    if (act) atomicAdd(a.dst_state + 3 * mb, 1);
    a.dst_rng_seed[slot] = a.src_rng_seed[i];
    a.dst_rng_row[slot] = a.src_rng_row[i];
    if (a.dst_row_sampling) a.dst_row_sampling[slot] = a.src_row_sampling[i];
    a.dst_out_len[slot] = a.src_out_len[i];
    a.dst_out_tokens[(size_t)slot * a.dst_steps] = a.src_out_tokens[(size_t)i * a.src_steps];
    if (a.dst_drawn) { a.dst_drawn[2 * slot] = a.src_drawn[2 * i]; a.dst_drawn[2 * slot + 1] = a.src_drawn[2 * i + 1]; }
    if (a.dst_logp) a.dst_logp[(size_t)slot * a.dst_steps] = a.src_logp[(size_t)i * a.src_steps];   // step 0's log-probability
  }
  const int hist = min(P + step, a.ycap);                                // prompt + the tokens sampled so far
  for (int t = tid; t < hist; t += 256) a.dst_ytok[(size_t)slot * a.ycap + t] = a.src_ytok[(size_t)i * a.ycap + t];
  for (int c = tid; c < a.d; c += 256) a.dst_ybuf[(size_t)slot * a.d + c] = a.src_ybuf[(size_t)i * a.d + c];
  if (a.dst_dump)                                                        // step 0's line of the [step][slots][V] dump
    for (int v = tid; v < a.V; v += 256) a.dst_dump[(size_t)slot * a.V + v] = a.src_dump[(size_t)i * a.V + v];
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

int launch_session_adopt(const AdoptArgs& a, hipStream_t s) {
  const int hg = a.H % 4 == 0 ? 4 : 1;
  const int runs = a.L * 2 * (a.H / hg);
  GSV_LAUNCH(session_adopt_kernel, dim3(a.n * runs + a.n), dim3(256), 0, s, a, hg);
  return GSV_OK;
}

int launch_session_embed(const int* state, int mb, const int* plen, const int* ytok, int ycap, const float* e_audio, const float* pe,
                         float alpha_a, int d, int V, int slots, float* ybuf, hipStream_t s) {
  GSV_LAUNCH(session_embed_kernel, dim3(slots), dim3(64), 0, s, state, mb, plen, ytok, ycap, e_audio, pe, alpha_a, d, V, ybuf);
  return GSV_OK;
}

int launch_session_release(int* state, int mb, const int* slot, int n, int slots, hipStream_t s) {
  GSV_LAUNCH(session_release_kernel, dim3(1), dim3(64), 0, s, state, mb, slot, n, slots);
  return GSV_OK;
}

}  // namespace gsv
