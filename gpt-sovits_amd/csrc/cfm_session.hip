// Flow-matching sessions (gsv_cfm_session_*): a pass whose rows carry their own time.  Every row has its own step count,
// step index and guidance rate; the pass is advanced a few Euler steps at a time, and rows enter (admit) and leave (fetch,
// release) between steps.  The modulation tables, the text stack and the DiT forward are cfm.hip's (cfm_engine.h); what is
// here is the slot store, the packing of the live rows into the DiT's input, and the per-row Euler step.
//
// Slots and DiT rows.  A session of rows_cap has rows_cap slots; slot s keeps, from admission to fetch, the row's Euler state
// x [T][mel] fp32, its text embedding [T][text_dim] and its cond columns [T][mel] (prompt frames, zeros after them), so that
// nothing of the caller's is read after admit has been issued.  One more text slot holds the null text embedding, computed
// with the first guided row of the session.  rows_cap counts DiT rows: a guided row takes two (itself and its unconditioned
// twin), and an admission that would bring the live DiT rows above rows_cap is refused before anything is launched.
//
// Packing.  A step runs the DiT over the live rows in ascending slot order, then the twins of the guided live rows in the same
// order -- for a session whose rows were admitted together into slots 0 .. B-1 with one setting, exactly the rows of the
// one-shot pass.  The packed input xin is rebuilt (one launch) only when the live set changed since the previous step: after an
// admission, a release, or a row's last step.  Between such changes a step is: one gather of the rows' modulation vectors into
// the dense per-step table [block][packed row][6D] (+ [packed row][2D] for the final layer), the DiT forward with the per-row
// forms of the launches that read a modulation vector, and the per-row Euler kernel, which also refreshes the x columns of xin.
// Tables of at most 64 rows travel as kernel arguments (as cfm.hip's row table does): no upload, no wait.
//
// Time.  Row b at its step i uses the vectors of table(n_steps_b)[i], where table(N) is what cfm.hip's modulations<T>(N)
// computes for a one-shot call of N steps: t_i = (float) of the double sum of i terms 1.0 / N, d = (float)(1.0 / N).  The tables
// are cached on the handle by step count (CfmSession::cache), so a row's modulations are bit for bit those of a one-shot call
// with its n_steps.  The cache holds at most kCacheEntries tables and kCacheBytes bytes; the least recently used table that no
// live row and no row of the admission at hand needs is dropped first, and an admission that needs more distinct live step
// counts than the cache holds is refused.
#include <algorithm>
#include <cmath>

#include "cfm_engine.h"

using namespace gsv;
using namespace gsveng;
using namespace gsvcfm;

namespace {

constexpr int kMaxRows = GSV_CFM_SESSION_MAX_ROWS;
static_assert(kMaxRows <= CFM_ROW_CHUNK, "the admission table is one CfmRowChunk");
constexpr int kCacheEntries = 8;
constexpr size_t kCacheBytes = (size_t)1 << 30;

enum { SLOT_FREE = 0, SLOT_LIVE = 1, SLOT_DONE = 2 };

struct SessSlot {
  int state = SLOT_FREE, n_steps = 0, step = 0, Tp = 0, adapter = -1, rp = 0;
  float rate = 0.f;
  bool guided = false;
};

struct ModsEntry { int N = 0; float* dev = nullptr; size_t bytes = 0; unsigned long long stamp = 0; };

// kernel-argument tables, one entry per packed row (pack, gather) or per live row (Euler, admission)
struct IntTab { int v[kMaxRows]; };
struct PackTab { int slot[kMaxRows], lora[kMaxRows]; };
struct GatherRow { const float* mods; int N, step; };
struct GatherTab { GatherRow r[kMaxRows]; };
struct StepRow { int slot, twin, Tp; float d, rate; };   // twin: packed index of the unconditioned twin, -1 = unguided
struct StepTab { StepRow r[kMaxRows]; };

}  // namespace

struct CfmSession {
  bool open = false;
  int cap = 0, Tn = 0;
  float temperature = 1.f;
  std::vector<SessSlot> slots;
  bool null_ready = false, dirty = true;
  int packed_rows = 0, packed_max_rp = 0;
  // device, sized at begin (workspace arena of the handle)
  float *xs = nullptr, *cs = nullptr, *v = nullptr, *dense_blk = nullptr, *dense_fin = nullptr;
  void *cond = nullptr, *te = nullptr, *xin = nullptr;
  int* lora_slot = nullptr;
  std::vector<ModsEntry> cache;
  unsigned long long clock = 0;
};

namespace {

// admission: row b of the call -> slot tab.v[b].  x0 [n][Tn][C] fp32 and the text embedding ta [n][Tn][td] move into the slot
// store; the cond columns are built from the row's prompt ([C][Tp] channels-first), zero after it
template <typename T>
__global__ void cfm_sess_store_kernel(IntTab tab, const CfmRow* __restrict__ rw, const float* __restrict__ x0, const T* __restrict__ ta, int Tn,
                                      int C, int td, float* __restrict__ xs, T* __restrict__ cond, T* __restrict__ te) {
  const int W = 2 * C + td;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * W) return;
  const int t = (int)(i / W), c = (int)(i - (long long)t * W);
  const int b = blockIdx.y, sl = tab.v[b];
  if (c < C) xs[((long long)sl * Tn + t) * C + c] = x0[((long long)b * Tn + t) * C + c];
  else if (c < 2 * C) {
    const float* prompt = rw[b].prompt;
    const int Tp = rw[b].Tp, cc = c - C;
    cond[((long long)sl * Tn + t) * C + cc] = (T)(prompt && t < Tp ? prompt[(long long)cc * Tp + t] : 0.f);
  } else te[((long long)sl * Tn + t) * td + (c - 2 * C)] = ta[((long long)b * Tn + t) * td + (c - 2 * C)];
}

// the packed DiT input of the live set: packed row p (blockIdx.y) is slot tab.slot[p]; p >= n_cond is a twin (zero cond
// columns, the null text embedding in text slot `null_slot`).  Columns: x | cond | text | zero pad.  Also the rows' LoRA slots.
template <typename T>
__global__ void cfm_sess_pack_kernel(PackTab tab, int n_cond, int null_slot, const float* __restrict__ xs, const T* __restrict__ cond,
                                     const T* __restrict__ te, int Tn, int C, int td, T* __restrict__ xin, int ldin, int* __restrict__ lora_slot) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y, sl = tab.slot[p];
  if (i == 0) lora_slot[p] = tab.lora[p];
  if (i >= (long long)Tn * ldin) return;
  const int t = (int)(i / ldin), c = (int)(i - (long long)t * ldin);
  const bool twin = p >= n_cond;
  T val = (T)0.f;
  if (c < C) val = (T)xs[((long long)sl * Tn + t) * C + c];
  else if (c < 2 * C) { if (!twin) val = cond[((long long)sl * Tn + t) * C + (c - C)]; }
  else if (c < 2 * C + td) val = te[((long long)(twin ? null_slot : sl) * Tn + t) * td + (c - 2 * C)];
  xin[((long long)p * Tn + t) * ldin + c] = val;
}

// this step's modulation vectors of every packed row, from the row's cached table at the row's own step:
// dense_blk[l][p][6D] = table_p[l][step_p][6D], dense_fin[p][2D] = table_p[depth][step_p][2D]   (blockIdx.z = l, depth = final)
__global__ void cfm_sess_gather_kernel(GatherTab tab, int DB, int depth, int D, float* __restrict__ dense_blk, float* __restrict__ dense_fin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y, l = blockIdx.z;
  const GatherRow r = tab.r[p];
  if (l < depth) {
    if (i < 6 * D) dense_blk[((size_t)l * DB + p) * 6 * D + i] = r.mods[((size_t)l * r.N + r.step) * 6 * D + i];
  } else if (i < 2 * D) {
    dense_fin[(size_t)p * 2 * D + i] = r.mods[(size_t)depth * r.N * 6 * D + (size_t)r.step * 2 * D + i];
  }
}

// The per-row form of cfm_euler_kernel: live row p (blockIdx.y) steps its slot's state with its own d and rate.  The two
// expressions are cfm_euler_kernel's, written the same way (v tested the same way) so that they compile to the same arithmetic:
// an unguided row takes the unguided one and never sees a rate, a guided row combines its estimate (packed row p) with its
// twin's (packed row r.twin).  The refreshed x goes into the x columns of the row's packed input, and of its twin's.
template <typename T>
__global__ void cfm_sess_euler_kernel(StepTab tab, float* __restrict__ xs, const float* __restrict__ v, int Tn, int C, T* __restrict__ xin,
                                      int ldin) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  const int t = (int)(i / C), c = (int)(i - (long long)t * C);
  const int p = blockIdx.y;
  const StepRow r = tab.r[p];
  float* x = xs + (long long)r.slot * Tn * C;
  const float d = r.d, rate = r.rate;
  const long long vi = (long long)p * Tn * C + i;
  float u = 0.f;
  if (t >= r.Tp) {
    if (r.twin >= 0) {
      u = x[i];
      if (v) {
        const float vp = v[vi], vn = v[(long long)r.twin * Tn * C + i];
        u += d * (vp + (vp - vn) * rate);
      }
    } else {
      u = x[i] + (v ? d * v[vi] : 0.f);
    }
  }
  x[i] = u;
  xin[((long long)p * Tn + t) * ldin + c] = (T)u;
  if (r.twin >= 0) xin[((long long)r.twin * Tn + t) * ldin + c] = (T)u;
}

// a finished slot's state, channels-last fp32 [Tn][C] -> channels-first [C][Tn], the prompt frames as the zeros they are held at
__global__ void cfm_sess_out_kernel(const float* __restrict__ x, int Tp, int Tn, int C, float* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Tn * C) return;
  const int c = (int)(i / Tn), t = (int)(i - (long long)c * Tn);
  out[i] = t < Tp ? 0.f : x[(long long)t * C + c];
}

// Finished slots straight into the vocoder's layout (fetch_mel): entry i (blockIdx.z) is slot tab.slot[i]; its generated frames
// t in [Tp, Tn) go, de-normalised and channels-first, to out[c][col0 + t - Tp] of the matrix out [C][ld].  One block moves a tile
// of kMelTile frames x kMelTile channels through LDS: a wave reads kMelTile consecutive channels of one frame and writes
// kMelTile consecutive frames of one channel, so both sides are contiguous (cfm_sess_out_kernel reads with a stride of C floats).
// The tile rows are padded by one float: the column reads of the write phase then fall into distinct banks.
// The arithmetic is TTS.denorm_spec's, in its order and uncontracted, so the bits are torch's: ((x + 1) / 2) * w + lo, w = hi - lo.
constexpr int kMelTile = 64;
struct MelTab { int slot[kMaxRows], Tp[kMaxRows], col0[kMaxRows]; };

__global__ __launch_bounds__(256) void cfm_sess_mel_kernel(MelTab tab, const float* __restrict__ xs, int Tn, int C, float w, float lo,
                                                           float* __restrict__ out, long long ld) {
  __shared__ float tile[kMelTile][kMelTile + 1];
  const int e = blockIdx.z, Tp = tab.Tp[e], len = Tn - Tp;
  const int g0 = blockIdx.x * kMelTile, c0 = blockIdx.y * kMelTile;
  if (g0 >= len) return;                                   // the whole block leaves: no barrier is missed
  const float* x = xs + ((long long)tab.slot[e] * Tn + Tp) * C;
  const int lane = threadIdx.x & (kMelTile - 1), row = threadIdx.x / kMelTile;       // 256 threads: 4 tile rows per pass
  for (int r = row; r < kMelTile; r += 256 / kMelTile) {
    const int g = g0 + r, c = c0 + lane;
    if (g < len && c < C) tile[r][lane] = x[(long long)g * C + c];
  }
  __syncthreads();
  float* o = out + tab.col0[e];
  for (int r = row; r < kMelTile; r += 256 / kMelTile) {
    const int c = c0 + r, g = g0 + lane;
    if (c < C && g < len) {
#pragma clang fp contract(off)
      const float v = tile[lane][r];
      o[(long long)c * ld + g] = ((v + 1.f) / 2.f) * w + lo;
    }
  }
}

int live_dit_rows(const CfmSession* ss) {
  int n = 0;
  for (const auto& sl : ss->slots) if (sl.state == SLOT_LIVE) n += sl.guided ? 2 : 1;
  return n;
}

ModsEntry* cache_find(CfmSession* ss, int N) {
  for (auto& e : ss->cache) if (e.N == N) return &e;
  return nullptr;
}

bool cache_pinned(const CfmSession* ss, int N, const std::vector<int>& wanted) {
  for (const auto& sl : ss->slots) if (sl.state == SLOT_LIVE && sl.n_steps == N) return true;
  return std::find(wanted.begin(), wanted.end(), N) != wanted.end();
}

// drops least recently used tables that nothing needs until `extra` more tables of `extra_bytes` fit the bounds; false = they
// cannot (every table that would have to go is pinned).  dry: only answer, drop nothing.
bool cache_make_room(CfmSession* ss, const std::vector<int>& wanted, int extra, size_t extra_bytes, bool dry) {
  std::vector<ModsEntry> keep = ss->cache;
  auto total = [&]() { size_t b = extra_bytes; for (auto& e : keep) b += e.bytes; return b; };
  while ((int)keep.size() + extra > kCacheEntries || (total() > kCacheBytes && !keep.empty())) {
    int victim = -1;
    for (int i = 0; i < (int)keep.size(); ++i)
      if (!cache_pinned(ss, keep[i].N, wanted) && (victim < 0 || keep[i].stamp < keep[victim].stamp)) victim = i;
    if (victim < 0) {
      if ((int)keep.size() + extra > kCacheEntries) return false;
      break;   // over the byte bound with pinned tables only: the rows at hand need them, they stay
    }
    if (!dry) {
      for (auto it = ss->cache.begin(); it != ss->cache.end(); ++it)
        if (it->N == keep[victim].N) { (void)hipFree(it->dev); ss->cache.erase(it); break; }   // hipFree waits for the device
    }
    keep.erase(keep.begin() + victim);
  }
  return true;
}

template <typename T>
int cache_fill(gsv_cfm* c, CfmSession* ss, hipStream_t s, int N) {
  float* mods = nullptr;
  GSV_RC(modulations<T>(c, s, N, &mods));
  ModsEntry e;
  e.N = N; e.bytes = mods_floats(c, N) * 4;
  GSV_HIP(hipMalloc((void**)&e.dev, e.bytes));
  hipError_t rc = hipMemcpyAsync(e.dev, mods, e.bytes, hipMemcpyDeviceToDevice, s);
  if (rc != hipSuccess) { (void)hipFree(e.dev); set_error("cfm_session: copy of the modulation table failed: %s", hipGetErrorString(rc)); return GSV_ERR_HIP; }
  e.stamp = ++ss->clock;
  ss->cache.push_back(e);
  return GSV_OK;
}

template <typename T>
int sess_begin(gsv_cfm* c, CfmSession* ss, hipStream_t s) {
  const auto& g = c->cfg;
  const int cap = ss->cap, Tn = ss->Tn, md = g.mel_dim, td = g.text_dim, D = g.dim, half = g.dim_head / 2;
  const size_t es = sizeof(T), R = (size_t)cap * Tn;
  GSV_RC(need(c, "cfms_x", R * md * 4, (void**)&ss->xs));
  GSV_RC(need(c, "cfms_cond", R * md * es, &ss->cond));
  GSV_RC(need(c, "cfms_te", (R + Tn) * td * es, &ss->te));
  GSV_RC(need(c, "cfms_mods", ((size_t)g.depth * 6 + 2) * cap * D * 4, (void**)&ss->dense_blk));
  ss->dense_fin = ss->dense_blk + (size_t)g.depth * cap * 6 * D;
  GSV_RC(need(c, "cfms_lora", (size_t)cap * sizeof(int), (void**)&ss->lora_slot));
  GSV_RC(need(c, "cfm_xin", R * c->ldin * es, &ss->xin));
  GSV_RC(need(c, "cfm_v", R * md * 4, (void**)&ss->v));
  GSV_RC(need(c, "cfm_cs", (size_t)Tn * half * 2 * 4, (void**)&ss->cs));
  return rope_table(s, Tn, half, ss->cs);
}

template <typename T>
int sess_admit(gsv_cfm* c, CfmSession* ss, hipStream_t s, int n, const int32_t* slots, const float* mu, const std::vector<CfmRow>& rows,
               const std::vector<int>& new_steps, bool want_null, const float* noise) {
  const auto& g = c->cfg;
  const int Tn = ss->Tn, md = g.mel_dim, td = g.text_dim;
  const size_t es = sizeof(T);
  for (int N : new_steps) GSV_RC(cache_fill<T>(c, ss, s, N));
  const int TB = n + (want_null ? 1 : 0);
  CfmRow* rw;
  float *x0, *gx;
  void *ta, *tb, *tw;
  GSV_RC(need(c, "cfm_rows", (size_t)n * sizeof(CfmRow), (void**)&rw));
  GSV_RC(need(c, "cfm_x", (size_t)n * Tn * md * 4, (void**)&x0));
  GSV_RC(need(c, "cfm_gx", (size_t)TB * 2 * td * 4, (void**)&gx));
  GSV_RC(need(c, "cfm_ta", (size_t)TB * Tn * td * es, &ta));
  GSV_RC(need(c, "cfm_tb", (size_t)TB * Tn * td * es, &tb));
  GSV_RC(need(c, "cfm_tw", (size_t)TB * Tn * 2 * td * es, &tw));
  GSV_RC(rows_upload(s, rows.data(), n, rw));
  GSV_RC(text_stack<T>(c, s, mu, n, TB, Tn, ta, tb, tw, gx));
  GSV_RC(init_x(s, noise, rw, ss->temperature, Tn, md, n, x0));
  IntTab tab{};
  std::copy_n(slots, n, tab.v);
  GSV_LAUNCH(cfm_sess_store_kernel<T>, cfm_grid((long long)Tn * (2 * md + td), n), dim3(256), 0, s, tab, rw, x0, (const T*)ta, Tn, md, td, ss->xs,
             (T*)ss->cond, (T*)ss->te);
  if (want_null) {   // text row n is the null text embedding: it depends on Tn alone, kept in text slot `cap` for every twin
    GSV_HIP(hipMemcpyAsync((char*)ss->te + (size_t)ss->cap * Tn * td * es, (const char*)ta + (size_t)n * Tn * td * es, (size_t)Tn * td * es,
                           hipMemcpyDeviceToDevice, s));
    ss->null_ready = true;
  }
  return GSV_OK;
}

template <typename T>
int sess_step(gsv_cfm* c, CfmSession* ss, hipStream_t s, int k) {
  const auto& g = c->cfg;
  const int Tn = ss->Tn, md = g.mel_dim, td = g.text_dim, D = g.dim, ldin = c->ldin;
  for (int it = 0; it < k; ++it) {
    // the packing of this step: live rows in ascending slot order, then the twins of the guided ones in the same order
    std::vector<int> live;
    for (int sl = 0; sl < ss->cap; ++sl) if (ss->slots[sl].state == SLOT_LIVE) live.push_back(sl);
    if (live.empty()) break;
    const int nl = (int)live.size();
    PackTab pt{};
    GatherTab gt{};
    StepTab st{};
    int DB = nl, max_rp = 0;
    for (int p = 0; p < nl; ++p) {
      SessSlot& sl = ss->slots[live[p]];
      ModsEntry* e = cache_find(ss, sl.n_steps);
      if (!e) { set_error("cfm_session_step: the modulation table of %d steps is gone", sl.n_steps); return GSV_ERR_ARG; }
      e->stamp = ++ss->clock;
      pt.slot[p] = live[p]; pt.lora[p] = sl.adapter;
      gt.r[p] = GatherRow{e->dev, sl.n_steps, sl.step};
      st.r[p] = StepRow{live[p], -1, sl.Tp, (float)(1.0 / sl.n_steps), sl.rate};
      max_rp = std::max(max_rp, sl.rp);
    }
    for (int p = 0; p < nl; ++p)
      if (ss->slots[live[p]].guided) {
        pt.slot[DB] = live[p]; pt.lora[DB] = pt.lora[p];
        gt.r[DB] = gt.r[p];
        st.r[p].twin = DB++;
      }
    if (DB > ss->cap) { set_error("cfm_session_step: %d live DiT rows exceed the session's %d", DB, ss->cap); return GSV_ERR_ARG; }
    if (ss->dirty) {
      GSV_LAUNCH(cfm_sess_pack_kernel<T>, cfm_grid((long long)Tn * ldin, DB), dim3(256), 0, s, pt, nl, ss->cap, ss->xs, (const T*)ss->cond,
                 (const T*)ss->te, Tn, md, td, (T*)ss->xin, ldin, ss->lora_slot);
      ss->dirty = false;
    }
    GSV_LAUNCH(cfm_sess_gather_kernel, dim3(nblk(6 * D), DB, g.depth + 1), dim3(256), 0, s, gt, DB, g.depth, D, ss->dense_blk, ss->dense_fin);
    DitMods m;
    m.blk = ss->dense_blk; m.blk_stride = (size_t)DB * 6 * D; m.fin = ss->dense_fin; m.rows = 1;
    GSV_RC(dit_forward<T>(c, s, ss->xin, DB, Tn, m, ss->lora_slot, 1, max_rp, ss->cs, ss->v));
    GSV_LAUNCH(cfm_sess_euler_kernel<T>, cfm_grid((long long)Tn * md, nl), dim3(256), 0, s, st, ss->xs, (const float*)ss->v, Tn, md, (T*)ss->xin,
               ldin);
    for (int p = 0; p < nl; ++p) {
      SessSlot& sl = ss->slots[live[p]];
      if (++sl.step >= sl.n_steps) { sl.state = SLOT_DONE; ss->dirty = true; }   // it takes no part in the next step
    }
  }
  return GSV_OK;
}

}  // namespace

namespace gsvcfm {

bool session_open(const gsv_cfm* c) { return c && c->sess && c->sess->open; }

bool session_uses_adapter(const gsv_cfm* c, int slot) {
  if (!session_open(c)) return false;
  for (const auto& sl : c->sess->slots) if (sl.state == SLOT_LIVE && sl.adapter == slot) return true;
  return false;
}

void session_destroy(gsv_cfm* c) {
  if (!c || !c->sess) return;
  for (auto& e : c->sess->cache) if (e.dev) (void)hipFree(e.dev);
  delete c->sess;
  c->sess = nullptr;
}

}  // namespace gsvcfm

extern "C" {

int gsv_cfm_session_begin(gsv_cfm_t* c, int rows_cap, int T, float temperature, gsv_stream_t stream) {
  GSV_REQUIRE(c && c->finalized, "cfm_session_begin: handle not finalized");
  GSV_REQUIRE(!session_open(c), "cfm_session_begin: a session is already open on this handle");
  GSV_REQUIRE(rows_cap >= 1 && rows_cap <= kMaxRows, "cfm_session_begin: rows_cap %d is outside [1, %d]", rows_cap, kMaxRows);
  GSV_REQUIRE(T > 0 && std::isfinite(temperature), "cfm_session_begin: bad T or temperature");
  if (!c->sess) c->sess = new CfmSession();
  CfmSession* ss = c->sess;
  ss->cap = rows_cap; ss->Tn = T; ss->temperature = temperature;
  ss->slots.assign(rows_cap, SessSlot{});
  ss->null_ready = false; ss->dirty = true;
  GSV_RC(GSV_WITH_T(c, sess_begin<T>(c, ss, (hipStream_t)stream)));
  ss->open = true;
  return GSV_OK;
}

int gsv_cfm_session_admit(gsv_cfm_t* c, int n, const int32_t* slots, const float* mu, const float* const* prompts, const int* Tp,
                          const int* adapters, const int* n_steps, const float* cfg_rate, const float* noise, const uint64_t* seeds,
                          gsv_stream_t stream) {
  GSV_REQUIRE(session_open(c), "cfm_session_admit: no open session");
  CfmSession* ss = c->sess;
  GSV_REQUIRE(n >= 1 && n <= ss->cap && slots && mu && Tp && n_steps && cfg_rate, "cfm_session_admit: bad argument");
  GSV_REQUIRE(noise || seeds, "cfm_session_admit: neither noise nor seeds given");
  std::vector<CfmRow> rows(n);
  std::vector<SessSlot> fresh(n);
  std::vector<int> wanted, missing;
  int new_dit = 0;
  bool any_guided = false;
  for (int b = 0; b < n; ++b) {
    GSV_REQUIRE(slots[b] >= 0 && slots[b] < ss->cap, "cfm_session_admit: row %d: slot %d is outside [0, %d)", b, slots[b], ss->cap);
    GSV_REQUIRE(ss->slots[slots[b]].state == SLOT_FREE, "cfm_session_admit: row %d: slot %d is occupied", b, slots[b]);
    for (int a = 0; a < b; ++a) GSV_REQUIRE(slots[a] != slots[b], "cfm_session_admit: slot %d is given twice", slots[b]);
    GSV_REQUIRE(n_steps[b] >= 1 && n_steps[b] <= 1024, "cfm_session_admit: row %d: %d steps are outside [1, 1024]", b, n_steps[b]);
    GSV_REQUIRE(std::isfinite(cfg_rate[b]), "cfm_session_admit: row %d: cfg_rate is not finite", b);
    GSV_REQUIRE(Tp[b] >= 0 && Tp[b] <= ss->Tn && (Tp[b] == 0 || (prompts && prompts[b])),
                "cfm_session_admit: row %d: prompt length %d does not fit %d frames, or its prompt is null", b, Tp[b], ss->Tn);
    const int ad = adapters ? adapters[b] : -1;
    GSV_REQUIRE(ad >= -1 && ad < GSV_CFM_MAX_ADAPTERS, "cfm_session_admit: row %d: adapter slot %d is outside [-1, %d)", b, ad, GSV_CFM_MAX_ADAPTERS);
    int rp = 0;
    if (ad >= 0) {
      GSV_REQUIRE(ad < (int)c->adapters.size() && c->adapters[ad].dev, "cfm_session_admit: row %d: no adapter in slot %d", b, ad);
      rp = c->adapters[ad].rp;
    }
    SessSlot& f = fresh[b];
    f.state = SLOT_LIVE; f.n_steps = n_steps[b]; f.step = 0; f.Tp = Tp[b]; f.adapter = ad; f.rp = rp; f.rate = cfg_rate[b];
    f.guided = cfg_rate[b] > CFM_CFG_THRESHOLD;
    any_guided |= f.guided;
    new_dit += f.guided ? 2 : 1;
    rows[b] = CfmRow{Tp[b] ? prompts[b] : nullptr, seeds ? (unsigned long long)seeds[b] : 0ull, Tp[b], ad};
    if (std::find(wanted.begin(), wanted.end(), n_steps[b]) == wanted.end()) {
      wanted.push_back(n_steps[b]);
      if (!cache_find(ss, n_steps[b])) missing.push_back(n_steps[b]);
    }
  }
  const int live = live_dit_rows(ss);
  GSV_REQUIRE(live + new_dit <= ss->cap, "cfm_session_admit: %d live DiT rows + %d new (a guided row counts 2) exceed rows_cap %d", live, new_dit,
              ss->cap);
  size_t missing_bytes = 0;
  for (int N : missing) missing_bytes += mods_floats(c, N) * 4;
  GSV_REQUIRE(cache_make_room(ss, wanted, (int)missing.size(), missing_bytes, true),
              "cfm_session_admit: more than %d distinct step counts among the live rows and this admission", kCacheEntries);
  // ---- nothing was launched or changed up to here.  From here on a failure (an allocation, a launch) admits no row and leaves
  // every slot as it was, but the cache may already have dropped or gained a table and the null text row may be in place:
  // both are caches of values that depend on nothing in the rows, so a later admission finds them correct
  cache_make_room(ss, wanted, (int)missing.size(), missing_bytes, false);
  const bool want_null = any_guided && !ss->null_ready;
  GSV_RC(GSV_WITH_T(c, sess_admit<T>(c, ss, (hipStream_t)stream, n, slots, mu, rows, missing, want_null, noise)));
  for (int b = 0; b < n; ++b) ss->slots[slots[b]] = fresh[b];
  ss->dirty = true;
  return GSV_OK;
}

int gsv_cfm_session_step(gsv_cfm_t* c, int k, gsv_stream_t stream) {
  GSV_REQUIRE(session_open(c), "cfm_session_step: no open session");
  GSV_REQUIRE(k >= 1, "cfm_session_step: k = %d", k);
  return GSV_WITH_T(c, sess_step<T>(c, c->sess, (hipStream_t)stream, k));
}

int gsv_cfm_session_fetch(gsv_cfm_t* c, int slot, float* out, gsv_stream_t stream) {
  GSV_REQUIRE(session_open(c), "cfm_session_fetch: no open session");
  CfmSession* ss = c->sess;
  GSV_REQUIRE(out && slot >= 0 && slot < ss->cap, "cfm_session_fetch: bad argument");
  SessSlot& sl = ss->slots[slot];
  GSV_REQUIRE(sl.state == SLOT_DONE, "cfm_session_fetch: slot %d is %s", slot, sl.state == SLOT_LIVE ? "still live" : "free");
  const int md = c->cfg.mel_dim;
  GSV_LAUNCH(cfm_sess_out_kernel, cfm_grid((long long)ss->Tn * md), dim3(256), 0, (hipStream_t)stream,
             (const float*)(ss->xs + (size_t)slot * ss->Tn * md), sl.Tp, ss->Tn, md, out);
  sl = SessSlot{};
  return GSV_OK;
}

int gsv_cfm_session_fetch_mel(gsv_cfm_t* c, int n, const int32_t* slots, const int* col0, long long ld, float lo, float hi, float* out,
                              gsv_stream_t stream) {
  GSV_REQUIRE(session_open(c), "cfm_session_fetch_mel: no open session");
  CfmSession* ss = c->sess;
  GSV_REQUIRE(n >= 1 && n <= ss->cap, "cfm_session_fetch_mel: n = %d is outside [1, %d]", n, ss->cap);
  GSV_REQUIRE(slots && col0 && out, "cfm_session_fetch_mel: null argument");
  GSV_REQUIRE(std::isfinite(lo) && std::isfinite(hi), "cfm_session_fetch_mel: lo or hi is not finite");
  MelTab tab{};
  int max_len = 0;
  for (int i = 0; i < n; ++i) {
    GSV_REQUIRE(slots[i] >= 0 && slots[i] < ss->cap, "cfm_session_fetch_mel: entry %d: slot %d is outside [0, %d)", i, slots[i], ss->cap);
    const SessSlot& sl = ss->slots[slots[i]];
    GSV_REQUIRE(sl.state == SLOT_DONE, "cfm_session_fetch_mel: entry %d: slot %d is %s", i, slots[i], sl.state == SLOT_LIVE ? "still live" : "free");
    for (int a = 0; a < i; ++a) GSV_REQUIRE(slots[a] != slots[i], "cfm_session_fetch_mel: slot %d is given twice", slots[i]);
    const int len = ss->Tn - sl.Tp;
    GSV_REQUIRE(col0[i] >= 0 && (long long)col0[i] + len <= ld,
                "cfm_session_fetch_mel: entry %d: columns [%d, %d + %d) do not fit a row of %lld", i, col0[i], col0[i], len, ld);
    tab.slot[i] = slots[i]; tab.Tp[i] = sl.Tp; tab.col0[i] = col0[i];
    max_len = std::max(max_len, len);
  }
  // ---- nothing was launched or changed up to here
  const int md = c->cfg.mel_dim;
  if (max_len > 0)
    GSV_LAUNCH(cfm_sess_mel_kernel, dim3(nblk(max_len, kMelTile), nblk(md, kMelTile), n), dim3(256), 0, (hipStream_t)stream, tab,
               (const float*)ss->xs, ss->Tn, md, hi - lo, lo, out, ld);
  for (int i = 0; i < n; ++i) ss->slots[slots[i]] = SessSlot{};
  return GSV_OK;
}

int gsv_cfm_session_release(gsv_cfm_t* c, int n, const int32_t* slots) {
  GSV_REQUIRE(session_open(c), "cfm_session_release: no open session");
  CfmSession* ss = c->sess;
  GSV_REQUIRE(n >= 0 && (n == 0 || slots), "cfm_session_release: bad argument");
  for (int i = 0; i < n; ++i) GSV_REQUIRE(slots[i] >= 0 && slots[i] < ss->cap, "cfm_session_release: slot %d is outside [0, %d)", slots[i], ss->cap);
  for (int i = 0; i < n; ++i) {
    if (ss->slots[slots[i]].state == SLOT_LIVE) ss->dirty = true;
    ss->slots[slots[i]] = SessSlot{};
  }
  return GSV_OK;
}

int gsv_cfm_session_state(gsv_cfm_t* c, int32_t* state) {
  GSV_REQUIRE(session_open(c), "cfm_session_state: no open session");
  GSV_REQUIRE(state, "cfm_session_state: null argument");
  const CfmSession* ss = c->sess;
  for (int sl = 0; sl < ss->cap; ++sl) {
    state[sl] = ss->slots[sl].state;
    state[ss->cap + sl] = ss->slots[sl].step;
    state[2 * ss->cap + sl] = ss->slots[sl].n_steps;
  }
  return GSV_OK;
}

int gsv_cfm_session_end(gsv_cfm_t* c) {
  GSV_REQUIRE(session_open(c), "cfm_session_end: no open session");
  c->sess->open = false;
  c->sess->slots.clear();
  return GSV_OK;
}

}  // extern "C"
