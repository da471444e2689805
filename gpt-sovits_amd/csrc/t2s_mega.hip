// Persistent AR decode engine for gfx950: every step of a decode call (reference AR/models/t2s_model.py:694-769: the
// `for idx in range(1500)` loop of infer_panel_batch_infer, 24 x T2SBlock.decode_next_token :176-221, ar_predict_layer,
// sample :AR/models/utils.py:140-199, EOS / early-stop bookkeeping) runs inside ONE kernel launch.
//
// Why: as five launches per layer the step is a chain of 122 dependent kernels of 4.6-7 us that each move 0.5-18 MB
// (round 1: 0.67 ms per step at B = 32, 11 % of the HBM roofline); nothing in it is bandwidth-bound, every kernel spends
// its life ramping up and waiting for its first bytes.  Here the chain's hand-offs stay on the chip and the weights are
// already in registers when a hand-off completes.
//
// Decomposition (measured first with tools/mega_probe.hip, profiles/r02_mega_probe.txt):
//   * rows are independent, so the batch is split into 8 GROUPS of R = ceil(B/8) rows (row b -> group b % 8); a group
//     is served by 32 workgroups (one per CU, 512 threads) that never talk to another group: no grid-wide barrier.
//   * inside a group the layer is tensor-parallel over the 32 members: member j = (head j/2, row parity j%2) computes
//     q,k,v of its head for its rows, appends K/V, attends (all local), then the out-projection, FFN1 and FFN2 are
//     split over output columns (16 / 64 / 16 columns per member).  Between phases the members all-gather the small
//     activation vector (R x 512 fp32, R x 512 fp16, R x 2048 fp16): 4 hops per layer.
//   * a hop = 8-byte {tag = epoch, value} granules written with sc1 (write-through) stores and swept with sc1 loads
//     until every tag matches (MI355X_MICROARCH.md, visibility: R2 "the data is the flag"; no fence, no flag, placement
//     independent).  Every spin is bounded; a timeout sets an error word and every workgroup leaves.
//   * waves 0-3 of a workgroup ("comm") sweep hops into LDS and do the LayerNorms; waves 4-7 ("compute") hold the
//     member's weight slices in REGISTERS, prefetched one phase ahead with perfectly coalesced 1 KiB wave loads from a
//     copy of the weights packed in exactly that order, run the MFMAs (K split over the 4 waves in the same 128-wide
//     chunks and summation order as dec_gemm_kernel), reduce through LDS and publish.
//   * K/V of the member's (head, rows) is prefetched into LDS by LDS-DMA (non-temporal) one layer ahead.
//   * blockIdx -> (group, member): the 8 workgroups that read the SAME weight slice (one per group) are placed on the
//     same XCD (blockIdx % 8 under the observed round-robin placement), so a slice is filled into that L2 once and hit
//     seven times; the hops are sc1 and do not care.  Correctness never depends on the placement.
//   * logits are split over the members too; row r of a group is sampled by member r (one wave, sample_core of
//     t2s_sample.h), which also emits the next input embedding: the step's tail is two more hops.
//   * (round 3) more than 32 rows: a group serves up to four QUADS of rows, phase by phase one after the other with the weight
//     slices it already holds; the comm waves sweep quad i + 1 into a second copy of the operand image while the compute
//     waves work on quad i (comm_role_pipe / compute_role_pipe).  The step is latency-bound, so rows are added in
//     time, not in tile width: 128 rows cost 0.79 ms per step against 4 x 0.30.
//   * the arithmetic of a phase (sweep + LayerNorm, reduce, publish, ...) is written once, as a "phase body" shared by the
//     single-quad and the pipelined roles; the four role functions are the two synchronisation skeletons.
//   * weight slices are loaded with the DEFAULT cache policy (the 8 same-slice workgroups of an XCD share one L2 fill), K/V
//     non-temporal (read once per step; keeps the weights in the Infinity Cache).
#include <math.h>
#include "t2s_mega.h"

namespace gsv {

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned gu32;
typedef unsigned long long u64;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
// Workgroup barrier WITHOUT __syncthreads()'s release fence: that fence is an s_waitcnt vmcnt(0), which would drain the
// weight prefetch (issued one phase ahead on purpose) at every barrier -- tools/mega_probe.hip measured hops and weight
// stream adding up instead of overlapping with it.  LDS traffic of this wave is complete (lgkmcnt(0)) before the barrier;
// the "memory" clobber keeps the compiler from moving memory operations across it.
#define MG_BAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// The (sticky) abort flag is tested ONCE per layer: read at the top of the layer, acted on behind the layer's first barrier.
// Round 2 tested it behind every barrier -- 14 LDS round trips of ~100 cycles per layer on the critical path; read right in
// front of the barrier instead, the round trip delays the barrier arrival (measured: -1 % at 32 rows, +1.7 % at 128).  A wave
// that has failed has set the error word and returned (a finished wave no longer counts at s_barrier); its workgroup follows
// within a layer, the other workgroups through their bounded hop waits, and the launch is re-run from the snapshot.
#define MG_BAR_AL(q) do { MG_BAR(); if (ab_l) return; } while (0)

namespace {

constexpr int MG_GROUPS = 8, MG_MEMBERS = 32, MG_NWG = MG_GROUPS * MG_MEMBERS, MG_THREADS = 512;
constexpr int RMAX = 4;                       // rows of a group served together: one QUAD (B <= 32: the group's only quad)
constexpr int QMAX = 4;                       // quads per group (B <= 128): phase by phase one quad after the other, see t2s_mega_kernel
constexpr int D = 512, NH = 16, HD = 32, FF = 2048;
constexpr int XS_LD = 528, HS_LD = 2064;      // LDS row strides in halfs (rows 32 B apart mod 256 B: conflict-free b128 reads)
constexpr int KV_CAP = 320;                   // cached positions per own row held in the LDS image (rest: global loads)
constexpr int VPAD = 1088;                    // logits row stride in the hop buffer (17 x 64)
constexpr unsigned SPIN_MAX = 1u << 18;

// packed weight geometry (KiB-instructions per compute wave)
constexpr int WI_P1 = 24, WI_P2 = 4, WI_P3 = 16, WI_P4 = 16, WI_LG = 12;
constexpr size_t P1_HALFS = (size_t)NH * 4 * WI_P1 * 512;                       // per layer, by head
constexpr size_t PM_HALFS = (size_t)MG_MEMBERS * 4 * (WI_P2 + WI_P3 + WI_P4) * 512;  // per layer, by member
constexpr size_t LAYER_HALFS = P1_HALFS + PM_HALFS;
constexpr size_t LOGIT_HALFS = (size_t)MG_MEMBERS * 4 * WI_LG * 512;

// hop buffers of one group, in granules
constexpr int HOP_A = 0;                            // [RMAX][512] fp32 y  + RMAX state granules
constexpr int HOP_ST = RMAX * 512;
constexpr int HOP_B = HOP_ST + 64;                  // [RMAX][256] half pairs (attention output)
constexpr int HOP_C = HOP_B + RMAX * 256;           // [RMAX][512] fp32 y1
constexpr int HOP_D = HOP_C + RMAX * 512;           // [RMAX][1024] half pairs (FFN hidden)
constexpr int HOP_E = HOP_D + RMAX * 1024;          // [RMAX][VPAD] fp32 logits
constexpr int HOP_GROUP = HOP_E + RMAX * VPAD;     // one quad's buffers
constexpr int HOP_GROUP_ALL = QMAX * HOP_GROUP;    // a group's buffers: quad after quad

// LDS carve (bytes); everything dynamic so the base stays 16-byte aligned
constexpr int L_XRES = 0;                                     // fp32 [RMAX][512]   LayerNorm output (residual operand); one quad per group
constexpr int L_RS = 0;                                       // f4 [2][QMAX][64]   the same 8 KB in pipelined launches: residual operands parked per quad (rs_at)
constexpr int L_XS = L_XRES + RMAX * 512 * 4;                 // half [2][RMAX][XS_LD] LayerNorm output (MFMA operand); second copy: pipelined quads
constexpr int L_AT = L_XS + 2 * RMAX * XS_LD * 2;             // half [2][RMAX][XS_LD] attention output of all heads
constexpr int L_HS = L_AT + 2 * RMAX * XS_LD * 2;             // half [2][RMAX][HS_LD] FFN hidden
constexpr int L_RED = L_HS + 2 * RMAX * HS_LD * 2;            // f4 [24][16] split-K partials: the RMAX valid batch rows of each 16 x 16 tile
constexpr int L_QKV = L_RED + 24 * 16 * 16;                   // half [2][3][32] q,k,v of the own rows
constexpr int L_ATT = L_QKV + 2 * 3 * 32 * 2;                 // float [8] m + [8 waves][4 rows of 16 lanes][36] acc,l partials
constexpr int L_STAGE = L_ATT + 32 + 8 * 4 * 36 * 4;          // 4 x 1 KB: per-wave transposition buffers of the publishers
constexpr int L_ST = L_STAGE + 4 * 1024;                      // int: active[QMAX * RMAX], kvlen[..], step[..], abort, -, barrier counter, flag
constexpr int ST_N = QMAX * RMAX;                             // rows of a group
constexpr int L_SR = L_ST + (3 * ST_N + 16) * 4;              // int: prompt length P_b[ST_N], RNG key seed lo[..], seed hi[..], row[..]
constexpr int L_SEEN = L_SR + 4 * ST_N * 4;                   // bytes [VPAD]
constexpr int L_KV = (L_SEEN + VPAD + 63) & ~63;              // [2 rows][K|V][KV_CAP][64 B]
constexpr int L_TOTAL = L_KV + 2 * 2 * KV_CAP * 64;
static_assert(L_TOTAL <= 160 * 1024, "LDS budget");
static_assert(L_STAGE % 16 == 0 && L_XS % 16 == 0 && L_AT % 16 == 0 && L_HS % 16 == 0 && L_RED % 16 == 0 && L_QKV % 16 == 0 && L_KV % 16 == 0, "LDS alignment");

__device__ __forceinline__ void gstore(gu64* p, unsigned tag, unsigned val) {
  __hip_atomic_store(p, ((u64)tag << 32) | val, RLX_AGENT);           // global_store_dwordx2 ... sc1 (one untorn granule)
}
__device__ __forceinline__ u64 gload(gu64* p) { return __hip_atomic_load(p, RLX_AGENT); }   // global_load_dwordx2 ... sc1

// Cross-lane reductions on the VALU's data-parallel primitives (DPP) instead of __shfl_xor: hipcc lowers a shuffle to
// ds_bpermute_b32, an LDS-crossbar round trip of ~100 cycles, and the reductions here are dependent chains of 6 (wave sum /
// max) to 36 (attention) of them per layer.  quad_perm swaps inside quads, row_half_mirror / row_mirror fold 8 / 16 lanes
// (a sum or max does not care that a mirror is not an xor), the four 16-lane rows are folded through v_readlane.
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
constexpr int DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
__device__ __forceinline__ float rl_f(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v += dpp_f<DPP_QUAD_XOR1>(v);
  v += dpp_f<DPP_QUAD_XOR2>(v);
  v += dpp_f<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_f<DPP_ROW_MIRROR>(v);
  return (rl_f(v, 0) + rl_f(v, 16)) + (rl_f(v, 32) + rl_f(v, 48));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = fmaxf(v, dpp_f<DPP_QUAD_XOR1>(v));
  v = fmaxf(v, dpp_f<DPP_QUAD_XOR2>(v));
  v = fmaxf(v, dpp_f<DPP_ROW_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_f<DPP_ROW_MIRROR>(v));
  return fmaxf(fmaxf(rl_f(v, 0), rl_f(v, 16)), fmaxf(rl_f(v, 32), rl_f(v, 48)));
}

__device__ __forceinline__ unsigned pack_h2(float a, float b) {
  const h2 v = (h2){(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, v);
}

// LDS-DMA of one KiB (16 B per lane, lane i -> lds_dst + 16 i), non-temporal; invisible to the compiler's vmcnt
// bookkeeping (cdna_hip_programming.md 5.7): the consumer waits with asm vmcnt(0) + a workgroup barrier
__device__ __forceinline__ void glds16_nt(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// fp32 parameters of one layer in the packed buffer (MegaArgs::fpack): offsets in floats
constexpr int FP_QKVB = 0, FP_OUTB = 1536, FP_B1 = 2048, FP_B2 = 4096, FP_N1W = 4608, FP_N1B = 5120, FP_N2W = 5632, FP_N2B = 6144,
              FP_LAYER = 6656;

struct Ctx {
  unsigned char* smem;
  int lane, wave, cw, tid_c;
  bool comm;
  int group, member, head, half, R;   // R = rows of the CURRENT quad
  int qd, Rtot;                       // current quad; rows of the group (all quads)
  gu64* hop;                    // this group's hop buffers of the current (step, layer) ring slot
  gu64* hop_base;               // slot 0
  gu32* err;
  int hint_miss16;              // hint phase ends when at most this many 16ths of the polled lines are still missing
  int hint_pipe;                // two hint polls in flight (GSV_MEGA_HINT bit 4)
  int hint_spread;              // each member polls a different publisher's line
  unsigned long long* prof;     // this wave's 32 stamp slots or null
  bool prof_on;
};

// in-kernel stamp (measurement runs: GSV_MEGA_PROF=<file>): 100 MHz real-time counter at point i of the profiled layer
#define MG_STAMP(q, i) do { if ((q).prof_on && (q).lane == 0) (q).prof[i] = __builtin_amdgcn_s_memrealtime(); } while (0)

// The row state lives in LDS and is addressed through LDS-typed pointers: through a generic pointer the volatile abort flag
// became a FLAT load, and a flat load is waited for with vmcnt(0) -- which drained the whole weight prefetch after every
// barrier (seen in the ISA; the dynamic LDS segment starts at LDS address 0: there is no static LDS in this kernel).
typedef __attribute__((address_space(3))) int lds_int;
typedef volatile __attribute__((address_space(3))) int lds_vint;
// the accessors return the CURRENT quad's four entries (local row lr = 4 * quad + r)
__device__ __forceinline__ lds_int* st_active(const Ctx& c) { return (lds_int*)(unsigned)L_ST + RMAX * c.qd; }
__device__ __forceinline__ lds_int* st_kvlen(const Ctx& c) { return (lds_int*)(unsigned)L_ST + ST_N + RMAX * c.qd; }
__device__ __forceinline__ lds_int* st_step(const Ctx& c) { return (lds_int*)(unsigned)L_ST + 2 * ST_N + RMAX * c.qd; }
__device__ __forceinline__ lds_vint* st_abort(const Ctx&) { return (lds_vint*)(unsigned)L_ST + 3 * ST_N; }
__device__ __forceinline__ lds_int* st_cbar(const Ctx&) { return (lds_int*)(unsigned)L_ST + 3 * ST_N + 2; }
// the samplers' per-row constants of a call (read once at kernel start): P_b and the counter-RNG key (seed_b, row_b)
__device__ __forceinline__ lds_int* st_plen(const Ctx& c) { return (lds_int*)(unsigned)L_SR + RMAX * c.qd; }
__device__ __forceinline__ lds_int* st_seed_lo(const Ctx& c) { return (lds_int*)(unsigned)L_SR + ST_N + RMAX * c.qd; }
__device__ __forceinline__ lds_int* st_seed_hi(const Ctx& c) { return (lds_int*)(unsigned)L_SR + 2 * ST_N + RMAX * c.qd; }
__device__ __forceinline__ lds_int* st_krow(const Ctx& c) { return (lds_int*)(unsigned)L_SR + 3 * ST_N + RMAX * c.qd; }

// Barrier among the 4 compute waves only (an s_barrier would also wait for the comm waves, which are busy issuing the next
// layer's K/V loads during P1): an arrival counter in LDS; LDS operations of a wave complete in order, so the add is behind
// the wave's earlier LDS writes.  `gen` counts arrivals expected so far (same in every compute wave).
__device__ __noinline__ void mega_fail(gu32* err, int lane, unsigned epoch, unsigned code);
__device__ __forceinline__ bool compute_barrier(const Ctx& q, int& gen) {
  gen += 4;
  if (q.lane == 0) __hip_atomic_fetch_add(st_cbar(q), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  unsigned spins = 0;
  int ab = *st_abort(q);           // returned to the caller: read in front of the spin, not behind it
  while (*(lds_vint*)st_cbar(q) < gen && !(ab = *st_abort(q)) && ++spins < (1u << 24)) __builtin_amdgcn_s_sleep(0);
  // a wave that gives up must not go on to reduce partial sums another wave has not written: like every other bounded spin
  // of the engine it sets the abort flag and the error word (code 0x40), and the caller returns at its abort test
  if (spins >= (1u << 24)) { mega_fail(q.err, q.lane, (unsigned)gen, 0x40u); ab = 1; }
  asm volatile("" ::: "memory");
  return ab != 0;
}

// by value: a `const Ctx&` parameter of a non-inlined function forces the whole Ctx into scratch memory, re-stored at the
// start of every phase (30 scratch instructions in the hot loops, seen in the ISA)
__device__ __noinline__ void mega_fail(gu32* err, int lane, unsigned epoch, unsigned code) {
  lds_vint* ab = (lds_vint*)(unsigned)L_ST + 3 * ST_N;                  // st_abort
  const int was = *ab;
  *ab = 1;
  // the FIRST failure of a workgroup is the one reported: its waves run on to the end of the layer (abort is tested once per
  // layer), and every bounded wait they still meet gives up at once
  if (lane == 0 && !was) {
    __hip_atomic_store(err + 1, epoch, RLX_AGENT);
    __hip_atomic_store(err + 2, (unsigned)blockIdx.x, RLX_AGENT);
    __hip_atomic_store(err + 3, code, RLX_AGENT);
    __hip_atomic_store(err, 1u, RLX_AGENT);
  }
}

// one wave re-reads N granules per lane (granule k*64 + lane) of ONE or TWO rows (g1 may be null) until every tag equals `epoch`
template <int N>
__device__ __forceinline__ bool sweep2(const Ctx& c, gu64* g0, gu64* g1, int nvalid, unsigned epoch, unsigned (&v0)[N],
                                       unsigned (&v1)[N], unsigned code, bool hint = true) {
  // Every producer writes whole 128-B lines (16 granules) with one store instruction, so the LAST granule of each line is
  // polled first: one load per lane and row covers 64 lines, a 16th of a full pass.  When most lines are there the rows are
  // read in full -- and still checked tag by tag (the hint is an optimisation: the data remains its own flag).  Full-row
  // polling by 4 waves x 256 CUs was ~8 TB/s of fabric traffic by itself.
  if (hint) {
    const int nlines = (nvalid + 15) >> 4;
    constexpr int NP = (N + 15) / 16;                     // hint loads per lane and row (64 lines each)
    // Two polls are kept in flight, half a round trip apart: a poll costs ~1 us of sc1 latency, so one at a time notices an
    // arrival on average half a microsecond late; c.hint_pipe = 0 restores the single poll (A/B switch GSV_MEGA_HINT bit 4).
    u64 pa[2 * NP], pb[2 * NP];
    auto issue = [&](u64 (&h)[2 * NP]) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int ln = j * 64 + c.lane;
        const int i = min(min(ln, nlines - 1) * 16 + 15, nvalid - 1);
        h[2 * j] = gload(g0 + i);
        h[2 * j + 1] = g1 ? gload(g1 + i) : ((u64)epoch << 32);
      }
    };
    auto landed = [&](const u64 (&h)[2 * NP]) {
      int miss = 0;
#pragma unroll
      for (int j = 0; j < NP; ++j)
        miss += ((unsigned)(h[2 * j] >> 32) != epoch) + ((unsigned)(h[2 * j + 1] >> 32) != epoch);
      // most lines there: the stragglers are at most one poll away, go on with full passes (one round trip fewer at the end)
      return __popcll(__ballot(miss != 0)) * 16 <= nlines * c.hint_miss16;
    };
    issue(pa);
    if (c.hint_pipe) __builtin_amdgcn_s_sleep(16);        // ~0.4 us: half a poll round trip
    for (unsigned spins = 0;; spins += 2) {
      if (c.hint_pipe) {
        issue(pb);
        if (landed(pa)) break;
        issue(pa);
        if (landed(pb)) break;
      } else {
        if (landed(pa)) break;
        if (spins < 16) __builtin_amdgcn_s_sleep(1); else __builtin_amdgcn_s_sleep(4);
        issue(pa);
      }
      if (spins > SPIN_MAX || *st_abort(c) || (spins & 1022u) == 1022u && __hip_atomic_load(c.err, RLX_AGENT) != 0u) {
        mega_fail(c.err, c.lane, epoch, code | 0x100u);
        return false;
      }
    }
  }
  for (unsigned spins = 0;; ++spins) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int i = k * 64 + c.lane;
      v0[k] = 0u; v1[k] = 0u;
      if (i < nvalid) {
        const u64 x = gload(g0 + i);
        v0[k] = (unsigned)x;
        ok &= (unsigned)(x >> 32) == epoch;
        if (g1) {
          const u64 y = gload(g1 + i);
          v1[k] = (unsigned)y;
          ok &= (unsigned)(y >> 32) == epoch;
        }
      }
    }
    if (__all(ok)) return true;
    if (spins > SPIN_MAX || *st_abort(c) || (spins & 1023u) == 1023u && __hip_atomic_load(c.err, RLX_AGENT) != 0u) {
      mega_fail(c.err, c.lane, epoch, code);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

template <int N>
__device__ __forceinline__ bool sweep(const Ctx& c, gu64* g, int nvalid, unsigned epoch, unsigned (&v)[N], unsigned code,
                                      bool hint = true) {
  unsigned dummy[N];
  return sweep2<N>(c, g, nullptr, nvalid, epoch, v, dummy, code, hint);
}

// A row's payload is read with 16-BYTE loads: NQ requests per lane instead of 2 NQ.  Lane m,
// piece j holds granules j * 128 + 2 m and + 1 (dwords: value, tag, value, tag); each 8-byte half is still one untorn granule
// with its own tag.  Measured on hop D alone (8 KB per row): 569 -> 514 us per step -- the sc1 path is bound by REQUESTS, an
// 8-byte-per-lane load moves 512 B per wave instruction.  The loads and their wait are ONE asm statement (the compiler never
// sees a half-loaded register); it waits for everything the wave has in flight, which at a hop is nothing else.
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
template <int NQ> __device__ __forceinline__ void wide_loads(const gu64* p0, u4v (&q)[NQ]);
template <> __device__ __forceinline__ void wide_loads<2>(const gu64* p0, u4v (&q)[2]) {
  asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:1024 sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(q[0]), "=&v"(q[1]) : "v"(p0) : "memory");
}
template <> __device__ __forceinline__ void wide_loads<4>(const gu64* p0, u4v (&q)[4]) {
  asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %4, off offset:1024 sc1\n\t"
               "global_load_dwordx4 %2, %4, off offset:2048 sc1\n\tglobal_load_dwordx4 %3, %4, off offset:3072 sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3]) : "v"(p0) : "memory");
}
template <> __device__ __forceinline__ void wide_loads<8>(const gu64* p0, u4v (&q)[8]) {
  const gu64* p1 = p0 + 512;
  asm volatile("global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %8, off offset:1024 sc1\n\t"
               "global_load_dwordx4 %2, %8, off offset:2048 sc1\n\tglobal_load_dwordx4 %3, %8, off offset:3072 sc1\n\t"
               "global_load_dwordx4 %4, %9, off sc1\n\tglobal_load_dwordx4 %5, %9, off offset:1024 sc1\n\t"
               "global_load_dwordx4 %6, %9, off offset:2048 sc1\n\tglobal_load_dwordx4 %7, %9, off offset:3072 sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3]), "=&v"(q[4]), "=&v"(q[5]), "=&v"(q[6]), "=&v"(q[7])
               : "v"(p0), "v"(p1) : "memory");
}
// The hint line of a member (GSV_MEGA_HINT bit 7, the default): the last line of publisher (member + 16) % 32 -- ANOTHER
// member's line, and a different one for every member of the group.  With every member polling the same line (round 2: the
// last line of the row) 32 workgroups re-read one address while its publisher was trying to write it: 297 -> 288 us per step
// when the polls are spread; two or four lines per member, polls in flight, slower paces all lose (profiles/r03_ab_hint_spread.txt).
#ifndef GSV_HINT_OFFSET
#define GSV_HINT_OFFSET 16          // whose line a member polls: member + this.  A publisher on ANOTHER XCD (members 4 x .. 4 x + 3 run
                                    // on XCD x): +1 / -1 cost 8 %, +4 / +8 / +16 are equal (profiles/r03_ab_hint_spread.txt, 11.)
#endif
template <int NLINES>
__device__ __forceinline__ int hint_line(const Ctx& c) {
  return ((c.member + GSV_HINT_OFFSET) & 31) * NLINES / 32 + (NLINES >= 64 ? 1 : 0);
}
// pauses (s_sleep units of 64 clocks) between hint polls and between full passes of sweep_wide (compile-time: A/B by library)
#ifndef GSV_HINT_SLEEP
#define GSV_HINT_SLEEP 1
#endif
#ifndef GSV_PASS_SLEEP
#define GSV_PASS_SLEEP 2
#endif
// one wave, one row of NQ * 128 granules
template <int NQ>
__device__ __forceinline__ bool sweep_wide(const Ctx& c, gu64* g, unsigned epoch, u4v (&q)[NQ], unsigned code, bool hint) {
  constexpr int NLINES = NQ * 8;                       // 16 granules per 128-byte line
  if (hint) {
    // ONE line per row is polled before the full pass (round 2 found every extra poll to cost: every 2nd, 4th, ... line, two
    // polls in flight, one polling wave per workgroup were all measured and are gone from this loop)
    const int ln = c.hint_spread ? hint_line<NLINES>(c) : NLINES - 1;
    gu64* hp = g + ln * 16 + 15;
    for (unsigned spins = 0;; ++spins) {
      if ((unsigned)__builtin_amdgcn_readfirstlane((int)(gload(hp) >> 32)) == epoch) break;     // one address for the wave
      if (spins > SPIN_MAX || *st_abort(c) || (spins & 1023u) == 1023u && __hip_atomic_load(c.err, RLX_AGENT) != 0u) {
        mega_fail(c.err, c.lane, epoch, code | 0x100u);
        return false;
      }
      if (spins < 8) __builtin_amdgcn_s_sleep(GSV_HINT_SLEEP); else __builtin_amdgcn_s_sleep(4);
    }
  }
  const gu64* p0 = g + 2 * c.lane;
  for (unsigned spins = 0;; ++spins) {
    wide_loads<NQ>(p0, q);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NQ; ++j) ok &= q[j][1] == epoch && q[j][3] == epoch;
    if (__all(ok)) return true;
    if (spins > SPIN_MAX || *st_abort(c) || (spins & 1023u) == 1023u && __hip_atomic_load(c.err, RLX_AGENT) != 0u) {
      mega_fail(c.err, c.lane, epoch, code);
      return false;
    }
    __builtin_amdgcn_s_sleep(GSV_PASS_SLEEP);
  }
}

// LayerNorm of one row delivered by sweep_wide<4>: lane m holds elements j * 128 + 2 m + {0, 1}; gm / bt in the same order;
// norm == false: identity (layer 0's input is the embedding itself).  The row goes to XS copy `copy` as the MFMA operand;
// what becomes of the fp32 values x (the residual operand) is the caller's: ln_row_wide, ln_row_pipe.
__device__ __forceinline__ void ln_core(const Ctx& c, int row, int copy, const u4v (&v)[4], bool norm, const float (&gm)[8], const float (&bt)[8], float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { x[2 * j] = __uint_as_float(v[j][0]); x[2 * j + 1] = __uint_as_float(v[j][2]); }
  if (norm) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += x[k];
    const float mean = wave_sum_dpp(s) * (1.f / D);
    float qq = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { const float dl = x[k] - mean; qq += dl * dl; }
    const float rstd = rsqrtf(wave_sum_dpp(qq) * (1.f / D) + 1e-5f);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (x[k] - mean) * rstd * gm[k] + bt[k];
  }
  _Float16* xs = (_Float16*)(c.smem + L_XS) + (copy * RMAX + row) * XS_LD + 2 * c.lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) *(h2*)(xs + j * 128) = (h2){(_Float16)x[2 * j], (_Float16)x[2 * j + 1]};
}

// single quad: XS copy 0, and the whole fp32 row -> XRES (the reducing waves read their residual columns from it)
__device__ __forceinline__ void ln_row_wide(const Ctx& c, int row, const u4v (&v)[4], bool norm, const float (&gm)[8], const float (&bt)[8]) {
  float x[8];
  ln_core(c, row, 0, v, norm, gm, bt, x);
  float* xr = (float*)(c.smem + L_XRES) + row * D + 2 * c.lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) *(f2*)(xr + j * 128) = (f2){x[2 * j], x[2 * j + 1]};
}

// pipelined quads: XS copy `buf`; XRES would be overwritten by the next quad's LayerNorm before the phase that needs it comes
// round, so only the member's 16 residual columns of the row are kept, parked per quad in rs[which][qd] (which = 0: operand of
// the out-projection, 1: of FFN2; f4 per lane of the reducing wave, 1 KB per quad)
__device__ __forceinline__ f4* rs_at(unsigned char* smem, int which, int qd, int lane) { return (f4*)(smem + L_RS) + (which * QMAX + qd) * 64 + lane; }
__device__ __forceinline__ void ln_row_pipe(const Ctx& c, int row, int buf, int which, const u4v (&v)[4], bool norm, const float (&gm)[8], const float (&bt)[8]) {
  float x[8];
  ln_core(c, row, buf, v, norm, gm, bt, x);
  // columns [16 member, +16) of this row: chunk j = member / 8, lanes 8 (member % 8) .. + 7, two elements each; the reducing
  // wave's lane r + 16 g holds columns 4 g .. 4 g + 3 of row r
  const int jm = c.member >> 3, m0 = 8 * (c.member & 7), dm = c.lane - m0;
  const float e0 = jm == 0 ? x[0] : jm == 1 ? x[2] : jm == 2 ? x[4] : x[6];
  const float e1 = jm == 0 ? x[1] : jm == 1 ? x[3] : jm == 2 ? x[5] : x[7];
  if (dm >= 0 && dm < 8)
    *(f2*)((float*)rs_at(c.smem, which, c.qd, row + 16 * (dm >> 1)) + 2 * (dm & 1)) = (f2){e0, e1};
}

// compute waves: NT tiles x 4 k-steps of this wave's 128-wide K chunk `kc` against the activation image `act`
// (half [RMAX][ld]); partial tiles go to red[(slot0 + t)][lane]
// a parked tile: lanes with (lane & 15) < RMAX, i.e. 4 row-lanes x 4 column groups = 16 f4 per tile
__device__ __forceinline__ int red_idx(int slot, int lane) { return slot * 16 + (lane >> 4) * 4 + (lane & 15); }

template <int NT>
__device__ __forceinline__ void gemm_chunk(const Ctx& c, const h8 (&w)[NT * 4], const _Float16* act, int ld, int kc, int slot0) {
  const int rowl = c.lane & 15, kg = c.lane >> 4;
  const _Float16* bp = act + (rowl & (RMAX - 1)) * ld + kc * 128 + 8 * kg;
  h8 b[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) b[ks] = *(const h8*)(bp + 32 * ks);
  f4* red = (f4*)(c.smem + L_RED);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[t * 4 + ks], b[ks], acc, 0, 0, 0);
    if (rowl < RMAX) red[red_idx(slot0 + t, c.lane)] = acc;     // only the tile's first RMAX batch rows hold rows of the quad
  }
}

// ONE 16-column tile over the whole K = 512 by one wave: FFN1's four tiles are split over the compute waves by COLUMN, so
// no partial sums meet in LDS (the split-K form cost a barrier + an LDS round trip + two idle waves per layer).  Four chains,
// one per 128-wide K chunk, summed ((c0 + c1) + c2) + c3: the order of the split-K reduce this replaces, bit for bit.  The
// operand fragments of k-step ks + 1 are in flight under the four MFMAs of k-step ks.
__device__ __forceinline__ f4 gemm_tile_k512(const Ctx& c, const h8 (&w)[16], const _Float16* act, int ld) {
  const int rowl = c.lane & 15, kg = c.lane >> 4;
  const _Float16* bp = act + (rowl & (RMAX - 1)) * ld + 8 * kg;
  f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f4){0.f, 0.f, 0.f, 0.f};
  h8 bA[4], bB[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bA[j] = *(const h8*)(bp + 128 * j);
#pragma unroll
  for (int ks = 0; ks < 4; ks += 2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) bB[j] = *(const h8*)(bp + 128 * j + 32 * (ks + 1));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[4 * j + ks], bA[j], acc[j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + 2 < 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bA[j] = *(const h8*)(bp + 128 * j + 32 * (ks + 2));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[4 * j + ks + 1], bB[j], acc[j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  f4 v = acc[0];
  v += acc[1]; v += acc[2]; v += acc[3];
  return v;
}

template <int N>
__device__ __forceinline__ void wload(h8 (&dst)[N], const h8* src) {
#pragma unroll
  // DEFAULT cache policy, not non-temporal: the 8 workgroups of an XCD that stream the same slice (one per row group) then
  // share one fill of the XCD's L2; with `nt` loads the line was kept only when the eight requests happened to arrive close
  // together -- that was the two run-to-run modes (~319 / ~343 us per step), and the memory-side traffic swinging between
  // 1.28 and 1.79 x the algorithmic bytes.  Measured, 5 alternating pairs: 334-345 -> 301-303 us per step at B = 32,
  // 838 -> 790 at B = 128 (-DGSV_MEGA_W_NT restores the non-temporal loads).
#ifdef GSV_MEGA_W_NT
  for (int i = 0; i < N; ++i) dst[i] = __builtin_nontemporal_load(src + (size_t)i * 64);
#else
  for (int i = 0; i < N; ++i) dst[i] = src[(size_t)i * 64];
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// The two roles are separate functions: a weight array defined under `if (!comm)` inside one body would have to keep
// its old value alive around the whole loop for the other role's lanes, i.e. all 240 weight registers live everywhere.
// Both roles execute the same sequence of workgroup barriers and take the same (LDS-uniform) exit decisions.
// ---------------------------------------------------------------------------------------------------------------
// Make the role's indices opaque to the optimiser at the start of every phase.  Without this, loop-invariant code motion
// hoists every per-lane address (weight, bias, hop, LDS pointers of all phases) out of the step and layer loops and keeps
// ~100 of them alive across the whole body: VGPR / SGPR spills in the critical path.  Recomputing an address is 2-3 ALU ops.
__device__ __forceinline__ void relaunder(Ctx& q) {
  int cw = __builtin_amdgcn_readfirstlane(q.cw), member = __builtin_amdgcn_readfirstlane(q.member),
      group = __builtin_amdgcn_readfirstlane(q.group);
  asm volatile("" : "+v"(q.lane), "+s"(cw), "+s"(member), "+s"(group));
  q.cw = cw; q.member = member; q.group = group; q.head = member >> 1; q.half = member & 1;
  q.tid_c = q.cw * 64 + q.lane;
}

// ONE set of hop buffers: the epoch in every granule tells (step, layer) apart.  Round 2 tried a ring of 16 sets used
// round-robin over the layers, so that the payload could be read with plain loads that allocate in L2 (the 4 members of a group
// on one XCD would fetch a line from the memory side once instead of four times).  MEASURED on MI355X: 16 sets alone cost 4 %
// (the one 0.9 MB set stays resident on the memory side, 14 MB of rotating lines do not), the L2-shared read gained nothing on
// top, and the run-time modulo this function then needed in every phase cost more; the option is gone (round 3).
__device__ __forceinline__ gu64* hop_slot(const Ctx& c, int s, int l) {
  (void)s; (void)l;
  return c.hop_base + (size_t)c.qd * HOP_GROUP;
}

__device__ __forceinline__ bool group_done(const Ctx& c) {
  int any = 0;
  for (int r = 0; r < c.Rtot; ++r) any |= ((lds_int*)(unsigned)L_ST)[r];      // every quad's rows
  return !any;
}
// make quad `qd` the current one: its rows, its state entries (through c.qd), and -- via hop_slot -- its hop buffers
__device__ __forceinline__ void set_quad(Ctx& c, int qd) {
  c.qd = __builtin_amdgcn_readfirstlane(qd);
  c.R = __builtin_amdgcn_readfirstlane(min(RMAX, c.Rtot - RMAX * qd));
}
// batch row of the current quad's local row r
__device__ __forceinline__ int batch_row(const Ctx& c, int r) { return c.group + MG_GROUPS * (RMAX * c.qd + r); }

// Attention of the member's own rows (H4: softmax(q K^T / sqrt(32)) V over the cached keys + this step's key): row ro is
// served by NW waves, its keys dealt to them in 16-key groups, 4 lanes per key (8 dims each).  Two passes over the
// LDS image (scores -> lane maximum -> weights), so there is no per-key rescaling; v_dot2_f32_f16 for q . k.
template <int NW>     // waves per row; aw = ro * NW + hq
__device__ __forceinline__ void attention_part(const MegaArgs& a, const Ctx& q, int l, int aw) {
  unsigned char* smem = q.smem;
  const int ro = aw / NW, hq = aw % NW, r = 2 * ro + q.half;
  const bool rv = r < q.R && st_active(q)[r];
  const int n_old = rv ? st_kvlen(q)[r] : 0;
  const int part = q.lane & 3, slot = q.lane >> 2;
  const float scale = 0.17677669529663687f;            // 1 / sqrt(32)
  const _Float16* qkv_s = (const _Float16*)(smem + L_QKV) + ro * 3 * HD;
  typedef _Float16 h2v __attribute__((ext_vector_type(2)));
  const h8 qv = *(const h8*)(qkv_s + part * 8);
  auto score = [&](const h8& kk) {
    float sc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sc = __builtin_amdgcn_fdot2((h2v){qv[2 * i], qv[2 * i + 1]}, (h2v){kk[2 * i], kk[2 * i + 1]}, sc, false);
    sc += dpp_f<DPP_QUAD_XOR1>(sc);            // the 4 lanes of a key are one quad
    sc += dpp_f<DPP_QUAD_XOR2>(sc);
    return sc * scale;
  };
  const unsigned char* kimg = smem + L_KV + (ro * 2 + 0) * KV_CAP * 64;
  const unsigned char* vimg = smem + L_KV + (ro * 2 + 1) * KV_CAP * 64;
  const int n_img = min(n_old, KV_CAP);
  constexpr int NT = KV_CAP / (16 * NW);               // image keys per lane
  // All 2 NT LDS reads are issued before the first use: taken one at a time (what the compiler emits when loads and uses
  // alternate) each costs a full LDS round trip, 2 NT + 2 of them in a row were ~2.5 us of the layer (in-kernel stamps).
  h8 kk[NT], vv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) kk[t] = *(const h8*)(kimg + ((NW * t + hq) * 16 + slot) * 64 + part * 16);
#pragma unroll
  for (int t = 0; t < NT; ++t) vv[t] = *(const h8*)(vimg + ((NW * t + hq) * 16 + slot) * 64 + part * 16);
  const h8 k_own = *(const h8*)(qkv_s + HD + part * 8), v_own = *(const h8*)(qkv_s + 2 * HD + part * 8);
  asm volatile("" ::: "memory");                       // keep the reads above the arithmetic
  float sc[NT + 1];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = (NW * t + hq) * 16 + slot;
    const float v = score(kk[t]);
    sc[t] = j < n_img ? v : -INFINITY;
    m = fmaxf(m, sc[t]);
  }
  {                                                    // this step's own key: wave hq == 0, key slot 0
    const float v = score(k_own);
    sc[NT] = (rv && hq == 0 && slot == 0) ? v : -INFINITY;
    m = fmaxf(m, sc[NT]);
  }
  // branch-free second pass: a masked key has p = exp(-inf) = 0 and its V is finite (the LDS image is zeroed at kernel start,
  // the K/V arena at creation: unwritten positions hold zeros or stale finite values), so 0 * V adds nothing
  const float mz = m == -INFINITY ? 0.f : m;
  float lsum = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
  for (int t = 0; t <= NT; ++t) {
    const h8 v8 = t < NT ? vv[t < NT ? t : 0] : v_own;
    const float p = __expf(sc[t] - mz);
    lsum += p;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += p * (float)v8[i];
  }
  if (n_old > KV_CAP) {                                // long rows: the tail comes straight from HBM (online update)
    const _Float16* kvb = a.kv + ((size_t)batch_row(q, r) * NH + q.head) * (size_t)a.smax * HD + part * 8;
    const _Float16* kg_ = kvb + (size_t)(l * 2 + 0) * a.kv_layer_stride;
    const _Float16* vg_ = kvb + (size_t)(l * 2 + 1) * a.kv_layer_stride;
    for (int j0 = KV_CAP + hq * 16; j0 < n_old; j0 += 16 * NW) {
      const int j = j0 + slot, jc = min(j, n_old - 1);
      const h8 kk = __builtin_nontemporal_load((const h8*)(kg_ + (size_t)jc * HD));
      const h8 vv = __builtin_nontemporal_load((const h8*)(vg_ + (size_t)jc * HD));
      const float v = score(kk);
      if (j < n_old) {
        const float mn = fmaxf(m, v);
        const float corr = m == -INFINITY ? 0.f : __expf(m - mn), p = __expf(v - mn);
        lsum = lsum * corr + p;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = acc[i] * corr + p * (float)vv[i];
        m = mn;
      }
    }
  }
  const float wm = wave_max_dpp(m);
  const float f = (m == -INFINITY) ? 0.f : __expf(m - wm);
  lsum *= f;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] *= f;
  // sum over the 4 key slots of each 16-lane row (lanes of equal `part`): two row shifts, lanes 12..15 hold the row's totals;
  // the 4 rows (and the row's other waves) are added by the combine step from LDS
  lsum += dpp_f<DPP_ROW_SHR4>(lsum);
  lsum += dpp_f<DPP_ROW_SHR8>(lsum);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc[i] += dpp_f<DPP_ROW_SHR4>(acc[i]);
    acc[i] += dpp_f<DPP_ROW_SHR8>(acc[i]);
  }
  float* s_m = (float*)(smem + L_ATT);
  float* s_acc = s_m + 8;                              // [aw][row][36]
  if ((q.lane & 15) >= 12) {
    const int row = q.lane >> 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) s_acc[(aw * 4 + row) * 36 + part * 8 + i] = acc[i];
    if (part == 0) s_acc[(aw * 4 + row) * 36 + 32] = lsum;
  }
  if (q.lane == 0) s_m[aw] = wm;
}

// K/V image staging by the comm waves: the cached K and V of the member's own rows for the NEXT layer go global -> registers
// (non-temporal 16-B lane loads = 1 KiB per wave instruction) and registers -> LDS after the current layer's attention has
// released the image.  A CU's vector-memory pipeline returns data in issue order ACROSS waves, so while long HBM loads are
// outstanding every poll of a hop waits behind them (measured: +2 us per hop with the loads in dedicated waves a layer ahead,
// 2.6 us of blocked issue per third of the image as LDS-DMA of the compute waves).  Therefore the loads are issued at B1 of
// P1 -- the start of the only poll-free stretch of a layer (QKV GEMM, reduce, attention: ~3 us; hop B cannot complete before
// the attention has finished anyway) -- by the comm waves, which have nothing else to do there and skip P1's inner barriers.
// KiB slot t of wave cw: row t / 10, K|V (t / 5) & 1, KiB 4 (t % 5) + cw.
constexpr int KV_T = KV_CAP / 16;            // KiB-instructions per (row, K|V) image = slots per wave (20)
struct KvStage { h8 r[KV_T]; };

// The row state is read ONCE per call: as written first, every one of the 20 loads sat behind two dependent LDS reads (active,
// kv_len), a readfirstlane and ~40 scalar address instructions -- the ISA showed the "burst" trickling out over ~3.5 us.
struct KvRows { int nki[2]; };
__device__ __forceinline__ KvRows kv_rows(const Ctx& q, int qd, int extra) {     // of quad qd (the one the image is staged for)
  KvRows k;
  const int Rq = min(RMAX, q.Rtot - RMAX * qd);
#pragma unroll
  for (int ro = 0; ro < 2; ++ro) {
    const int r = 2 * ro + q.half;                   // < RMAX
    const int act = ((lds_int*)(unsigned)L_ST)[RMAX * qd + r], len = ((lds_int*)(unsigned)L_ST + ST_N)[RMAX * qd + r];
    k.nki[ro] = __builtin_amdgcn_readfirstlane(r < Rq && act ? (min(len + extra, KV_CAP) + 15) >> 4 : 0);
  }
  return k;
}

__device__ __forceinline__ void kv_stage_load(const MegaArgs& a, const Ctx& q, int layer, int qd, int extra, KvStage& st) {
  const KvRows k = kv_rows(q, qd, extra);
  const h8* base[2][2];
#pragma unroll
  for (int ro = 0; ro < 2; ++ro)
#pragma unroll
    for (int which = 0; which < 2; ++which)
      // the arena is allocated to smax positions per (row, head): a partly valid KiB reads allocated memory
      base[ro][which] = (const h8*)(a.kv + (size_t)(layer * 2 + which) * a.kv_layer_stride +
                                    ((size_t)(q.group + MG_GROUPS * (RMAX * qd + 2 * ro + q.half)) * NH + q.head) * (size_t)a.smax * HD) + q.lane;
#pragma unroll
  for (int t = 0; t < KV_T; ++t) {
    const int ro = t / (KV_T / 2), which = (t / (KV_T / 4)) & 1, i = 4 * (t % (KV_T / 4)) + q.cw;
    if (i < k.nki[ro]) st.r[t] = __builtin_nontemporal_load(base[ro][which] + (size_t)i * (16 * HD / 8));
  }
}

__device__ __forceinline__ void kv_stage_store(const Ctx& q, int qd, int extra, const KvStage& st) {
  const KvRows k = kv_rows(q, qd, extra);
#pragma unroll
  for (int t = 0; t < KV_T; ++t) {
    const int ro = t / (KV_T / 2), which = (t / (KV_T / 4)) & 1, i = 4 * (t % (KV_T / 4)) + q.cw;
    if (i < k.nki[ro]) *((h8*)(q.smem + L_KV + (ro * 2 + which) * KV_CAP * 64 + i * 1024) + q.lane) = st.r[t];
  }
}

// sampling of the group's local row `member` by wave 0 of that member (reference utils.py:140-199, t2s_model.py:706-769): after the
// logits of every quad have been published, so that the samplers of all quads work side by side.  A MACRO, not a function: as an
// (inlined) function taking the context by reference the same text cost > 1000 spilled VGPRs in every kernel variant.
// Expects a, q, sp, s, ep0, EPS, seen in scope.
// LOGP (a compile-time constant): the taken token's log-probability goes to sp.logp (gsv_t2s_set_logprobs), computed from
// the raw logits this lane has just stored to logits_out and reads back -- taken from lv[] they stay live across sample_core
// next to its own 17 registers: ~400 spilled VGPRs.  As a run-time branch on the pointer alone even the read-back form costs
// the kernels that never take it 13 VGPRs and 80 bytes of scratch per lane, so those carry no trace of it and
// launch_t2s_mega picks a LOGP kernel only when the pointer is set (DESIGN.md section 4p has the table).
// The row's sampling values and its EOS horizon, early stop and budget come from sp.row_sampling[b] / sp.row_limits[b], one
// 16-byte load each per sampled step: the host fills both for every row (decode_begin, the sessions' admissions).
#define MG_RUN_SAMPLER(LOGP) do { \
  const int V = a.V, EOS = a.V - 1; \
  const unsigned epE = ep0 + 4 * a.L + 2; \
    relaunder(q); \
    set_quad(q, q.member / RMAX); \
    q.hop = hop_slot(q, s, a.L); \
    const int r = q.member % RMAX, b = batch_row(q, r); \
    const unsigned epN = ep0 + (unsigned)EPS + 1; \
    const int was_active = st_active(q)[r]; \
    int now_active = 0; \
    float x0[8]; \
  _Pragma("unroll") \
    for (int k = 0; k < 8; ++k) x0[k] = 0.f; \
 \
 \
    unsigned lv[17]; \
    const bool ok = sweep<17>(q, q.hop + HOP_E + r * VPAD, V, epE, lv, 7u); \
    if (was_active && ok) { \
      const int step = st_step(q)[r]; \
      const RowLimits rl = load_row_limits(sp.row_limits, b); \
      const int Veff = step < rl.eos_mask_steps ? V - 1 : V; \
      const RowSampling rs = load_row_sampling(sp.row_sampling, b); \
      float x[17]; \
  _Pragma("unroll") \
      for (int i = 0; i < 17; ++i) { \
        const int v = q.lane + 64 * i; \
        if (v < V) a.logits_out[(size_t)b * V + v] = __uint_as_float(lv[i]); \
        x[i] = v < Veff ? __uint_as_float(lv[i]) : -INFINITY; \
        if (rs.rep_penalty != 1.0f && v < Veff && seen[v]) x[i] = x[i] < 0.f ? x[i] * rs.rep_penalty : x[i] / rs.rep_penalty; \
      } \
      const float* nrow = nullptr; \
      if (sp.noise) nrow = sp.noise + ((size_t)step * sp.noise_rows + (sp.noise_rows > 1 ? b : 0)) * V; \
      int smp, amx; \
      const unsigned long long seed_b = ((unsigned long long)(unsigned)st_seed_hi(q)[r] << 32) | (unsigned)st_seed_lo(q)[r]; \
      sample_core<17>(x, Veff, rs.top_k, rs.top_p, rs.temperature, nrow, seed_b, st_krow(q)[r], step, &smp, &amx); \
      if (sp.dump) { \
  _Pragma("unroll") \
        for (int i = 0; i < 17; ++i) { \
          const int v = q.lane + 64 * i; \
          if (v < V) sp.dump[((size_t)step * a.B + b) * V + v] = __uint_as_float(lv[i]); \
        } \
      } \
      if (sp.drawn && q.lane == 0) { int* dr = sp.drawn + ((size_t)step * a.B + b) * 2; dr[0] = smp; dr[1] = amx; } \
      if (sp.force) { smp = sp.force[(size_t)b * sp.max_steps + step]; amx = smp; } \
      if constexpr (LOGP) if (sp.logp) { \
        float xr[17]; \
  _Pragma("unroll") \
        for (int i = 0; i < 17; ++i) { \
          const int v = q.lane + 64 * i; \
          xr[i] = v < Veff ? a.logits_out[(size_t)b * V + v] : -INFINITY;   /* this lane's own stores above: the raw logits */ \
        } \
        const float lpv = token_logprob<17>(xr, Veff, smp); \
        if (q.lane == 0) sp.logp[(size_t)b * sp.max_steps + step] = lpv; \
      } \
      const bool fin = smp == EOS || amx == EOS; \
      const bool early = (rl.early_stop_num != -1 && (step + 1) > rl.early_stop_num) || step >= rl.max_steps - 1; \
      const int P_b = st_plen(q)[r]; \
      const int prev_len = P_b + step; \
      if (q.lane == 0) { \
        if (prev_len < a.ycap) a.ytok[(size_t)b * a.ycap + prev_len] = smp; \
        if (smp >= 0 && smp < VPAD) seen[smp] = 1; \
        if (fin || early) { \
          a.active[b] = 0; \
          sp.out_len[b] = step; \
          atomicSub(a.n_active, 1); \
        } else { \
          sp.out_tokens[(size_t)b * sp.max_steps + step] = smp; \
          a.kv_len[b] = st_kvlen(q)[r] + 1; \
        } \
        a.step_ctr[b] = step + 1; \
      } \
      if (!(fin || early)) { \
        now_active = 1; \
        const int tok = min(max(smp, 0), V - 1); \
        const float* e = a.e_audio + (size_t)tok * D; \
        const float* p = a.pe + (size_t)(P_b + step) * D; \
  _Pragma("unroll") \
        for (int k = 0; k < 8; ++k) x0[k] = e[k * 64 + q.lane] + a.alpha_a * p[k * 64 + q.lane]; \
      } \
    } \
    if (ok && s + 1 < a.nsteps) { \
      gu64* hn = hop_slot(q, s + 1, 0); \
  _Pragma("unroll") \
      for (int k = 0; k < 8; ++k) gstore(hn + HOP_A + r * 512 + k * 64 + q.lane, epN, __float_as_uint(x0[k])); \
      if (q.lane == 0) gstore(hn + HOP_ST + r, epN, (unsigned)now_active); \
    } \
} while (0)

// ---------------------------------------------------------------------------------------------------------------
// Phase bodies.  Each is written ONCE and used by the single-quad roles (comm_role / compute_role) and by the pipelined
// ones (comm_role_pipe / compute_role_pipe).  What differs between the two is a parameter: the copy of the operand image,
// the residual operand (read from XRES by the single quad, parked per quad by the pipelined LayerNorm), the hop buffers of
// the quad.  The roles below hold only the synchronisation skeleton: barriers, weight requests, hop epochs.
// Form: the bodies take their few scalars and pointers BY VALUE (the sampler as a function taking the context by
// reference cost > 1000 spilled VGPRs, see MG_RUN_SAMPLER) and weight arrays as array references, like gemm_chunk.
// ---------------------------------------------------------------------------------------------------------------
// copy `copy` (0 | 1) of the operand images; the single quad uses copy 0 only
__device__ __forceinline__ _Float16* xs_img(unsigned char* smem, int copy) { return (_Float16*)(smem + L_XS) + copy * RMAX * XS_LD; }
__device__ __forceinline__ _Float16* at_img(unsigned char* smem, int copy) { return (_Float16*)(smem + L_AT) + copy * RMAX * XS_LD; }
__device__ __forceinline__ _Float16* hs_img(unsigned char* smem, int copy) { return (_Float16*)(smem + L_HS) + copy * RMAX * HS_LD; }

// this wave's packed weight slices: P1 by head; out-projection | FFN1 | FFN2 by member (`off` in KiB-instructions); logits
__device__ __forceinline__ const h8* p1_src(const MegaArgs& a, const Ctx& q, int layer) {
  return a.wpack + ((size_t)layer * LAYER_HALFS + ((size_t)q.head * 4 + q.cw) * WI_P1 * 512) / 8 + q.lane;
}
__device__ __forceinline__ const h8* pm_src(const MegaArgs& a, const Ctx& q, int layer, int off) {
  return a.wpack + ((size_t)layer * LAYER_HALFS + P1_HALFS + (((size_t)q.member * 4 + q.cw) * (WI_P2 + WI_P3 + WI_P4) + off) * 512) / 8 + q.lane;
}
__device__ __forceinline__ const h8* lg_src(const MegaArgs& a, const Ctx& q) {
  return a.lpack + (((size_t)q.member * 4 + q.cw) * WI_LG * 512) / 8 + q.lane;
}

// ---- comm waves ----
// One row of hop A, hop C or the tail's hop A' (at `g`) -> LayerNorm -> XS copy `copy`.  ya != null: the call's first
// step reads its input embedding from there instead of sweeping (s == 0 && l == 0).  The single quad keeps the fp32 row in
// XRES; PIPE parks the member's residual columns in rs[which] of the current quad.
template <bool PIPE>
__device__ __forceinline__ void sweep_ln(const Ctx& q, int ra, gu64* g, unsigned ep, unsigned code, bool hint, const float* ya,
                                         int copy, int which, bool norm, const float (&gm)[8], const float (&bt)[8]) {
  if (ra >= q.R) return;
  u4v qa[4];
  bool ok = true;
  if (ya) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { const f2 y2 = *(const f2*)(ya + 2 * q.lane + j * 128); qa[j] = (u4v){__float_as_uint(y2[0]), 0u, __float_as_uint(y2[1]), 0u}; }
  } else {
    ok = sweep_wide<4>(q, g + ra * 512, ep, qa, code, hint);
  }
  if (!ok) return;
  if constexpr (PIPE) ln_row_pipe(q, ra, copy, which, qa, norm, gm, bt);
  else ln_row_wide(q, ra, qa, norm, gm, bt);
}

// One row of hop B (NQ = 2: attention output) or hop D (NQ = 8: FFN hidden) at `g` -> the row of the AT / HS copy `img`
template <int NQ>
__device__ __forceinline__ void sweep_img(const Ctx& q, int ra, gu64* g, unsigned ep, unsigned code, bool hint, _Float16* img, int ld) {
  if (ra >= q.R) return;
  u4v v[NQ];
  if (sweep_wide<NQ>(q, g + ra * NQ * 128, ep, v, code, hint)) {
    unsigned* d = (unsigned*)img + ra * (ld / 2) + 2 * q.lane;
#pragma unroll
    for (int j = 0; j < NQ; ++j) *(u2v*)(d + j * 128) = (u2v){v[j][0], v[j][2]};
  }
}

// Row state published by the samplers with the embedding: {active} per row.  ALL quads' rows, in front of the step's first
// barrier, so that every later slot of the step (K/V prefetch, exit test) sees the step's state.  One wave.
__device__ __forceinline__ void sweep_row_state(const Ctx& q, int nq, int s, unsigned ep) {
  for (int q2 = 0; q2 < nq; ++q2) {
    Ctx t = q;
    set_quad(t, q2);
    unsigned sv[1];
    if (sweep<1>(t, hop_slot(t, s, 0) + HOP_ST, t.R, ep, sv, 2u) && t.lane < t.R) {
      const int was = st_active(t)[t.lane], now = (int)(sv[0] & 1u);
      if (was) { st_step(t)[t.lane] += 1; if (now) st_kvlen(t)[t.lane] += 1; }
      st_active(t)[t.lane] = now;
    }
  }
}

// LayerNorm parameters of a layer, loaded in P1's poll-free stretch (a load issued right before a sweep would sit in front
// of its polls: a wave's memory operations return in order): norm1 for hop C, norm2 for the next hop A / the tail
__device__ __forceinline__ void ln_params_load(const float* lp, int lane, float (&gC)[8], float (&bC)[8], float (&gA)[8], float (&bA)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int el = (k >> 1) * 128 + 2 * lane + (k & 1);      // the element sweep_wide<4> delivers in slot k
    gC[k] = lp[FP_N1W + el]; bC[k] = lp[FP_N1B + el];
    gA[k] = lp[FP_N2W + el]; bA[k] = lp[FP_N2B + el];
  }
}

// ---- compute waves ----
// lane j < 24 of every wave reduces 4 values of q | k | v of the wave's OWN attention row (qkv_reduce): their bias
__device__ __forceinline__ f4 qkv_bias(const float* lp, int lane, int head) {
  const int rj_which = (lane >> 3) % 3, rj_e = 4 * (lane & 7);
  return lane < 24 ? *(const f4*)(lp + FP_QKVB + rj_which * D + head * HD + rj_e) : (f4){0.f, 0.f, 0.f, 0.f};
}
// split-K reduce of q, k, v (+ bias) by the wave that consumes them: each attention wave sums the 96 values of ITS row
// (both waves of a row do, and write identical bytes), so that no barrier stands between the reduce and the attention
// -- the workgroup-wide reduce + compute-only barrier here were 0.7 us of every layer (stamps 4-7).  Same summation
// order as before: ((w0 + w1) + w2) + w3 + bias.
__device__ __forceinline__ void qkv_reduce(unsigned char* smem, int lane, int cw, int half, int R, f4 p1_bias) {
  const int rj_which = (lane >> 3) % 3, rj_e = 4 * (lane & 7);
  const f4* red = (const f4*)(smem + L_RED);
  _Float16* qkv_s = (_Float16*)(smem + L_QKV);
  const int ro = cw / 2, r = 2 * ro + half;
  if (lane < 24 && r < R) {
    const int tile = rj_which * 2 + (rj_e >> 4), ln = r + 16 * ((rj_e & 15) >> 2);
    const f4 v0 = red[red_idx(0 * 6 + tile, ln)], v1 = red[red_idx(1 * 6 + tile, ln)], v2 = red[red_idx(2 * 6 + tile, ln)],
             v3 = red[red_idx(3 * 6 + tile, ln)];
    f4 v = v0;
    v += v1; v += v2; v += v3;
    v += p1_bias;
    *(h4*)(qkv_s + (ro * 3 + rj_which) * HD + rj_e) = (h4){(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};    // the arena append of k, v follows (arena_append)
  }
  asm volatile("" ::: "memory");                      // the attention's reads of qkv_s stay behind the writes (same wave: in order)
}

// one wave combines the partials of the 2 attention waves of each own row (lane = ro * 32 + e) and publishes hop B
__device__ __forceinline__ void attn_combine_publish(unsigned char* smem, int lane, int head, int half, int R, gu64* hop_b, unsigned ep) {
  const float* s_m = (const float*)(smem + L_ATT);
  const float* s_acc = s_m + 8;
  const int ro = lane >> 5, e = lane & 31, r = 2 * ro + half;
  float M = -INFINITY;
#pragma unroll
  for (int w = 0; w < 2; ++w) M = fmaxf(M, s_m[2 * ro + w]);
  float o = 0.f;
  if (M != -INFINITY) {
    float Lsum = 0.f, num = 0.f;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const float mw = s_m[2 * ro + w];
      const float ew = mw == -INFINITY ? 0.f : __expf(mw - M);
      const float* pa = s_acc + (2 * ro + w) * 4 * 36;
      Lsum += ((pa[32] + pa[36 + 32]) + (pa[72 + 32] + pa[108 + 32])) * ew;
      num += ((pa[e] + pa[36 + e]) + (pa[72 + e] + pa[108 + e])) * ew;
    }
    o = num / Lsum;
  }
  const float o2 = dpp_f<DPP_QUAD_XOR1>(o);            // lane ^ 1
  // 16 granules (one 128-B line) per own row, written by one wave instruction
  if (r < R && !(e & 1)) gstore(hop_b + r * 256 + (head * HD + e) / 2, ep, pack_h2(o, o2));
}

// K/V arena append of this step's k, v of the own rows (rows 2 ro + half of the quad whose state and first batch row are
// given), from the LDS copy the attention used; lanes 0..31 of one wave
__device__ __forceinline__ void arena_append(const MegaArgs& a, unsigned char* smem, int lane, int l, int head, int half, int R,
                                             int b0, const lds_int* active, const lds_int* kvlen) {
  const int ro = lane >> 4, which = (lane >> 3) & 1, e = 4 * (lane & 7), r = 2 * ro + half;
  if (r < R && active[r]) {
    const int pos = kvlen[r];
    if (pos < a.smax)
      *(h4*)(a.kv + ((size_t)(l * 2 + which)) * a.kv_layer_stride + ((size_t)(b0 + MG_GROUPS * r) * NH + head) * (size_t)a.smax * HD +
             (size_t)pos * HD + e) = *(const h4*)((const _Float16*)(smem + L_QKV) + (ro * 3 + 1 + which) * HD + e);
  }
}

// test hook (gsv_t2s_debug_stall, tests only): that member of group 0 skips ONE publish of hop C, so that the group's
// bounded waits must end the launch with an error instead of hanging
__device__ __forceinline__ bool stall_hook(const MegaArgs& a, int member, int group, int s, int l, int qd) {
  return a.test_stall && member == a.test_stall - 1 && group == 0 && s == 2 && l == 3 && qd == 0;
}

// One wave: split-K reduce of the member's 16 columns + bias + residual `xr` (the lane's f4 of the LayerNorm output the
// GEMM's input came from) -> fp32 row segment published at `dst` (+ row * 512): the out-projection's y1 to hop C, FFN2's
// y2 to hop A of the next layer (hop A' of the logits after the last).  skip: stall_hook.
__device__ __forceinline__ void reduce_residual_publish(unsigned char* smem, int lane, int member, int R, f4 bias, f4 xr, gu64* dst,
                                                        unsigned ep, bool skip) {
  const f4* red = (const f4*)(smem + L_RED);
  const int r = lane & 15;
  if (r < R) {
    const f4 v0 = red[red_idx(0, lane)], v1 = red[red_idx(1, lane)], v2 = red[red_idx(2, lane)], v3 = red[red_idx(3, lane)];
    f4 v = v0;
    v += v1; v += v2; v += v3;
    v += bias;
    v += xr;
    *(f4*)((float*)(smem + L_STAGE) + r * 16 + 4 * (lane >> 4)) = v;
  }
  // transposed through LDS (same wave): lane = row * 16 + column, so each row's 16 granules = one 128-B line
  // written whole by ONE store instruction (scattered 8-B write-through stores made every hop 2-3x slower)
  if (lane < R * 16 && !skip)
    gstore(dst + (lane >> 4) * 512 + 16 * member + (lane & 15), ep, __float_as_uint(((const float*)(smem + L_STAGE))[lane]));
}

// FFN1: every wave publishes its own tile (+ bias, ReLU) to hop D: 16 columns = 8 half-pair granules = 64 contiguous bytes
// per row, the rows of the quad by one store instruction (transposed through the wave's own LDS patch: lane = row * 8 + granule)
__device__ __forceinline__ void ffn1_publish(unsigned char* smem, int lane, int cw, int member, int R, f4 v, f4 bias, gu64* hop_d, unsigned ep) {
  const int r = lane & 15;
  unsigned* stage = (unsigned*)(smem + L_STAGE) + cw * 64;
  v += bias;
  if (r < R) {
    const int w0 = r * 8 + 2 * (lane >> 4);
    stage[w0] = pack_h2(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f));
    stage[w0 + 1] = pack_h2(fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
  }
  if (lane < R * 8) gstore(hop_d + (lane >> 3) * 1024 + 32 * member + 8 * cw + (lane & 7), ep, stage[lane]);
}

// FFN2 over K = 2048: each wave chains its 4 chunks of 128 of the hidden image `hs` into ONE accumulator (the MFMA forwards
// a dependent accumulator without a stall): one partial per wave like the other phases, instead of 16 per workgroup through
// LDS.  The operand reads of chunk cc + 1 are in flight under the MFMAs of chunk cc (two register sets of 4 fragments; same
// MFMA order, bit-identical): 295.8 -> 292.6 us per step over 4 pairs (3 of 4), profiles/r03_ab_ffn2_operand_prefetch.txt
__device__ __forceinline__ void ffn2_chunks(const h8 (&w)[WI_P4], const _Float16* hs, unsigned char* smem, int lane, int cw) {
  const int rowl = lane & 15, kg = lane >> 4;
  f4* red = (f4*)(smem + L_RED);
  f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
  const _Float16* bp0 = hs + (rowl & (RMAX - 1)) * HS_LD + (4 * cw) * 128 + 8 * kg;
  h8 bA[4], bB[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) bA[ks] = *(const h8*)(bp0 + 32 * ks);
#pragma unroll
  for (int cc = 0; cc < 4; cc += 2) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) bB[ks] = *(const h8*)(bp0 + (cc + 1) * 128 + 32 * ks);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[cc * 4 + ks], bA[ks], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (cc + 2 < 4) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bA[ks] = *(const h8*)(bp0 + (cc + 2) * 128 + 32 * ks);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[(cc + 1) * 4 + ks], bB[ks], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (rowl < RMAX) red[red_idx(cw, lane)] = acc;
}

// logits: wave t < 3 reduces and publishes tile t of the member (tiles member, member + 32, and tile 64 on member 0) to hop E
__device__ __forceinline__ void logits_publish(unsigned char* smem, int lane, int t, int member, int R, int V, gu64* hop_e, unsigned ep) {
  const f4* red = (const f4*)(smem + L_RED);
  const int r = lane & 15;
  const int tile = t == 0 ? member : (t == 1 ? member + 32 : 64);
  float* stage = (float*)(smem + L_STAGE) + t * 256;
  if (r < R) {
    f4 v = red[red_idx(0 * 3 + t, lane)];
    v += red[red_idx(1 * 3 + t, lane)]; v += red[red_idx(2 * 3 + t, lane)]; v += red[red_idx(3 * 3 + t, lane)];
    *(f4*)(stage + r * 16 + 4 * (lane >> 4)) = v;
  }
  if (lane < R * 16 && (t < 2 || member == 0) && 16 * tile + (lane & 15) < V)
    gstore(hop_e + (lane >> 4) * VPAD + 16 * tile + (lane & 15), ep, __float_as_uint(stage[lane]));
}

// ---------------------------------------------------------------------------------------------------------------
// One quad per group (B <= 32).  Every phase waits out its hop: the comm waves sweep it into the operand image, B1, the
// compute waves multiply, B2, reduce and publish.
// ---------------------------------------------------------------------------------------------------------------
template <bool PROF, bool LOGP>
__device__ __forceinline__ void comm_role(const MegaArgs& a, const Ctx& c0, const StepParams& sp) {
  Ctx q = c0;
  unsigned char* smem = c0.smem;
  const bool sampler = c0.member < c0.Rtot && c0.cw == 0;   // wave 0 of member m samples the group's local row m
  const int EPS = 4 * a.L + 2;                       // hops per step
  unsigned char* seen = smem + L_SEEN;
  KvStage kvs;
  set_quad(q, 0);
  kv_stage_load(a, q, 0, 0, 0, kvs);
  kv_stage_store(q, 0, 0, kvs);                      // layer 0's image (the attention waves read it after B1 + two compute barriers)
  float gC[8], bC[8], gA[8], bA[8];                  // see ln_params_load
#pragma unroll
  for (int k = 0; k < 8; ++k) gC[k] = bC[k] = gA[k] = bA[k] = 0.f;
  const int ra = c0.cw;                              // this wave's row
  for (int s = 0; s < a.nsteps; ++s) {
    const unsigned ep0 = a.ep_base + (unsigned)s * (unsigned)EPS;  // epoch of hop i of this step = ep0 + i + 1
    for (int l = 0; l < a.L; ++l) {
      const int ab_l = *st_abort(q);       // the abort test of this layer: read here, acted on behind the first barrier
      const float* lp = a.fpack + (size_t)l * FP_LAYER;
      q.prof_on = PROF && s == a.prof_step && l == a.prof_layer;
      // ================= P1: hop A (y of the previous layer, or the step's input embedding) -> LayerNorm -> XS / XRES;
      // the compute waves run QKV and the attention
      relaunder(q);
      q.hop = hop_slot(q, s, l);
      MG_STAMP(q, 0);
      sweep_ln<false>(q, ra, q.hop + HOP_A, ep0 + 4 * l + 1, 1u, a.hint_mask & 1,
                      s == 0 && l == 0 ? a.ybuf + (size_t)batch_row(q, ra) * D : nullptr, 0, 0, l > 0, gA, bA);   // layer 0's input is the embedding itself
      if (l == 0 && s > 0 && q.cw == 0) sweep_row_state(q, 1, s, ep0 + 1);
      MG_STAMP(q, 1);
      MG_BAR_AL(q);                                                       // B1
      if (l == 0 && s > 0 && group_done(q)) return;                       // every row of the group has finished
      MG_STAMP(q, 2);
      // K/V of the NEXT layer (across the step boundary the rows hold one more position: appended at this step's layer 0);
      // the compute waves run the QKV GEMM, the reduce and the attention meanwhile, synchronised among themselves
      const int kv_nl = l + 1 < a.L ? l + 1 : 0, kv_extra = l + 1 < a.L ? 0 : 1;
      const bool kv_more = l + 1 < a.L || s + 1 < a.nsteps;
      if (kv_more) kv_stage_load(a, q, kv_nl, 0, kv_extra, kvs);
      ln_params_load(lp, q.lane, gC, bC, gA, bA);    // after hop A: its LayerNorm above still needed the previous layer's norm2
      MG_STAMP(q, 4);
      MG_BAR();                                                          // B4: the attention is done, the K/V image is free
      MG_STAMP(q, 5);
      relaunder(q);
      if (kv_more) kv_stage_store(q, 0, kv_extra, kvs);
      // ================= P2: hop B (attention output of all heads) -> AT
      relaunder(q);
      q.hop = hop_slot(q, s, l);
      sweep_img<2>(q, ra, q.hop + HOP_B, ep0 + 4 * l + 2, 3u, a.hint_mask & 2, at_img(smem, 0), XS_LD);
      MG_STAMP(q, 6);
      MG_BAR();                                                           // B1
      MG_STAMP(q, 7);
      MG_BAR();                                                          // B2
      MG_STAMP(q, 8);
      // ================= P3: hop C (y1) -> LayerNorm1 -> XS / XRES
      relaunder(q);
      q.hop = hop_slot(q, s, l);
      sweep_ln<false>(q, ra, q.hop + HOP_C, ep0 + 4 * l + 3, 4u, a.hint_mask & 4, nullptr, 0, 1, true, gC, bC);
      MG_STAMP(q, 9);
      MG_BAR();                                                           // B1 (no B2: see compute_role)
      MG_STAMP(q, 10);
      MG_STAMP(q, 11);
      // ================= P4: hop D (FFN hidden) -> HS
      relaunder(q);
      q.hop = hop_slot(q, s, l);
      sweep_img<8>(q, ra, q.hop + HOP_D, ep0 + 4 * l + 4, 5u, a.hint_mask & 8, hs_img(smem, 0), HS_LD);
      MG_STAMP(q, 12);
      MG_BAR();                                                           // B1
      MG_STAMP(q, 13);
      MG_BAR();                                                          // B2
      MG_STAMP(q, 14);
    }
    // ---- tail: hop A' -> LayerNorm2 of the last layer -> XS, logits by the compute waves
    relaunder(q);
    q.hop = hop_slot(q, s, a.L);
    q.prof_on = false;
    sweep_ln<false>(q, ra, q.hop + HOP_A, ep0 + 4 * a.L + 1, 6u, a.hint_mask & 1, nullptr, 0, 0, true, gA, bA);
    MG_BAR();                                                             // B1
    MG_BAR();                                                            // B2
    if (sampler) MG_RUN_SAMPLER(LOGP);
  }
}

template <bool PROF>
__device__ __forceinline__ void compute_role(const MegaArgs& a, const Ctx& c0) {
  Ctx q = c0;
  unsigned char* smem = c0.smem;
  const int V = a.V;
  const int EPS = 4 * a.L + 2;
  // P1's slice is held as two halves (tiles q0 q1 k0 | k1 v0 v1): the second half is requested one phase later than the
  // first, so that FFN2's slice + the whole next P1 slice are never live together (160 + operands would spill)
  h8 wA0[WI_P1 / 2], wA1[WI_P1 / 2], wB[WI_P2], wC[WI_P3], wD[WI_P4];       // the logits slice reuses wA0
  int cgen = 0;                                       // compute_barrier generation
  // Weight slices are requested right AFTER a hop has landed (B1), never right after a publish: a load issued behind a
  // publish sits in the CU's in-order memory pipeline in front of the sweep waves' polls of the next hop.
  wload(wA0, p1_src(a, q, 0));
  wload(wA1, p1_src(a, q, 0) + (size_t)(WI_P1 / 2) * 64);

  for (int s = 0; s < a.nsteps; ++s) {
    const unsigned ep0 = a.ep_base + (unsigned)s * (unsigned)EPS;
    for (int l = 0; l < a.L; ++l) {
      const int ab_l = *st_abort(q);       // the abort test of this layer: read here, acted on behind the first barrier
      const float* lp = a.fpack + (size_t)l * FP_LAYER;
      q.prof_on = PROF && s == a.prof_step && l == a.prof_layer;
      // ================= P1: q,k,v of head `head` for the own rows, attention (K/V append: see P2)
      {
        relaunder(q);
        q.hop = hop_slot(q, s, l);
        MG_STAMP(q, 0);
        const f4 p1_bias = qkv_bias(lp, q.lane, q.head);
        MG_STAMP(q, 1);
        MG_BAR_AL(q);                                                       // B1: XS / XRES hold LN(y)
        if (l == 0 && s > 0 && group_done(q)) return;
        MG_STAMP(q, 2);
        wload(wB, pm_src(a, q, l, 0));
        gemm_chunk<3>(q, wA0, xs_img(smem, 0), XS_LD, q.cw, q.cw * 6);
        gemm_chunk<3>(q, wA1, xs_img(smem, 0), XS_LD, q.cw, q.cw * 6 + 3);
        MG_STAMP(q, 3);
        if (compute_barrier(q, cgen)) return;                              // B2 (compute waves only)
        MG_STAMP(q, 4);
        qkv_reduce(smem, q.lane, q.cw, q.half, q.R, p1_bias);
        MG_STAMP(q, 5);
        MG_STAMP(q, 6);
        MG_STAMP(q, 7);
        attention_part<2>(a, q, l, q.cw);
        MG_STAMP(q, 8);
        // the partials of a row's two waves meet through LDS.  This barrier is B4 itself (the attention has released the K/V
        // image): the comm waves only have to ISSUE the next layer's K/V loads before it, which takes ~1.5 us since the row
        // state is read once per call (it was 3.5 us, and a compute-only barrier stood here so that the publish did not wait)
        MG_BAR();                                                           // B4
        MG_STAMP(q, 9);
        if (q.cw == 0) attn_combine_publish(smem, q.lane, q.head, q.half, q.R, q.hop + HOP_B, ep0 + 4 * l + 2);
        MG_STAMP(q, 10);
      }
      // ================= P2: out-projection columns [16 member, +16) + bias + residual -> y1
      {
        relaunder(q);
        q.hop = hop_slot(q, s, l);
        const f4 p_bias = *(const f4*)(lp + FP_OUTB + 16 * q.member + 4 * (q.lane >> 4));
        MG_STAMP(q, 11);
        MG_BAR();                                                           // B1: AT holds the attention output
        MG_STAMP(q, 12);
        wload(wC, pm_src(a, q, l, WI_P2));
        gemm_chunk<1>(q, wB, at_img(smem, 0), XS_LD, q.cw, q.cw);
        MG_STAMP(q, 13);
        MG_BAR();                                                          // B2
        MG_STAMP(q, 14);
        if (q.cw == 0)
          reduce_residual_publish(smem, q.lane, q.member, q.R, p_bias,
                                  *(const f4*)((const float*)(smem + L_XRES) + (q.lane & 15) * D + 16 * q.member + 4 * (q.lane >> 4)),
                                  q.hop + HOP_C, ep0 + 4 * l + 3, stall_hook(a, q.member, q.group, s, l, 0));
        // wave 1 is idle while wave 0 publishes.  K/V arena append: not in P1 where k, v are produced -- there the store has
        // to queue behind the comm waves' K/V burst of the next layer in the CU's memory pipeline (1.3 us of blocked issue in
        // the stamps); nothing reads the arena row before the next step's staging
        if (q.cw == 1 && q.lane < 32) arena_append(a, smem, q.lane, l, q.head, q.half, q.R, batch_row(q, 0), st_active(q), st_kvlen(q));
      }
      // ================= P3: FFN1 columns [64 member, +64), ReLU -> h
      {
        relaunder(q);
        q.hop = hop_slot(q, s, l);
        const f4 p_bias = *(const f4*)(lp + FP_B1 + 64 * q.member + 16 * q.cw + 4 * (q.lane >> 4));       // tile cw of the member's four
        MG_STAMP(q, 15);
        MG_BAR();                                                           // B1: XS / XRES hold LN1(y1)
        MG_STAMP(q, 16);
        wload(wD, pm_src(a, q, l, WI_P2 + WI_P3));
        const f4 v = gemm_tile_k512(q, wC, xs_img(smem, 0), XS_LD);
        MG_STAMP(q, 17);
        // no B2: the next writer of XS is hop A of the next layer, two workgroup barriers away
        MG_STAMP(q, 18);
        ffn1_publish(smem, q.lane, q.cw, q.member, q.R, v, p_bias, q.hop + HOP_D, ep0 + 4 * l + 4);
      }
      // ================= P4: FFN2 columns [16 member, +16) over K = 2048 -> y2
      {
        relaunder(q);
        q.hop = hop_slot(q, s, l);
        const f4 p_bias = *(const f4*)(lp + FP_B2 + 16 * q.member + 4 * (q.lane >> 4));
        MG_STAMP(q, 19);
        MG_BAR();                                                           // B1: HS holds the FFN hidden
        MG_STAMP(q, 20);
        if (l + 1 < a.L) wload(wA0, p1_src(a, q, l + 1));                  // P1 has finished with wA0
        else wload(wA0, lg_src(a, q));
        ffn2_chunks(wD, hs_img(smem, 0), smem, q.lane, q.cw);
        // second half of the next P1 slice: FFN2 is done, and the request is still in front of the publish
        wload(wA1, p1_src(a, q, l + 1 < a.L ? l + 1 : 0) + (size_t)(WI_P1 / 2) * 64);
        MG_STAMP(q, 21);
        MG_BAR();                                                          // B2
        MG_STAMP(q, 22);
        if (q.cw == 0)                     // y2 feeds hop A of the next layer, or hop A' (the logits' LayerNorm) after the last layer
          reduce_residual_publish(smem, q.lane, q.member, q.R, p_bias,
                                  *(const f4*)((const float*)(smem + L_XRES) + (q.lane & 15) * D + 16 * q.member + 4 * (q.lane >> 4)),
                                  hop_slot(q, s, l + 1) + HOP_A, ep0 + 4 * (l + 1) + 1, false);
        MG_STAMP(q, 23);
      }
    }
    // ================= tail: logits split over the members
    relaunder(q);
    q.hop = hop_slot(q, s, a.L);
    q.prof_on = false;
    MG_BAR();                                                             // B1: XS holds LN2(y) of the last layer
    gemm_chunk<3>(q, wA0, xs_img(smem, 0), XS_LD, q.cw, q.cw * 3);
    wload(wA0, p1_src(a, q, 0));                                         // next step's layer 0 (two hops away; wA1 is there already)
    MG_BAR();                                                            // B2
    if (q.cw < 3) logits_publish(smem, q.lane, q.cw, q.member, q.R, V, q.hop + HOP_E, ep0 + 4 * a.L + 2);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Pipelined quads (32 < B <= 128): a group serves up to QMAX quads of rows, phase by phase one after the other with the
// weight slices it already holds.  Run like the single quad, every quad would wait out its sweep round trip (~1.1 us even
// when the data arrived long ago) in front of its GEMM: a GEMM-phase slot cost 1.8-2.7 us, a layer 44 us for four quads
// (in-kernel stamps of the removed sequential-quad mode).  Here the comm waves sweep quad i + 1's hop into the
// SECOND copy of the operand image while the compute waves multiply, reduce and publish quad i -- one workgroup barrier
// per slot:
//     comm:    sweep(0) | B | sweep(1)              | B | sweep(2)              | B | ...
//     compute:          | B | gemm(0) cb reduce(0)  | B | gemm(1) cb reduce(1)  | B | ...
// and P1 (QKV + attention) keeps two barriers per slot: B_a (the previous quad's attention has released the K/V image,
// LN(hop A) of this quad is in its XS copy) and B_b (the image of this quad is stored; the QKV partials are parked).
// The member's 16 residual columns of every row are parked per quad by the LayerNorm itself (no XRES image).
// ---------------------------------------------------------------------------------------------------------------
template <bool LOGP>
__device__ __forceinline__ void comm_role_pipe(const MegaArgs& a, const Ctx& c0, const StepParams& sp) {
  Ctx q = c0;
  unsigned char* smem = c0.smem;
  const int Rtot = c0.Rtot;
  const int nq = (Rtot + RMAX - 1) / RMAX;
  const bool sampler = c0.member < Rtot && c0.cw == 0;   // wave 0 of member m samples the group's local row m (quad m / 4, row m % 4)
  const int EPS = 4 * a.L + 2;
  unsigned char* seen = smem + L_SEEN;
  KvStage kvs;
  set_quad(q, 0);
  kv_stage_load(a, q, 0, 0, 0, kvs);                 // image of (layer 0, quad 0): stored by the first P1 slot like every other
  float gC[8], bC[8], gA[8], bA[8];                  // see ln_params_load
#pragma unroll
  for (int k = 0; k < 8; ++k) gC[k] = bC[k] = gA[k] = bA[k] = 0.f;
  const int ra = c0.cw;                              // this wave's row of every quad
  for (int s = 0; s < a.nsteps; ++s) {
    const unsigned ep0 = a.ep_base + (unsigned)s * (unsigned)EPS;
    // a sweep's preamble: quad qd becomes the current one (its rows, state entries and hop buffers)
    auto enter = [&](int qd, int l) { relaunder(q); set_quad(q, qd); q.hop = hop_slot(q, s, l); };
    for (int l = 0; l < a.L; ++l) {
      const int ab_l = *st_abort(q);       // the abort test of this layer: read here, acted on behind the first barrier
      const float* lp = a.fpack + (size_t)l * FP_LAYER;
      // ================= P1: hop A of quad qd -> LayerNorm -> XS copy qd & 1 (+ the residual columns of the out-projection)
      auto sweep_a = [&](int qd) {
        enter(qd, l);
        sweep_ln<true>(q, ra, q.hop + HOP_A, ep0 + 4 * l + 1, 1u, a.hint_mask & 1,
                       s == 0 && l == 0 ? a.ybuf + (size_t)batch_row(q, ra) * D : nullptr, qd & 1, 0, l > 0, gA, bA);
      };
      sweep_a(0);
      if (l == 0 && s > 0 && q.cw == 0) sweep_row_state(q, nq, s, ep0 + 1);
      for (int qd = 0; qd < nq; ++qd) {
        MG_BAR_AL(q);                                                       // B_a
        if (l == 0 && s > 0 && qd == 0 && group_done(q)) return;
        relaunder(q);
        // the image of THIS slot's quad (requested one slot ago) -> LDS.  At (l = 0, qd = 0) of a step after the first the rows'
        // state has just advanced: the image was requested with extra = 1 at the end of the previous step, the store uses the
        // advanced state with extra = 0 -- the same positions
        kv_stage_store(q, qd, 0, kvs);
        MG_BAR();                                                           // B_b
        // the NEXT slot's image: the next quad of this layer, else quad 0 of the next layer (across the step boundary the rows
        // hold one more position: appended at this step's layer 0); the compute waves run the reduce and the attention meanwhile
        const bool kv_same = qd + 1 < nq;
        const int kv_nq = kv_same ? qd + 1 : 0;
        const int kv_nl = kv_same ? l : (l + 1 < a.L ? l + 1 : 0), kv_extra = (kv_same || l + 1 < a.L) ? 0 : 1;
        if (kv_same || l + 1 < a.L || s + 1 < a.nsteps) kv_stage_load(a, q, kv_nl, kv_nq, kv_extra, kvs);
        if (kv_same) sweep_a(qd + 1);
        else ln_params_load(lp, q.lane, gC, bC, gA, bA);    // after the LAST quad's hop A: every quad's LayerNorm still needed the previous layer's norm2
      }
      // ================= P2: hop B -> AT copies
      auto sweep_b = [&](int qd) {
        enter(qd, l);
        sweep_img<2>(q, ra, q.hop + HOP_B, ep0 + 4 * l + 2, 3u, a.hint_mask & 2, at_img(smem, qd & 1), XS_LD);
      };
      sweep_b(0);
      for (int qd = 0; qd < nq; ++qd) {
        MG_BAR();
        if (qd + 1 < nq) sweep_b(qd + 1);
      }
      // ================= P3: hop C -> LayerNorm1 -> XS copies (+ the residual columns of FFN2)
      auto sweep_c = [&](int qd) {
        enter(qd, l);
        sweep_ln<true>(q, ra, q.hop + HOP_C, ep0 + 4 * l + 3, 4u, a.hint_mask & 4, nullptr, qd & 1, 1, true, gC, bC);
      };
      sweep_c(0);                       // no barrier between the phases: this sweep overlaps the last out-projection slot
      for (int qd = 0; qd < nq; ++qd) {
        MG_BAR();
        if (qd + 1 < nq) sweep_c(qd + 1);
      }
      // ================= P4: hop D -> HS copies
      auto sweep_d = [&](int qd) {
        enter(qd, l);
        sweep_img<8>(q, ra, q.hop + HOP_D, ep0 + 4 * l + 4, 5u, a.hint_mask & 8, hs_img(smem, qd & 1), HS_LD);
      };
      sweep_d(0);
      for (int qd = 0; qd < nq; ++qd) {
        MG_BAR();
        if (qd + 1 < nq) sweep_d(qd + 1);
      }
    }
    // ---- tail: hop A' -> LayerNorm2 of the last layer -> XS copies; logits by the compute waves
    auto sweep_t = [&](int qd) {
      enter(qd, a.L);
      sweep_ln<true>(q, ra, q.hop + HOP_A, ep0 + 4 * a.L + 1, 6u, a.hint_mask & 1, nullptr, qd & 1, 0, true, gA, bA);
    };
    sweep_t(0);
    for (int qd = 0; qd < nq; ++qd) {
      MG_BAR();
      if (qd + 1 < nq) sweep_t(qd + 1);
    }
    MG_BAR();                 // end of the step's GEMMs: the last logits GEMM has read its XS copy (the next step's first sweep rewrites copy 0)
    if (sampler) MG_RUN_SAMPLER(LOGP);
  }
}

__device__ __forceinline__ void compute_role_pipe(const MegaArgs& a, const Ctx& c0) {
  Ctx q = c0;
  unsigned char* smem = c0.smem;
  const int nq = (c0.Rtot + RMAX - 1) / RMAX;
  const int V = a.V;
  const int EPS = 4 * a.L + 2;
  h8 wA0[WI_P1 / 2], wA1[WI_P1 / 2], wB[WI_P2], wC[WI_P3], wD[WI_P4];       // as in compute_role
  int cgen = 0;
  wload(wA0, p1_src(a, q, 0));
  wload(wA1, p1_src(a, q, 0) + (size_t)(WI_P1 / 2) * 64);
  for (int s = 0; s < a.nsteps; ++s) {
    const unsigned ep0 = a.ep_base + (unsigned)s * (unsigned)EPS;
    // a slot's preamble: quad qd becomes the current one (its rows, state entries and hop buffers)
    auto enter = [&](int qd, int l) { relaunder(q); set_quad(q, qd); q.hop = hop_slot(q, s, l); };
    for (int l = 0; l < a.L; ++l) {
      const int ab_l = *st_abort(q);       // the abort test of this layer: read here, acted on behind the first barrier
      const float* lp = a.fpack + (size_t)l * FP_LAYER;
      // ================= P1.  The first slot's barrier and the next phase's weight request stand in FRONT of the quad loop: a
      // request inside the loop is either conditional (`if (qd == 0)`: a conditional definition keeps the register array's old
      // contents alive around the whole loop, ~100 spilled VGPRs) or repeated per quad -- and with non-temporal weight loads
      // the repeats missed L2 and every quad streamed the layer's slice again from the memory side: 6 GB per step at
      // B = 128, 1.07 ms per step
      MG_BAR_AL(q);                                                         // B_a of quad 0
      if (l == 0 && s > 0 && group_done(q)) return;
      relaunder(q);
      wload(wB, pm_src(a, q, l, 0));
      for (int qd = 0; qd < nq; ++qd) {
        if (qd > 0) {
          MG_BAR();                                                         // B_a: XS copy qd & 1 holds LN(y); the image is free
        }
        enter(qd, l);
        const f4 p1_bias = qkv_bias(lp, q.lane, q.head);
        gemm_chunk<3>(q, wA0, xs_img(smem, qd & 1), XS_LD, q.cw, q.cw * 6);
        gemm_chunk<3>(q, wA1, xs_img(smem, qd & 1), XS_LD, q.cw, q.cw * 6 + 3);
        MG_BAR();                                                           // B_b: partials parked, this quad's K/V image stored
        qkv_reduce(smem, q.lane, q.cw, q.half, q.R, p1_bias);
        attention_part<2>(a, q, l, q.cw);
        if (compute_barrier(q, cgen)) return;                              // the partials of a row's two waves meet (compute waves only)
        if (q.cw == 0) attn_combine_publish(smem, q.lane, q.head, q.half, q.R, q.hop + HOP_B, ep0 + 4 * l + 2);
        // the next quad's reduce overwrites the q/k/v copy before P2 comes round, so the arena append happens here (the
        // comm waves' K/V burst of the next slot was issued a whole attention ago and has drained)
        if (q.cw == 1 && q.lane < 32) arena_append(a, smem, q.lane, l, q.head, q.half, q.R, batch_row(q, 0), st_active(q), st_kvlen(q));
      }
      // ================= P2: out-projection
      MG_BAR();                                                             // AT copy 0 holds quad 0's attention output
      relaunder(q);
      wload(wC, pm_src(a, q, l, WI_P2));
      for (int qd = 0; qd < nq; ++qd) {
        if (qd > 0) {
          MG_BAR();                                                         // AT copy qd & 1 holds the attention output
        }
        enter(qd, l);
        const f4 p_bias = *(const f4*)(lp + FP_OUTB + 16 * q.member + 4 * (q.lane >> 4));
        gemm_chunk<1>(q, wB, at_img(smem, qd & 1), XS_LD, q.cw, q.cw);
        if (compute_barrier(q, cgen)) return;
        if (q.cw == 0)
          reduce_residual_publish(smem, q.lane, q.member, q.R, p_bias, *rs_at(smem, 0, qd, q.lane), q.hop + HOP_C, ep0 + 4 * l + 3,
                                  stall_hook(a, q.member, q.group, s, l, qd));
      }
      // ================= P3: FFN1 + ReLU
      MG_BAR();                                                             // XS copy 0 holds LN1(y1) of quad 0
      relaunder(q);
      wload(wD, pm_src(a, q, l, WI_P2 + WI_P3));
      for (int qd = 0; qd < nq; ++qd) {
        if (qd > 0) {
          MG_BAR();                                                         // XS copy qd & 1 holds LN1(y1)
        }
        enter(qd, l);
        const f4 p_bias = *(const f4*)(lp + FP_B1 + 64 * q.member + 16 * q.cw + 4 * (q.lane >> 4));
        const f4 v = gemm_tile_k512(q, wC, xs_img(smem, qd & 1), XS_LD);
        ffn1_publish(smem, q.lane, q.cw, q.member, q.R, v, p_bias, q.hop + HOP_D, ep0 + 4 * l + 4);
      }
      // ================= P4: FFN2
      MG_BAR();                                                             // HS copy 0 holds quad 0's FFN hidden
      relaunder(q);
      if (l + 1 < a.L) wload(wA0, p1_src(a, q, l + 1));                    // P1 has finished with both halves for every quad
      else wload(wA0, lg_src(a, q));
      wload(wA1, p1_src(a, q, l + 1 < a.L ? l + 1 : 0) + (size_t)(WI_P1 / 2) * 64);
      for (int qd = 0; qd < nq; ++qd) {
        if (qd > 0) {
          MG_BAR();                                                         // HS copy qd & 1 holds the FFN hidden
        }
        enter(qd, l);
        const f4 p_bias = *(const f4*)(lp + FP_B2 + 16 * q.member + 4 * (q.lane >> 4));
        ffn2_chunks(wD, hs_img(smem, qd & 1), smem, q.lane, q.cw);
        if (compute_barrier(q, cgen)) return;
        if (q.cw == 0)                     // y2 feeds hop A of the next layer, or hop A' (the logits' LayerNorm) after the last layer
          reduce_residual_publish(smem, q.lane, q.member, q.R, p_bias, *rs_at(smem, 1, qd, q.lane), hop_slot(q, s, l + 1) + HOP_A,
                                  ep0 + 4 * (l + 1) + 1, false);
      }
    }
    // ================= tail: logits
    for (int qd = 0; qd < nq; ++qd) {
      enter(qd, a.L);
      MG_BAR();                                                             // XS copy qd & 1 holds LN2(y) of the last layer
      gemm_chunk<3>(q, wA0, xs_img(smem, qd & 1), XS_LD, q.cw, q.cw * 3);
      if (compute_barrier(q, cgen)) return;
      if (q.cw < 3) logits_publish(smem, q.lane, q.cw, q.member, q.R, V, q.hop + HOP_E, ep0 + 4 * a.L + 2);
    }
    MG_BAR();                                                               // end of the step's GEMMs
    wload(wA0, p1_src(a, q, 0));                                           // the next step's first slice follows the logits slice's last reader
  }
}

// PIPE = false: one quad per group (B <= 32); true: several quads, pipelined (32 < B <= 128)
// PROF: the in-kernel stamps (tools/mega_prof.py) are compiled in only for measurement launches -- as run-time tests they
// cost ~100 scalar instructions per layer and wave.  Only the single-quad roles carry stamps.
// LOGP: the sampler also writes the taken token's log-probability (MG_RUN_SAMPLER).
template <bool PIPE, bool PROF, bool LOGP>
__global__ __launch_bounds__(MG_THREADS, 1) void t2s_mega_kernel(MegaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Ctx c;
  c.smem = smem;
  const int tid = threadIdx.x;
  c.lane = tid & 63; c.wave = __builtin_amdgcn_readfirstlane(tid >> 6); c.comm = c.wave < 4; c.cw = c.wave & 3; c.tid_c = tid - 256;
  if (a.map_shared == 2) {
    // Roles dealt by the XCD a workgroup actually RUNS on (HW_REG_XCC_ID) and its arrival order there: the 8 workgroups that
    // stream the same weight slice (one per row group) share an L2 whatever the dispatcher did.  blockIdx % 8 is only a label
    // of which blocks share an XCD under strict round-robin placement; when a CU is still busy at launch the dispatcher
    // deviates from it and a slice is then pulled into several L2s (the ~6 % slower of the two modes seen run to run).
    // Speed only: any assignment of the 256 (group, member) roles is correct.  32 workgroups of this footprint fit an XCD
    // (one per CU); a 33rd ticket means the device is not what the census assumed: error exit, the host falls back.
    if (tid == 0) {
      unsigned xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      xcc &= 7u;
      const unsigned t = __hip_atomic_fetch_add((gu32*)a.err + 8 + xcc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ((volatile int*)smem)[0] = (int)xcc;
      ((volatile int*)smem)[1] = (int)t;
    }
    __syncthreads();
    const int xcd = __builtin_amdgcn_readfirstlane(((volatile int*)smem)[0]), t = __builtin_amdgcn_readfirstlane(((volatile int*)smem)[1]);
    __syncthreads();                                 // (uniform values: keep them, and everything derived from them, in SGPRs)
    if (t >= 32) {
      if (tid == 0) { __hip_atomic_store((gu32*)a.err + 3, 0x50u, RLX_AGENT); __hip_atomic_store((gu32*)a.err, 1u, RLX_AGENT); }
      return;
    }
    c.member = xcd * 4 + (t >> 3); c.group = t & 7;
  } else if (a.map_shared) { const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3; c.member = xcd * 4 + (slot >> 3); c.group = slot & 7; }
  else { c.group = blockIdx.x & 7; c.member = blockIdx.x >> 3; }
  c.head = c.member >> 1; c.half = c.member & 1;
  c.member = __builtin_amdgcn_readfirstlane(c.member); c.group = __builtin_amdgcn_readfirstlane(c.group);
  c.head = c.member >> 1; c.half = c.member & 1;
  c.Rtot = a.B > c.group ? (a.B - c.group + MG_GROUPS - 1) / MG_GROUPS : 0;     // rows of this group: batch rows group, group + 8, ...
  if (c.Rtot == 0) return;
  set_quad(c, 0);
  c.hop_base = (gu64*)a.hop + (size_t)c.group * HOP_GROUP_ALL;
  c.hop = c.hop_base;
  c.err = (gu32*)a.err;
  c.prof = a.prof ? a.prof + ((size_t)blockIdx.x * 8 + c.wave) * 32 : nullptr;
  c.prof_on = false;
  c.hint_miss16 = (a.hint_mask >> 8) & 31;
  c.hint_pipe = (a.hint_mask >> 4) & 1;
  c.hint_spread = (a.hint_mask >> 7) & 1;
  const int lane = c.lane, Rtot = c.Rtot;
  const StepParams sp = *a.sp;

  // ---- init: zero the activation images, load the row state, build the samplers' seen-map ----
  for (int i = tid; i < L_RED / 4; i += MG_THREADS) ((unsigned*)smem)[i] = 0u;
  for (int i = tid; i < (L_TOTAL - L_KV) / 4; i += MG_THREADS) ((unsigned*)(smem + L_KV))[i] = 0u;   // attention_part relies on finite image cells
  if (tid < 3 * ST_N + 16) ((int*)(smem + L_ST))[tid] = 0;
  __syncthreads();
  if (tid < Rtot) {                                   // local row tid = 4 * quad + r
    const int b = c.group + MG_GROUPS * tid;
    ((int*)(smem + L_ST))[tid] = a.active[b];
    ((int*)(smem + L_ST))[ST_N + tid] = a.kv_len[b];
    ((int*)(smem + L_ST))[2 * ST_N + tid] = a.step_ctr[b];
    const unsigned long long seed_b = sp.rng_seed[b];
    ((int*)(smem + L_SR))[tid] = sp.plen[b];
    ((int*)(smem + L_SR))[ST_N + tid] = (int)(unsigned)seed_b;
    ((int*)(smem + L_SR))[2 * ST_N + tid] = (int)(unsigned)(seed_b >> 32);
    ((int*)(smem + L_SR))[3 * ST_N + tid] = sp.rng_row[b];
  }
  if (c.member < Rtot && c.wave == 0) {
    unsigned char* seen = smem + L_SEEN;
    for (int v = lane; v < VPAD; v += 64) seen[v] = 0;
    const int b = c.group + MG_GROUPS * c.member;
    const int prev_len = sp.plen[b] + a.step_ctr[b];
    const int* yrow = a.ytok + (size_t)b * a.ycap;
    __builtin_amdgcn_s_waitcnt(0);
    for (int t = lane; t < prev_len; t += 64) {
      const int tok = yrow[t];
      if (tok >= 0 && tok < a.V) seen[tok] = 1;
    }
  }
  __syncthreads();
  if (group_done(c)) return;
  if constexpr (PIPE) {
    if (c.comm) comm_role_pipe<LOGP>(a, c, sp);
    else compute_role_pipe(a, c);
  } else {
    if (c.comm) comm_role<PROF, LOGP>(a, c, sp);
    else compute_role<PROF>(a, c);
  }
}

// census: are 256 workgroups of the engine's footprint co-resident?  Every workgroup arrives on a counter and waits
// (bounded) for all of them; a workgroup that gives up reports it.
__global__ __launch_bounds__(MG_THREADS, 1) void mega_census_kernel(unsigned* ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  smem[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ws, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    while (__hip_atomic_load(ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)MG_NWG) {
      if (++spins > (1u << 20)) { __hip_atomic_fetch_add(ws + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
      __builtin_amdgcn_s_sleep(4);
    }
  }
}

}  // namespace

bool mega_shape_ok(int dim, int n_head, int ffn, int vocab) { return dim == D && n_head == NH && ffn == FF && vocab >= 64 && vocab <= VPAD; }
size_t mega_layer_pack_halfs() { return LAYER_HALFS; }
size_t mega_logits_pack_halfs() { return LOGIT_HALFS; }
size_t mega_hop_bytes(int ring) { return (size_t)(ring > 0 ? ring : 1) * MG_GROUPS * HOP_GROUP_ALL * 8; }

// fragment of one KiB-instruction: lane ln holds W[row0 + (ln & 15)][k0 + 8 (ln >> 4) .. +8]
static void pack_frag(const float* w, int ldw, int row0, int nrows, int k0, _Float16* dst) {
  for (int ln = 0; ln < 64; ++ln) {
    const int row = row0 + (ln & 15), k = k0 + 8 * (ln >> 4);
    for (int e = 0; e < 8; ++e) dst[ln * 8 + e] = row < nrows ? (_Float16)w[(size_t)row * ldw + k + e] : (_Float16)0.f;
  }
}

void mega_pack_layer(const float* qkv_w, const float* out_w, const float* w1, const float* w2, _Float16* dst) {
  // P1 by head: tiles q0 q1 k0 k1 v0 v1, wave = K chunk of 128, 4 k-steps of 32
  for (int h = 0; h < NH; ++h)
    for (int w = 0; w < 4; ++w)
      for (int t = 0; t < 6; ++t)
        for (int ks = 0; ks < 4; ++ks)
          pack_frag(qkv_w, D, (t >> 1) * D + h * HD + 16 * (t & 1), 3 * D, 128 * w + 32 * ks,
                    dst + (((size_t)h * 4 + w) * WI_P1 + t * 4 + ks) * 512);
  _Float16* pm = dst + P1_HALFS;
  const int per = WI_P2 + WI_P3 + WI_P4;
  for (int j = 0; j < MG_MEMBERS; ++j)
    for (int w = 0; w < 4; ++w) {
      _Float16* base = pm + ((size_t)j * 4 + w) * per * 512;
      for (int ks = 0; ks < 4; ++ks) pack_frag(out_w, D, 16 * j, D, 128 * w + 32 * ks, base + (size_t)ks * 512);
      // FFN1: wave w owns tile w (columns 64 j + 16 w, +16) over the whole K: slot 4 c + ks = K chunk c, k-step ks
      for (int c = 0; c < 4; ++c)
        for (int ks = 0; ks < 4; ++ks)
          pack_frag(w1, D, 64 * j + 16 * w, FF, 128 * c + 32 * ks, base + (size_t)(WI_P2 + c * 4 + ks) * 512);
      for (int cc = 0; cc < 4; ++cc)
        for (int ks = 0; ks < 4; ++ks)
          pack_frag(w2, FF, 16 * j, D, 128 * (4 * w + cc) + 32 * ks, base + (size_t)(WI_P2 + WI_P3 + cc * 4 + ks) * 512);
    }
}

void mega_pack_logits(const float* pred_w, int V, _Float16* dst) {
  for (int j = 0; j < MG_MEMBERS; ++j)
    for (int w = 0; w < 4; ++w)
      for (int t = 0; t < 3; ++t) {
        const int tile = t == 0 ? j : (t == 1 ? j + 32 : 64);
        for (int ks = 0; ks < 4; ++ks)
          pack_frag(pred_w, D, 16 * tile, V, 128 * w + 32 * ks, dst + (((size_t)j * 4 + w) * WI_LG + t * 4 + ks) * 512);
      }
}

int mega_census(hipStream_t s, unsigned* d_scratch, unsigned* h_pinned) {
  GSV_HIP(hipFuncSetAttribute((const void*)mega_census_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL));
  GSV_HIP(hipMemsetAsync(d_scratch, 0, 16, s));
  hipLaunchKernelGGL(mega_census_kernel, dim3(MG_NWG), dim3(MG_THREADS), L_TOTAL, s, d_scratch);
  GSV_HIP(hipGetLastError());
  GSV_HIP(hipMemcpyAsync(h_pinned, d_scratch, 8, hipMemcpyDeviceToHost, s));
  GSV_HIP(hipStreamSynchronize(s));
  return (h_pinned[0] == (unsigned)MG_NWG && h_pinned[1] == 0u) ? 1 : 0;
}

int launch_t2s_mega(const MegaArgs& a, bool logp, hipStream_t s) {
  // every launch: the attribute belongs to the (function, device) pair, and TTS.set_device may have moved the handle's owner
  // to another GPU of the process since the last launch (mega_census does the same)
#define GSV_MEGA_LAUNCH(PIPE, PROF, LOGP)                                                                                      \
  do {                                                                                                                        \
    GSV_HIP(hipFuncSetAttribute((const void*)t2s_mega_kernel<PIPE, PROF, LOGP>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                L_TOTAL));                                                                                    \
    hipLaunchKernelGGL((t2s_mega_kernel<PIPE, PROF, LOGP>), dim3(MG_NWG), dim3(MG_THREADS), L_TOTAL, s, a);                   \
  } while (0)
  // Five kernels.  More than one quad per group (B > 32): pipelined quads, which carry no stamps -- a profiling request
  // (a.prof, tools/mega_prof.py) at B > 32 runs this kernel all the same and its stamp buffer stays zero.  One quad: stamps
  // compiled in for measurement launches only.  logp (the decode's StepParams hold a log-probability pointer): the two
  // kernels whose sampler writes it, which carry no stamps either.
  if (logp && a.B > RMAX * MG_GROUPS) GSV_MEGA_LAUNCH(true, false, true);
  else if (logp) GSV_MEGA_LAUNCH(false, false, true);
  else if (a.B > RMAX * MG_GROUPS) GSV_MEGA_LAUNCH(true, false, false);
  else if (a.prof != nullptr) GSV_MEGA_LAUNCH(false, true, false);
  else GSV_MEGA_LAUNCH(false, false, false);
#undef GSV_MEGA_LAUNCH
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

}  // namespace gsv
