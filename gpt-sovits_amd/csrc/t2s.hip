// AR semantic-token decoder engine (H1-H5) for gfx950: the kernels and launchers of the decode step, load / finalize,
// gsv_t2s_decode, and the debug / timing hooks.  The engine state (gsv_t2s, RowState) is in t2s_engine.h, the prefill in
// t2s_prefill.hip, the persistent decode engine in t2s_mega.hip, the decode sessions in t2s_session.hip.
//
// State lives in HBM behind an opaque handle: weights in the engine dtype, a head-major KV
// arena [layer][k|v][row][head][pos][head_dim] (so one (row, head) stream is contiguous and a
// wave reads it as 1 KiB wave-instructions), per-row lengths/flags, and the token history.
// The reference re-concatenates the cache every step (t2s_model.py:186-187) and
// index_selects finished rows away on the host (:727-745); here rows are appended in place and
// finished rows are flagged on the device, so a decode step has no host synchronisation.
//
// gsv_t2s_decode samples step 0 from the prefill's last position and then has two ways through the remaining steps:
//  * the persistent engine (fp16, v1/v2 shape, B <= 128): ONE launch of t2s_mega.hip's kernel runs every step; a hand-off
//    timeout restores the row state and the batch continues on the other path;
//  * the launch-per-phase step (fp32, other shapes, gsv_t2s_set_mega(0), GSV_T2S_NO_MEGA=1, fallback): per layer 4 GEMM
//    launches (QKV+append, out-proj, FFN1, FFN2) and one attention launch, LayerNorm fused into the consumer's prologue,
//    split-K across the waves of a workgroup with an LDS combine (no global partials), then logits + a one-wave-per-row
//    sampling kernel; the step is captured once per batch size and replayed as one hipGraph.
// gsv_t2s_session_* (t2s_session.hip) run the same two paths, through run_chunk, a chunk of steps at a time over slots that are
// admitted and freed one by one.
#include <math.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>

#include "t2s_engine.h"

namespace gsv {

typedef float f4v __attribute__((ext_vector_type(4)));

// =======================================================================================
// kernels
// =======================================================================================

// ---------------------------------------------------------------------------------------
// Decode-step skinny GEMM:  Y[b][n] = sum_k X[b][k] W[n][k]   for b < B (B <= 16*CB)
// Workgroup = one 16-row tile of W (n0..n0+15), NW waves each owning K/NW of the contraction,
// partial 16x16 accumulators combined through LDS.  MFMA 16x16x32 f16 / 16x16x4 f32.
// ---------------------------------------------------------------------------------------
enum { EPI_QKV = 0, EPI_RESID = 1, EPI_RELU = 2, EPI_LOGITS = 3 };

struct DecGemmArgs {   // a kernel argument: trivially copyable, every field zero unless set
  // X source (exactly one of yin / xin)
  const float* yin = nullptr;     // fp32 pre-LN stream [B][K] -> LN(gamma,beta) (or plain convert if gamma==null) -> LDS
  const float* gamma = nullptr;
  const float* beta = nullptr;
  float* xres_out = nullptr;      // if non-null, workgroup 0 writes the normalised fp32 rows here [B][K]
  const void* xin = nullptr;      // T activations [B][K] read straight from HBM/L2
  const void* w = nullptr;        // T [N][K]
  const float* bias = nullptr;    // [N] or null
  int B = 0, K = 0, N = 0;
  int epi = 0;
  // epilogue targets
  void* out_t = nullptr;          // EPI_RELU: T [B][N]; EPI_QKV: q buffer T [B][d]
  float* out_f = nullptr;         // EPI_RESID / EPI_LOGITS: fp32 [B][N]
  const float* xres = nullptr;    // EPI_RESID: fp32 residual [B][N]
  void* kc = nullptr; void* vc = nullptr;   // EPI_QKV: cache bases for this layer
  const int* kv_len = nullptr;    // EPI_QKV
  const int* active = nullptr;
  int d = 0, H = 0, smax = 0;
};
static_assert(std::is_trivially_copyable<DecGemmArgs>::value, "DecGemmArgs is passed to kernels by value");

template <typename T> struct Frag16;
template <> struct Frag16<_Float16> { typedef h8 type; static constexpr int KS = 32; };
template <> struct Frag16<float> { typedef f4 type; static constexpr int KS = 16; };

__device__ __forceinline__ void mma16(f4v& acc, const h8& a, const h8& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(f4v& acc, const f4& a, const f4& b) {
  // lane group g = lane>>4 holds k = k0 + 4g + i; MFMA i contracts {k0+i, k0+4+i, k0+8+i, k0+12+i}
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], acc, 0, 0, 0);
}

template <typename T, int CB, int NW, int KSL, int KV4>
__global__ __launch_bounds__(NW * 64) void dec_gemm_kernel(DecGemmArgs a) {
  // KSL = K / NW (k-slice per wave, compile time so every load is issued up front);
  // KV4 > 0: LayerNorm prologue with K = 32*KV4, 8 threads per row, the row held in registers.
  typedef typename Frag16<T>::type F;
  constexpr int G = DT<T>::G;
  constexpr int KS = Frag16<T>::KS;  // k per MFMA group step
  constexpr int NKS = KSL / KS;
  constexpr bool LNPRO = KV4 > 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int b0 = blockIdx.y * CB * 16;   // batch-row block of this workgroup (grid.y > 1 only for narrow-N kernels)
  const int K = a.K;
  const int ldx = K + G;  // padded LDS row (elements): breaks the power-of-two row stride
  T* xs = (T*)smem;
  float* red = (float*)smem;   // the split-K combine buffer reuses the X image (barrier below)

  const int rowl = lane & 15, kg = lane >> 4;
  const int kbeg = wave * KSL;
  const bool wok = (n0 + rowl) < a.N;
  const T* wrow = (const T*)a.w + (long long)(wok ? n0 + rowl : 0) * K + kbeg + G * kg;
  // weight stream first: its HBM latency overlaps the LayerNorm prologue
  F af[NKS];
#pragma unroll
  for (int i = 0; i < NKS; ++i) af[i] = *(const F*)(wrow + i * KS);   // unconditional: wrow is clamped to row 0 when n0 + rowl >= N,
                                                                       // and those output rows are never stored

  // epilogue operands (bias, residual, row state) are fetched now, not after the LDS combine, so the
  // kernel has one exposed memory round trip instead of two
  constexpr int ITEMS = (CB + NW - 1) / NW;
  f4 pre_bias[ITEMS], pre_res[ITEMS];
  int pre_act[ITEMS], pre_pos[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int item = tid + it * NW * 64;
    const int ln = item & 63;
    const int b = b0 + (item >> 6) * 16 + (ln & 15);
    const int n = n0 + 4 * (ln >> 4);
    const bool ok = item < CB * 64 && b < a.B && n < a.N;
    pre_bias[it] = (f4){0.f, 0.f, 0.f, 0.f};
    pre_res[it] = (f4){0.f, 0.f, 0.f, 0.f};
    pre_act[it] = 0; pre_pos[it] = 0;
    if (ok) {
      if (a.bias) {
        if (n + 3 < a.N) pre_bias[it] = *(const f4*)(a.bias + n);
        else for (int i = 0; i < 4; ++i) if (n + i < a.N) pre_bias[it][i] = a.bias[n + i];
      }
      if (a.epi == EPI_RESID) {
        if (n + 3 < a.N) pre_res[it] = *(const f4*)(a.xres + (long long)b * a.N + n);
        else for (int i = 0; i < 4; ++i) if (n + i < a.N) pre_res[it][i] = a.xres[(long long)b * a.N + n + i];
      } else if (a.epi == EPI_QKV) {
        pre_act[it] = a.active[b];
        pre_pos[it] = a.kv_len[b];
      }
    }
  }

  if (LNPRO) {
    constexpr int TPR = 8;                       // threads per row
    constexpr int RPP = NW * 64 / TPR;           // rows per pass
    constexpr int NV = KV4 > 0 ? KV4 : 1;
    const int sub = tid & (TPR - 1);
    f4 gm[NV], bt[NV];
    if (a.gamma) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        gm[j] = *(const f4*)(a.gamma + (j * TPR + sub) * 4);
        bt[j] = *(const f4*)(a.beta + (j * TPR + sub) * 4);
      }
    }
    for (int r0 = 0; r0 < CB * 16; r0 += RPP) {
      const int row = r0 + tid / TPR;
      if (row >= CB * 16) break;
      const bool live = b0 + row < a.B;
      f4 v[NV];
      const float* src = a.yin + (long long)(live ? b0 + row : 0) * K;
#pragma unroll
      for (int j = 0; j < NV; ++j) v[j] = live ? *(const f4*)(src + (j * TPR + sub) * 4) : (f4){0.f, 0.f, 0.f, 0.f};
      if (a.gamma) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
        const float mean = s / (float)K;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { float dl = v[j][e] - mean; q += dl * dl; }
        }
        q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
        const float rstd = rsqrtf(q / (float)K + 1e-5f);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = live ? (v[j][e] - mean) * rstd * gm[j][e] + bt[j][e] : 0.f;
        }
      }
      T* dst = xs + (long long)row * ldx;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        typedef T T4 __attribute__((ext_vector_type(4)));
        *(T4*)(dst + (j * TPR + sub) * 4) = (T4){(T)v[j][0], (T)v[j][1], (T)v[j][2], (T)v[j][3]};
        if (a.xres_out && blockIdx.x == 0 && live) *(f4*)(a.xres_out + (long long)(b0 + row) * K + (j * TPR + sub) * 4) = v[j];
      }
    }
    __syncthreads();
  }

  f4v acc[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) acc[cb] = (f4v){0.f, 0.f, 0.f, 0.f};
  const T* xg = (const T*)a.xin;
  F bf[NKS][CB];
#pragma unroll
  for (int i = 0; i < NKS; ++i) {
    const int k = kbeg + i * KS + G * kg;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int brow = cb * 16 + rowl;
      if (LNPRO) bf[i][cb] = *(const F*)(xs + (long long)brow * ldx + k);
      else if (b0 + brow < a.B) bf[i][cb] = *(const F*)(xg + (long long)(b0 + brow) * K + k);
      else {
#pragma unroll
        for (int e = 0; e < G; ++e) bf[i][cb][e] = 0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NKS; ++i)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) mma16(acc[cb], af[i], bf[i][cb]);
  // combine the NW partial tiles through LDS (fixed summation order: deterministic)
  if (LNPRO) __syncthreads();   // every wave has its B fragments in registers: the X image may be overwritten
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) *(f4v*)(red + ((wave * CB + cb) * 64 + lane) * 4) = acc[cb];
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int item = tid + it * NW * 64;
    if (item >= CB * 64) break;
    const int cb = item >> 6, ln = item & 63;
    f4v v = (f4v){0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < NW; ++w) v += *(const f4v*)(red + ((w * CB + cb) * 64 + ln) * 4);
    // D layout of 16x16: col = ln & 15 (batch row), rows 4*(ln>>4) + i (output channel)
    const int b = b0 + cb * 16 + (ln & 15);
    const int n = n0 + 4 * (ln >> 4);
    if (b >= a.B || n >= a.N) continue;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = v[i] + pre_bias[it][i];
    const bool full = n + 3 < a.N;
    if (a.epi == EPI_RESID) {
      float* op = a.out_f + (long long)b * a.N + n;
      if (full) *(f4*)op = (f4){o[0] + pre_res[it][0], o[1] + pre_res[it][1], o[2] + pre_res[it][2], o[3] + pre_res[it][3]};
      else for (int i = 0; i < 4; ++i) if (n + i < a.N) op[i] = o[i] + pre_res[it][i];
    } else if (a.epi == EPI_RELU) {
      T* op = (T*)a.out_t + (long long)b * a.N + n;
      typedef T T4 __attribute__((ext_vector_type(4)));
      if (full) *(T4*)op = (T4){(T)fmaxf(o[0], 0.f), (T)fmaxf(o[1], 0.f), (T)fmaxf(o[2], 0.f), (T)fmaxf(o[3], 0.f)};
      else for (int i = 0; i < 4; ++i) if (n + i < a.N) op[i] = (T)fmaxf(o[i], 0.f);
    } else if (a.epi == EPI_LOGITS) {
      float* op = a.out_f + (long long)b * a.N + n;
      for (int i = 0; i < 4; ++i) if (n + i < a.N) op[i] = o[i];     // N = 1025: rows are not 16-byte aligned
    } else {  // EPI_QKV: n in [0,3d): q -> qbuf, k/v -> cache row kv_len[b]
      typedef T T4 __attribute__((ext_vector_type(4)));
      const int d = a.d, hd = d / a.H;
      const int which = n / d, c = n - which * d;
      const T4 ov = (T4){(T)o[0], (T)o[1], (T)o[2], (T)o[3]};
      if (which == 0) {
        *(T4*)((T*)a.out_t + (long long)b * d + c) = ov;
      } else if (pre_act[it]) {
        const int h = c / hd, e = c - h * hd;
        const int pos = pre_pos[it];
        if (pos < a.smax) {
          T* base = (T*)(which == 1 ? a.kc : a.vc);
          *(T4*)(base + (((long long)b * a.H + h) * a.smax + pos) * hd + e) = ov;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Decode attention (H4): one workgroup per (row, head); the KV stream of that pair is
// contiguous [pos][hd], read as 16-byte lane loads (1 KiB per wave-instruction), keys dealt
// round-robin to the 4 waves, per-lane online softmax, one LDS combine at the end.
// This is the HBM-bound kernel of the step: algorithmic bytes = 2*hd*sizeof(T) per cached key.
// ---------------------------------------------------------------------------------------
template <typename T, int HD>
__global__ __launch_bounds__(256) void decode_attn_kernel(const T* __restrict__ q, const T* __restrict__ kc,
                                                          const T* __restrict__ vc, const int* __restrict__ kv_len,
                                                          const int* __restrict__ active, int H, int smax,
                                                          T* __restrict__ out) {
  constexpr int G = DT<T>::G;
  constexpr int LPK = HD / G;      // lanes per key
  constexpr int KPI = 64 / LPK;    // keys per wave-instruction
  typedef typename Frag16<T>::type F;
  const int h = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int part = lane % LPK, slot = lane / LPK;
  const int d = H * HD;
  const T* kb = kc + ((long long)b * H + h) * smax * HD;
  const T* vb = vc + ((long long)b * H + h) * smax * HD;
  // q and the first SPEC key groups are fetched before the row state is known: the arena is
  // allocated to smax, so the addresses are valid and groups beyond kv_len are simply masked.
  // This takes the kv_len -> K/V dependency off the critical path (prompt + text is always longer
  // than SPEC*4*KPI keys in practice, so nothing extra is streamed).
  // The K/V stream (440 MB per step at the benchmark shape, read exactly once per step) is loaded NON-TEMPORAL so that it
  // does not evict the 152 MB of decoder weights from the 256 MB Infinity Cache between steps (GSV_KV_TEMPORAL=1 at build
  // time restores plain loads for A/B).
#ifdef GSV_KV_TEMPORAL
#define KVLOAD(p) (*(const F*)(p))
#else
#define KVLOAD(p) __builtin_nontemporal_load((const F*)(p))
#endif
  constexpr int SPEC = 3;
  const F qv = *(const F*)(q + (long long)b * d + h * HD + part * G);
  F ksp[SPEC], vsp[SPEC];
#pragma unroll
  // Every K/V load below is UNCONDITIONAL with a clamped key index (lanes past the end re-read the last valid row, which
  // costs no extra traffic, and are masked in consume()): per-lane conditional loads were compiled as one exec-masked
  // block per group with vmcnt(0) at each join, i.e. the NEXT groups were five dependent memory round trips.
  for (int i = 0; i < SPEC; ++i) {
    const int j = min((wave + 4 * i) * KPI + slot, smax - 1);
    ksp[i] = KVLOAD(kb + (long long)j * HD + part * G);
    vsp[i] = KVLOAD(vb + (long long)j * HD + part * G);
  }
  if (!active[b]) return;
  const int n = min(kv_len[b] + 1, smax);
  float qf[G];
  {
    const float scale = rsqrtf((float)HD);
#pragma unroll
    for (int i = 0; i < G; ++i) qf[i] = to_f(qv[i]) * scale;
  }
  float m = -INFINITY, l = 0.f, acc[G];
#pragma unroll
  for (int i = 0; i < G; ++i) acc[i] = 0.f;
  auto consume = [&](const F& kv, const F& vv, bool ok) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < G; ++i) s += qf[i] * to_f(kv[i]);
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) s += __shfl_xor(s, o, 64);
    if (ok) {
      const float mn = fmaxf(m, s);
      const float corr = __expf(m - mn);
      const float p = __expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int i = 0; i < G; ++i) acc[i] = acc[i] * corr + p * to_f(vv[i]);
      m = mn;
    }
  };
  // second batch: as soon as kv_len is known, the next NEXT groups are requested BEFORE the speculative
  // ones are consumed, so both batches share one memory round trip (up to (SPEC+NEXT)*4*KPI = 512 fp16 keys)
  constexpr int NEXT = 5;
  F kn[NEXT], vn[NEXT];
#pragma unroll
  for (int i = 0; i < NEXT; ++i) {
    const int j = min((wave + 4 * (SPEC + i)) * KPI + slot, n - 1);
    kn[i] = KVLOAD(kb + (long long)j * HD + part * G);
    vn[i] = KVLOAD(vb + (long long)j * HD + part * G);
  }
#pragma unroll
  for (int i = 0; i < SPEC; ++i) consume(ksp[i], vsp[i], (wave + 4 * i) * KPI + slot < n);
#pragma unroll
  for (int i = 0; i < NEXT; ++i) consume(kn[i], vn[i], (wave + 4 * (SPEC + i)) * KPI + slot < n);
  // keys past the first (SPEC+NEXT) groups (long sequences): batches of TB groups, two register sets alternated so the
  // next batch is in flight while the current one is consumed (all loads unconditional with a clamped key index).
  {
    constexpr int TB = 4, STR = 4 * KPI;
    int j0 = (wave + 4 * (SPEC + NEXT)) * KPI;
    if (j0 < n) {
      F ka[TB], va[TB], kq[TB], vq[TB];
      auto loadb = [&](F* kk, F* vv, int base) {
#pragma unroll
        for (int i = 0; i < TB; ++i) {
          const int jc = min(base + i * STR + slot, n - 1);
          kk[i] = KVLOAD(kb + (long long)jc * HD + part * G);
          vv[i] = KVLOAD(vb + (long long)jc * HD + part * G);
        }
      };
      auto consb = [&](const F* kk, const F* vv, int base) {
#pragma unroll
        for (int i = 0; i < TB; ++i) consume(kk[i], vv[i], base + i * STR + slot < n);
      };
      loadb(ka, va, j0);
      for (; j0 < n; j0 += 2 * TB * STR) {
        loadb(kq, vq, j0 + TB * STR);
        consb(ka, va, j0);
        loadb(ka, va, j0 + 2 * TB * STR);
        consb(kq, vq, j0 + TB * STR);
      }
    }
  }
  // combine: global max, rescale, sum over key slots (lanes with equal `part`) and waves
  __shared__ float s_m[4];
  __shared__ float s_acc[4][HD + 1];
  float wm = wave_max(m);
  if (lane == 0) s_m[wave] = wm;
  __syncthreads();
  const float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
  const float f = (m == -INFINITY) ? 0.f : __expf(m - M);
  l *= f;
#pragma unroll
  for (int i = 0; i < G; ++i) acc[i] *= f;
#pragma unroll
  for (int o = LPK; o < 64; o <<= 1) {
    l += __shfl_xor(l, o, 64);
#pragma unroll
    for (int i = 0; i < G; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
  }
  if (lane < LPK) {
#pragma unroll
    for (int i = 0; i < G; ++i) s_acc[wave][lane * G + i] = acc[i];
    if (lane == 0) s_acc[wave][HD] = l;
  }
  __syncthreads();
  if (threadIdx.x < HD) {
    const int e = threadIdx.x;
    const float L = s_acc[0][HD] + s_acc[1][HD] + s_acc[2][HD] + s_acc[3][HD];
    const float v = s_acc[0][e] + s_acc[1][e] + s_acc[2][e] + s_acc[3][e];
    out[(long long)b * d + h * HD + e] = (T)(v / L);
  }
#undef KVLOAD
}

// step tail: sample every row, update row state, emit the next step's input embedding
// (t2s_model.py:714-769).  grid = B, block = 64.  Row b's sampling values, EOS horizon, early stop and budget come from
// sp.row_sampling[b] / sp.row_limits[b], which decode_begin and the sessions' admissions fill for every row.
template <int NPL>
__global__ __launch_bounds__(64) void sample_step_kernel(const float* __restrict__ logits, int V, int EOS,
                                                         const StepParams* __restrict__ spp, int* __restrict__ ytok,
                                                         int ycap, int* __restrict__ kv_len, int* __restrict__ active,
                                                         int* __restrict__ step_ctr, int* __restrict__ n_active,
                                                         const float* __restrict__ e_audio, const float* __restrict__ pe,
                                                         float alpha_a, int d, float* __restrict__ ybuf) {
  extern __shared__ unsigned char seen[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const StepParams sp = *spp;
  const int step = step_ctr[b];
  if (!active[b]) return;
  const RowLimits rl = load_row_limits(sp.row_limits, b);
  const int Veff = (step < rl.eos_mask_steps) ? V - 1 : V;
  const int P = sp.plen[b];
  const int prev_len = P + step;
  int* yrow = ytok + (long long)b * ycap;
  const float* nrow = nullptr;
  if (sp.noise)
    nrow = sp.noise + ((long long)step * sp.noise_rows + (sp.noise_rows > 1 ? b : 0)) * V;
  int smp, amx;
  const RowSampling rs = load_row_sampling(sp.row_sampling, b);
  sample_row<NPL>(logits + (long long)b * V, V, Veff, yrow, prev_len, rs.top_k, rs.top_p, rs.temperature,
                  rs.rep_penalty, nrow, sp.rng_seed[b], sp.rng_row[b], step, seen, &smp, &amx);
  if (sp.dump)
    for (int v = lane; v < V; v += 64) sp.dump[((long long)step * gridDim.x + b) * V + v] = logits[(long long)b * V + v];
  if (sp.drawn && lane == 0) { int* dr = sp.drawn + ((long long)step * gridDim.x + b) * 2; dr[0] = smp; dr[1] = amx; }
  if (sp.force) { smp = sp.force[(long long)b * sp.max_steps + step]; amx = smp; }    // teacher forcing (parity hook)
  if (sp.logp) {     // the taken token's log-probability from the raw logits (sample_row penalised its own copy)
    float xr[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int v = lane + 64 * i;
      xr[i] = v < Veff ? logits[(long long)b * V + v] : -INFINITY;
    }
    const float lp = token_logprob<NPL>(xr, Veff, smp);
    if (lane == 0) sp.logp[(long long)b * sp.max_steps + step] = lp;
  }
  const bool fin = (smp == EOS) || (amx == EOS);
  const bool early = (rl.early_stop_num != -1 && (step + 1) > rl.early_stop_num) || (step >= rl.max_steps - 1);
  if (lane == 0) {
    if (prev_len < ycap) yrow[prev_len] = smp;
    if (fin || early) {
      active[b] = 0;
      sp.out_len[b] = step;
      atomicSub(n_active, 1);
    } else {
      sp.out_tokens[(long long)b * sp.max_steps + step] = smp;
      if (step > 0) kv_len[b] += 1;
    }
    step_ctr[b] = step + 1;
  }
  if (!(fin || early)) {
    const int tok = min(max(smp, 0), V - 1);
    const float* e = e_audio + (long long)tok * d;
    const float* p = pe + (long long)(P + step) * d;
    for (int c = lane; c < d; c += 64) ybuf[(long long)b * d + c] = e[c] + alpha_a * p[c];
  }
}

template <int NPL>
__global__ __launch_bounds__(64) void sample_only_kernel(const float* __restrict__ logits, int V, int Veff,
                                                         const int* __restrict__ prev, int prev_len, int top_k, float top_p,
                                                         float temperature, float rp, const float* __restrict__ noise,
                                                         unsigned long long seed, int step, int* __restrict__ sampled,
                                                         int* __restrict__ argmax_tok,
                                                         const RowSampling* __restrict__ rows /* [B] or null */) {
  extern __shared__ unsigned char seen[];
  const int b = blockIdx.x;
  int smp, amx;
  if (rows) {
    const RowSampling rs = load_row_sampling(rows, b);
    top_k = rs.top_k; top_p = rs.top_p; temperature = rs.temperature; rp = rs.rep_penalty;
  }
  sample_row<NPL>(logits + (long long)b * V, V, Veff, prev + (long long)b * prev_len, prev_len, top_k, top_p, temperature,
                  rp, noise ? noise + (long long)b * V : nullptr, seed, b, step, seen, &smp, &amx);
  if (threadIdx.x == 0) { sampled[b] = smp; argmax_tok[b] = amx; }
}

// the logits' rows of a batch -> out[b] = token_logprob of tokens[b] (gsv_op_token_logprob): grid = B, block = 64
template <int NPL>
__global__ __launch_bounds__(64) void token_logprob_kernel(const float* __restrict__ logits, int V, int Veff,
                                                           const int* __restrict__ tokens, float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float x[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int v = lane + 64 * i;
    x[i] = v < Veff ? logits[(long long)b * V + v] : -INFINITY;
  }
  const float lp = token_logprob<NPL>(x, Veff, tokens[b]);
  if (lane == 0) out[b] = lp;
}

}  // namespace gsv

// =======================================================================================
// engine
// =======================================================================================
using namespace gsv;
using namespace gsveng;

namespace {

template <typename T, int CB, int NW, int KSL, int KV4>
int launch_dec_gemm_inst(const DecGemmArgs& a, hipStream_t s) {
  constexpr int G = DT<T>::G;
  size_t lds = (size_t)NW * CB * 64 * 16;
  if (KV4 > 0) lds = std::max(lds, (size_t)CB * 16 * (a.K + G) * sizeof(T));
  auto kern = dec_gemm_kernel<T, CB, NW, KSL, KV4>;
  if (lds > 64 * 1024) GSV_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  GSV_LAUNCH(kern, dim3(cdiv(a.N, 16), cdiv(a.B, CB * 16)), dim3(NW * 64), lds, s, a);
  return GSV_OK;
}

// K = NW * KSL with KSL = 128 (64 for the 64-wide test model); LayerNorm prologue needs K = 32*KV4
template <typename T, int CB>
int launch_dec_gemm_cb(const DecGemmArgs& a, bool lnpro, hipStream_t s) {
  const int K = a.K;
#define GSV_DG_CASE(NWV, KSLV, KV4V) return launch_dec_gemm_inst<T, CB, NWV, KSLV, KV4V>(a, s)
  if (lnpro) {
    if (K == 512) GSV_DG_CASE(4, 128, 16);
    if (K == 256) GSV_DG_CASE(2, 128, 8);
    if (K == 128) GSV_DG_CASE(1, 128, 4);
    if (K == 64) GSV_DG_CASE(1, 64, 2);
    if (K == 1024) GSV_DG_CASE(8, 128, 32);
  } else {
    if (K == 2048) GSV_DG_CASE(16, 128, 0);
    if (K == 1024) GSV_DG_CASE(8, 128, 0);
    if (K == 512) GSV_DG_CASE(4, 128, 0);
    if (K == 256) GSV_DG_CASE(2, 128, 0);
    if (K == 128) GSV_DG_CASE(1, 128, 0);
    if (K == 64) GSV_DG_CASE(1, 64, 0);
    if (K == 4096) GSV_DG_CASE(16, 256, 0);
  }
#undef GSV_DG_CASE
  set_error("dec_gemm: unsupported contraction length K=%d (lnpro=%d)", K, (int)lnpro);
  return GSV_ERR_ARG;
}

template <typename T>
int launch_dec_gemm(const DecGemmArgs& a, bool lnpro, hipStream_t s) {
  // narrow outputs (N/16 < 64 workgroups, i.e. the N = 512 projections) are bound by what ONE CU can pull
  // (its weight tile plus the whole X operand): give every 16-row batch block its own workgroup so twice
  // as many CUs share the X traffic (the weight tile is then read once per block, from L2)
  if (!lnpro && a.N / 16 < 64 && a.B > 16) return launch_dec_gemm_cb<T, 1>(a, lnpro, s);
  const int cb = cdiv(a.B, 16);
  if (cb <= 1) return launch_dec_gemm_cb<T, 1>(a, lnpro, s);
  if (cb <= 2) return launch_dec_gemm_cb<T, 2>(a, lnpro, s);
  if (cb <= 4) return launch_dec_gemm_cb<T, 4>(a, lnpro, s);
  if (cb <= 8) return launch_dec_gemm_cb<T, 8>(a, lnpro, s);
  set_error("dec_gemm: batch %d too large", a.B);
  return GSV_ERR_ARG;
}

// one wave samples a row with its logits in registers, NPL per lane (64 * NPL >= V): the instantiation for a vocabulary,
// shared by sample_step_kernel and sample_only_kernel
template <typename F>
int with_npl(int V, F&& f) {
  if (V <= 128) return f(std::integral_constant<int, 2>{});
  if (V <= 1088) return f(std::integral_constant<int, 17>{});
  return f(std::integral_constant<int, 32>{});
}

// The two X-operand forms of the decode GEMMs.  LayerNorm prologue: X = LN(r.ybuf) with gamma / beta (null: plain convert),
// the normalised fp32 rows also go to xres, the residual of the layer's next EPI_RESID; the caller adds the epilogue targets.
DecGemmArgs ln_gemm(const gsv_t2s* h, const RowState& r, const float* gamma, const float* beta, const void* w, const float* bias,
                    int N, int epi) {
  DecGemmArgs a;
  a.yin = r.ybuf; a.gamma = gamma; a.beta = beta; a.xres_out = h->xres;
  a.w = w; a.bias = bias; a.B = r.B; a.K = h->cfg.dim; a.N = N; a.epi = epi;
  return a;
}
// Plain form: ybuf = xin W^T + bias + xres, xin [B][K] in the engine dtype
DecGemmArgs resid_gemm(const gsv_t2s* h, const void* xin, const void* w, const float* bias, int K) {
  DecGemmArgs a;
  a.xin = xin; a.w = w; a.bias = bias; a.B = h->rows.B; a.K = K; a.N = h->cfg.dim; a.epi = EPI_RESID;
  a.out_f = h->rows.ybuf; a.xres = h->xres;
  return a;
}

template <typename T>
int launch_decode_attn(const void* q, const void* kc, const void* vc, const int* kv_len, const int* active, int B, int H, int smax,
                       void* out, hipStream_t s) {
  GSV_LAUNCH((decode_attn_kernel<T, 32>), dim3(H, B), dim3(256), 0, s, (const T*)q, (const T*)kc, (const T*)vc, kv_len, active,
             H, smax, (T*)out);
  return GSV_OK;
}

// the layers of one decode step of h->rows; only_attn: the attention launches alone (gsv_t2s_time_step)
template <typename T>
int launch_decode_layers(gsv_t2s* h, hipStream_t s, bool only_attn) {
  const auto& c = h->cfg;
  const RowState& r = h->rows;
  const int d = c.dim, H = c.n_head;
  for (int li = 0; li < c.n_layer; ++li) {
    const LayerW& L = h->layers[li];
    if (!only_attn) {
      // the previous layer's LN2 is this GEMM's prologue (layer 0: ybuf is the embedding, converted as it is)
      const LayerW* prev = li > 0 ? &h->layers[li - 1] : nullptr;
      DecGemmArgs a = ln_gemm(h, r, prev ? prev->n2w : nullptr, prev ? prev->n2b : nullptr, L.qkv_w, L.qkv_b, 3 * d, EPI_QKV);
      a.out_t = h->qbuf; a.kc = kv_ptr(h, r, li, 0); a.vc = kv_ptr(h, r, li, 1); a.kv_len = r.kv_len(); a.active = r.active();
      a.d = d; a.H = H; a.smax = r.max_seq;
      GSV_RC(launch_dec_gemm<T>(a, true, s));
    }
    GSV_RC(launch_decode_attn<T>(h->qbuf, kv_ptr(h, r, li, 0), kv_ptr(h, r, li, 1), r.kv_len(), r.active(), r.B, H, r.max_seq,
                                 h->abuf, s));
    if (only_attn) continue;
    GSV_RC(launch_dec_gemm<T>(resid_gemm(h, h->abuf, L.out_w, L.out_b, d), false, s));
    DecGemmArgs f1 = ln_gemm(h, r, L.n1w, L.n1b, L.w1, L.b1, c.ffn_dim, EPI_RELU);
    f1.out_t = h->hbuf;
    GSV_RC(launch_dec_gemm<T>(f1, true, s));
    GSV_RC(launch_dec_gemm<T>(resid_gemm(h, h->hbuf, L.w2, L.b2, c.ffn_dim), false, s));
  }
  return GSV_OK;
}

// logits (LN2 prologue of the last layer) + sampling/state update of the rows of r
template <typename T>
int launch_tail(gsv_t2s* h, RowState& r, hipStream_t s) {
  const auto& c = h->cfg;
  const LayerW& L = h->layers[c.n_layer - 1];
  DecGemmArgs a = ln_gemm(h, r, L.n2w, L.n2b, h->pred_w, nullptr, c.vocab, EPI_LOGITS);
  a.xres_out = nullptr;   // no residual follows the last LayerNorm
  a.out_f = r.logits;
  GSV_RC(launch_dec_gemm<T>(a, true, s));
  const int V = c.vocab, EOS = c.vocab - 1;
  return with_npl(V, [&](auto npl) -> int {
    GSV_LAUNCH(sample_step_kernel<decltype(npl)::value>, dim3(r.B), dim3(64), (size_t)((V + 15) & ~15), s, r.logits, V, EOS, r.sp,
               r.ytok, h->ycap, r.kv_len(), r.active(), r.step(), r.n_active(), h->e_audio, h->pe, h->alpha_a, c.dim, r.ybuf);
    return GSV_OK;
  });
}

template <typename T>
int launch_step(gsv_t2s* h, hipStream_t s) {
  GSV_RC(launch_decode_layers<T>(h, s, false));
  return launch_tail<T>(h, h->rows, s);
}

// ---- gsv_t2s_decode in the order it runs: decode_begin, step 0 (launch_tail), then run_chunk: run_mega and / or run_steps, all
// ---- three on h->rows ----

// rows -> the device array dst, unless `up`, the host copy of what dst holds, says that they are there already
template <typename R>
int upload_rows(const std::vector<R>& rows, std::vector<R>& up, void* dst, hipStream_t s) {
  if (rows.size() == up.size() && memcmp(rows.data(), up.data(), rows.size() * sizeof(R)) == 0) return GSV_OK;
  GSV_HIP(hipMemcpyAsync(dst, rows.data(), rows.size() * sizeof(R), hipMemcpyHostToDevice, s));
  up = rows;
  return GSV_OK;
}

// Builds and uploads the call's row tables -- every row's sampling values, limits and counter-RNG key -- and checks that the
// request fits the arena, the position table and the token history.  Returns the step budget (>= 1) or an error code (< 0).
int decode_begin(gsv_t2s* h, const gsv_sampling_params* sp, const float* noise, int noise_rows, int32_t* out_tokens,
                 int32_t* out_len, hipStream_t s) {
  const RowState& r = h->rows;
  const size_t B = (size_t)r.B;
  StepParams p = step_params(sp->max_steps, r, take_outputs(h, out_tokens, out_len));
  p.noise = noise; p.noise_rows = noise ? noise_rows : 0;
  // The tables: what gsv_t2s_set_row_rng / _row_sampling / _row_limits gave for this call, else the call's scalars for every
  // row ((seed, b) for the keys: the draws of a batch without keys).  The setters' vectors stay until gsv_t2s_decode returns.
  const std::vector<gsv_row_sampling_t>& rsn = h->row_sampling_next;
  const std::vector<gsv_row_limits_t>& rln = h->row_limits_next;
  const bool keyed = !h->rng_seed_next.empty();
  const int nkeys = (int)h->rng_seed_next.size();
  std::vector<unsigned long long> seeds(B, (unsigned long long)sp->seed);
  std::vector<int> rows(B);
  for (size_t b = 0; b < B; ++b) rows[b] = (int)b;
  if (keyed && nkeys == r.B) { seeds = h->rng_seed_next; rows = h->rng_row_next; }
  h->rng_seed_next.clear(); h->rng_row_next.clear();
  GSV_REQUIRE(!keyed || nkeys == r.B, "t2s_decode: gsv_t2s_set_row_rng gave %d keys for a batch of %d rows", nkeys, r.B);
  GSV_REQUIRE(rsn.empty() || rsn.size() == B, "t2s_decode: gsv_t2s_set_row_sampling gave %d rows for a batch of %d rows",
              (int)rsn.size(), r.B);
  GSV_REQUIRE(rln.empty() || rln.size() == B, "t2s_decode: gsv_t2s_set_row_limits gave %d rows for a batch of %d rows",
              (int)rln.size(), r.B);
  GSV_RC(check_row_limits_steps("t2s_decode", rln, sp->max_steps));
  const std::vector<gsv_row_sampling_t> sampling = rsn.empty() ? std::vector<gsv_row_sampling_t>(B, sampling_of(*sp)) : rsn;
  const std::vector<gsv_row_limits_t> limits = rln.empty() ? std::vector<gsv_row_limits_t>(B, limits_of(*sp)) : rln;
  // Every row is held to its own budget before anything is uploaded or launched: row b ends at kv0[b] + budget_b - 1 cached
  // positions, and its sampling tail reads pe[P_b + step] and writes token history [P_b + step].  A request that does not fit
  // is refused here: the kernels clamp out-of-range appends, which would otherwise yield silently wrong tokens with rc 0.
  // The launch runs the largest budget.
  int budget = 1;
  for (int b = 0; b < r.B; ++b) {
    const int bb = step_budget(limits[b]);
    budget = bb > budget ? bb : budget;
    GSV_REQUIRE(r.kv0[b] + bb <= r.max_seq,
                "t2s_decode: row %d: %d cached positions + %d steps exceed the K/V arena (max_seq %d); lower max_steps / "
                "early_stop_num (the row's own, if it has limits) or create the engine with a larger max_seq", b, r.kv0[b], bb,
                r.max_seq);
    GSV_REQUIRE(r.pl[b] + bb <= h->pe_rows, "t2s_decode: row %d: prompt %d + %d steps exceed the position table (%d rows)", b,
                r.pl[b], bb, h->pe_rows);
    GSV_REQUIRE(r.pl[b] + bb <= h->ycap, "t2s_decode: row %d: prompt %d + %d steps exceed the token history (%d)", b, r.pl[b], bb,
                h->ycap);
  }
  GSV_RC(upload_rows(sampling, h->row_sampling_up, r.row_sampling, s));
  GSV_RC(upload_rows(limits, h->row_limits_up, r.row_limits, s));
  GSV_RC(upload_rows(seeds, h->rng_seed_up, r.rng_seed, s));
  GSV_RC(upload_rows(rows, h->rng_row_up, r.rng_row, s));
  GSV_HIP(hipMemcpyAsync(r.sp, &p, sizeof(p), hipMemcpyHostToDevice, s));
  GSV_HIP(hipStreamSynchronize(s));
  return budget;
}

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// arguments of the persistent-engine launch that runs steps 1 .. budget - 1; its knobs are read once per process
MegaArgs mega_args(gsv_t2s* h, int budget) {
  static const bool map_local = getenv("GSV_MEGA_GROUP_XCD") != nullptr;
  static const int map_mode = env_int("GSV_MEGA_MAP", 2);   // 2: roles by the XCD a workgroup runs on, 1: by blockIdx % 8
  // bits 0-3: hops A-D poll ONE hint line before the full pass (hop B, 2 KB per row, is faster polled in full: 288 -> 284 us
  // per step); bit 4: sweep2 keeps two polls in flight (measured 3 % slower, left off); bit 7: every member polls ANOTHER
  // publisher's line instead of all 32 polling the row's last line (297 -> 288 us); bits 8-12: 16ths of the lines that may
  // still be missing when sweep2's full passes start (logits hop)
  static const int hint_mask = env_int("GSV_MEGA_HINT", 13 | (1 << 7) | (2 << 8));
  MegaState& m = h->mega;
  const RowState& r = h->rows;
  MegaArgs a;
  memset(&a, 0, sizeof(a));
  a.wpack = (const h8*)m.wpack; a.lpack = (const h8*)m.lpack; a.fpack = m.fpack;
  a.kv = (_Float16*)r.kv; a.kv_layer_stride = r.kv_layer_stride; a.smax = r.max_seq;
  a.kv_len = r.kv_len(); a.active = r.active(); a.step_ctr = r.step(); a.n_active = r.n_active();
  a.ytok = r.ytok; a.ycap = h->ycap; a.sp = r.sp; a.e_audio = h->e_audio; a.pe = h->pe; a.alpha_a = h->alpha_a;
  a.ybuf = r.ybuf; a.logits_out = r.logits; a.hop = m.hop; a.err = m.err; a.B = r.B; a.L = h->cfg.n_layer; a.V = h->cfg.vocab;
  a.nsteps = budget - 1; a.map_shared = map_local ? 0 : map_mode;
  a.hint_mask = hint_mask;
  a.ring = m.ring;
  m.launch_gen = (m.launch_gen + 1) & 2047;
  a.ep_base = m.launch_gen << 20;                       // 1500 steps x 98 hops < 2^20
  a.test_stall = h->dbg_stall; h->dbg_stall = 0;        // tests only (gsv_t2s_debug_stall): this launch loses one publish
  return a;
}

// Measurement runs: GSV_MEGA_PROF=<file> dumps in-kernel shader-clock stamps of one (step, layer) for every wave.
// mega_prof_arm puts the stamp buffer into the launch arguments, mega_prof_dump copies it back, writes the file and frees it.
constexpr size_t MEGA_PROF_N = (size_t)256 * 8 * 32;

int mega_prof_arm(MegaArgs& a, int budget, hipStream_t s) {
  if (!getenv("GSV_MEGA_PROF") || budget <= 8) return GSV_OK;
  GSV_HIP(hipMalloc((void**)&a.prof, MEGA_PROF_N * 8));
  GSV_HIP(hipMemsetAsync(a.prof, 0, MEGA_PROF_N * 8, s));
  a.prof_step = env_int("GSV_MEGA_PROF_STEP", 5);
  a.prof_layer = env_int("GSV_MEGA_PROF_LAYER", 7);
  return GSV_OK;
}

int mega_prof_dump(const MegaArgs& a, float decode_ms) {
  std::vector<unsigned long long> hp(MEGA_PROF_N);
  GSV_HIP(hipMemcpy(hp.data(), a.prof, MEGA_PROF_N * 8, hipMemcpyDeviceToHost));
  (void)hipFree(a.prof);
  if (FILE* f = fopen(getenv("GSV_MEGA_PROF"), "w")) {
    fprintf(f, "# decode %.3f ms for %d steps; stamps of step %d layer %d: wg wave stamp0 then deltas to stamp0\n", decode_ms,
            a.nsteps, a.prof_step, a.prof_layer);
    for (int wg = 0; wg < 256; ++wg)
      for (int w = 0; w < 8; ++w) {
        const unsigned long long* p = &hp[((size_t)wg * 8 + w) * 32];
        if (!p[0]) continue;
        fprintf(f, "%d %d %llu", wg, w, p[0]);
        for (int i = 1; i < 24; ++i) fprintf(f, " %lld", p[i] ? (long long)(p[i] - p[0]) : -1ll);
        fprintf(f, "\n");
      }
    fclose(f);
  }
  return GSV_OK;
}

// Steps 1 .. budget - 1 on the persistent engine.  MEGA_DONE: every row is finished; MEGA_FELL_BACK: the engine cannot run on
// this device, or a hand-off timed out and the row state is again what step 0 left -- the caller continues on the launch
// path; < 0: error.
enum { MEGA_DONE = 0, MEGA_FELL_BACK = 1 };

int run_mega(gsv_t2s* h, int budget, int32_t* out_len, hipStream_t s) {
  MegaState& m = h->mega;
  if (m.census < 0) {
    // once per handle: are the engine's 256 workgroups co-resident on this device?  If not, a hand-off could wait
    // for a workgroup that never starts: the launch-per-phase step is used instead (gsv_t2s_decode_info reports it)
    const int rc = mega_census(s, m.err, m.h_err);
    if (rc < 0) return rc;
    m.census = rc;
  }
  if (m.census != 1) return MEGA_FELL_BACK;
  GSV_HIP(hipMemsetAsync(m.hop, 0, m.hop_bytes, s));      // no tag survives a call (epochs are unique per launch as well: ep_base)
  GSV_HIP(hipMemsetAsync(m.err, 0, 64, s));
  // the row state as step 0 left it: if the launch ends in a hand-off timeout the batch is re-run from here on the
  // launch-per-phase path (the engine only appends K/V behind kv_len and token history behind P_b + step: restoring the
  // counters makes both invisible again; ybuf, the first step's input, is read-only for the engine; P_b and the RNG keys
  // are read-only during a decode call)
  const RowState& r = h->rows;
  const size_t ns = r.state_ints();
  GSV_HIP(hipMemcpyAsync(m.snap, r.state, ns * 4, hipMemcpyDeviceToDevice, s));
  GSV_HIP(hipMemcpyAsync(m.snap + ns, out_len, r.B * 4, hipMemcpyDeviceToDevice, s));
  MegaArgs a = mega_args(h, budget);
  GSV_RC(mega_prof_arm(a, budget, s));
  GSV_HIP(hipEventRecord(h->mega_ev[0], s));
  GSV_RC(launch_t2s_mega(a, h->logp_on, s));
  GSV_HIP(hipEventRecord(h->mega_ev[1], s));
  GSV_HIP(hipMemcpyAsync(m.h_err, m.err, 16, hipMemcpyDeviceToHost, s));
  GSV_HIP(hipMemcpyAsync(h->h_pinned, r.step(), 4, hipMemcpyDeviceToHost, s));
  GSV_HIP(hipStreamSynchronize(s));
  if (m.h_err[0] != 0u) {
    // A hand-off timed out (a member was not running: another kernel held its CU, or a fault).  The request is not
    // failed: the row state is restored to what step 0 left and THIS batch is re-run by the caller on the launch-per-phase
    // path.  A transient cause (a foreign kernel held a CU) is given another chance: census again at the next call; three
    // strikes disable the engine for the handle (census = 0, gsv_t2s_engine_stats reports it).
    // GSV_MEGA_STRICT=1 restores the old behaviour (GSV_ERR_STATE) for tests of the error path.
    set_error("t2s_decode: persistent engine hand-off timed out (epoch %u, workgroup %u, hop code 0x%x); the handle now uses "
              "the launch-per-phase step (GSV_T2S_NO_MEGA=1 selects it from the start)", m.h_err[1], m.h_err[2], m.h_err[3]);
    m.fallbacks += 1;
    m.census = m.fallbacks >= 3 ? 0 : -1;
    m.last_err[0] = m.h_err[1]; m.last_err[1] = m.h_err[2]; m.last_err[2] = m.h_err[3];
    if (a.prof) (void)hipFree(a.prof);
    if (getenv("GSV_MEGA_STRICT")) return GSV_ERR_STATE;
    GSV_HIP(hipMemcpyAsync(r.state, m.snap, ns * 4, hipMemcpyDeviceToDevice, s));
    GSV_HIP(hipMemcpyAsync(out_len, m.snap + ns, r.B * 4, hipMemcpyDeviceToDevice, s));
    return MEGA_FELL_BACK;
  }
  (void)hipEventElapsedTime(&h->last_decode_ms, h->mega_ev[0], h->mega_ev[1]);
  if (a.prof) GSV_RC(mega_prof_dump(a, h->last_decode_ms));
  // every row ends by the budget's last step (early == step >= max_steps - 1); row 0's step counter tells how
  // far the longest-running group got only for its own group, so report the budget like the launch loop does
  h->last_decode_mode = 1; h->last_decode_steps = budget - 1;
  return MEGA_DONE;
}

// Steps 1 .. budget - 1 one launch-per-phase step at a time: captured once per batch size and replayed; n_active is polled
// every 8 steps so a batch whose rows have all finished stops early.  Returns the steps run, step 0 included, in *steps_run.
template <typename T>
int run_steps(gsv_t2s* h, int budget, int* steps_run, hipStream_t s) {
  const int B = h->rows.B;
  hipGraphExec_t exec = nullptr;
  auto it = h->graphs.find(B);
  if (it != h->graphs.end()) exec = it->second;
  else if (s != nullptr && !getenv("GSV_T2S_NO_GRAPH") && hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    hipGraph_t graph;
    int rc = launch_step<T>(h, s);
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc) return rc;
    GSV_HIP(e);
    GSV_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    h->graphs[B] = exec;
  } else {
    (void)hipGetLastError();  // legacy default stream cannot capture: eager launches instead
  }
  const int check_every = 8;
  int steps = 1;
  while (steps < budget) {
    if (exec) GSV_HIP(hipGraphLaunch(exec, s));
    else GSV_RC(launch_step<T>(h, s));
    ++steps;
    if (steps % check_every == 0 || steps == budget) {
      GSV_HIP(hipMemcpyAsync(h->h_pinned, h->rows.n_active(), 4, hipMemcpyDeviceToHost, s));
      GSV_HIP(hipStreamSynchronize(s));
      if (h->h_pinned[0] <= 0) break;
    }
  }
  GSV_HIP(hipStreamSynchronize(s));
  if (steps_run) *steps_run = steps;
  return GSV_OK;
}

int decode(gsv_t2s* h, const gsv_sampling_params* sp, const float* noise, int noise_rows, int32_t* out_tokens, int32_t* out_len,
           int* steps_run, hipStream_t s) {
  const int budget = decode_begin(h, sp, noise, noise_rows, out_tokens, out_len, s);
  if (budget < 0) return budget;
  GSV_RC(t2s_step0_tail(h, h->rows, s));
  h->last_decode_mode = 0; h->last_decode_ms = 0.f; h->last_decode_steps = 0;
  return run_chunk(h, budget, out_len, steps_run, s);
}

// gsv_t2s_time_step: in-situ timing of the launch-per-phase step at the current cache state.  (a) The full per-layer kernel
// sequence (QKV+append, attention, out-proj, FFN1, FFN2) is launched eagerly on the stream, 2 warm-up passes and then
// `iters` passes between one event pair.  Rows are forced active for the measurement (finished rows skip attention) and
// restored afterwards; no row state advances because the sampling tail is not launched.
template <typename T>
int time_step(gsv_t2s* h, int iters, float* step_ms, float* attn_ms, hipStream_t s) {
  const int L = h->cfg.n_layer, B = h->rows.B;
  int* d_active = h->rows.active();
  std::vector<int> saved(B), ones(B, 1);
  GSV_HIP(hipMemcpy(saved.data(), d_active, B * 4, hipMemcpyDeviceToHost));
  GSV_HIP(hipMemcpy(d_active, ones.data(), B * 4, hipMemcpyHostToDevice));
  hipEvent_t ev[4];
  for (auto& e : ev) GSV_HIP(hipEventCreate(&e));
  int rc = GSV_OK;
  for (int w = 0; w < 2 && !rc; ++w) rc = launch_decode_layers<T>(h, s, false);
  GSV_HIP(hipEventRecord(ev[2], s));
  for (int i = 0; i < iters && !rc; ++i) rc = launch_decode_layers<T>(h, s, false);
  GSV_HIP(hipEventRecord(ev[3], s));
  GSV_HIP(hipStreamSynchronize(s));
  // (b) the attention kernel alone: iters x L launches back to back between ONE event pair (an event pair
  // per launch adds ~3 us of its own); the L layers' arenas are distinct memory (L x bytes > Infinity Cache
  // at the benchmark shape), so every launch streams its K/V from HBM like it does inside a step
  float attn_total = 0.f;
  if (!rc) {
    GSV_HIP(hipEventRecord(ev[0], s));
    for (int i = 0; i < iters && !rc; ++i) rc = launch_decode_layers<T>(h, s, true);
    GSV_HIP(hipEventRecord(ev[1], s));
    GSV_HIP(hipStreamSynchronize(s));
    if (!rc) GSV_HIP(hipEventElapsedTime(&attn_total, ev[0], ev[1]));
  }
  GSV_HIP(hipMemcpy(d_active, saved.data(), B * 4, hipMemcpyHostToDevice));
  if (!rc) {
    if (attn_ms) *attn_ms = attn_total / (float)(iters * L);
    float ms = 0.f;
    GSV_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
    if (step_ms) *step_ms = ms / iters;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

}  // namespace

int t2s_step0_tail(gsv_t2s* h, RowState& r, hipStream_t s) { return GSV_WITH_T(h, launch_tail<T>(h, r, s)); }

int run_chunk(gsv_t2s* h, int budget, int32_t* out_len, int* steps_run, hipStream_t s) {
  if (h->mega.ready && h->mega_on && h->rows.B <= MEGA_MAX_B && budget > 1) {
    const int r = run_mega(h, budget, out_len, s);
    if (r < 0) return r;
    if (r == MEGA_DONE) {
      if (steps_run) *steps_run = budget;
      return GSV_OK;
    }
  }
  return GSV_WITH_T(h, run_steps<T>(h, budget, steps_run, s));   // also after MEGA_FELL_BACK: the snapshot is back
}

int check_row_limits_steps(const char* who, const std::vector<gsv_row_limits_t>& rows, int max_steps) {
  for (size_t b = 0; b < rows.size(); ++b)
    GSV_REQUIRE(rows[b].max_steps <= max_steps, "%s: row %d: its limits' max_steps %d exceed the call's %d", who, (int)b,
                rows[b].max_steps, max_steps);
  return GSV_OK;
}

int check_row_sampling(const char* who, const gsv_row_sampling_t* rows, int B) {
  for (int b = 0; b < B; ++b) {
    const gsv_row_sampling_t& r = rows[b];
    GSV_REQUIRE(r.top_k >= 0, "%s: row %d: top_k %d must be >= 0", who, b, r.top_k);
    GSV_REQUIRE(r.top_p > 0.f && r.top_p <= 1.f, "%s: row %d: top_p %g must be in (0, 1]", who, b, (double)r.top_p);
    GSV_REQUIRE(isfinite(r.temperature) && r.temperature >= 0.f, "%s: row %d: temperature %g must be finite and >= 0", who,
                b, (double)r.temperature);
    GSV_REQUIRE(isfinite(r.repetition_penalty) && r.repetition_penalty > 0.f,
                "%s: row %d: repetition_penalty %g must be finite and > 0", who, b, (double)r.repetition_penalty);
  }
  return GSV_OK;
}

int check_rng_rows(const char* who, const int32_t* rows, int B) {
  for (int b = 0; b < B; ++b)
    GSV_REQUIRE(rows[b] >= 0 && rows[b] < (1 << 24), "%s: row %d: RNG row %d must be in [0, 2^24)", who, b, rows[b]);
  return GSV_OK;
}

extern "C" {

int gsv_t2s_create(const gsv_t2s_config* cfg, int dtype, int max_batch, int max_seq, gsv_t2s_t** out) {
  GSV_REQUIRE(cfg && out, "t2s_create: null argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "t2s_create: bad dtype");
  GSV_REQUIRE((cfg->dim == 64 || cfg->dim == 128 || cfg->dim == 256 || cfg->dim == 512 || cfg->dim == 1024) && cfg->ffn_dim == 4 * cfg->dim,
              "t2s_create: dim must be 64/128/256/512/1024 with ffn_dim = 4*dim (got %d, %d)", cfg->dim, cfg->ffn_dim);
  GSV_REQUIRE(cfg->dim / cfg->n_head == 32, "t2s_create: head_dim must be 32 (got %d)", cfg->dim / cfg->n_head);
  GSV_REQUIRE(cfg->vocab <= 2048, "t2s_create: vocab %d > 2048", cfg->vocab);
  GSV_REQUIRE(max_batch >= 1 && max_batch <= (dtype == GSV_F32 ? 64 : 128), "t2s_create: max_batch %d out of range", max_batch);
  GSV_RC(require_device());
  gsv_t2s* h = new gsv_t2s();
  h->cfg = *cfg;
  h->dtype = dtype;
  h->max_batch = max_batch;
  h->rows.max_seq = max_seq; h->rows.mb = max_batch;
  h->layers.resize(cfg->n_layer);
  *out = h;
  return GSV_OK;
}

void gsv_t2s_destroy(gsv_t2s_t* h) {
  if (!h) return;
  for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.second);
  free_ctx(h);
  if (h->h_pinned) (void)hipHostFree(h->h_pinned);
  if (h->mega.h_err) (void)hipHostFree(h->mega.h_err);
  for (auto& e : h->mega_ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ses.ev) if (e) (void)hipEventDestroy(e);
  delete h;
}

int gsv_t2s_load_tensor(gsv_t2s_t* h, const char* name, const float* data, int64_t numel) {
  if (name && strncmp(name, "model.", 6) == 0) name += 6;
  return stage_tensor(h, name, data, numel);
}

int gsv_t2s_finalize(gsv_t2s_t* h) {
  GSV_REQUIRE(h && !h->finalized, "t2s_finalize: bad handle");
  const auto& c = h->cfg;
  const size_t d = c.dim, ff = c.ffn_dim, V = c.vocab, PV = c.phoneme_vocab, BD = c.bert_dim;
  GSV_RC(make_mat(h, "bert_proj.weight", d * BD, &h->bert_w));
  GSV_RC(make_vec(h, "bert_proj.bias", d, &h->bert_b));
  GSV_RC(make_vec(h, "ar_text_embedding.word_embeddings.weight", PV * d, &h->e_text));
  GSV_RC(make_vec(h, "ar_audio_embedding.word_embeddings.weight", V * d, &h->e_audio));
  {
    std::vector<float> a;
    if (!fetch(h, "ar_text_position.alpha", 1, 1, a)) return GSV_ERR_ARG;
    h->alpha_t = a[0];
    if (!fetch(h, "ar_audio_position.alpha", 1, 1, a)) return GSV_ERR_ARG;
    h->alpha_a = a[0];
  }
  {
    auto it = h->staged.find("pe");
    GSV_REQUIRE(it != h->staged.end() && it->second.size() % d == 0, "t2s: missing sinusoid table 'pe' [n_pos][dim]");
    h->pe_rows = (int)(it->second.size() / d);
    GSV_REQUIRE(h->rows.max_seq <= h->pe_rows, "t2s: max_seq %d exceeds the position table (%d rows)", h->rows.max_seq, h->pe_rows);
    GSV_RC(up_f32(h, it->second.data(), it->second.size(), &h->pe));
  }
  GSV_RC(make_mat(h, "ar_predict_layer.weight", V * d, &h->pred_w));
  for (int i = 0; i < c.n_layer; ++i) {
    std::string p = "h.layers." + std::to_string(i) + ".";
    LayerW& L = h->layers[i];
    GSV_RC(make_mat(h, p + "self_attn.in_proj_weight", 3 * d * d, &L.qkv_w));
    GSV_RC(make_vec(h, p + "self_attn.in_proj_bias", 3 * d, &L.qkv_b));
    GSV_RC(make_mat(h, p + "self_attn.out_proj.weight", d * d, &L.out_w));
    GSV_RC(make_vec(h, p + "self_attn.out_proj.bias", d, &L.out_b));
    GSV_RC(make_mat(h, p + "linear1.weight", ff * d, &L.w1));
    GSV_RC(make_vec(h, p + "linear1.bias", ff, &L.b1));
    GSV_RC(make_mat(h, p + "linear2.weight", d * ff, &L.w2));
    GSV_RC(make_vec(h, p + "linear2.bias", d, &L.b2));
    GSV_RC(make_vec(h, p + "norm1.weight", d, &L.n1w));
    GSV_RC(make_vec(h, p + "norm1.bias", d, &L.n1b));
    GSV_RC(make_vec(h, p + "norm2.weight", d, &L.n2w));
    GSV_RC(make_vec(h, p + "norm2.bias", d, &L.n2b));
  }
  if (h->dtype == GSV_F16 && mega_shape_ok(c.dim, c.n_head, c.ffn_dim, c.vocab) && !getenv("GSV_T2S_NO_MEGA")) {
    // second copy of the decoder weights in the persistent engine's load order (every wave load = 1 KiB contiguous)
    MegaState& m = h->mega;
    const size_t lh = mega_layer_pack_halfs(), gh = mega_logits_pack_halfs();
    GSV_RC(dalloc(h, &m.wpack, (size_t)c.n_layer * lh * 2));
    GSV_RC(dalloc(h, &m.lpack, gh * 2));
    std::vector<_Float16> tmp(std::max(lh, gh));
    for (int i = 0; i < c.n_layer; ++i) {
      std::string p = "h.layers." + std::to_string(i) + ".";
      mega_pack_layer(h->staged[p + "self_attn.in_proj_weight"].data(), h->staged[p + "self_attn.out_proj.weight"].data(),
                      h->staged[p + "linear1.weight"].data(), h->staged[p + "linear2.weight"].data(), tmp.data());
      GSV_HIP(hipMemcpy((char*)m.wpack + (size_t)i * lh * 2, tmp.data(), lh * 2, hipMemcpyHostToDevice));
    }
    mega_pack_logits(h->staged["ar_predict_layer.weight"].data(), c.vocab, tmp.data());
    GSV_HIP(hipMemcpy(m.lpack, tmp.data(), gh * 2, hipMemcpyHostToDevice));
    // fp32 parameters of a layer side by side (no pointer chasing inside the kernel)
    GSV_RC(dalloc(h, (void**)&m.fpack, (size_t)c.n_layer * MEGA_FP_LAYER * 4));
    for (int i = 0; i < c.n_layer; ++i) {
      const LayerW& L = h->layers[i];
      float* dst = m.fpack + (size_t)i * MEGA_FP_LAYER;
      const float* srcs[8] = {L.qkv_b, L.out_b, L.b1, L.b2, L.n1w, L.n1b, L.n2w, L.n2b};
      const size_t ns[8] = {3 * d, d, ff, d, d, d, d, d};
      for (int k = 0; k < 8; ++k) {
        GSV_HIP(hipMemcpy(dst, srcs[k], ns[k] * 4, hipMemcpyDeviceToDevice));
        dst += ns[k];
      }
    }
    m.ring = 1;                                            // one hop buffer set (t2s_mega.hip hop_slot)
    m.hop_bytes = mega_hop_bytes(m.ring);
    GSV_RC(dalloc(h, (void**)&m.hop, m.hop_bytes));
    GSV_RC(dalloc(h, (void**)&m.err, 64));
    GSV_RC(dalloc(h, (void**)&m.snap, ((size_t)4 * h->max_batch + 4) * 4));
    GSV_HIP(hipHostMalloc((void**)&m.h_err, 64));
    GSV_HIP(hipEventCreate(&h->mega_ev[0]));
    GSV_HIP(hipEventCreate(&h->mega_ev[1]));
    m.ready = true;
  }
  h->staged.clear();
  const size_t B = h->max_batch, es = esz(h);
  RowState& r = h->rows;   // max_seq and mb are gsv_t2s_create's
  r.kv_layer_stride = B * d * (size_t)r.max_seq;
  GSV_RC(dalloc(h, &r.kv, (size_t)c.n_layer * 2 * r.kv_layer_stride * es));
  GSV_RC(dalloc(h, (void**)&h->d_x_len, B * 4));
  GSV_RC(dalloc(h, (void**)&h->d_row_off, B * 4));
  GSV_RC(dalloc(h, (void**)&h->d_ph_off, B * 4));
  GSV_RC(dalloc(h, (void**)&r.state, r.state_ints() * 4));
  h->ycap = r.max_seq + 8;
  GSV_RC(dalloc(h, (void**)&r.ytok, B * h->ycap * 4));
  GSV_RC(dalloc(h, (void**)&r.plen, 2 * B * 4));
  GSV_RC(dalloc(h, (void**)&r.rng_seed, B * 8));
  GSV_RC(dalloc(h, (void**)&r.rng_row, B * 4));
  GSV_RC(dalloc(h, (void**)&r.row_sampling, B * sizeof(RowSampling)));
  GSV_RC(dalloc(h, (void**)&r.row_limits, B * sizeof(RowLimits)));
  GSV_RC(dalloc(h, (void**)&r.sp, sizeof(StepParams)));
  GSV_HIP(hipHostMalloc((void**)&h->h_pinned, 64));
  GSV_RC(dalloc(h, (void**)&r.ybuf, B * d * 4));
  GSV_RC(dalloc(h, (void**)&h->xres, B * d * 4));
  GSV_RC(dalloc(h, (void**)&r.logits, B * V * 4));
  GSV_RC(dalloc(h, &h->qbuf, B * d * es));
  GSV_RC(dalloc(h, &h->abuf, B * d * es));
  GSV_RC(dalloc(h, &h->hbuf, B * ff * es));
  GSV_HIP(hipMemset(r.logits, 0, B * V * 4));
  h->finalized = true;
  return GSV_OK;
}

int gsv_t2s_set_row_rng(gsv_t2s_t* h, const uint64_t* seeds, const int32_t* rows, int B) {
  GSV_REQUIRE(h && h->finalized, "t2s_set_row_rng: handle not finalized");
  GSV_REQUIRE(seeds && rows && B >= 1 && B <= h->max_batch, "t2s_set_row_rng: bad argument (B = %d)", B);
  GSV_RC(check_rng_rows("t2s_set_row_rng", rows, B));
  h->rng_seed_next.assign(seeds, seeds + B);
  h->rng_row_next.assign(rows, rows + B);
  return GSV_OK;
}

int gsv_t2s_set_row_sampling(gsv_t2s_t* h, const gsv_row_sampling_t* rows, int B) {
  GSV_REQUIRE(h && h->finalized, "t2s_set_row_sampling: handle not finalized");
  GSV_REQUIRE(rows && B >= 1 && B <= h->max_batch, "t2s_set_row_sampling: bad argument (B = %d)", B);
  GSV_RC(check_row_sampling("t2s_set_row_sampling", rows, B));
  h->row_sampling_next.assign(rows, rows + B);
  return GSV_OK;
}

int gsv_t2s_set_row_limits(gsv_t2s_t* h, const gsv_row_limits_t* rows, int B) {
  GSV_REQUIRE(h && h->finalized, "t2s_set_row_limits: handle not finalized");
  GSV_REQUIRE(rows && B >= 1 && B <= h->max_batch, "t2s_set_row_limits: bad argument (B = %d)", B);
  for (int b = 0; b < B; ++b) {
    const gsv_row_limits_t& r = rows[b];
    GSV_REQUIRE(r.eos_mask_steps >= 0, "t2s_set_row_limits: row %d: eos_mask_steps %d must be >= 0", b, r.eos_mask_steps);
    GSV_REQUIRE(r.early_stop_num >= -1, "t2s_set_row_limits: row %d: early_stop_num %d must be >= -1", b, r.early_stop_num);
    GSV_REQUIRE(r.max_steps >= 1, "t2s_set_row_limits: row %d: max_steps %d must be >= 1", b, r.max_steps);
    GSV_REQUIRE(r.reserved == 0, "t2s_set_row_limits: row %d: reserved must be 0", b);
  }
  if (h->ses.open)
    GSV_RC(check_row_limits_steps("t2s_set_row_limits", std::vector<gsv_row_limits_t>(rows, rows + B), h->ses.sp.max_steps));
  h->row_limits_next.assign(rows, rows + B);
  return GSV_OK;
}

int gsv_t2s_decode(gsv_t2s_t* h, const gsv_sampling_params* sp, const float* noise, int noise_rows,
                   int32_t* out_tokens, int32_t* out_len, int* steps_run, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized, "t2s_decode: handle not finalized");
  GSV_T2S_NO_SESSION(h, "t2s_decode");
  GSV_REQUIRE(h->rows.B > 0, "t2s_decode: call gsv_t2s_prefill first");
  // the per-row sampling parameters and limits are this call's alone, whatever becomes of it
  struct Clear { gsv_t2s_t* h; ~Clear() { h->row_sampling_next.clear(); h->row_limits_next.clear(); } } clear{h};
  GSV_REQUIRE(sp && out_tokens && out_len, "t2s_decode: null argument");
  GSV_REQUIRE(sp->max_steps >= 1, "t2s_decode: max_steps must be >= 1");
  GSV_REQUIRE(noise == nullptr || noise_rows == 1 || noise_rows == h->rows.B, "t2s_decode: noise_rows must be 1 or B");
  return decode(h, sp, noise, noise_rows, out_tokens, out_len, steps_run, (hipStream_t)stream);
}

int gsv_t2s_set_mega(gsv_t2s_t* h, int on) {
  GSV_REQUIRE(h, "t2s_set_mega: null handle");
  h->mega_on = on != 0;
  return GSV_OK;
}

int gsv_t2s_debug_kv(gsv_t2s_t* h, int layer, int which, int row, int n_pos, void* out) {
  GSV_REQUIRE(h && h->finalized && out, "t2s_debug_kv: null argument or handle not finalized");
  GSV_REQUIRE(layer >= 0 && layer < h->cfg.n_layer && (which == 0 || which == 1) && row >= 0 && row < h->max_batch && n_pos >= 1 &&
                  n_pos <= h->rows.max_seq, "t2s_debug_kv: layer %d / which %d / row %d / n_pos %d outside the arena", layer, which, row, n_pos);
  const size_t es = esz(h), H = h->cfg.n_head, pitch = (size_t)h->rows.max_seq * 32 * es;
  GSV_HIP(hipDeviceSynchronize());
  GSV_HIP(hipMemcpy2D(out, (size_t)n_pos * 32 * es, (const char*)kv_ptr(h, h->rows, layer, which) + (size_t)row * H * pitch, pitch,
                      (size_t)n_pos * 32 * es, H, hipMemcpyDeviceToHost));
  return GSV_OK;
}

int gsv_t2s_set_prefill_gemm(gsv_t2s_t* h, int mode) {
  GSV_REQUIRE(h, "t2s_set_prefill_gemm: null handle");
  GSV_REQUIRE(mode >= 0 && mode <= 2, "t2s_set_prefill_gemm: mode %d (0 dispatcher, 1 panel, 2 panel from the threshold)", mode);
  h->prefill_gemm = mode;
  return GSV_OK;
}

int gsv_t2s_set_debug(gsv_t2s_t* h, const int32_t* force_tokens, float* logits_dump, int32_t* drawn_dump) {
  GSV_REQUIRE(h && h->finalized, "t2s_set_debug: handle not finalized");
  h->next.force = force_tokens; h->next.dump = logits_dump; h->next.drawn = drawn_dump;
  return GSV_OK;
}

int gsv_t2s_set_logprobs(gsv_t2s_t* h, float* out_logp) {
  GSV_REQUIRE(h && h->finalized, "t2s_set_logprobs: handle not finalized");
  h->next.logp = out_logp;
  return GSV_OK;
}

int gsv_t2s_debug_stall(gsv_t2s_t* h, int member) {
  GSV_REQUIRE(h && h->finalized && member >= 0 && member < 32, "t2s_debug_stall: bad argument");
  h->dbg_stall = member + 1;
  return GSV_OK;
}

int gsv_t2s_engine_stats(gsv_t2s_t* h, int* engine_available, int* fallbacks, unsigned* last_error3) {
  GSV_REQUIRE(h && h->finalized, "t2s_engine_stats: handle not finalized");
  if (engine_available) *engine_available = h->mega.ready && h->mega.census != 0 ? 1 : 0;
  if (fallbacks) *fallbacks = h->mega.fallbacks;
  if (last_error3) { last_error3[0] = h->mega.last_err[0]; last_error3[1] = h->mega.last_err[1]; last_error3[2] = h->mega.last_err[2]; }
  return GSV_OK;
}

int gsv_t2s_decode_info(gsv_t2s_t* h, int* mode, float* device_ms, int* steps) {
  GSV_REQUIRE(h && h->finalized, "t2s_decode_info: handle not finalized");
  if (mode) *mode = h->last_decode_mode;
  if (device_ms) *device_ms = h->last_decode_ms;
  if (steps) *steps = h->last_decode_steps;
  return GSV_OK;
}

int gsv_t2s_debug_logits(gsv_t2s_t* h, float* out, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized && out && h->rows.B > 0, "t2s_debug_logits: bad state");
  GSV_HIP(hipMemcpyAsync(out, h->rows.logits, (size_t)h->rows.B * h->cfg.vocab * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return GSV_OK;
}

int64_t gsv_t2s_step_bytes(gsv_t2s_t* h, int64_t* attn_bytes) {
  if (!h || !h->finalized) return 0;
  const auto& c = h->cfg;
  const int64_t es = (int64_t)esz(h), d = c.dim, ff = c.ffn_dim;
  const int B = h->rows.B;
  std::vector<int> kvl(B > 0 ? B : 1, 0);
  int64_t keys = 0;
  if (B > 0) {
    (void)hipMemcpy(kvl.data(), h->rows.kv_len(), B * 4, hipMemcpyDeviceToHost);
    for (int b = 0; b < B; ++b) keys += kvl[b] + 1;
  }
  // per cached key and layer: K and V rows of d elements
  const int64_t attn = keys * 2 * d * es;              // one layer's launch
  const int64_t weights = ((int64_t)c.n_layer * (3 * d * d + d * d + 2 * d * ff) + (int64_t)c.vocab * d) * es;
  if (attn_bytes) *attn_bytes = attn;
  return weights + attn * c.n_layer + (int64_t)B * 2 * d * es * c.n_layer;
}

int gsv_t2s_time_step(gsv_t2s_t* h, int iters, float* step_ms, float* attn_ms, gsv_stream_t stream) {
  GSV_REQUIRE(h && h->finalized && h->rows.B > 0 && iters > 0, "t2s_time_step: bad state");
  return GSV_WITH_T(h, time_step<T>(h, iters, step_ms, attn_ms, (hipStream_t)stream));
}

int gsv_t2s_debug_set_state(gsv_t2s_t* h, int B, int kv_len) {
  // measurement hook: pretend B rows hold kv_len cached positions each (cache contents are whatever the
  // arena holds); used by tools/attn_sweep.py to time the decode-attention kernel at other (B, S) points
  GSV_REQUIRE(h && h->finalized, "t2s_debug_set_state: handle not finalized");
  RowState& r = h->rows;
  GSV_REQUIRE(B >= 1 && B <= h->max_batch && kv_len >= 1 && kv_len + 2 <= r.max_seq, "t2s_debug_set_state: out of range");
  std::vector<int> kv(B, kv_len), zero(B, 0), plen(B, r.P);
  GSV_HIP(hipMemcpy(r.kv_len(), kv.data(), B * 4, hipMemcpyHostToDevice));
  GSV_HIP(hipMemcpy(r.plen, plen.data(), B * 4, hipMemcpyHostToDevice));   // every row: the last prefill's longest prompt
  GSV_HIP(hipMemcpy(r.active(), zero.data(), B * 4, hipMemcpyHostToDevice));
  GSV_HIP(hipMemset(r.ybuf, 0, (size_t)B * h->cfg.dim * 4));
  GSV_HIP(hipMemset(r.kv, 0, (size_t)h->cfg.n_layer * 2 * r.kv_layer_stride * esz(h)));
  r.B = B; r.kv0.assign(B, kv_len); r.pl.assign(B, r.P);
  return GSV_OK;
}

int gsv_op_decode_attn(const void* q, const void* kc, const void* vc, const int32_t* kv_len, const int32_t* active, int B, int H,
                       int smax, int dtype, void* out, gsv_stream_t stream) {
  GSV_REQUIRE(q && kc && vc && kv_len && active && out, "op_decode_attn: null pointer");
  GSV_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && smax >= 1, "op_decode_attn: bad shape B=%d H=%d smax=%d", B, H, smax);
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_decode_attn: bad dtype %d", dtype);
  return GSV_WITH_DTYPE(dtype, launch_decode_attn<T>(q, kc, vc, kv_len, active, B, H, smax, out, (hipStream_t)stream));
}

int gsv_op_sample(const float* logits, int B, int vocab, int vocab_eff, const int32_t* prev, int prev_len,
                  const gsv_sampling_params* sp, const float* noise, int step, int32_t* sampled, int32_t* argmax_tok,
                  gsv_stream_t stream) {
  GSV_REQUIRE(logits && sp && sampled && argmax_tok && B > 0, "op_sample: null argument");
  GSV_REQUIRE(vocab <= 2048 && vocab_eff <= vocab, "op_sample: vocab too large");
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)((vocab + 15) & ~15);
  return with_npl(vocab, [&](auto npl) -> int {
    GSV_LAUNCH(sample_only_kernel<decltype(npl)::value>, dim3(B), dim3(64), lds, s, logits, vocab, vocab_eff, prev, prev_len,
               sp->top_k, sp->top_p, sp->temperature, sp->repetition_penalty, noise, (unsigned long long)sp->seed, step, sampled,
               argmax_tok, (const RowSampling*)nullptr);
    return GSV_OK;
  });
}

int gsv_op_token_logprob(const float* logits, int B, int vocab, int vocab_eff, const int32_t* tokens, float* out,
                         gsv_stream_t stream) {
  GSV_REQUIRE(logits && tokens && out && B > 0, "op_token_logprob: null argument");
  GSV_REQUIRE(vocab >= 1 && vocab <= 2048 && vocab_eff >= 1 && vocab_eff <= vocab, "op_token_logprob: bad vocab %d / %d", vocab,
              vocab_eff);
  return with_npl(vocab, [&](auto npl) -> int {
    GSV_LAUNCH(token_logprob_kernel<decltype(npl)::value>, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, vocab, vocab_eff,
               tokens, out);
    return GSV_OK;
  });
}

int gsv_op_sample_rows(const float* logits, int B, int vocab, int vocab_eff, const int32_t* prev, int prev_len,
                       const gsv_row_sampling_t* rows, uint64_t seed, const float* noise, int step, int32_t* sampled,
                       int32_t* argmax_tok, gsv_stream_t stream) {
  GSV_REQUIRE(logits && rows && sampled && argmax_tok && B > 0, "op_sample_rows: null argument");
  GSV_REQUIRE(vocab <= 2048 && vocab_eff <= vocab, "op_sample_rows: vocab too large");
  GSV_RC(check_row_sampling("op_sample_rows", rows, B));
  hipStream_t s = (hipStream_t)stream;
  // a test hook, not a hot path: the rows travel through a scratch array and the call waits for the kernel
  RowSampling* d_rows = nullptr;
  GSV_HIP(hipMalloc((void**)&d_rows, (size_t)B * sizeof(RowSampling)));
  int rc = hipMemcpy(d_rows, rows, (size_t)B * sizeof(RowSampling), hipMemcpyHostToDevice) == hipSuccess ? GSV_OK : GSV_ERR_HIP;
  if (rc) set_error("op_sample_rows: upload of the rows failed");
  const size_t lds = (size_t)((vocab + 15) & ~15);
  if (!rc)
    rc = with_npl(vocab, [&](auto npl) -> int {
      GSV_LAUNCH(sample_only_kernel<decltype(npl)::value>, dim3(B), dim3(64), lds, s, logits, vocab, vocab_eff, prev, prev_len, 0,
                 1.f, 1.f, 1.f, noise, (unsigned long long)seed, step, sampled, argmax_tok, (const RowSampling*)d_rows);
      return GSV_OK;
    });
  if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("op_sample_rows: the kernel failed"); rc = GSV_ERR_HIP; }
  (void)hipFree(d_rows);
  return rc;
}

}  // extern "C"
