// SOLA stitching of vocoder fragments (H17, reference TTS_infer_pack/TTS.py:1611-1637) for gfx950.
//
// For each neighbouring pair (f1, f2): cross-correlate the last `ov` samples of f1 with the first `ov` samples of f2
// (F.conv1d with padding ov/2, last output dropped), idx = first argmax; f1 loses its last ov-idx samples, f2 its
// first idx samples, and the first ov-idx samples of what is left of f2 are cross-faded with f1's tail under a periodic
// Hann window of length 2(ov-idx).  Everything (correlation, argmax, cross-fade, compaction) stays on the device;
// the argmax offsets never visit the host, only the final length does.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "resample.h"

namespace gsv {

// corr[j] = sum_k w1[j + k - ov/2] * w2[k], zero padded, j in [0, ov)   (one workgroup per output)
__global__ __launch_bounds__(256) void sola_corr_kernel(const float* __restrict__ w1, const float* __restrict__ w2, int ov,
                                                        float* __restrict__ corr) {
  __shared__ float red[4];
  const int j = blockIdx.x;
  const int off = j - ov / 2;
  float s = 0.f;
  for (int k = threadIdx.x; k < ov; k += 256) {
    const int i = off + k;
    if (i >= 0 && i < ov) s += w1[i] * w2[k];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) corr[j] = red[0] + red[1] + red[2] + red[3];
}

// first argmax of corr[0..ov) -> idx[pair]
__global__ __launch_bounds__(256) void sola_argmax_kernel(const float* __restrict__ corr, int ov, int* __restrict__ idx_out) {
  __shared__ float bv[256];
  __shared__ int bi[256];
  float best = -INFINITY;
  int b = 0x7fffffff;
  for (int j = threadIdx.x; j < ov; j += 256) {
    const float v = corr[j];
    if (v > best || (v == best && j < b)) { best = v; b = j; }
  }
  bv[threadIdx.x] = best; bi[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float v = bv[threadIdx.x + o]; const int i2 = bi[threadIdx.x + o];
      if (v > bv[threadIdx.x] || (v == bv[threadIdx.x] && i2 < bi[threadIdx.x])) { bv[threadIdx.x] = v; bi[threadIdx.x] = i2; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *idx_out = bi[0] == 0x7fffffff ? 0 : bi[0];
}

// f2[idx + m] = win[m] * f2[idx + m] + win[n + m] * f1_tail[ov - n + m],  n = ov - idx, win = periodic Hann(2n)
__global__ void sola_blend_kernel(const float* __restrict__ f1_tail, float* __restrict__ f2, int ov, const int* __restrict__ idx_p) {
  const int idx = *idx_p, n = ov - idx;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const float N = (float)(2 * n);
  const float wa = 0.5f - 0.5f * cosf(6.283185307179586f * (float)m / N);
  const float wb = 0.5f - 0.5f * cosf(6.283185307179586f * (float)(n + m) / N);
  f2[idx + m] = wa * f2[idx + m] + wb * f1_tail[ov - n + m];
}

// piece i = frag_i[start_i : len_i - trim_i], start_0 = 0, start_i = idx[i-1], trim_i = ov - idx[i] (0 for the last)
__global__ void sola_offsets_kernel(const int* __restrict__ lens, const int* __restrict__ idx, int n, int ov, long long* __restrict__ dst_off,
                                    int* __restrict__ total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long o = 0;
  for (int i = 0; i < n; ++i) {
    dst_off[i] = o;
    const int start = i > 0 ? idx[i - 1] : 0;
    const int trim = i < n - 1 ? ov - idx[i] : 0;
    o += lens[i] - start - trim;
  }
  dst_off[n] = o;
  *total = (int)o;
}

__global__ void sola_gather_kernel(const float* __restrict__ frags, const long long* __restrict__ src_off, const int* __restrict__ idx,
                                   const long long* __restrict__ dst_off, int n, float* __restrict__ out) {
  const int i = blockIdx.y;
  const int start = i > 0 ? idx[i - 1] : 0;
  const long long cnt = dst_off[i + 1] - dst_off[i];
  const float* src = frags + src_off[i] + start;
  float* dst = out + dst_off[i];
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += (long long)gridDim.x * blockDim.x) dst[k] = src[k];
}

// ---- H13: peak normalisation + silence gaps + int16 conversion (reference TTS.py:1377-1429) --------------------------
// One workgroup per fragment, fragments already in output order.  Pass 1: peak = max|x| over the fragment (a NaN anywhere
// makes the reference's `max > 1` test false, so it disables the division here too).  Pass 2 (served from L2): the
// reference's arithmetic in the fragment's own dtype T -- x / peak in T when peak > 1, then * 32768 in T (numpy keeps
// float16 for float16 * int) -- truncated to int32 and wrapped to int16, followed by `gap` zero samples.
struct PostTable {
  const void* src[32];
  long long dst[32];
  int len[32];
};

// O = short: the int16 PCM; O = float: the same fragments as fp32 before the x32768 / int16 step (what the reference's
// super-sampling path concatenates and feeds to AP_BWE, TTS.py:1397-1417)
template <typename T, typename O = short>
__global__ __launch_bounds__(1024) void postprocess_kernel(PostTable tab, int gap, O* __restrict__ out) {
  __shared__ float red[16];
  __shared__ int red_nan[16];
  const T* __restrict__ x = (const T*)tab.src[blockIdx.x];
  const int n = tab.len[blockIdx.x];
  O* __restrict__ o = out + tab.dst[blockIdx.x];
  float peak = 0.f;
  int nan = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float v = fabsf((float)x[i]);
    nan |= (v != v);
    peak = fmaxf(peak, v);
  }
  peak = wave_max(peak);
  nan = __any(nan);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = peak; red_nan[threadIdx.x >> 6] = nan; }
  __syncthreads();
  peak = red[0];
  nan = red_nan[0];
  for (int w = 1; w < 16; ++w) { peak = fmaxf(peak, red[w]); nan |= red_nan[w]; }
  const bool divide = !nan && peak > 1.f;
  const T denom = (T)peak;                                     // exact: the peak is one of the fragment's values
  for (int i = threadIdx.x; i < n; i += 1024) {
    T v = x[i];
    if (divide) v = (T)((float)v / (float)denom);
    if constexpr (std::is_same<O, float>::value) {
      o[i] = (float)v;
    } else {
      const T m = (T)((float)v * 32768.f);
      o[i] = (short)(int)(float)m;
    }
  }
  for (int i = threadIdx.x; i < gap; i += 1024) o[n + i] = (O)0;
}

// ---- gsv_postprocess_groups: the same arithmetic, tiled ----------------------------------------------------------------
// A server step hands over the fragments of several requests at once: n sentences in groups, each group with its own gap.
// Every sentence is cut into tiles of kGroupTile samples (an empty sentence keeps one tile, which writes its gap), one
// workgroup per tile, so one long sentence is spread over many CUs.  Two launches: the first reduces each tile's peak and
// combines the tiles of a sentence with an atomic max on the bit pattern of |x| -- order-preserving for non-negative floats,
// and a NaN (> 0x7f800000) outranks every number, so the one word carries the NaN flag too; the second converts and writes.
// The table (sentences, then tiles) is filled on the host, uploaded with one copy and read from device memory.
constexpr int kGroupTile = 4096;
struct GroupSent {
  const void* src;
  long long dst;       // first output sample
  int len, gap;
  unsigned peak;       // max over the sentence of the bits of |x|; uploaded as 0
  int pad;
};
struct GroupTile { int sent, start; };
static_assert(sizeof(GroupSent) == 32 && sizeof(GroupTile) == 8, "table layout");

template <typename T> struct GroupVec;
template <> struct GroupVec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct GroupVec<_Float16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };
typedef short short8_t __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ unsigned abs_bits(T v) { return __float_as_uint(fabsf((float)v)); }

// elements from p to the next 16-byte boundary (p is element-aligned), at most n
template <typename T>
__device__ __forceinline__ int head_count(const T* p, int n) {
  const int h = (int)(((16u - (unsigned)((size_t)p & 15u)) & 15u) / sizeof(T));
  return h < n ? h : n;
}

template <typename T>
__global__ __launch_bounds__(256) void post_groups_peak_kernel(GroupSent* __restrict__ sent, const GroupTile* __restrict__ tiles) {
  typedef typename GroupVec<T>::type V;
  constexpr int E = 16 / sizeof(T);
  __shared__ unsigned red[4];
  const GroupTile t = tiles[blockIdx.x];
  const T* __restrict__ x = (const T*)sent[t.sent].src + t.start;
  const int left = sent[t.sent].len - t.start, n = left < kGroupTile ? left : kGroupTile;
  const int tid = threadIdx.x;
  unsigned m = 0;
  const int head = head_count(x, n);                            // the loads of the body are 16-byte aligned
  if (tid < head) m = abs_bits(x[tid]);
  const int body = (n - head) / E;
  const V* __restrict__ xv = (const V*)(x + head);
  for (int i = tid; i < body; i += 256) {
    const V v = xv[i];
#pragma unroll
    for (int k = 0; k < E; ++k) { const unsigned b = abs_bits((T)v[k]); m = b > m ? b : m; }
  }
  const int tail = head + body * E;
  if (tail + tid < n) { const unsigned b = abs_bits(x[tail + tid]); m = b > m ? b : m; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned b = (unsigned)__shfl_xor((int)m, o, 64); m = b > m ? b : m; }
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    if (m) atomicMax(&sent[t.sent].peak, m);
  }
}

// zeros into o[0..n), 16-byte stores where o allows
__device__ __forceinline__ void zero_fill(short* __restrict__ o, int n, int tid) {
  const int head = head_count(o, n);
  if (tid < head) o[tid] = 0;
  const int body = (n - head) / 8;
  short8_t* __restrict__ ov = (short8_t*)(o + head);
  const short8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < body; i += 256) ov[i] = z;
  const int tail = head + body * 8;
  if (tail + tid < n) o[tail + tid] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void post_groups_write_kernel(const GroupSent* __restrict__ sent, const GroupTile* __restrict__ tiles,
                                                                short* __restrict__ out) {
  typedef typename GroupVec<T>::type V;
  const GroupTile t = tiles[blockIdx.x];
  const GroupSent S = sent[t.sent];
  const T* __restrict__ x = (const T*)S.src + t.start;
  short* __restrict__ o = out + S.dst + t.start;
  const int left = S.len - t.start, n = left < kGroupTile ? left : kGroupTile;
  const int tid = threadIdx.x;
  const bool divide = S.peak > 0x3f800000u && S.peak <= 0x7f800000u;     // peak > 1 and no NaN
  const T denom = (T)__uint_as_float(S.peak);                            // exact: the peak is one of the sentence's values
  auto pcm = [&](T v) -> short {                                         // postprocess_kernel's arithmetic, in T
    if (divide) v = (T)((float)v / (float)denom);
    const T m = (T)((float)v * 32768.f);
    return (short)(int)(float)m;
  };
  // the stores of the body are 16-byte aligned; its loads are aligned to the element only (a torch.split view)
  const int head = head_count(o, n);
  if (tid < head) o[tid] = pcm(x[tid]);
  const int body = (n - head) / 8;
  short8_t* __restrict__ ov = (short8_t*)(o + head);
  for (int i = tid; i < body; i += 256) {
    const T* p = x + head + 8 * i;
    short8_t r;
    if constexpr (sizeof(T) == 2) {
      V v;
      __builtin_memcpy(&v, p, 16);
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = pcm((T)v[k]);
    } else {
      V v0, v1;
      __builtin_memcpy(&v0, p, 16);
      __builtin_memcpy(&v1, p + 4, 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) { r[k] = pcm((T)v0[k]); r[4 + k] = pcm((T)v1[k]); }
    }
    ov[i] = r;
  }
  const int tail = head + body * 8;
  if (tail + tid < n) o[tail + tid] = pcm(x[tail + tid]);
  if (left <= kGroupTile) zero_fill(o + n, S.gap, tid);                  // the sentence's last tile (its only one when empty)
}

// ---- gsv_postprocess_groups_rate: the groups at another sample rate and in another encoding -------------
// Group g is the virtual stream X_g = concat_i [norm(x_i), gap zeros] (what postprocess_kernel<T, float> writes for it alone),
// resampled as resample_poly_seg_kernel does (resample.hip: one thread per output, one fp32 accumulator, fmaf over its taps in
// ascending input index) and converted.  The peaks come from post_groups_peak_kernel; GroupSent::dst is here the sentence's first
// sample in its group's stream.  One workgroup per kRsTile consecutive outputs of one group: it finds the sentence under the first
// sample of its input window once, walks sentences and gaps from there and stages the window in LDS as normalised fp32 (the gaps
// are zeros written to LDS, never loaded), with the filter behind it where HLDS.  The LDS reads of the tap loop are those of
// resample_poly_seg_kernel, whose header counts their bank conflicts.  The results go back to LDS, over the window, so that the
// conversion can store 16 bytes per lane where the output's address allows.
struct RateGroup {
  long long out;       // first output sample
  long long n;         // N_g: samples of the virtual stream
  int sent0, n_sent;   // its sentences in the table
  int m, tile0;        // outputs, first workgroup
};
static_assert(sizeof(RateGroup) == 32, "table layout");

__device__ __forceinline__ short rate_s16(float y) {                     // saturates; a NaN ends at the lower bound
  return (short)(int)fminf(fmaxf(y * 32768.f, -32768.f), 32767.f);
}
// ITU-T G.711 of an int16 sample, segment search by the position of the highest set bit
__device__ __forceinline__ unsigned char rate_mulaw(short s) {
  int v = (int)s >> 2;                                                   // 14 bits
  const int mask = v < 0 ? 0x7f : 0xff;
  v = v < 0 ? -v : v;
  v = (v > 8159 ? 8159 : v) + 33;                                        // clip, bias
  const int seg = max(0, 26 - __clz(v));                                 // first segment whose end 0x3f << seg | ... holds v
  return (unsigned char)((seg >= 8 ? 0x7f : ((seg << 4) | ((v >> (seg + 1)) & 0xf))) ^ mask);
}
__device__ __forceinline__ unsigned char rate_alaw(short s) {
  int v = (int)s >> 3;                                                   // 13 bits
  const int mask = v < 0 ? 0x55 : 0xd5;
  v = v < 0 ? -v - 1 : v;
  const int seg = max(0, 27 - __clz(v));                                 // v <= 4095: seg <= 7
  return (unsigned char)(((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 0xf)) ^ mask);
}

template <int FMT> struct RateOut;
template <> struct RateOut<GSV_OUT_S16> { typedef short type; static __device__ __forceinline__ short cvt(float y) { return rate_s16(y); } };
template <> struct RateOut<GSV_OUT_MULAW> { typedef unsigned char type; static __device__ __forceinline__ unsigned char cvt(float y) { return rate_mulaw(rate_s16(y)); } };
template <> struct RateOut<GSV_OUT_ALAW> { typedef unsigned char type; static __device__ __forceinline__ unsigned char cvt(float y) { return rate_alaw(rate_s16(y)); } };
template <> struct RateOut<GSV_OUT_F32> { typedef float type; static __device__ __forceinline__ float cvt(float y) { return y; } };

// The window walk that the rate kernel and the loudness meter share.  The stream is made of the sentences [s0, s0 + ns) of the
// table; SPAN = false: sentence i sits at sent[i].dst and is followed by its gap (a group's stream, sent[s0].dst = 0); SPAN = true:
// the stream starts at sentence s0 and `gaps` says whether the gaps belong to it.  For every sentence that overlaps the window
// [w0, w0 + wn) the walk calls seg(S, first, live, cnt, at): cnt stream samples land at window offset `at`, the first `live` of them
// are S.src[first ..], the rest are the gap's zeros.
template <bool SPAN, typename F>
__device__ __forceinline__ void walk_window(const GroupSent* __restrict__ sent, int s0, int ns, bool gaps, long long w0, int wn, F seg) {
  const long long w1 = w0 + wn;
  const long long base = SPAN ? sent[s0].dst : 0;
  auto pos = [&](int si, const GroupSent& S) -> long long {
    if (!SPAN) return S.dst;
    return S.dst - base - (gaps ? 0LL : (long long)(si - s0) * S.gap);
  };
  // the sentence under w0: the last one that starts at or before it (an empty sentence without a gap covers nothing)
  int sa = s0, sb = s0 + ns - 1;
  while (sa < sb) {
    const int mid = (sa + sb + 1) >> 1;
    if (pos(mid, sent[mid]) <= w0) sa = mid; else sb = mid - 1;
  }
  for (int si = sa; si < s0 + ns; ++si) {
    const GroupSent S = sent[si];
    const long long at0 = pos(si, S);
    if (at0 >= w1) break;
    const long long b = at0 > w0 ? at0 : w0;                            // [b, e): this sentence and its gap inside the window
    const long long e = min(at0 + S.len + ((!SPAN || gaps) ? S.gap : 0), w1);
    const int cnt = (int)(e - b), at = (int)(b - w0);
    const int first = (int)(b - at0);                                    // sample of the sentence at b (>= len: inside the gap)
    const int live = max(0, min(cnt, S.len - first));                    // samples that are loaded; the rest are the gap's zeros
    seg(S, first, live, cnt, at);
  }
}

struct LoudReport { double lufs; float gain; unsigned flags; };
static_assert(sizeof(LoudReport) == 16 && sizeof(gsv_loud_report) == 16, "report layout");

// GAIN: a sentence whose GroupSent::pad names a span (index + 1) is multiplied by that span's gain where it is staged
template <typename T, int FMT, bool HLDS, bool GAIN>
__device__ __forceinline__ void post_groups_rate_body(const GroupSent* __restrict__ sent, const RateGroup* __restrict__ groups,
                                                      int n_groups, const float* __restrict__ h, int L, int up, int down,
                                                      void* __restrict__ out, int win_cap, const LoudReport* __restrict__ rep) {
  typedef typename RateOut<FMT>::type O;
  constexpr int E = 16 / sizeof(O);
  typedef O OV __attribute__((ext_vector_type(E)));
  extern __shared__ float rate_lds[];
  float* xs = rate_lds;                                                  // max(win_cap, kRsTile) floats
  const int h_at = win_cap > kRsTile ? win_cap : kRsTile;
  const float* hs = HLDS ? rate_lds + h_at : h;
  const int tid = threadIdx.x;
  int lo = 0, hi = n_groups - 1;                                         // the last group whose first workgroup is <= this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const RateGroup G = groups[lo];
  const long long n = G.n;
  const int half = L >> 1;
  const int o0 = ((int)blockIdx.x - G.tile0) * kRsTile, o1 = min(G.m, o0 + kRsTile);
  if (o0 >= o1) return;                                                  // the host launches no such tile
  // the window [w0, w0 + wn) of the stream that outputs [o0, o1) read
  const long long a0 = (long long)o0 * down + half - (L - 1);
  const long long w0 = a0 <= 0 ? 0 : (a0 + up - 1) / up;
  const long long wl = min(n - 1, ((long long)(o1 - 1) * down + half) / up);
  const int wn = (int)min((long long)win_cap, max(0LL, wl - w0 + 1));
  walk_window<false>(sent, G.sent0, G.n_sent, true, w0, wn, [&](const GroupSent& S, int first, int live, int cnt, int at) {
    const T* __restrict__ x = (const T*)S.src + first;
    const bool divide = S.peak > 0x3f800000u && S.peak <= 0x7f800000u;   // peak > 1 and no NaN
    const T denom = (T)__uint_as_float(S.peak);
    float g = 1.f;
    if constexpr (GAIN) { if (S.pad) g = rep[S.pad - 1].gain; }
    for (int i = tid; i < cnt; i += 256) {
      float f = 0.f;
      if (i < live) {
        T v = x[i];
        if (divide) v = (T)((float)v / (float)denom);                    // postprocess_kernel's arithmetic, in T
        f = (float)v;
        if constexpr (GAIN) f *= g;
      }
      xs[at + i] = f;
    }
  });
  if (HLDS) for (int i = tid; i < L; i += 256) rate_lds[h_at + i] = h[i];
  __syncthreads();
  float acc[kRsTile / 256];
#pragma unroll
  for (int r = 0; r < kRsTile / 256; ++r) {
    const int o = o0 + tid + 256 * r;
    acc[r] = 0.f;
    if (o < o1) {
      const long long c = (long long)o * down + half;
      const long long a = c - (L - 1);
      const long long ja = a <= 0 ? 0 : (a + up - 1) / up;
      const long long jb = min(n - 1, c / up);
      int k = (int)(c - ja * up);                                        // filter index of the first tap, in [0, L)
      const int q0 = (int)(ja - w0), q1 = min((int)(jb - w0), wn - 1);
      float s = 0.f;
      for (int q = q0; q <= q1; ++q, k -= up) s = fmaf(hs[k], xs[q], s);
      acc[r] = s;
    }
  }
  __syncthreads();                                                       // every tap is read: the results take the window's place
#pragma unroll
  for (int r = 0; r < kRsTile / 256; ++r) xs[tid + 256 * r] = acc[r];
  __syncthreads();
  const int cnt = o1 - o0;
  O* __restrict__ o = (O*)out + G.out + o0;
  const int head = head_count(o, cnt);                                   // the stores of the body are 16-byte aligned
  if (tid < head) o[tid] = RateOut<FMT>::cvt(xs[tid]);
  const int body = (cnt - head) / E;
  OV* __restrict__ ov = (OV*)(o + head);
  for (int i = tid; i < body; i += 256) {
    OV r;
#pragma unroll
    for (int k = 0; k < E; ++k) r[k] = RateOut<FMT>::cvt(xs[head + E * i + k]);
    ov[i] = r;
  }
  const int tail = head + body * E;
  if (tail + tid < cnt) o[tail + tid] = RateOut<FMT>::cvt(xs[tail + tid]);
}

template <typename T, int FMT, bool HLDS>
__global__ __launch_bounds__(256) void post_groups_rate_kernel(const GroupSent* __restrict__ sent, const RateGroup* __restrict__ groups,
                                                               int n_groups, const float* __restrict__ h, int L, int up, int down,
                                                               void* __restrict__ out, int win_cap) {
  post_groups_rate_body<T, FMT, HLDS, false>(sent, groups, n_groups, h, L, up, down, out, win_cap, nullptr);
}

template <typename T, int FMT, bool HLDS>
__global__ __launch_bounds__(256) void post_groups_loud_kernel(const GroupSent* __restrict__ sent, const RateGroup* __restrict__ groups,
                                                               int n_groups, const float* __restrict__ h, int L, int up, int down,
                                                               void* __restrict__ out, int win_cap, const LoudReport* __restrict__ rep) {
  post_groups_rate_body<T, FMT, HLDS, true>(sent, groups, n_groups, h, L, up, down, out, win_cap, rep);
}

// ---- loudness meter (ITU-R BS.1770 K-weighting, gated) -----------------------------------------------------
// The two biquads are one 4-state linear recurrence s' = A s + B x, y = C s + D x (both in transposed direct form II), run in
// fp64.  A span is cut into tiles of kLoudTile samples, one workgroup each, every lane owning a chunk of kLoudChunk samples.
//   state   each chunk from zero state; an in-wave Kogge-Stone scan over s_{k+1} = M s_k + e_k (M = A^16, its squarings in
//           LoudConst::P) and a serial combine of the four waves give the tile's zero-state end state
//   carry   one lane per span walks its tiles in order, s_{t+1} = A^4096 s_t + e_t: the true start state of every tile
//   energy  the same scan again; lane k starts from I_{k-1} + M^k P_w (P_w the wave's start state, M^k from LoudConst::Mk),
//           re-runs its chunk and adds y^2 to the (at most three) sub-blocks the tile touches; fixed slots per tile
//   gate    one workgroup per span: sub-block energies from the slots in tile order, both gates, L, the gain, the report
// Every sum has a fixed order that depends on the span alone, and no workgroup waits for another.
constexpr int kLoudTile = 4096, kLoudChunk = 16;
static_assert(kLoudTile == 256 * kLoudChunk, "one chunk per lane");
struct LoudConst {
  double bq[10];        // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
  double P[6][16];      // A^(16 * 2^j): the scan steps
  double W[16];         // A^1024: one wave
  double TT[16];        // A^4096: one tile
  double Mk[64][16];    // A^(16 k): lane k's share of its wave's start state
  int s, pad[3];        // samples per sub-block
};
struct LoudSpan {
  int first, count, gaps;
  int n;                // samples
  int tile0, sub0;      // first tile, first sub-block energy
  float target, peak_db;
};
struct LoudTile { int span, t; };
static_assert(sizeof(LoudSpan) == 32 && sizeof(LoudTile) == 8 && sizeof(LoudConst) % 16 == 0, "table layout");

__device__ __forceinline__ double kw_step(const double* __restrict__ k, double (&s)[4], double x) {
  const double y1 = k[0] * x + s[0];
  s[0] = k[1] * x - k[3] * y1 + s[1];
  s[1] = k[2] * x - k[4] * y1;
  const double y = k[5] * y1 + s[2];
  s[2] = k[6] * y1 - k[8] * y + s[3];
  s[3] = k[7] * y1 - k[9] * y;
  return y;
}
// r = M v + a
__device__ __forceinline__ void mat_vec_add(const double* __restrict__ M, const double (&v)[4], const double (&a)[4], double (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = M[4 * i] * v[0] + M[4 * i + 1] * v[1] + M[4 * i + 2] * v[2] + M[4 * i + 3] * v[3] + a[i];
}

__device__ __forceinline__ int loud_lds(int p) { return p + (p >> 4); }      // a chunk per lane: stride 17 spreads the banks

// Stages tile t of the span as normalised fp32 (16-byte loads where the source allows, scalar heads and tails), runs every
// lane's chunk from zero state and scans inside the wave: x = the lane's samples, I = the state after chunks [wave start .. lane]
// from zero at the wave's start, wt[w] = wave w's total (valid after the barrier this ends with).
template <typename T>
__device__ __forceinline__ void loud_tile_scan(const GroupSent* __restrict__ sent, const LoudSpan& sp, int t, const LoudConst* __restrict__ C,
                                               float* xs, double (*wt)[4], float (&x)[kLoudChunk], double (&I)[4]) {
  typedef typename GroupVec<T>::type V;
  constexpr int E = 16 / sizeof(T);
  const int tid = threadIdx.x;
  const long long w0 = (long long)t * kLoudTile;
  const int wn = (int)min((long long)kLoudTile, (long long)sp.n - w0);
  for (int i = wn + tid; i < kLoudTile; i += 256) xs[loud_lds(i)] = 0.f;
  walk_window<true>(sent, sp.first, sp.count, sp.gaps != 0, w0, wn, [&](const GroupSent& S, int first, int live, int cnt, int at) {
    const T* __restrict__ src = (const T*)S.src + first;
    const bool divide = S.peak > 0x3f800000u && S.peak <= 0x7f800000u;   // peak > 1 and no NaN
    const T denom = (T)__uint_as_float(S.peak);
    auto put = [&](int i, T v) {
      if (divide) v = (T)((float)v / (float)denom);                      // postprocess_kernel's arithmetic, in T
      xs[loud_lds(at + i)] = (float)v;
    };
    const int head = head_count(src, live);
    if (tid < head) put(tid, src[tid]);
    const int body = (live - head) / E;
    const V* __restrict__ sv = (const V*)(src + head);
    for (int i = tid; i < body; i += 256) {
      const V v = sv[i];
#pragma unroll
      for (int k = 0; k < E; ++k) put(head + E * i + k, (T)v[k]);
    }
    const int tail = head + body * E;
    if (tail + tid < live) put(tail + tid, src[tail + tid]);
    for (int i = live + tid; i < cnt; i += 256) xs[loud_lds(at + i)] = 0.f;
  });
  __syncthreads();
  double s[4] = {0., 0., 0., 0.};
#pragma unroll
  for (int i = 0; i < kLoudChunk; ++i) {
    x[i] = xs[17 * tid + i];
    kw_step(C->bq, s, (double)x[i]);
  }
  const int lane = tid & 63;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double r[4], q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = __shfl_up(s[i], 1u << j, 64);
    mat_vec_add(C->P[j], r, s, q);
    if (lane >= (1 << j)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = q[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) I[i] = s[i];
  if (lane == 63) {
#pragma unroll
    for (int i = 0; i < 4; ++i) wt[tid >> 6][i] = s[i];
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void loud_state_kernel(const GroupSent* __restrict__ sent, const LoudSpan* __restrict__ spans,
                                                         const LoudTile* __restrict__ tiles, const LoudConst* __restrict__ C,
                                                         double* __restrict__ end_state) {
  __shared__ float xs[kLoudTile + kLoudTile / 16];
  __shared__ double wt[4][4];
  const LoudTile tl = tiles[blockIdx.x];
  const LoudSpan sp = spans[tl.span];
  float x[kLoudChunk];
  double I[4];
  loud_tile_scan<T>(sent, sp, tl.t, C, xs, wt, x, I);
  if (threadIdx.x == 0) {
    double p[4] = {wt[0][0], wt[0][1], wt[0][2], wt[0][3]};
    for (int w = 1; w < 4; ++w) {
      double q[4];
      mat_vec_add(C->W, p, wt[w], q);
      for (int i = 0; i < 4; ++i) p[i] = q[i];
    }
    for (int i = 0; i < 4; ++i) end_state[4 * (size_t)blockIdx.x + i] = p[i];
  }
}

// state[tile] : the tile's zero-state end state on entry, its true start state on return
__global__ __launch_bounds__(64) void loud_carry_kernel(const LoudSpan* __restrict__ spans, int n_spans, const LoudConst* __restrict__ C,
                                                        double* __restrict__ state) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_spans) return;
  const LoudSpan sp = spans[k];
  const int nt = (sp.n + kLoudTile - 1) / kLoudTile;
  double st[4] = {0., 0., 0., 0.};
  for (int t = 0; t < nt; ++t) {
    double* p = state + 4 * (size_t)(sp.tile0 + t);
    const double e[4] = {p[0], p[1], p[2], p[3]};
    for (int i = 0; i < 4; ++i) p[i] = st[i];
    double q[4];
    mat_vec_add(C->TT, st, e, q);
    for (int i = 0; i < 4; ++i) st[i] = q[i];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void loud_energy_kernel(const GroupSent* __restrict__ sent, const LoudSpan* __restrict__ spans,
                                                          const LoudTile* __restrict__ tiles, const LoudConst* __restrict__ C,
                                                          const double* __restrict__ state, double* __restrict__ partial) {
  __shared__ float xs[kLoudTile + kLoudTile / 16];
  __shared__ double wt[4][4];
  __shared__ double red[4][3];
  const LoudTile tl = tiles[blockIdx.x];
  const LoudSpan sp = spans[tl.span];
  float x[kLoudChunk];
  double I[4];
  loud_tile_scan<T>(sent, sp, tl.t, C, xs, wt, x, I);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double p[4];
  for (int i = 0; i < 4; ++i) p[i] = state[4 * (size_t)blockIdx.x + i];
  for (int w = 0; w < wave; ++w) {                                       // the wave's start state
    double q[4];
    mat_vec_add(C->W, p, wt[w], q);
    for (int i = 0; i < 4; ++i) p[i] = q[i];
  }
  double prev[4], s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    prev[i] = __shfl_up(I[i], 1u, 64);
    if (lane == 0) prev[i] = 0.;
  }
  mat_vec_add(C->Mk[lane], p, prev, s);
  // sub-blocks: the tile starts inside j0; a chunk of 16 < s samples touches at most two, the tile at most three (s > 2048)
  const int sb = C->s;
  const long long t0 = (long long)tl.t * kLoudTile, c0 = t0 + kLoudChunk * tid;
  const int j0 = (int)(t0 / sb);
  int j = (int)(c0 / sb);
  long long edge = (long long)(j + 1) * sb;
  double v0 = 0., v1 = 0., v2 = 0.;
#pragma unroll
  for (int i = 0; i < kLoudChunk; ++i) {
    const long long q = c0 + i;
    if (q == edge) { ++j; edge += sb; }
    const double y = kw_step(C->bq, s, (double)x[i]);
    const double e = q < sp.n ? y * y : 0.;
    const int slot = j - j0;
    v0 += slot == 0 ? e : 0.;
    v1 += slot == 1 ? e : 0.;
    v2 += slot == 2 ? e : 0.;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v0 += __shfl_xor(v0, o, 64);
    v1 += __shfl_xor(v1, o, 64);
    v2 += __shfl_xor(v2, o, 64);
  }
  if (lane == 0) { red[wave][0] = v0; red[wave][1] = v1; red[wave][2] = v2; }
  __syncthreads();
  if (tid < 3) partial[3 * (size_t)blockIdx.x + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__device__ __forceinline__ double loud_level(double z) { return -0.691 + 10. * log10(z); }

// fixed-order sum of (v, c) over the workgroup; every thread gets the result
__device__ __forceinline__ void loud_block_sum(double& v, int& c, double (*rv)[2], int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); c += __shfl_xor(c, o, 64); }
  __syncthreads();                                                       // the last use of rv is over
  if ((tid & 63) == 0) { rv[tid >> 6][0] = v; rv[tid >> 6][1] = (double)c; }
  __syncthreads();
  v = ((rv[0][0] + rv[1][0]) + rv[2][0]) + rv[3][0];
  c = (int)(((rv[0][1] + rv[1][1]) + rv[2][1]) + rv[3][1]);
}

__global__ __launch_bounds__(256) void loud_gate_kernel(const GroupSent* __restrict__ sent, const LoudSpan* __restrict__ spans,
                                                        const LoudConst* __restrict__ C, const double* __restrict__ partial,
                                                        double* __restrict__ energies, LoudReport* __restrict__ rep) {
  __shared__ double rv[4][2];
  const LoudSpan sp = spans[blockIdx.x];
  const int tid = threadIdx.x;
  const long long sb = C->s;
  const int N = sp.n, J = (int)(N / sb), Jt = (int)((N + sb - 1) / sb);
  double* __restrict__ e = energies + sp.sub0;
  double all = 0.;
  int unused = 0;
  for (int j = tid; j < Jt; j += 256) {
    const long long a = j * sb, b = min(a + sb, (long long)N) - 1;       // the sub-block's first and last sample
    double v = 0.;
    for (int t = (int)(a / kLoudTile); t <= (int)(b / kLoudTile); ++t)
      v += partial[3 * (size_t)(sp.tile0 + t) + (j - (int)((long long)t * kLoudTile / sb))];
    e[j] = v;
    all += v;
  }
  __syncthreads();                                                       // e[] is read back by other threads of this workgroup
  double lufs = -INFINITY;
  if (N > 0) {
    const bool shortspan = J < 4;
    if (shortspan) loud_block_sum(all, unused, rv, tid);                 // Jt <= 4: lanes 0..3 hold one sub-block each
    const int nb = shortspan ? 1 : J - 3;
    auto block = [&](int b) -> double { return shortspan ? all / (double)N : (((e[b] + e[b + 1]) + e[b + 2]) + e[b + 3]) / (4. * (double)sb); };
    double sum = 0.;
    int cnt = 0;
    for (int b = tid; b < nb; b += 256) {
      const double z = block(b);
      if (loud_level(z) > -70.) { sum += z; ++cnt; }
    }
    loud_block_sum(sum, cnt, rv, tid);
    if (cnt > 0) {
      const double gate = loud_level(sum / cnt) - 10.;
      sum = 0.;
      cnt = 0;
      for (int b = tid; b < nb; b += 256) {
        const double z = block(b), l = loud_level(z);
        if (l > -70. && l > gate) { sum += z; ++cnt; }
      }
      loud_block_sum(sum, cnt, rv, tid);
      if (cnt > 0) lufs = loud_level(sum / cnt);
    }
  }
  if (tid != 0) return;
  unsigned flags = 0;
  float peak = 0.f;                                                      // P: the span's peak in the stream
  for (int i = sp.first; i < sp.first + sp.count; ++i) {
    const unsigned pb = sent[i].peak;
    if (pb > 0x7f800000u) flags |= GSV_LOUD_NAN;
    else peak = fmaxf(peak, fminf(__uint_as_float(pb), 1.f));
  }
  if (!(lufs > -INFINITY) && !(flags & GSV_LOUD_NAN)) flags |= GSV_LOUD_SILENT;
  double g = 1.;
  if (!flags && sp.target == sp.target) {
    g = pow(10., ((double)sp.target - lufs) / 20.);
    const double c = pow(10., (double)sp.peak_db / 20.);
    if (g * (double)peak > c) { g = c / (double)peak; flags |= GSV_LOUD_LIMITED; }
  }
  rep[blockIdx.x] = LoudReport{lufs, (float)g, flags};
}

}  // namespace gsv

extern "C" int gsv_sola(float* frags, const int* lens, int n, int overlap, float* out, int* out_len, gsv_stream_t stream) {
  using namespace gsv;
  GSV_REQUIRE(frags && lens && out && out_len && n >= 1, "sola: bad argument");
  GSV_REQUIRE(overlap >= 2 && overlap % 2 == 0, "sola: overlap length %d must be even and >= 2", overlap);
  hipStream_t s = (hipStream_t)stream;
  std::vector<long long> off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    GSV_REQUIRE(lens[i] >= 2 * overlap || n == 1, "sola: fragment %d has %d samples, need >= 2 * overlap (%d)", i, lens[i], 2 * overlap);
    off[i + 1] = off[i] + lens[i];
  }
  // device scratch: corr[ov] | idx[n] | lens[n] | src_off[n+1] | dst_off[n+1] | total
  char* scratch = nullptr;
  const size_t b_corr = (size_t)overlap * 4, b_int = (size_t)n * 4, b_ll = (size_t)(n + 1) * 8;
  const size_t a_idx = (b_corr + 15) / 16 * 16, a_len = a_idx + (b_int + 15) / 16 * 16, a_src = a_len + (b_int + 15) / 16 * 16;
  const size_t a_dst = a_src + (b_ll + 15) / 16 * 16, a_tot = a_dst + (b_ll + 15) / 16 * 16, total_bytes = a_tot + 16;
  GSV_HIP(hipMalloc((void**)&scratch, total_bytes));
  float* corr = (float*)scratch;
  int* idx = (int*)(scratch + a_idx);
  int* dlens = (int*)(scratch + a_len);
  long long* src_off = (long long*)(scratch + a_src);
  long long* dst_off = (long long*)(scratch + a_dst);
  int* total = (int*)(scratch + a_tot);
  int rc = GSV_OK;
  auto fail = [&](hipError_t e, const char* what) { set_error("sola: %s -> %s", what, hipGetErrorString(e)); rc = GSV_ERR_HIP; };
  hipError_t e;
  if ((e = hipMemsetAsync(idx, 0, b_int, s)) != hipSuccess) fail(e, "memset");
  if (rc == GSV_OK && (e = hipMemcpyAsync(dlens, lens, b_int, hipMemcpyHostToDevice, s)) != hipSuccess) fail(e, "copy lens");
  if (rc == GSV_OK && (e = hipMemcpyAsync(src_off, off.data(), b_ll, hipMemcpyHostToDevice, s)) != hipSuccess) fail(e, "copy offsets");
  if (rc == GSV_OK && (e = hipStreamSynchronize(s)) != hipSuccess) fail(e, "sync");   // `off` is a stack vector
  for (int i = 0; rc == GSV_OK && i + 1 < n; ++i) {
    float* f1 = frags + off[i];
    float* f2 = frags + off[i + 1];
    const float* tail = f1 + lens[i] - overlap;
    hipLaunchKernelGGL(sola_corr_kernel, dim3(overlap), dim3(256), 0, s, tail, (const float*)f2, overlap, corr);
    hipLaunchKernelGGL(sola_argmax_kernel, dim3(1), dim3(256), 0, s, (const float*)corr, overlap, idx + i);
    hipLaunchKernelGGL(sola_blend_kernel, dim3(cdiv(overlap, 256)), dim3(256), 0, s, tail, f2, overlap, (const int*)(idx + i));
    if ((e = hipGetLastError()) != hipSuccess) fail(e, "launch");
  }
  if (rc == GSV_OK) {
    hipLaunchKernelGGL(sola_offsets_kernel, dim3(1), dim3(64), 0, s, (const int*)dlens, (const int*)idx, n, overlap, dst_off, total);
    hipLaunchKernelGGL(sola_gather_kernel, dim3(256, n), dim3(256), 0, s, (const float*)frags, (const long long*)src_off, (const int*)idx,
                       (const long long*)dst_off, n, out);
    if ((e = hipGetLastError()) != hipSuccess) fail(e, "launch");
  }
  if (rc == GSV_OK && (e = hipMemcpyAsync(out_len, total, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) fail(e, "copy length");
  e = hipStreamSynchronize(s);
  if (rc == GSV_OK && e != hipSuccess) fail(e, "sync");
  (void)hipFree(scratch);
  return rc;
}


namespace gsv {

template <typename O>
static int postprocess_t(const void* const* frags, const int* lens, int n, int dtype, int gap, O* out, gsv_stream_t stream) {
  GSV_REQUIRE(n >= 0 && gap >= 0 && (dtype == GSV_F16 || dtype == GSV_F32), "postprocess: bad argument");
  if (n == 0) return GSV_OK;
  GSV_REQUIRE(frags && lens && out, "postprocess: null pointer");
  hipStream_t s = (hipStream_t)stream;
  long long off = 0;
  for (int base = 0; base < n; base += 32) {
    PostTable tab{};
    const int m = n - base < 32 ? n - base : 32;
    for (int i = 0; i < m; ++i) {
      GSV_REQUIRE(lens[base + i] >= 0 && (lens[base + i] == 0 || frags[base + i]), "postprocess: fragment %d is null", base + i);
      tab.src[i] = frags[base + i];
      tab.len[i] = lens[base + i];
      tab.dst[i] = off;
      off += (long long)lens[base + i] + gap;
    }
    if (dtype == GSV_F16) hipLaunchKernelGGL((postprocess_kernel<_Float16, O>), dim3(m), dim3(1024), 0, s, tab, gap, out);
    else hipLaunchKernelGGL((postprocess_kernel<float, O>), dim3(m), dim3(1024), 0, s, tab, gap, out);
    GSV_HIP(hipGetLastError());
  }
  return GSV_OK;
}

}  // namespace gsv

extern "C" int gsv_postprocess(const void* const* frags, const int* lens, int n, int dtype, int gap, int16_t* out,
                               gsv_stream_t stream) {
  return gsv::postprocess_t<short>(frags, lens, n, dtype, gap, (short*)out, stream);
}

extern "C" int gsv_postprocess_f32(const void* const* frags, const int* lens, int n, int dtype, int gap, float* out,
                                   gsv_stream_t stream) {
  return gsv::postprocess_t<float>(frags, lens, n, dtype, gap, out, stream);
}

static inline long long groups_tiles(int len) { return len <= 0 ? 1 : ((long long)len + gsv::kGroupTile - 1) / gsv::kGroupTile; }

extern "C" long long gsv_postprocess_groups_workspace(const int* lens, int n) {
  if (n < 0 || (n > 0 && !lens)) return -1;
  long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] < 0) return -1;
    tiles += groups_tiles(lens[i]);
  }
  return (long long)n * (long long)sizeof(gsv::GroupSent) + tiles * (long long)sizeof(gsv::GroupTile);
}

extern "C" int gsv_postprocess_groups(const void* const* frags, const int* lens, int n, int dtype, const int* group_n,
                                      const int* group_gap, int n_groups, int16_t* out, long long* group_off, void* table,
                                      void* workspace, gsv_stream_t stream) {
  using namespace gsv;
  GSV_REQUIRE(n >= 0 && n_groups >= 0 && (dtype == GSV_F16 || dtype == GSV_F32), "postprocess_groups: bad argument");
  GSV_REQUIRE(n_groups == 0 || (group_n && group_gap && group_off), "postprocess_groups: null group table");
  long long in_groups = 0;
  for (int g = 0; g < n_groups; ++g) {
    GSV_REQUIRE(group_n[g] >= 0 && group_gap[g] >= 0, "postprocess_groups: group %d has %d sentences, gap %d", g, group_n[g], group_gap[g]);
    in_groups += group_n[g];
  }
  GSV_REQUIRE(in_groups == n, "postprocess_groups: the groups hold %lld sentences, n is %d", in_groups, n);
  if (n == 0) {
    for (int g = 0; g <= n_groups && group_off; ++g) group_off[g] = 0;
    return GSV_OK;
  }
  GSV_REQUIRE(frags && lens && out && table && workspace, "postprocess_groups: null pointer");
  GroupSent* sent = (GroupSent*)table;
  GroupTile* tiles = (GroupTile*)(sent + n);
  long long off = 0, n_tiles = 0;
  int i = 0;
  for (int g = 0; g < n_groups; ++g) {
    group_off[g] = off;
    for (int k = 0; k < group_n[g]; ++k, ++i) {
      GSV_REQUIRE(lens[i] >= 0 && (lens[i] == 0 || frags[i]), "postprocess_groups: sentence %d is null", i);
      sent[i] = GroupSent{frags[i], off, lens[i], group_gap[g], 0u, 0};
      for (long long t = 0, nt = groups_tiles(lens[i]); t < nt; ++t) tiles[n_tiles++] = GroupTile{i, (int)(t * kGroupTile)};
      off += (long long)lens[i] + group_gap[g];
    }
  }
  group_off[n_groups] = off;
  GSV_REQUIRE(n_tiles <= 0x7fffffffLL, "postprocess_groups: %lld tiles", n_tiles);
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)n * sizeof(GroupSent) + (size_t)n_tiles * sizeof(GroupTile);
  GSV_HIP(hipMemcpyAsync(workspace, table, bytes, hipMemcpyHostToDevice, s));
  GroupSent* dsent = (GroupSent*)workspace;
  const GroupTile* dtiles = (const GroupTile*)(dsent + n);
  if (dtype == GSV_F16) {
    hipLaunchKernelGGL((post_groups_peak_kernel<_Float16>), dim3((unsigned)n_tiles), dim3(256), 0, s, dsent, dtiles);
    hipLaunchKernelGGL((post_groups_write_kernel<_Float16>), dim3((unsigned)n_tiles), dim3(256), 0, s, (const GroupSent*)dsent, dtiles, (short*)out);
  } else {
    hipLaunchKernelGGL((post_groups_peak_kernel<float>), dim3((unsigned)n_tiles), dim3(256), 0, s, dsent, dtiles);
    hipLaunchKernelGGL((post_groups_write_kernel<float>), dim3((unsigned)n_tiles), dim3(256), 0, s, (const GroupSent*)dsent, dtiles, (short*)out);
  }
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

extern "C" long long gsv_postprocess_groups_rate_workspace(const int* lens, int n, int n_groups) {
  if (n < 0 || n_groups < 0 || (n > 0 && !lens)) return -1;
  long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    if (lens[i] < 0) return -1;
    tiles += ((long long)lens[i] + gsv::kGroupTile - 1) / gsv::kGroupTile;       // the peak pass; an empty sentence has none
  }
  return (long long)n * (long long)sizeof(gsv::GroupSent) + (long long)n_groups * (long long)sizeof(gsv::RateGroup) +
         tiles * (long long)sizeof(gsv::GroupTile);
}

namespace gsv {

template <typename T, int FMT>
static int rate_launch(bool hlds, unsigned tiles, size_t lds, hipStream_t s, const GroupSent* sent, const RateGroup* groups, int n_groups,
                       const float* h, int L, int up, int down, void* out, int win_cap, const LoudReport* rep) {
  if (rep) {                                                             // the GAIN variant
    if (hlds) GSV_LAUNCH((post_groups_loud_kernel<T, FMT, true>), dim3(tiles), dim3(256), lds, s, sent, groups, n_groups, h, L, up, down, out, win_cap, rep);
    else GSV_LAUNCH((post_groups_loud_kernel<T, FMT, false>), dim3(tiles), dim3(256), lds, s, sent, groups, n_groups, h, L, up, down, out, win_cap, rep);
    return GSV_OK;
  }
  if (hlds) GSV_LAUNCH((post_groups_rate_kernel<T, FMT, true>), dim3(tiles), dim3(256), lds, s, sent, groups, n_groups, h, L, up, down, out, win_cap);
  else GSV_LAUNCH((post_groups_rate_kernel<T, FMT, false>), dim3(tiles), dim3(256), lds, s, sent, groups, n_groups, h, L, up, down, out, win_cap);
  return GSV_OK;
}

template <typename T, typename... A>
static int rate_launch_fmt(int out_fmt, A... a) {
  switch (out_fmt) {
    case GSV_OUT_S16: return rate_launch<T, GSV_OUT_S16>(a...);
    case GSV_OUT_MULAW: return rate_launch<T, GSV_OUT_MULAW>(a...);
    case GSV_OUT_ALAW: return rate_launch<T, GSV_OUT_ALAW>(a...);
    default: return rate_launch<T, GSV_OUT_F32>(a...);
  }
}

}  // namespace gsv

namespace gsv {

// what gsv_postprocess_groups_loud and gsv_op_loudness add to a gsv_postprocess_groups_rate call
struct LoudArgs {
  int rate;
  const gsv_loud_span* spans;
  int n_spans;
  LoudReport* report;
  double* energies;        // gsv_op_loudness: the caller's array; else null (the workspace's)
  long long* energy_off;   // gsv_op_loudness
  bool write;              // false: meter only
};

static inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }
static inline long long loud_sub(int rate) { return (long long)std::llround(0.1 * (double)rate); }

static void mat_mul(const long double* a, const long double* b, long double* r) {   // r may be a or b
  long double t[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      long double v = 0;
      for (int k = 0; k < 4; ++k) v += a[4 * i + k] * b[4 * k + j];
      t[4 * i + j] = v;
    }
  for (int i = 0; i < 16; ++i) r[i] = t[i];
}

// the K-weighting biquads for `rate` (include/gsv.h) and the powers of their state matrix that the kernels read
static void loud_constants(int rate, LoudConst* c) {
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / rate), Vh = std::pow(10., G / 20.), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1. + K / Q + K * K;
    c->bq[0] = (Vh + Vb * K / Q + K * K) / a0;
    c->bq[1] = 2. * (K * K - Vh) / a0;
    c->bq[2] = (Vh - Vb * K / Q + K * K) / a0;
    c->bq[3] = 2. * (K * K - 1.) / a0;
    c->bq[4] = (1. - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / rate), d = 1. + K / Q + K * K;
    c->bq[5] = 1.;
    c->bq[6] = -2.;
    c->bq[7] = 1.;
    c->bq[8] = 2. * (K * K - 1.) / d;
    c->bq[9] = (1. - K / Q + K * K) / d;
  }
  // A: kw_step with x = 0 on the unit vectors (column j is the image of e_j)
  const double* k = c->bq;
  long double A[16];
  for (int j = 0; j < 4; ++j) {
    long double s[4] = {0, 0, 0, 0};
    s[j] = 1;
    const long double y1 = s[0], y = (long double)k[5] * y1 + s[2];
    const long double r[4] = {-(long double)k[3] * y1 + s[1], -(long double)k[4] * y1,
                              (long double)k[6] * y1 - (long double)k[8] * y + s[3], (long double)k[7] * y1 - (long double)k[9] * y};
    for (int i = 0; i < 4; ++i) A[4 * i + j] = r[i];
  }
  long double M[16], pw[16];
  for (int i = 0; i < 16; ++i) { M[i] = A[i]; pw[i] = (i % 5 == 0) ? 1 : 0; }
  for (int q = 0; q < 4; ++q) mat_mul(M, M, M);                          // A^16
  for (int l = 0; l < 64; ++l) {
    for (int i = 0; i < 16; ++i) c->Mk[l][i] = (double)pw[i];
    mat_mul(pw, M, pw);
  }
  for (int j = 0; j < 6; ++j) {
    for (int i = 0; i < 16; ++i) c->P[j][i] = (double)M[i];
    mat_mul(M, M, M);
  }
  for (int i = 0; i < 16; ++i) c->W[i] = (double)M[i];                   // A^1024
  mat_mul(M, M, M);
  mat_mul(M, M, M);
  for (int i = 0; i < 16; ++i) c->TT[i] = (double)M[i];                  // A^4096
  c->s = (int)loud_sub(rate);
  c->pad[0] = c->pad[1] = c->pad[2] = 0;
}

// loud_constants per rate, kept for the few rates a process meters at (the models' and 48 kHz): a server step copies 9 KB
// instead of redoing some eighty 4x4 products
static void loud_constants_cached(int rate, LoudConst* out) {
  static std::mutex mu;
  static struct { int rate; LoudConst c; } cache[4];
  static int used = 0, next = 0;
  std::lock_guard<std::mutex> lock(mu);
  for (int i = 0; i < used; ++i)
    if (cache[i].rate == rate) { *out = cache[i].c; return; }
  loud_constants(rate, out);
  const int at = used < 4 ? used++ : (next++ & 3);
  cache[at].rate = rate;
  cache[at].c = *out;
}

static int groups_rate_impl(const void* const* frags, const int* lens, int n, int dtype, const int* group_n, const int* group_gap,
                            int n_groups, void* out, long long* group_off, void* table, void* workspace, const float* h, int h_len,
                            int up, int down, int out_fmt, gsv_stream_t stream, const LoudArgs* loud) {
  GSV_REQUIRE(n >= 0 && n_groups >= 0 && (dtype == GSV_F16 || dtype == GSV_F32), "postprocess_groups_rate: bad argument");
  GSV_REQUIRE(out_fmt == GSV_OUT_S16 || out_fmt == GSV_OUT_MULAW || out_fmt == GSV_OUT_ALAW || out_fmt == GSV_OUT_F32,
              "postprocess_groups_rate: out_fmt = %d is none of GSV_OUT_S16, _MULAW, _ALAW, _F32", out_fmt);
  GSV_REQUIRE(up >= 1 && down >= 1, "postprocess_groups_rate: up = %d, down = %d (both >= 1)", up, down);
  GSV_REQUIRE(h_len >= 1 && (h_len & 1), "postprocess_groups_rate: h_len = %d must be odd (the filter is centred)", h_len);
  GSV_REQUIRE(h_len <= kRsMaxFilter, "postprocess_groups_rate: h_len = %d, the kernel takes filters up to %d taps", h_len, kRsMaxFilter);
  const long long win = rs_window(kRsTile, up, down, h_len);
  GSV_REQUIRE(win <= kRsLdsFloats, "postprocess_groups_rate: %d -> %d with %d taps needs an input window of %lld samples per tile, "
              "the kernel holds %d", down, up, h_len, win, kRsLdsFloats);
  GSV_REQUIRE(n_groups == 0 || (group_n && group_gap && group_off), "postprocess_groups_rate: null group table");
  long long in_groups = 0;
  for (int g = 0; g < n_groups; ++g) {
    GSV_REQUIRE(group_n[g] >= 0 && group_gap[g] >= 0, "postprocess_groups_rate: group %d has %d sentences, gap %d", g, group_n[g], group_gap[g]);
    in_groups += group_n[g];
  }
  GSV_REQUIRE(in_groups == n, "postprocess_groups_rate: the groups hold %lld sentences, n is %d", in_groups, n);
  if (n == 0) {
    for (int g = 0; g <= n_groups && group_off; ++g) group_off[g] = 0;
    GSV_REQUIRE(!loud || loud->n_spans == 0, "postprocess_groups_loud: %d spans and no sentence", loud->n_spans);
    return GSV_OK;
  }
  GSV_REQUIRE(frags && lens && out && table && workspace && h, "postprocess_groups_rate: null pointer");
  if (loud) {                                                            // every descriptor is checked before the first launch
    GSV_REQUIRE(loud->spans && loud->report, "postprocess_groups_loud: null span table or report");
    GSV_REQUIRE(loud->rate > 0, "postprocess_groups_loud: rate = %d must be positive", loud->rate);
    GSV_REQUIRE(loud_sub(loud->rate) > kLoudTile / 2, "postprocess_groups_loud: rate = %d: a 100 ms sub-block has to be longer than %d "
                "samples (a tile of the meter touches at most three)", loud->rate, kLoudTile / 2);
    int g = 0, g_first = 0, prev_end = 0;
    for (int k = 0; k < loud->n_spans; ++k) {
      const gsv_loud_span& sp = loud->spans[k];
      GSV_REQUIRE(sp.count >= 1 && sp.first >= 0 && (long long)sp.first + sp.count <= n,
                  "postprocess_groups_loud: span %d names sentences [%d, %d + %d) of %d", k, sp.first, sp.first, sp.count, n);
      GSV_REQUIRE(sp.first >= prev_end, "postprocess_groups_loud: span %d starts at sentence %d, the span before it ends at %d "
                  "(spans are sorted and do not overlap)", k, sp.first, prev_end);
      while (g < n_groups && sp.first >= g_first + group_n[g]) g_first += group_n[g++];
      GSV_REQUIRE(g < n_groups && sp.first + sp.count <= g_first + group_n[g], "postprocess_groups_loud: span %d crosses a group border", k);
      GSV_REQUIRE(sp.gaps == 0 || sp.gaps == 1, "postprocess_groups_loud: span %d has gaps = %d (0 or 1)", k, sp.gaps);
      GSV_REQUIRE(sp.peak_db <= 0.f, "postprocess_groups_loud: span %d has peak_db = %g (a ceiling is at most 0 dBFS)", k, (double)sp.peak_db);
      GSV_REQUIRE(sp.target != sp.target || (sp.target >= -70.f && sp.target <= 0.f),
                  "postprocess_groups_loud: span %d has target = %g LUFS (-70 .. 0, or NaN to meter only)", k, (double)sp.target);
      prev_end = sp.first + sp.count;
    }
  }
  GroupSent* sent = (GroupSent*)table;
  RateGroup* groups = (RateGroup*)(sent + n);
  GroupTile* tiles = (GroupTile*)(groups + n_groups);
  long long off = 0, n_peak = 0, n_tiles = 0;
  int i = 0;
  for (int g = 0; g < n_groups; ++g) {
    group_off[g] = off;
    const int sent0 = i;
    long long at = 0;                                                    // position in the group's stream
    for (int k = 0; k < group_n[g]; ++k, ++i) {
      GSV_REQUIRE(lens[i] >= 0 && (lens[i] == 0 || frags[i]), "postprocess_groups_rate: sentence %d is null", i);
      sent[i] = GroupSent{frags[i], at, lens[i], group_gap[g], 0u, 0};
      for (long long t = 0; t * kGroupTile < lens[i]; ++t) tiles[n_peak++] = GroupTile{i, (int)(t * kGroupTile)};
      at += (long long)lens[i] + group_gap[g];
    }
    const long long m = (at * up + down - 1) / down;
    GSV_REQUIRE(at <= 0x7fffffffLL && m <= 0x7fffffffLL, "postprocess_groups_rate: group %d has %lld samples, %lld outputs", g, at, m);
    GSV_REQUIRE(n_tiles <= 0x7fffffffLL, "postprocess_groups_rate: %lld tiles are too many for one launch", n_tiles);
    groups[g] = RateGroup{off, at, sent0, group_n[g], (int)m, (int)n_tiles};
    n_tiles += (m + kRsTile - 1) / kRsTile;
    off += m;
  }
  group_off[n_groups] = off;
  GSV_REQUIRE(n_peak <= 0x7fffffffLL && n_tiles <= 0x7fffffffLL, "postprocess_groups_rate: %lld tiles are too many for one launch",
              n_peak > n_tiles ? n_peak : n_tiles);
  hipStream_t s = (hipStream_t)stream;
  size_t bytes = (size_t)n * sizeof(GroupSent) + (size_t)n_groups * sizeof(RateGroup) + (size_t)n_peak * sizeof(GroupTile);
  // the meter's tables behind the rate call's: constants | spans | tiles are uploaded; states | partials | energies stay on the device
  const size_t at_const = align16(bytes);
  long long n_mtiles = 0, n_sub = 0;
  if (loud) {
    LoudConst* lc = (LoudConst*)((char*)table + at_const);
    loud_constants_cached(loud->rate, lc);
    LoudSpan* lsp = (LoudSpan*)(lc + 1);
    LoudTile* lt = (LoudTile*)(lsp + loud->n_spans);
    for (int k = 0; k < loud->n_spans; ++k) {
      const gsv_loud_span& sp = loud->spans[k];
      long long N = 0;
      for (int j = sp.first; j < sp.first + sp.count; ++j) {
        N += (long long)sent[j].len + (sp.gaps ? sent[j].gap : 0);
        sent[j].pad = k + 1;
      }
      lsp[k] = LoudSpan{sp.first, sp.count, sp.gaps, (int)N, (int)n_mtiles, (int)n_sub, sp.target, sp.peak_db};
      if (loud->energy_off) loud->energy_off[k] = n_sub;
      for (long long t = 0; t * kLoudTile < N; ++t) lt[n_mtiles++] = LoudTile{k, (int)t};
      n_sub += (N + lc->s - 1) / lc->s;
    }
    GSV_REQUIRE(n_mtiles <= 0x7fffffffLL && n_sub <= 0x7fffffffLL, "postprocess_groups_loud: %lld tiles are too many for one launch", n_mtiles);
    if (loud->energy_off) loud->energy_off[loud->n_spans] = n_sub;
    bytes = at_const + sizeof(LoudConst) + (size_t)loud->n_spans * sizeof(LoudSpan) + (size_t)n_mtiles * sizeof(LoudTile);
  }
  GSV_HIP(hipMemcpyAsync(workspace, table, bytes, hipMemcpyHostToDevice, s));
  GroupSent* dsent = (GroupSent*)workspace;
  const RateGroup* dgroups = (const RateGroup*)(dsent + n);
  const GroupTile* dtiles = (const GroupTile*)(dgroups + n_groups);
  if (n_peak) {
    if (dtype == GSV_F16) GSV_LAUNCH((post_groups_peak_kernel<_Float16>), dim3((unsigned)n_peak), dim3(256), 0, s, dsent, dtiles);
    else GSV_LAUNCH((post_groups_peak_kernel<float>), dim3((unsigned)n_peak), dim3(256), 0, s, dsent, dtiles);
  }
  const LoudReport* drep = nullptr;
  if (loud) {
    const LoudConst* dc = (const LoudConst*)((char*)workspace + at_const);
    const LoudSpan* dsp = (const LoudSpan*)(dc + 1);
    const LoudTile* dlt = (const LoudTile*)(dsp + loud->n_spans);
    double* state = (double*)((char*)workspace + align16(bytes));
    double* partial = state + 4 * (size_t)n_mtiles;
    double* energies = loud->energies ? loud->energies : partial + 3 * (size_t)n_mtiles;
    const GroupSent* cs = dsent;
    if (n_mtiles) {                                                      // none: every span is empty
      const dim3 grid((unsigned)n_mtiles);
      if (dtype == GSV_F16) GSV_LAUNCH((loud_state_kernel<_Float16>), grid, dim3(256), 0, s, cs, dsp, dlt, dc, state);
      else GSV_LAUNCH((loud_state_kernel<float>), grid, dim3(256), 0, s, cs, dsp, dlt, dc, state);
      GSV_LAUNCH(loud_carry_kernel, dim3((unsigned)cdiv(loud->n_spans, 64)), dim3(64), 0, s, dsp, loud->n_spans, dc, state);
      if (dtype == GSV_F16) GSV_LAUNCH((loud_energy_kernel<_Float16>), grid, dim3(256), 0, s, cs, dsp, dlt, dc, (const double*)state, partial);
      else GSV_LAUNCH((loud_energy_kernel<float>), grid, dim3(256), 0, s, cs, dsp, dlt, dc, (const double*)state, partial);
    }
    GSV_LAUNCH(loud_gate_kernel, dim3((unsigned)loud->n_spans), dim3(256), 0, s, cs, dsp, dc, (const double*)partial, energies, loud->report);
    if (!loud->write) return GSV_OK;
    drep = loud->report;
  }
  if (n_tiles == 0) return GSV_OK;
  const int win_cap = (int)win, h_at = win_cap > kRsTile ? win_cap : kRsTile;
  const bool hlds = (long long)h_at + h_len <= kRsLdsFloats;
  const size_t lds = sizeof(float) * (size_t)(h_at + (hlds ? h_len : 0));
  if (dtype == GSV_F16)
    return rate_launch_fmt<_Float16>(out_fmt, hlds, (unsigned)n_tiles, lds, s, (const GroupSent*)dsent, dgroups, n_groups, h, h_len, up, down,
                                     out, win_cap, drep);
  return rate_launch_fmt<float>(out_fmt, hlds, (unsigned)n_tiles, lds, s, (const GroupSent*)dsent, dgroups, n_groups, h, h_len, up, down, out,
                                win_cap, drep);
}

}  // namespace gsv

extern "C" int gsv_postprocess_groups_rate(const void* const* frags, const int* lens, int n, int dtype, const int* group_n,
                                           const int* group_gap, int n_groups, void* out, long long* group_off, void* table,
                                           void* workspace, const float* h, int h_len, int up, int down, int out_fmt,
                                           gsv_stream_t stream) {
  return gsv::groups_rate_impl(frags, lens, n, dtype, group_n, group_gap, n_groups, out, group_off, table, workspace, h, h_len, up, down,
                               out_fmt, stream, nullptr);
}

extern "C" long long gsv_postprocess_groups_loud_workspace(const int* lens, int n, const int* group_n, const int* group_gap, int n_groups,
                                                           int rate, int n_spans) {
  using namespace gsv;
  const long long base = gsv_postprocess_groups_rate_workspace(lens, n, n_groups);
  if (base < 0 || n_spans < 0 || rate <= 0 || loud_sub(rate) < 1 || (n_groups > 0 && (!group_n || !group_gap))) return -1;
  long long total = 0;                                                   // samples of all streams; spans do not overlap
  int i = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (group_n[g] < 0 || group_gap[g] < 0 || (long long)i + group_n[g] > n) return -1;
    for (int k = 0; k < group_n[g]; ++k, ++i) total += (long long)lens[i] + group_gap[g];
  }
  const long long tiles = total / kLoudTile + n_spans, subs = total / loud_sub(rate) + n_spans;
  return (long long)align16((size_t)base) + (long long)sizeof(LoudConst) + (long long)n_spans * (long long)sizeof(LoudSpan) +
         tiles * (long long)sizeof(LoudTile) + 16 + tiles * 7 * 8 + subs * 8;
}

extern "C" int gsv_postprocess_groups_loud(const void* const* frags, const int* lens, int n, int dtype, const int* group_n,
                                           const int* group_gap, int n_groups, void* out, long long* group_off, void* table,
                                           void* workspace, const float* h, int h_len, int up, int down, int out_fmt, int rate,
                                           const gsv_loud_span* spans, int n_spans, gsv_loud_report* report, gsv_stream_t stream) {
  GSV_REQUIRE(n_spans >= 0, "postprocess_groups_loud: n_spans = %d", n_spans);
  const gsv::LoudArgs loud{rate, spans, n_spans, (gsv::LoudReport*)report, nullptr, nullptr, true};
  return gsv::groups_rate_impl(frags, lens, n, dtype, group_n, group_gap, n_groups, out, group_off, table, workspace, h, h_len, up, down,
                               out_fmt, stream, n_spans ? &loud : nullptr);
}

extern "C" int gsv_op_loudness(const void* const* frags, const int* lens, int n, int dtype, const int* group_n, const int* group_gap,
                               int n_groups, int rate, const gsv_loud_span* spans, int n_spans, double* energies, long long* energy_off,
                               gsv_loud_report* report, void* table, void* workspace, gsv_stream_t stream) {
  GSV_REQUIRE(n_spans >= 1 && n_groups >= 1 && energies && energy_off, "op_loudness: needs a group, a span, energies and energy_off");
  static const float one = 1.f;                                          // the write launch is left out: neither is read
  std::vector<long long> group_off((size_t)n_groups + 1);
  const gsv::LoudArgs loud{rate, spans, n_spans, (gsv::LoudReport*)report, energies, energy_off, false};
  return gsv::groups_rate_impl(frags, lens, n, dtype, group_n, group_gap, n_groups, (void*)energies, group_off.data(), table, workspace,
                               &one, 1, 1, 1, GSV_OUT_F32, stream, &loud);
}
