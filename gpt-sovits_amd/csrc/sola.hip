// SOLA stitching of vocoder fragments (H17, reference TTS_infer_pack/TTS.py:1611-1637) for gfx950.
//
// For each neighbouring pair (f1, f2): cross-correlate the last `ov` samples of f1 with the first `ov` samples of f2
// (F.conv1d with padding ov/2, last output dropped), idx = first argmax; f1 loses its last ov-idx samples, f2 its
// first idx samples, and the first ov-idx samples of what is left of f2 are cross-faded with f1's tail under a periodic
// Hann window of length 2(ov-idx).  Everything (correlation, argmax, cross-fade, compaction) stays on the device;
// the argmax offsets never visit the host, only the final length does.
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

template <typename T, int FMT, bool HLDS>
__global__ __launch_bounds__(256) void post_groups_rate_kernel(const GroupSent* __restrict__ sent, const RateGroup* __restrict__ groups,
                                                               int n_groups, const float* __restrict__ h, int L, int up, int down,
                                                               void* __restrict__ out, int win_cap) {
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
  const long long w1 = w0 + wn;
  // the sentence under w0: the last one that starts at or before it (an empty sentence without a gap covers nothing)
  int sa = G.sent0, sb = G.sent0 + G.n_sent - 1;
  while (sa < sb) {
    const int mid = (sa + sb + 1) >> 1;
    if (sent[mid].dst <= w0) sa = mid; else sb = mid - 1;
  }
  for (int si = sa; si < G.sent0 + G.n_sent; ++si) {
    const GroupSent S = sent[si];
    if (S.dst >= w1) break;
    const long long b = S.dst > w0 ? S.dst : w0;                        // [b, e): this sentence and its gap inside the window
    const long long e = min(S.dst + S.len + S.gap, w1);
    const int cnt = (int)(e - b), at = (int)(b - w0);
    const int first = (int)(b - S.dst);                                  // sample of the sentence at b (>= len: inside the gap)
    const int live = max(0, min(cnt, S.len - first));                    // samples that are loaded; the rest are the gap's zeros
    const T* __restrict__ x = (const T*)S.src + first;
    const bool divide = S.peak > 0x3f800000u && S.peak <= 0x7f800000u;   // peak > 1 and no NaN
    const T denom = (T)__uint_as_float(S.peak);
    for (int i = tid; i < cnt; i += 256) {
      float f = 0.f;
      if (i < live) {
        T v = x[i];
        if (divide) v = (T)((float)v / (float)denom);                    // postprocess_kernel's arithmetic, in T
        f = (float)v;
      }
      xs[at + i] = f;
    }
  }
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
                       const float* h, int L, int up, int down, void* out, int win_cap) {
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

extern "C" int gsv_postprocess_groups_rate(const void* const* frags, const int* lens, int n, int dtype, const int* group_n,
                                           const int* group_gap, int n_groups, void* out, long long* group_off, void* table,
                                           void* workspace, const float* h, int h_len, int up, int down, int out_fmt,
                                           gsv_stream_t stream) {
  using namespace gsv;
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
    return GSV_OK;
  }
  GSV_REQUIRE(frags && lens && out && table && workspace && h, "postprocess_groups_rate: null pointer");
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
  const size_t bytes = (size_t)n * sizeof(GroupSent) + (size_t)n_groups * sizeof(RateGroup) + (size_t)n_peak * sizeof(GroupTile);
  GSV_HIP(hipMemcpyAsync(workspace, table, bytes, hipMemcpyHostToDevice, s));
  GroupSent* dsent = (GroupSent*)workspace;
  const RateGroup* dgroups = (const RateGroup*)(dsent + n);
  const GroupTile* dtiles = (const GroupTile*)(dgroups + n_groups);
  if (n_peak) {
    if (dtype == GSV_F16) GSV_LAUNCH((post_groups_peak_kernel<_Float16>), dim3((unsigned)n_peak), dim3(256), 0, s, dsent, dtiles);
    else GSV_LAUNCH((post_groups_peak_kernel<float>), dim3((unsigned)n_peak), dim3(256), 0, s, dsent, dtiles);
  }
  if (n_tiles == 0) return GSV_OK;
  const int win_cap = (int)win, h_at = win_cap > kRsTile ? win_cap : kRsTile;
  const bool hlds = (long long)h_at + h_len <= kRsLdsFloats;
  const size_t lds = sizeof(float) * (size_t)(h_at + (hlds ? h_len : 0));
  if (dtype == GSV_F16)
    return rate_launch_fmt<_Float16>(out_fmt, hlds, (unsigned)n_tiles, lds, s, (const GroupSent*)dsent, dgroups, n_groups, h, h_len, up, down,
                                     out, win_cap);
  return rate_launch_fmt<float>(out_fmt, hlds, (unsigned)n_tiles, lds, s, (const GroupSent*)dsent, dgroups, n_groups, h, h_len, up, down, out,
                                win_cap);
}
