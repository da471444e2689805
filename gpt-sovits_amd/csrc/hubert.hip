// The two kernels of the packed HuBERT pass (gsv/feature_extractor/cnhubert.py HubertModel.batch) that the
// row-wise launches cannot stand in for: the per-channel normalisation over time restricted to each audio's own rows, and a row
// gather that lays the audios out with gaps for the positional conv and packs them densely again after it.
#include <algorithm>

#include "common.h"
#include "engine.h"

namespace gsv {

// ---------------------------------------------------------------------------------------------------------------
// gsv_op_channel_norm_seg: y = act((x - mean_{s,c}) * rstd_{s,c} * gamma_c + beta_c) on the rows of segment s, 0 elsewhere.
// Memory bound (x is read twice and y written once; nothing else is of that order), so every access is a 16-byte one: a lane
// owns VEC = 16 / sizeof(T) adjacent channels, a wave one row of 64 * VEC channels (1 KiB contiguous), a workgroup four rows
// at a time.  Three launches:
//   stats    one workgroup per (chunk, channel tile); a chunk is kCnChunk rows counted from ITS SEGMENT'S first row.  Wave w
//            sums d and d^2, d = x - (the segment's first row), over rows w, w + 4, .. of the chunk in fp32, the four waves meet in
//            LDS in the order 0..3, one partial (sum, sum of squares) per (chunk, channel) goes to scratch.  The shift keeps
//            E[d^2] - E[d]^2 from cancelling where a channel's mean is large against its deviation: unshifted fp32 partials
//            (cnorm_stats_kernel's) lost 2.6e-4 of y at mean / std = 34, 5 x the fp32 bar of the test.
//   finalize one thread per (segment, channel): the segment's partials in chunk order, in double, as cnorm_apply_kernel does;
//            mean and rstd * gamma go to scratch behind the partials.
//   apply    one wave per 8 rows of the whole array: y = act((x - mean) * (rstd * gamma) + beta); a row outside every segment
//            is stored as 0.
// Nothing above depends on where a segment lies or on which others share the call, so a segment's output bits do not either.
// Table entry (int4, the library's segment-table slots): first row, rows, first chunk, chunks.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCnChunk = 256;          // rows per partial (gsv.h states the scratch size with this number)
constexpr int kCnApplyRows = 8;        // rows per wave of the apply pass

template <typename T> struct CnVec;
template <> struct CnVec<_Float16> { typedef h8 type; static constexpr int VEC = 8; };
template <> struct CnVec<float> { typedef f4 type; static constexpr int VEC = 4; };

// the segment whose chunk range holds `chunk` (stats) / the last segment that starts at or before `row`, -1 if none (apply)
__device__ __forceinline__ int cn_find(const int4* __restrict__ tab, int n_seg, int key, bool by_chunk) {
  int lo = 0, hi = n_seg - 1;
  if ((by_chunk ? tab[0].z : tab[0].x) > key) return -1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((by_chunk ? tab[mid].z : tab[mid].x) <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename T>
__global__ __launch_bounds__(256) void cnorm_seg_stats_kernel(const T* __restrict__ x, int C, const int4* __restrict__ tab, int n_seg,
                                                              float* __restrict__ part /*[chunks][2][C]*/) {
  typedef typename CnVec<T>::type V;
  constexpr int VEC = CnVec<T>::VEC, TILE = 64 * VEC;
  __shared__ float red[4][2][VEC][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x, c = blockIdx.y * TILE + lane * VEC;
  const int4 sg = tab[cn_find(tab, n_seg, chunk, true)];
  const int r0 = (chunk - sg.z) * kCnChunk, r1 = min(sg.y, r0 + kCnChunk);     // rows relative to the segment's first
  float s[VEC], q[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = q[j] = 0.f;
  if (c < C) {
    const T* xp = x + (long long)sg.x * C + c;
    const V kv = *(const V*)xp;                 // the shift: the segment's first row
    float k[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) k[j] = to_f(kv[j]);
    int r = r0 + wave;
    for (; r + 12 < r1; r += 16) {              // four independent 16-byte loads in flight per lane
      V v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const V*)(xp + (long long)(r + 4 * u) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < VEC; ++j) { const float f = to_f(v[u][j]) - k[j]; s[j] += f; q[j] += f * f; }
    }
    for (; r < r1; r += 4) {
      const V v = *(const V*)(xp + (long long)r * C);
#pragma unroll
      for (int j = 0; j < VEC; ++j) { const float f = to_f(v[j]) - k[j]; s[j] += f; q[j] += f * f; }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) { red[wave][0][j][lane] = s[j]; red[wave][1][j][lane] = q[j]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * TILE; i += 256) {
    const int k = i / TILE, cc = i % TILE, co = blockIdx.y * TILE + cc;
    if (co >= C) continue;
    const int j = cc % VEC, ln = cc / VEC;
    const float v = ((red[0][k][j][ln] + red[1][k][j][ln]) + red[2][k][j][ln]) + red[3][k][j][ln];
    part[((long long)chunk * 2 + k) * C + co] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void cnorm_seg_finalize_kernel(const T* __restrict__ x, const float* __restrict__ part, int C,
                                                                 const int4* __restrict__ tab, const float* __restrict__ gamma, float eps,
                                                                 float* __restrict__ coef /*[n_seg][2][C]: mean, rstd * gamma*/) {
  const int c = blockIdx.x * 256 + threadIdx.x, sgi = blockIdx.y;
  if (c >= C) return;
  const int4 sg = tab[sgi];
  double s = 0.0, q = 0.0;
  const float* p = part + (long long)sg.z * 2 * C + c;
#pragma unroll 4
  for (int k = 0; k < sg.w; ++k) { s += p[(long long)(2 * k) * C]; q += p[(long long)(2 * k + 1) * C]; }
  const int Tn = sg.y;
  const double shift = (double)to_f(x[(long long)sg.x * C + c]), sm = s / Tn;
  const float var = fmaxf((float)(q / Tn - sm * sm), 0.f);
  coef[((long long)sgi * 2 + 0) * C + c] = (float)(shift + sm);
  coef[((long long)sgi * 2 + 1) * C + c] = rsqrtf(var + eps) * gamma[c];
}

template <typename T>
__global__ __launch_bounds__(256) void cnorm_seg_apply_kernel(const T* __restrict__ x, int Tn, int C, const int4* __restrict__ tab, int n_seg,
                                                              const float* __restrict__ coef, const float* __restrict__ beta, int act,
                                                              T* __restrict__ y) {
  typedef typename CnVec<T>::type V;
  constexpr int VEC = CnVec<T>::VEC, TILE = 64 * VEC, R = kCnApplyRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.y * TILE + lane * VEC;
  const int row0 = (blockIdx.x * 4 + wave) * R;
  if (c >= C || row0 >= Tn) return;
  V v[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int row = min(row0 + u, Tn - 1);
    v[u] = *(const V*)(x + (long long)row * C + c);
  }
  int sgi = cn_find(tab, n_seg, row0, false), loaded = -2;
  float mean[VEC], a[VEC], b[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) b[j] = beta[c + j];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int row = row0 + u;
    if (row >= Tn) break;
    while (sgi + 1 < n_seg && tab[sgi + 1].x <= row) ++sgi;
    const bool inside = sgi >= 0 && row < tab[sgi].x + tab[sgi].y;
    V o;
    if (inside) {
      if (loaded != sgi) {
        const float* ca = coef + (long long)sgi * 2 * C + c;
#pragma unroll
        for (int j = 0; j < VEC; ++j) { mean[j] = ca[j]; a[j] = ca[C + j]; }
        loaded = sgi;
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = (T)post_act_f(act, (to_f(v[u][j]) - mean[j]) * a[j] + b[j]);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = (T)0.f;
    }
    *(V*)(y + (long long)row * C + c) = o;
  }
}

template <typename T>
static int channel_norm_seg(const void* x, int Tn, int C, int n_seg, const int4* tab, int chunks, const float* gamma, const float* beta,
                            float eps, int act, float* scratch, void* y, hipStream_t s) {
  constexpr int TILE = 64 * CnVec<T>::VEC;
  float* coef = scratch + (long long)chunks * 2 * C;
  GSV_LAUNCH(cnorm_seg_stats_kernel<T>, dim3(chunks, cdiv(C, TILE)), dim3(256), 0, s, (const T*)x, C, tab, n_seg, scratch);
  GSV_LAUNCH(cnorm_seg_finalize_kernel<T>, dim3(cdiv(C, 256), n_seg), dim3(256), 0, s, (const T*)x, (const float*)scratch, C, tab, gamma, eps,
             coef);
  GSV_LAUNCH(cnorm_seg_apply_kernel<T>, dim3(cdiv(Tn, 4 * kCnApplyRows), cdiv(C, TILE)), dim3(256), 0, s, (const T*)x, Tn, C, tab, n_seg,
             (const float*)coef, beta, act, (T*)y);
  return GSV_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// gsv_op_gather_rows: y[r] = x[idx[r]], a zero row for idx[r] < 0, a NaN row for idx[r] >= rows_in (gsv_op_embed_ln's convention
// for an id outside its table: the device cannot report).  One thread per 16-byte piece of an output row.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ x, int rows_in, const int* __restrict__ idx,
                                                          int rows_out, int pieces /* 16-byte pieces per row */, uint4 nan16,
                                                          uint4* __restrict__ y) {
  const long long n = (long long)rows_out * pieces;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int r = (int)(i / pieces), p = (int)(i - (long long)r * pieces);
    const int src = idx[r];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (src >= rows_in) v = nan16;
    else if (src >= 0) v = x[(long long)src * pieces + p];
    y[i] = v;
  }
}

}  // namespace gsv

extern "C" {

int gsv_op_channel_norm_seg(const void* x, int Tn, int C, int n_seg, const int32_t* seg_start, const int32_t* seg_len,
                            const float* gamma, const float* beta, float eps, int act, float* scratch, void* y, int dtype,
                            gsv_stream_t stream) {
  GSV_REQUIRE(x && y && gamma && beta && scratch && seg_start && seg_len && Tn > 0 && C > 0, "op_channel_norm_seg: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_channel_norm_seg: bad dtype");
  GSV_REQUIRE(n_seg >= 1 && n_seg <= gsveng::kSegTableMax, "op_channel_norm_seg: %d segments (1 .. %d)", n_seg, gsveng::kSegTableMax);
  const int vec = dtype == GSV_F16 ? 8 : 4;
  GSV_REQUIRE(C % vec == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0,
              "op_channel_norm_seg: C = %d must be a multiple of %d and x / y 16-byte aligned", C, vec);
  long long end = 0, chunks = 0;
  for (int i = 0; i < n_seg; ++i) {
    GSV_REQUIRE(seg_len[i] >= 1, "op_channel_norm_seg: segment %d has length %d", i, seg_len[i]);
    GSV_REQUIRE(seg_start[i] >= end, "op_channel_norm_seg: segment %d starts at row %d, before row %lld where the one before it ends "
                "(segments are disjoint and ascending)", i, seg_start[i], end);
    end = (long long)seg_start[i] + seg_len[i];
    GSV_REQUIRE(end <= Tn, "op_channel_norm_seg: segment %d ends at row %lld of %d", i, end, Tn);
    chunks += gsv::cdiv(seg_len[i], gsv::kCnChunk);
  }
  gsveng::SegTable tb;                              // holds the library context until it goes out of scope
  GSV_RC(gsveng::seg_table_begin(&tb));
  int chunk0 = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int nc = gsv::cdiv(seg_len[i], gsv::kCnChunk);
    tb.image[4 * i] = seg_start[i]; tb.image[4 * i + 1] = seg_len[i]; tb.image[4 * i + 2] = chunk0; tb.image[4 * i + 3] = nc;
    chunk0 += nc;
  }
  hipStream_t s = (hipStream_t)stream;
  GSV_RC(gsveng::seg_table_upload(&tb, n_seg, s));
  const int4* tab = (const int4*)tb.dev;
  GSV_RC(GSV_WITH_DTYPE(dtype, gsv::channel_norm_seg<T>(x, Tn, C, n_seg, tab, (int)chunks, gamma, beta, eps, act, scratch, y, s)));
  return gsveng::seg_table_end(&tb, s);
}

int gsv_op_gather_rows(const void* x, int rows_in, const int32_t* idx, int rows_out, int C, void* y, int dtype, gsv_stream_t stream) {
  GSV_REQUIRE(x && idx && y && rows_in > 0 && rows_out > 0 && C > 0, "op_gather_rows: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_gather_rows: bad dtype");
  const long long row_bytes = (long long)C * (long long)gsv::dt_size(dtype);
  GSV_REQUIRE(row_bytes % 16 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0,
              "op_gather_rows: rows of %lld bytes: rows and both arrays must be multiples of 16 bytes", row_bytes);
  const int pieces = (int)(row_bytes / 16);
  const unsigned nan = dtype == GSV_F16 ? 0x7e007e00u : 0x7fc00000u;
  const long long n = (long long)rows_out * pieces;
  const int blocks = (int)std::min<long long>((n + 255) / 256, 1 << 16);
  GSV_LAUNCH(gsv::gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, rows_in, idx, rows_out, pieces,
             make_uint4(nan, nan, nan, nan), (uint4*)y);
  return GSV_OK;
}

}
