// Small shared kernels: error state, dtype conversion, row LayerNorm.
#include "common.h"
#include "engine.h"

namespace gsv {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

static thread_local unsigned long long g_conv_route = 0;
static thread_local unsigned long long g_pair_route = 0;   // the last fused-pair launch, kept aside: a decode ends in conv_post
void set_conv_route(unsigned long long code) {
  g_conv_route = code;
  if ((code & 255) == ROUTE_CONV_PAIR) g_pair_route = code;
}
static thread_local unsigned g_attn_route = 0;             // family | qt << 8 of the last attention launch (common.h)
void set_attn_route(int family, int qt) { g_attn_route = (unsigned)(family & 255) | (unsigned)(qt & 255) << 8; }

template <typename T> __global__ void convert_kernel(const float* __restrict__ s, T* __restrict__ d, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) d[i] = (T)s[i];
}

int launch_convert(const float* src, void* dst, int dtype, long long n, hipStream_t s) {
  if (n <= 0) return GSV_OK;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (dtype == GSV_F16) hipLaunchKernelGGL(convert_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, src, (_Float16*)dst, n);
  else hipLaunchKernelGGL(convert_kernel<float>, dim3(blocks), dim3(256), 0, s, src, (float*)dst, n);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

// One wave per row.  y = LN(x + res) * gamma + beta, statistics in fp32 (two-pass).
template <typename TX, typename TR, typename TY>
__global__ void layernorm_kernel(const TX* __restrict__ x, const TR* __restrict__ res, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, TY* __restrict__ y, int rows, int C, float eps,
                                 const int* __restrict__ row_seg) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (row_seg && row_seg[row] < 0) {           // segmented decode: a gap row is stored as 0 (ConvArgs::row_seg)
    for (int c = lane; c < C; c += 64) y[(long long)row * C + c] = (TY)0.f;
    return;
  }
  const TX* xr = x + (long long)row * C;
  const TR* rr = res ? res + (long long)row * C : nullptr;
  if (C <= 512) {
    // the row fits in 8 registers per lane: ONE pass over global memory instead of three dependent ones
    float v[8];
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < C ? to_f(xr[c]) + (rr ? to_f(rr[c]) : 0.f) : 0.f;
      s1 += v[i];
    }
    const float mean1 = wave_sum(s1) / (float)C;
    float q1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = (lane + 64 * i < C) ? v[i] - mean1 : 0.f;
      q1 += d * d;
    }
    const float rstd1 = rsqrtf(wave_sum(q1) / (float)C + eps);
    TY* yr1 = y + (long long)row * C;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = lane + 64 * i;
      if (c < C) yr1[c] = (TY)((v[i] - mean1) * rstd1 * gamma[c] + beta[c]);
    }
    return;
  }
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += to_f(xr[c]) + (rr ? to_f(rr[c]) : 0.f);
  const float mean = wave_sum(sum) / (float)C;
  float var = 0.f;
  for (int c = lane; c < C; c += 64) {
    float d = to_f(xr[c]) + (rr ? to_f(rr[c]) : 0.f) - mean;
    var += d * d;
  }
  const float rstd = rsqrtf(wave_sum(var) / (float)C + eps);
  TY* yr = y + (long long)row * C;
  for (int c = lane; c < C; c += 64) {
    float v = to_f(xr[c]) + (rr ? to_f(rr[c]) : 0.f);
    yr[c] = (TY)((v - mean) * rstd * gamma[c] + beta[c]);
  }
}

// BERT's embedding stage: y[i] = LN(word[ids[i]] + pos[pos_ids[i]] + add) * gamma + beta, fp32 tables, sums and statistics, fp16
// rows out.  One wave per row, the row held in registers (C <= 1024): the tables are read once.  A row whose id or position
// lies outside its table reads nothing and is stored as NaN: the host checks its own ids, the device cannot report.
__global__ __launch_bounds__(256) void embed_ln_kernel(const float* __restrict__ word, const float* __restrict__ pos,
                                                       const float* __restrict__ add, const int* __restrict__ ids,
                                                       const int* __restrict__ pos_ids, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, _Float16* __restrict__ y, int rows, int C,
                                                       int n_word, int n_pos, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int id = ids[row], pi = pos_ids[row];
  _Float16* yr = y + (long long)row * C;
  if (id < 0 || id >= n_word || pi < 0 || pi >= n_pos) {
    for (int c = lane; c < C; c += 64) yr[c] = (_Float16)__builtin_nanf("");
    return;
  }
  const float* wr = word + (long long)id * C;
  const float* pr = pos + (long long)pi * C;
  float v[16];
  float s1 = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < C ? wr[c] + pr[c] + (add ? add[c] : 0.f) : 0.f;
    s1 += v[i];
  }
  const float mean = wave_sum(s1) / (float)C;
  float q1 = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float d = (lane + 64 * i < C) ? v[i] - mean : 0.f;
    q1 += d * d;
  }
  const float rstd = rsqrtf(wave_sum(q1) / (float)C + eps);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = lane + 64 * i;
    if (c < C) yr[c] = (_Float16)((v[i] - mean) * rstd * gamma[c] + beta[c]);
  }
}

template <typename TX, typename TR, typename TY>
static int ln_launch(const void* x, const void* res, const float* g, const float* b, void* y, int rows, int C, float eps,
                     hipStream_t s, const int* row_seg) {
  hipLaunchKernelGGL((layernorm_kernel<TX, TR, TY>), dim3(cdiv(rows, 4)), dim3(256), 0, s, (const TX*)x, (const TR*)res,
                     g, b, (TY*)y, rows, C, eps, row_seg);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

int launch_layernorm(int dtype, const void* x, int x_f32, const void* res, int res_f32, const float* gamma,
                     const float* beta, void* y, int y_f32, int rows, int C, float eps, hipStream_t s, const int* row_seg) {
  if (rows <= 0) return GSV_OK;
  const bool h = dtype == GSV_F16;
  const bool xf = x_f32 || !h, rf = res_f32 || !h, yf = y_f32 || !h;
  if (xf && rf && yf) return ln_launch<float, float, float>(x, res, gamma, beta, y, rows, C, eps, s, row_seg);
  if (xf && rf && !yf) return ln_launch<float, float, _Float16>(x, res, gamma, beta, y, rows, C, eps, s, row_seg);
  if (xf && !rf && !yf) return ln_launch<float, _Float16, _Float16>(x, res, gamma, beta, y, rows, C, eps, s, row_seg);
  if (!xf && !rf && !yf) return ln_launch<_Float16, _Float16, _Float16>(x, res, gamma, beta, y, rows, C, eps, s, row_seg);
  if (!xf && !rf && yf) return ln_launch<_Float16, _Float16, float>(x, res, gamma, beta, y, rows, C, eps, s, row_seg);
  if (!xf && rf && !yf) return ln_launch<_Float16, float, _Float16>(x, res, gamma, beta, y, rows, C, eps, s, row_seg);
  set_error("layernorm: unsupported dtype combination");
  return GSV_ERR_ARG;
}


// ---------------------------------------------------------------------------------------------------------------
// Reference-audio front-end helpers: framing of a waveform into a GEMM operand, STFT
// magnitude, per-channel normalisation over time (HuBERT's GroupNorm(512, 512)).  The GEMMs themselves are conv_gemm.
// ---------------------------------------------------------------------------------------------------------------
// out[t][k] = x[reflect(t * hop + k - pad)] for k < flen, 0 for flen <= k < ld   (torch.stft / F.pad(mode="reflect") framing;
// pad = 0: plain strided frames, the operand of a Conv1d(1, C, flen, stride = hop))
template <typename T>
__global__ void frame_kernel(const float* __restrict__ x, int n, int flen, int hop, int pad, int ld, int T_out, T* __restrict__ out) {
  const int t = blockIdx.x;
  if (t >= T_out) return;
  for (int k = threadIdx.x; k < ld; k += blockDim.x) {
    float v = 0.f;
    if (k < flen) {
      int i = t * hop + k - pad;
      if (i < 0) i = -i;                       // reflect without repeating the edge sample
      if (i >= n) i = 2 * (n - 1) - i;
      v = (i >= 0 && i < n) ? x[i] : 0.f;
    }
    out[(long long)t * ld + k] = (T)v;
  }
}

// frame_kernel per segment: row r of segment s = (tab[s].z <= r < tab[s].z + tab[s].w) frames the audio x[tab[s].x ..][tab[s].y],
// reflected at that audio's own ends; a row between segments is left alone.  tab: int4 (first sample, samples, first row, rows).
template <typename T>
__global__ void frame_seg_kernel(const float* __restrict__ x, const int4* __restrict__ tab, int n_seg, int flen, int hop, int pad, int ld,
                                 int row0, T* __restrict__ out) {
  const int row = row0 + blockIdx.x;
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].z <= row) lo = mid; else hi = mid - 1;
  }
  const int4 sg = tab[lo];
  const int t = row - sg.z, n = sg.y;
  if (t < 0 || t >= sg.w) return;
  const float* xs = x + (long long)sg.x;
  for (int k = threadIdx.x; k < ld; k += blockDim.x) {
    float v = 0.f;
    if (k < flen) {
      int i = t * hop + k - pad;
      if (i < 0) i = -i;
      if (i >= n) i = 2 * (n - 1) - i;
      v = (i >= 0 && i < n) ? xs[i] : 0.f;
    }
    out[(long long)row * ld + k] = (T)v;
  }
}

// spec[b][t] = sqrt(re^2 + im^2 + eps), ri [T][2 * bins] (re | im column blocks) -> spec [bins][T]  (mel_processing.py:73)
__global__ void magnitude_kernel(const float* __restrict__ ri, int T, int bins, float eps, float* __restrict__ spec) {
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, b = b0 + tx;
    float v = 0.f;
    if (t < T && b < bins) {
      const float re = ri[(long long)t * 2 * bins + b], im = ri[(long long)t * 2 * bins + bins + b];
      v = eps < 0.f ? re * re + im * im : sqrtf(re * re + im * im + eps);
    }
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int b = b0 + i, t = t0 + tx;
    if (b < bins && t < T) spec[(long long)b * T + t] = tile[tx][i];
  }
}

// same magnitude kept frame-major [T][ld] (zero up to ld): the left operand of the mel-filterbank GEMM
__global__ void magnitude_tm_kernel(const float* __restrict__ ri, int T, int bins, int ld, float eps, float* __restrict__ spec) {
  const int b = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  if (b >= ld) return;
  float v = 0.f;
  if (b < bins) {
    const float re = ri[(long long)t * 2 * bins + b], im = ri[(long long)t * 2 * bins + bins + b];
    v = eps < 0.f ? re * re + im * im : sqrtf(re * re + im * im + eps);
  }
  spec[(long long)t * ld + b] = v;
}

// attentional feature fusion mix (eres2net/fusion.py:22-27 with t = tanh(local_att)): out = x (1 + t) + y (1 - t)
__global__ void aff_mix_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ t, long long n,
                               float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { const float a = t[i]; out[i] = x[i] * (1.f + a) + y[i] * (1.f - a); }
}

// out[c] = mean over t of x[t][c]  (ERes2NetV2.forward3's temporal mean, ERes2NetV2.py:258); one thread per column, 64-column
// workgroups x 16 time slices reduced through LDS
__global__ __launch_bounds__(1024) void time_mean_kernel(const float* __restrict__ x, int T, int ld, float* __restrict__ out) {
  __shared__ float part[16][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), sl = threadIdx.x >> 6;
  float s = 0.f;
  if (c < ld) for (int t = sl; t < T; t += 16) s += x[(long long)t * ld + c];
  part[sl][threadIdx.x & 63] = s;
  __syncthreads();
  if (sl == 0 && c < ld) {
    float v = 0.f;
    for (int k = 0; k < 16; ++k) v += part[k][threadIdx.x & 63];
    out[c] = v / (float)T;
  }
}

// The packed speaker-embedding pass (ERes2NetV2.forward3_segments): the audios lie back to back on the time
// axis, and these two kernels keep each to itself.
// zero_rows: 0 to rows[0 .. n_rows) of n_maps maps [T][4 * pieces] (blockIdx.y = map), one thread per 16-byte piece.  The base
// pointers are kernel arguments: no table in memory, one launch for the four sub-band maps of a block.
__global__ __launch_bounds__(256) void zero_rows_kernel(gsv_zero_maps maps, int T, int pieces, const int* __restrict__ rows, int n_rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n_rows * pieces) return;
  const int r = (int)(i / pieces), p = (int)(i - (long long)r * pieces);
  const int row = rows[r];
  if (row < 0 || row >= T) return;             // the host checked its copy of the list; the device's own is not trusted further
  f4* base = (f4*)maps.p[blockIdx.y];
  base[(long long)row * pieces + p] = f4{0.f, 0.f, 0.f, 0.f};
}

// out[s][c] = mean over the rows of segment s of x[t][c], in time_mean_kernel's order counted from the segment's first row, so the
// bits of a segment depend on its own rows alone.  A lane owns four adjacent columns (16-byte loads, a wave reads 1 KiB of a
// row), a workgroup 256 columns x 16 time slices; tab: int4 per segment (first row, rows, -, -).
__global__ __launch_bounds__(1024) void time_mean_seg_kernel(const float* __restrict__ x, int ld, const int4* __restrict__ tab,
                                                             float* __restrict__ out) {
  __shared__ float part[16][4][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const int4 sg = tab[blockIdx.y];
  const float* xs = x + (long long)sg.x * ld;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < ld)
    for (int t = sl; t < sg.y; t += 16) {
      const f4 v = *(const f4*)(xs + (long long)t * ld + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += v[j];
    }
#pragma unroll
  for (int j = 0; j < 4; ++j) part[sl][j][lane] = s[j];
  __syncthreads();
  if (sl == 0 && c < ld) {
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = 0.f;
      for (int k = 0; k < 16; ++k) v += part[k][j][lane];
      o[j] = v / (float)sg.y;
    }
    *(f4*)(out + (long long)blockIdx.y * ld + c) = o;
  }
}

// y[t][c] = act((x[t][c] - mean_c) * rstd_c * gamma[c] + beta[c]), statistics over t (biased variance), channels-last.
// Two kernels: per-(channel block, time slice) partial sums -> finalize + apply.
template <typename T>
__global__ void cnorm_stats_kernel(const T* __restrict__ x, int Tn, int C, int slices, float* __restrict__ part /*[slices][2][C]*/) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, sl = blockIdx.y;
  if (c >= C) return;
  const int per = (Tn + slices - 1) / slices, t0 = sl * per, t1 = min(Tn, t0 + per);
  float s = 0.f, q = 0.f;
  for (int t = t0; t < t1; ++t) { const float v = to_f(x[(long long)t * C + c]); s += v; q += v * v; }
  part[((long long)sl * 2 + 0) * C + c] = s;
  part[((long long)sl * 2 + 1) * C + c] = q;
}
template <typename T>
__global__ void cnorm_apply_kernel(const T* __restrict__ x, int Tn, int C, int slices, const float* __restrict__ part,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int act, T* __restrict__ y) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int sl = 0; sl < slices; ++sl) { s += part[((long long)sl * 2 + 0) * C + c]; q += part[((long long)sl * 2 + 1) * C + c]; }
  const float mean = (float)(s / Tn);
  const float var = fmaxf((float)(q / Tn - (s / Tn) * (s / Tn)), 0.f);
  const float a = rsqrtf(var + eps) * gamma[c], b = beta[c] - mean * a;
  const int per = (Tn + gridDim.y - 1) / gridDim.y, t0 = blockIdx.y * per, t1 = min(Tn, t0 + per);
  for (int t = t0; t < t1; ++t) y[(long long)t * C + c] = (T)post_act_f(act, to_f(x[(long long)t * C + c]) * a + b);
}

}  // namespace gsv

extern "C" {
const char* gsv_last_error(void) { return gsv::get_error(); }
int gsv_abi_version(void) { return 1; }
uint64_t gsv_debug_last_conv_route(int reset) {
  const uint64_t code = gsv::g_conv_route;
  if (reset) gsv::g_conv_route = 0;
  return code;
}

uint64_t gsv_debug_last_pair_route(int reset) {
  const uint64_t r = gsv::g_pair_route;
  if (reset) gsv::g_pair_route = 0;
  return r;
}
uint64_t gsv_debug_last_attn_route(int reset) {
  const uint64_t r = gsv::g_attn_route;
  if (reset) gsv::g_attn_route = 0;
  return r;
}
int gsv_init(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    gsv::set_error("gsv_init: no HIP device (%s)", hipGetErrorString(e));
    return GSV_ERR_HIP;
  }
  if (device < 0 || device >= n) {
    gsv::set_error("gsv_init: device %d out of range (%d devices)", device, n);
    return GSV_ERR_ARG;
  }
  GSV_HIP(hipSetDevice(device));
  hipDeviceProp_t p;
  GSV_HIP(hipGetDeviceProperties(&p, device));
  if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
    gsv::set_error("gsv_init: device %d is %s, this library is built for gfx950 only", device, p.gcnArchName);
    return GSV_ERR_HIP;
  }
  return GSV_OK;
}

int gsv_op_layernorm(const void* x, const void* res, const float* gamma, const float* beta, void* y, int rows, int C,
                     float eps, int dtype, gsv_stream_t stream) {
  return gsv::launch_layernorm(dtype, x, 0, res, 0, gamma, beta, y, 0, rows, C, eps, (hipStream_t)stream);
}

int gsv_op_flash_attn64(const void* qkv, int T, int heads, float scale, void* vt_scratch, void* out, gsv_stream_t stream) {
  const int inner = heads * 64;
  return gsv::launch_flash_attn64_f16(qkv, 3 * inner, (const _Float16*)qkv + inner, 3 * inner, (const _Float16*)qkv + 2 * inner, 3 * inner,
                                      vt_scratch, T, heads, scale, out, inner, (hipStream_t)stream);
}

int gsv_op_flash_attn64_seg(const void* qkv, int n_seg, const int32_t* seg_lens, int heads, float scale, void* vt_scratch, void* out,
                            gsv_stream_t stream) {
  const int inner = heads * 64;
  return gsv::launch_flash_attn64_f16_seg(qkv, 3 * inner, (const _Float16*)qkv + inner, 3 * inner, (const _Float16*)qkv + 2 * inner,
                                          3 * inner, vt_scratch, n_seg, seg_lens, heads, scale, out, inner, (hipStream_t)stream);
}

int gsv_op_flash_attn64_rows(const void* qkv, int T, int heads, int rows, float scale, const float* rope_cs, int rope_half, int qt,
                             void* vt_scratch, void* out, gsv_stream_t stream) {
  GSV_REQUIRE(qkv && vt_scratch && out, "op_flash_attn64_rows: null pointer");
  GSV_REQUIRE(T >= 1 && rows >= 1 && heads >= 1, "op_flash_attn64_rows: bad shape T=%d rows=%d heads=%d", T, rows, heads);
  GSV_REQUIRE(qt == 0 || qt == 1 || qt == 2 || qt == 4, "op_flash_attn64_rows: qt %d is not 0 (by shape), 1, 2 or 4", qt);
  GSV_REQUIRE((long long)heads * 64 * 3 * ((long long)T + 8) <= 0x7fffffffLL, "op_flash_attn64_rows: T=%d x heads=%d exceeds the index range", T, heads);
  const int inner = heads * 64;
  GSV_REQUIRE(rope_half >= 0 && 2 * (long long)rope_half <= inner, "op_flash_attn64_rows: rope_half %d outside [0, %d]", rope_half, inner / 2);
  GSV_REQUIRE(rope_cs || rope_half == 0, "op_flash_attn64_rows: rope_half %d without a cos / sin table", rope_half);
  const int ld = 3 * inner, ldv = (T + 31) / 32 * 32;
  const long long xz = ((long long)T + 8) * ld, vtz = (long long)inner * ldv + 64, oz = ((long long)T + 8) * inner;
  return gsv::launch_flash_attn64_f16_rows(qkv, ld, (const _Float16*)qkv + inner, ld, (const _Float16*)qkv + 2 * inner, ld, vt_scratch, T, heads,
                                           scale, out, inner, (hipStream_t)stream, rope_cs, rope_cs ? rope_half : 0, rows, xz, vtz, oz, qt);
}

int gsv_op_flash_attn64_seg_qt(const void* qkv, int n_seg, const int32_t* seg_lens, int heads, float scale, int qt, void* vt_scratch,
                               void* out, gsv_stream_t stream) {
  const int inner = heads * 64;
  return gsv::launch_flash_attn64_f16_seg(qkv, 3 * inner, (const _Float16*)qkv + inner, 3 * inner, (const _Float16*)qkv + 2 * inner,
                                          3 * inner, vt_scratch, n_seg, seg_lens, heads, scale, out, inner, (hipStream_t)stream, qt);
}

int gsv_op_attention(const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0, int Tq, int Tk, int heads, int kc,
                     float scale, const float* rel_k, const float* rel_v, const int32_t* kr, int dtype, int route, void* out, int ldo,
                     gsv_stream_t stream) {
  GSV_REQUIRE(q && kv && out, "op_attention: null pointer");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_attention: bad dtype %d", dtype);
  GSV_REQUIRE(route >= 0 && route <= 2, "op_attention: unknown route %d", route);
  GSV_REQUIRE(Tq >= 1 && Tk >= 1 && heads >= 1 && heads <= 65535 && kc >= 1, "op_attention: bad shape Tq=%d Tk=%d heads=%d kc=%d", Tq, Tk, heads, kc);
  GSV_REQUIRE(qcol0 >= 0 && kcol0 >= 0 && vcol0 >= 0 && (long long)qcol0 + (long long)heads * kc <= ldq &&
              (long long)(kcol0 > vcol0 ? kcol0 : vcol0) + (long long)heads * kc <= ldkv && (long long)heads * kc <= ldo,
              "op_attention: the head columns do not fit the leading dimensions");
  GSV_REQUIRE((long long)heads * Tq * Tk <= 0x7fffffffLL / 4, "op_attention: %d x %d x %d scores exceed the index range", heads, Tq, Tk);
  GSV_REQUIRE(!rel_k == !rel_v, "op_attention: rel_k and rel_v come together");
  if (route == 1) {
    GSV_REQUIRE(dtype == GSV_F16, "op_attention: route 1 (fused) is fp16 only");
    GSV_REQUIRE(kc == 96, "op_attention: route 1 (fused) is built for kc 96, not %d", kc);
    GSV_REQUIRE(rel_k && rel_v, "op_attention: route 1 (fused) needs rel_k and rel_v");
    GSV_REQUIRE(Tq == Tk, "op_attention: route 1 (fused) needs Tq == Tk");
  }
  gsveng::Ctx c("op_attention");
  c.dtype = dtype;
  const bool fused = route == 1 || (route == 0 && gsveng::attention_is_fused(&c, q, ldq, kv, ldkv, Tq, Tk, kc, rel_k, rel_v));
  if (kr) {
    for (int i = 0; i < Tq; ++i) {
      const int lo = kr[2 * i], hi = kr[2 * i + 1];
      GSV_REQUIRE(lo >= 0 && hi <= Tk && lo <= hi, "op_attention: key range [%d, %d) of query %d leaves [0, %d]", lo, hi, i, Tk);
      // the fused kernel skips the chunks in front of its first row's lo and behind its last row's hi, and divides by the row's mass
      GSV_REQUIRE(!fused || (lo < hi && (i == 0 || (lo >= kr[2 * i - 2] && hi >= kr[2 * i - 1]))),
                  "op_attention: key range [%d, %d) of query %d is empty or descends (the fused kernel needs non-decreasing, non-empty ranges)",
                  lo, hi, i);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  int* d_kr = nullptr;
  int rc = GSV_OK;
  if (kr) {
    if (hipMalloc((void**)&d_kr, (size_t)Tq * 8) != hipSuccess || hipMemcpy(d_kr, kr, (size_t)Tq * 8, hipMemcpyHostToDevice) != hipSuccess) {
      gsv::set_error("op_attention: key-range upload failed");
      rc = GSV_ERR_HIP;
    }
  }
  if (!rc) {
    rc = gsveng::attention_routed(&c, s, q, ldq, qcol0, kv, ldkv, kcol0, vcol0, Tq, Tk, heads, kc, scale, rel_k, rel_v, out, ldo, d_kr, fused);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) { gsv::set_error("op_attention: a kernel failed"); rc = GSV_ERR_HIP; }
  }
  gsveng::free_ctx(&c);
  (void)hipFree(d_kr);
  return rc;
}

int gsv_op_embed_ln(const float* word, int n_word, const float* pos, int n_pos, const float* add, const int32_t* ids,
                    const int32_t* pos_ids, const float* gamma, const float* beta, void* y, int rows, int C, float eps,
                    gsv_stream_t stream) {
  GSV_REQUIRE(word && pos && ids && pos_ids && gamma && beta && y && rows > 0 && n_word > 0 && n_pos > 0, "op_embed_ln: bad argument");
  GSV_REQUIRE(C >= 1 && C <= 1024, "op_embed_ln: C = %d, the row is held in registers up to 1024", C);
  hipLaunchKernelGGL(gsv::embed_ln_kernel, dim3(gsv::cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, word, pos, add, ids, pos_ids,
                     gamma, beta, (_Float16*)y, rows, C, n_word, n_pos, eps);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

int gsv_op_flash_rel96(const void* qkv, int T, int heads, float scale, const float* rel_k, const float* rel_v, void* vt_scratch,
                       void* out, gsv_stream_t stream) {
  const int H = heads * 96;
  return gsv::launch_flash_rel96_f16(qkv, 3 * H, (const _Float16*)qkv + H, 3 * H, (const _Float16*)qkv + 2 * H, 3 * H, vt_scratch, T, heads,
                                     scale, rel_k, rel_v, out, H, (hipStream_t)stream);
}

// gsv_conv_desc -> the launchers' argument block (gsv_op_conv1d and gsv_op_gemm_panel take the same descriptor)
static gsv::ConvArgs conv_desc_args(const gsv_conv_desc* d) {
  gsv::ConvArgs a;
  a.x = d->x; a.w = d->w; a.bias = d->bias; a.y = d->y; a.res = d->res; a.gate = d->gate;
  a.T_in = d->T_in; a.T_out = d->T_out; a.Cin = d->Cin; a.Cout = d->Cout; a.taps = d->taps;
  a.stride = d->stride; a.dil = d->dil; a.pad = d->pad;
  a.ldx = d->Cin; a.ldw = d->taps * d->Cin;
  a.pre_act = d->pre_act; a.pre_slope = d->pre_slope; a.post_act = d->post_act; a.scale = d->scale;
  a.accumulate = d->accumulate; a.out_f32 = d->out_f32;
  a.res_f32 = d->res_dtype == 0 ? d->out_f32 : d->res_dtype == 1;
  a.y_col0 = d->y_col0; a.w_nt = d->w_nt; a.z_res = d->z_res;
  a.gate_rows = d->gate_rows; a.gate_ld = d->gate_ld;
  if (d->ups_u > 0) {
    // transposed conv restated as a polyphase conv: Cout = u * real_cout virtual channels
    a.ups_u = d->ups_u; a.ups_pad = d->ups_pad; a.ups_cout = d->Cout / d->ups_u;
    a.ldy = a.ups_cout; a.ldr = a.ups_cout;
    a.T_virt = d->T_in + d->taps - 1;
  } else {
    a.ldy = d->Cout; a.ldr = d->Cout;
    a.T_virt = d->T_out;
  }
  if (d->ldx > 0) a.ldx = d->ldx;
  if (d->ldw > 0) a.ldw = d->ldw;
  if (d->ldy > 0) { a.ldy = d->ldy; a.ldr = d->ldy; }
  if (d->ldr > 0) a.ldr = d->ldr;
  if (d->Z > 1) { a.Z = d->Z; a.xz = d->xz; a.wz = d->wz; a.yz = d->yz; a.bz = d->bz; a.rz = d->rz ? d->rz : d->yz; }
  return a;
}

int gsv_op_conv1d(const gsv_conv_desc* d, int dtype, gsv_stream_t stream) {
  return gsv::launch_conv_gemm(dtype, conv_desc_args(d), (hipStream_t)stream);
}

int gsv_op_gemm_panel(const gsv_conv_desc* d, int dtype, int tile, gsv_stream_t stream) {
  GSV_REQUIRE(d, "op_gemm_panel: null descriptor");
  GSV_REQUIRE(tile >= 0 && tile <= 4, "op_gemm_panel: tile %d is not a member of the family (0 = by shape, 1..4)", tile);
  const gsv::ConvArgs a = conv_desc_args(d);
  GSV_REQUIRE(gsv::gemm_panel_eligible(dtype, a), "op_gemm_panel: the descriptor is not one of the prefill's three GEMM forms");
  const int rc = gsv::launch_gemm_panel(dtype, a, tile, (hipStream_t)stream);
  GSV_REQUIRE(rc != 1, "op_gemm_panel: not eligible");
  return rc;
}

int gsv_op_frame(const float* x, int n, int frame_len, int hop, int pad, int ld, int T_out, void* out, int dtype, gsv_stream_t stream) {
  GSV_REQUIRE(x && out && n > 0 && frame_len > 0 && hop > 0 && ld >= frame_len && T_out > 0, "op_frame: bad argument");
  GSV_REQUIRE(pad >= 0 && pad < n, "op_frame: reflect padding %d needs more than %d samples", pad, pad);
  GSV_REQUIRE((long long)(T_out - 1) * hop + frame_len - pad <= (long long)n + pad, "op_frame: frames run past the (padded) signal");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_frame: bad dtype");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == GSV_F16) hipLaunchKernelGGL(gsv::frame_kernel<_Float16>, dim3(T_out), dim3(256), 0, s, x, n, frame_len, hop, pad, ld, T_out, (_Float16*)out);
  else hipLaunchKernelGGL(gsv::frame_kernel<float>, dim3(T_out), dim3(256), 0, s, x, n, frame_len, hop, pad, ld, T_out, (float*)out);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

int gsv_op_frame_seg(const float* x, int n_x, int frame_len, int hop, int pad, int ld, int n_seg, const int32_t* x_start,
                     const int32_t* x_len, const int32_t* row_start, const int32_t* row_len, int rows, void* out, int dtype,
                     gsv_stream_t stream) {
  GSV_REQUIRE(x && out && x_start && x_len && row_start && row_len && n_x > 0 && frame_len > 0 && hop > 0 && ld >= frame_len && rows > 0 &&
              pad >= 0, "op_frame_seg: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_frame_seg: bad dtype");
  GSV_REQUIRE(n_seg >= 1 && n_seg <= gsveng::kSegTableMax, "op_frame_seg: %d segments (1 .. %d)", n_seg, gsveng::kSegTableMax);
  long long x_end = 0, r_end = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int n = x_len[i], T = row_len[i];
    GSV_REQUIRE(n >= 1 && T >= 1, "op_frame_seg: segment %d has %d samples and %d frames", i, n, T);
    GSV_REQUIRE(pad < n, "op_frame_seg: reflect padding %d needs more than %d samples, segment %d has %d", pad, pad, i, n);
    GSV_REQUIRE((long long)(T - 1) * hop + frame_len - pad <= (long long)n + pad, "op_frame_seg: the frames of segment %d run past its "
                "(padded) signal", i);
    GSV_REQUIRE(x_start[i] >= x_end && row_start[i] >= r_end, "op_frame_seg: segment %d starts before the one before it ends (sample and "
                "row ranges are disjoint and ascending)", i);
    x_end = (long long)x_start[i] + n;
    r_end = (long long)row_start[i] + T;
    GSV_REQUIRE(x_end <= n_x && r_end <= rows, "op_frame_seg: segment %d ends at sample %lld of %d, row %lld of %d", i, x_end, n_x, r_end, rows);
  }
  gsveng::SegTable tb;                              // holds the library context until it goes out of scope
  GSV_RC(gsveng::seg_table_begin(&tb));
  for (int i = 0; i < n_seg; ++i) {
    tb.image[4 * i] = x_start[i]; tb.image[4 * i + 1] = x_len[i]; tb.image[4 * i + 2] = row_start[i]; tb.image[4 * i + 3] = row_len[i];
  }
  hipStream_t s = (hipStream_t)stream;
  GSV_RC(gsveng::seg_table_upload(&tb, n_seg, s));
  const int4* tab = (const int4*)tb.dev;
  const int r0 = row_start[0], nr = (int)r_end - r0;  // rows in front of the first segment and behind the last get no workgroup
  if (dtype == GSV_F16)
    GSV_LAUNCH(gsv::frame_seg_kernel<_Float16>, dim3(nr), dim3(256), 0, s, x, tab, n_seg, frame_len, hop, pad, ld, r0, (_Float16*)out);
  else
    GSV_LAUNCH(gsv::frame_seg_kernel<float>, dim3(nr), dim3(256), 0, s, x, tab, n_seg, frame_len, hop, pad, ld, r0, (float*)out);
  return gsveng::seg_table_end(&tb, s);
}

int gsv_op_magnitude(const float* re_im, int T, int bins, float eps, int frame_ld, float* spec, gsv_stream_t stream) {
  GSV_REQUIRE(re_im && spec && T > 0 && bins > 0, "op_magnitude: bad argument");
  GSV_REQUIRE(frame_ld == 0 || frame_ld >= bins, "op_magnitude: frame_ld %d is smaller than %d bins", frame_ld, bins);
  if (frame_ld == 0)
    hipLaunchKernelGGL(gsv::magnitude_kernel, dim3(gsv::cdiv(T, 32), gsv::cdiv(bins, 32)), dim3(256), 0, (hipStream_t)stream, re_im, T, bins, eps, spec);
  else
    hipLaunchKernelGGL(gsv::magnitude_tm_kernel, dim3(gsv::cdiv(frame_ld, 256), T), dim3(256), 0, (hipStream_t)stream, re_im, T, bins, frame_ld, eps, spec);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

int gsv_op_conv_pair(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, int T, int C, int taps,
                     int dil, float scale, int accumulate, gsv_stream_t stream) {
  GSV_REQUIRE(gsv::conv_pair_supported(GSV_F16, C, taps, dil, T, false), "op_conv_pair: C must be 16, 32 or 64, taps 3, 5, 7, 9 or 11, (taps - 1) / 2 * dil <= 25, T >= 256");
  gsv::ConvPairArgs a;
  a.x = (const _Float16*)x; a.w1 = (const _Float16*)w1; a.b1 = b1; a.w2 = (const _Float16*)w2; a.b2 = b2; a.y = (_Float16*)y;
  a.T = T; a.C = C; a.taps = taps; a.dil = dil; a.ldx = C; a.ldy = C; a.scale = scale; a.accumulate = accumulate;
  return gsv::launch_conv_pair(a, (hipStream_t)stream);
}

int gsv_op_conv_pair_seg(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, int T, int C, int taps,
                         int dil, float scale, int accumulate, const int32_t* row_seg, gsv_stream_t stream) {
  GSV_REQUIRE(row_seg, "op_conv_pair_seg: row_seg is null (gsv_op_conv_pair is the unmasked pair)");
  GSV_REQUIRE(gsv::conv_pair_supported(GSV_F16, C, taps, dil, T, true), "op_conv_pair_seg: C must be 16 or 32, taps 3, 5, 7, 9 or 11, (taps - 1) / 2 * dil <= 25, T >= 256");
  gsv::ConvPairArgs a;
  a.x = (const _Float16*)x; a.w1 = (const _Float16*)w1; a.b1 = b1; a.w2 = (const _Float16*)w2; a.b2 = b2; a.y = (_Float16*)y;
  a.T = T; a.C = C; a.taps = taps; a.dil = dil; a.ldx = C; a.ldy = C; a.scale = scale; a.accumulate = accumulate;
  return gsv::launch_conv_pair_seg(a, row_seg, (hipStream_t)stream);
}

int gsv_op_aff_mix(const float* x, const float* y, const float* t, long long n, float* out, gsv_stream_t stream) {
  GSV_REQUIRE(x && y && t && out && n > 0, "op_aff_mix: bad argument");
  hipLaunchKernelGGL(gsv::aff_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, t, n, out);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

int gsv_op_time_mean(const float* x, int T, int ld, float* out, gsv_stream_t stream) {
  GSV_REQUIRE(x && out && T > 0 && ld > 0, "op_time_mean: bad argument");
  hipLaunchKernelGGL(gsv::time_mean_kernel, dim3(gsv::cdiv(ld, 64)), dim3(1024), 0, (hipStream_t)stream, x, T, ld, out);
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}

int gsv_op_zero_rows(const gsv_zero_maps* maps, int n_maps, int T, int ld, const int32_t* rows, const int32_t* rows_host, int n_rows,
                     gsv_stream_t stream) {
  GSV_REQUIRE(maps && rows && rows_host && T > 0 && ld > 0 && n_rows >= 0, "op_zero_rows: bad argument");
  GSV_REQUIRE(n_maps >= 1 && n_maps <= 8, "op_zero_rows: %d maps (1 .. 8)", n_maps);
  GSV_REQUIRE(ld % 4 == 0, "op_zero_rows: ld = %d must be a multiple of 4 floats", ld);
  for (int i = 0; i < n_maps; ++i)
    GSV_REQUIRE(maps->p[i] && ((uintptr_t)maps->p[i] % 16) == 0, "op_zero_rows: map %d is null or not 16-byte aligned", i);
  for (int i = 0; i < n_rows; ++i)
    GSV_REQUIRE(rows_host[i] >= 0 && rows_host[i] < T, "op_zero_rows: row %d (entry %d) is outside [0, %d)", rows_host[i], i, T);
  if (n_rows == 0) return GSV_OK;
  const int pieces = ld / 4;
  const long long blocks = ((long long)n_rows * pieces + 255) / 256;
  GSV_REQUIRE(blocks <= 0x7fffffffLL, "op_zero_rows: %d rows of %d floats are too many for one launch", n_rows, ld);
  GSV_LAUNCH(gsv::zero_rows_kernel, dim3((unsigned)blocks, n_maps), dim3(256), 0, (hipStream_t)stream, *maps, T, pieces, rows, n_rows);
  return GSV_OK;
}

int gsv_op_time_mean_seg(const float* x, int T, int ld, int n_seg, const int32_t* seg_start, const int32_t* seg_len, float* out,
                         gsv_stream_t stream) {
  GSV_REQUIRE(x && out && seg_start && seg_len && T > 0 && ld > 0, "op_time_mean_seg: bad argument");
  GSV_REQUIRE(n_seg >= 1 && n_seg <= gsveng::kSegTableMax, "op_time_mean_seg: %d segments (1 .. %d)", n_seg, gsveng::kSegTableMax);
  GSV_REQUIRE(ld % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0,
              "op_time_mean_seg: ld = %d must be a multiple of 4 and x / out 16-byte aligned", ld);
  long long end = 0;
  for (int i = 0; i < n_seg; ++i) {
    GSV_REQUIRE(seg_len[i] >= 1, "op_time_mean_seg: segment %d has length %d", i, seg_len[i]);
    GSV_REQUIRE(seg_start[i] >= end, "op_time_mean_seg: segment %d starts at row %d, before row %lld where the one before it ends "
                "(segments are disjoint and ascending)", i, seg_start[i], end);
    end = (long long)seg_start[i] + seg_len[i];
    GSV_REQUIRE(end <= T, "op_time_mean_seg: segment %d ends at row %lld of %d", i, end, T);
  }
  gsveng::SegTable tb;                              // holds the library context until it goes out of scope
  GSV_RC(gsveng::seg_table_begin(&tb));
  for (int i = 0; i < n_seg; ++i) {
    tb.image[4 * i] = seg_start[i]; tb.image[4 * i + 1] = seg_len[i]; tb.image[4 * i + 2] = 0; tb.image[4 * i + 3] = 0;
  }
  hipStream_t s = (hipStream_t)stream;
  GSV_RC(gsveng::seg_table_upload(&tb, n_seg, s));
  GSV_LAUNCH(gsv::time_mean_seg_kernel, dim3(gsv::cdiv(ld, 256), n_seg), dim3(1024), 0, s, x, ld, (const int4*)tb.dev, out);
  return gsveng::seg_table_end(&tb, s);
}

int gsv_op_channel_norm(const void* x, int T, int C, const float* gamma, const float* beta, float eps, int act, float* scratch,
                        void* y, int dtype, gsv_stream_t stream) {
  GSV_REQUIRE(x && y && gamma && beta && scratch && T > 0 && C > 0, "op_channel_norm: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_channel_norm: bad dtype");
  const int slices = 64;                      // scratch: 64 * 2 * C floats
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(gsv::cdiv(C, 64), slices);
  if (dtype == GSV_F16) {
    hipLaunchKernelGGL(gsv::cnorm_stats_kernel<_Float16>, grid, dim3(64), 0, s, (const _Float16*)x, T, C, slices, scratch);
    hipLaunchKernelGGL(gsv::cnorm_apply_kernel<_Float16>, grid, dim3(64), 0, s, (const _Float16*)x, T, C, slices, scratch, gamma, beta, eps, act, (_Float16*)y);
  } else {
    hipLaunchKernelGGL(gsv::cnorm_stats_kernel<float>, grid, dim3(64), 0, s, (const float*)x, T, C, slices, scratch);
    hipLaunchKernelGGL(gsv::cnorm_apply_kernel<float>, grid, dim3(64), 0, s, (const float*)x, T, C, slices, scratch, gamma, beta, eps, act, (float*)y);
  }
  GSV_HIP(hipGetLastError());
  return GSV_OK;
}
}
