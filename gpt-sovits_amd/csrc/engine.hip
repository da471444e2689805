// The engine context's helpers (engine.h, gsveng::Ctx): tensor staging and upload, the workspace arena, the conv and attention
// launches on a handle's dtype, and the small kernels only these helpers launch.  Every engine handle derives from Ctx and
// passes itself here.
#include "engine.h"

namespace gsv {

// segment map of an upsampled resolution: every boundary (segment start, length, gap) scales by the same factor `up`
__global__ void expand_seg_kernel(const int* __restrict__ seg, int up, long long n, int* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = seg[i / up];
}

// drop the gaps from the padded waveform: segment s's samples move left by s gaps of `gap` samples
__global__ void compact_wav_kernel(const float* __restrict__ src, const int* __restrict__ seg_f, int up, long long gap, long long n,
                                   float* __restrict__ wav) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int sg = seg_f[t / up];
  if (sg >= 0) wav[t - sg * gap] = src[t];
}

// fp32 channels-first [C_total][T] -> T channels-last [T][C] (first C channels)
template <typename T>
__global__ void cf_to_cl_kernel(const float* __restrict__ src, int Tn, int C, T* __restrict__ dst, int ldd = 0) {
  if (ldd == 0) ldd = C;
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < Tn) ? src[(long long)c * Tn + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    int t = t0 + i, c = c0 + tx;
    if (t < Tn && c < C) dst[(long long)t * ldd + c] = (T)tile[tx][i];
  }
}

// Vt[z][c][j] = src[j][col0 + z*kc + c], zero padded to ldv columns
template <typename T>
__global__ void transpose_v_kernel(const T* __restrict__ src, int ld, int col0, int kc, int Tk, int ldv, T* __restrict__ vt) {
  __shared__ float tile[32][33];
  const int z = blockIdx.z;
  const int j0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    int j = j0 + i, c = c0 + tx;
    tile[i][tx] = (j < Tk && c < kc) ? to_f(src[(long long)j * ld + col0 + z * kc + c]) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    int c = c0 + i, j = j0 + tx;
    if (c < kc && j < ldv) vt[((long long)z * kc + c) * ldv + j] = (T)(j < Tk ? tile[tx][i] : 0.f);
  }
}

// Row softmax of fp32 scores [Z][Tq][Tk] -> P (T, row stride ldp, zero padded).  With a relative
// window (w > 0): scores[i][j] += qs_i . rel_k[j-i+w] for |j-i| <= w before the softmax
// (attentions.py:238-243, qs = q/sqrt(kc) is folded via `qscale`), and the 2w+1 band
// probabilities are kept in `band` for the relative-value term (attentions.py:253-256).
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ scores, int Tq, int Tk, int ldp,
                                                           T* __restrict__ P, const T* __restrict__ q, int ldq, int kc,
                                                           const float* __restrict__ rel_k, int w, float qscale,
                                                           float* __restrict__ band, const int* __restrict__ kr) {
  const int i = blockIdx.x, z = blockIdx.y;
  const float* srow = scores + ((long long)z * Tq + i) * Tk;
  T* prow = P + ((long long)z * Tq + i) * ldp;
  // segmented decode (kr != null): row i sees keys [kr[2i], kr[2i+1]) only; an empty range gives a zero row
  const int klo = kr ? kr[2 * i] : 0, khi = kr ? kr[2 * i + 1] : Tk;
  if (khi <= klo) {
    for (int j = threadIdx.x; j < ldp; j += 256) prow[j] = (T)0.f;
    if (w > 0 && threadIdx.x < 2 * w + 1) band[((long long)z * Tq + i) * (2 * w + 1) + threadIdx.x] = 0.f;
    return;
  }
  __shared__ float s_bias[16];
  __shared__ float s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (w > 0) {
    // 2w+1 dot products of length kc: one wave per offset (strided)
    for (int r = wave; r < 2 * w + 1; r += 4) {
      float s = 0.f;
      const T* qp = q + (long long)i * ldq + z * kc;
      for (int c = lane; c < kc; c += 64) s += to_f(qp[c]) * rel_k[r * kc + c];
      s = wave_sum(s);
      if (lane == 0) s_bias[r] = s * qscale;
    }
    __syncthreads();
  }
  // the biased row is kept in LDS (<= 12288 keys) so the fp32 scores are read from HBM once, not three times
  extern __shared__ float s_row[];
  const bool cached = Tk <= 12288;
  float m = -INFINITY;
  for (int j = tid; j < Tk; j += 256) {
    float v = srow[j];
    if (w > 0) { int r = j - i + w; if (r >= 0 && r <= 2 * w) v += s_bias[r]; }
    if (j < klo || j >= khi) v = -INFINITY;
    if (cached) s_row[j] = v;
    m = fmaxf(m, v);
  }
  m = wave_max(m);
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  float sum = 0.f;
  for (int j = tid; j < Tk; j += 256) {
    float v;
    if (cached) v = s_row[j];
    else {
      v = srow[j];
      if (w > 0) { int r = j - i + w; if (r >= 0 && r <= 2 * w) v += s_bias[r]; }
      if (j < klo || j >= khi) v = -INFINITY;
    }
    const float e = expf(v - m);
    if (cached) s_row[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) s_red[4 + wave] = sum;
  __syncthreads();
  sum = s_red[4] + s_red[5] + s_red[6] + s_red[7];
  const float inv = 1.f / sum;
  for (int j = tid; j < ldp; j += 256) {
    float p = 0.f;
    if (j < Tk) {
      int r = j - i + w;
      const bool inband = w > 0 && r >= 0 && r <= 2 * w;
      if (cached) p = s_row[j] * inv;
      else {
        float v = srow[j];
        if (inband) v += s_bias[r];
        p = (j < klo || j >= khi) ? 0.f : expf(v - m) * inv;
      }
      if (inband) band[((long long)z * Tq + i) * (2 * w + 1) + r] = p;
    }
    prow[j] = (T)p;
  }
  if (w > 0 && tid < 2 * w + 1) {
    int j = i + tid - w;
    if (j < 0 || j >= Tk || j < klo || j >= khi) band[((long long)z * Tq + i) * (2 * w + 1) + tid] = 0.f;
  }
}

// out[i][z*kc + c] += sum_r band[z][i][r] * rel_v[r][c]
template <typename T>
__global__ void relv_add_kernel(const float* __restrict__ band, const float* __restrict__ rel_v, int Tq, int kc, int nz,
                                int w, T* __restrict__ out, int ldo) {
  const int i = blockIdx.x;
  for (int e = threadIdx.x; e < nz * kc; e += blockDim.x) {
    int z = e / kc, c = e - z * kc;
    const float* b = band + ((long long)z * Tq + i) * (2 * w + 1);
    float s = 0.f;
    for (int r = 0; r < 2 * w + 1; ++r) s += b[r] * rel_v[r * kc + c];
    T* o = out + (long long)i * ldo + e;
    *o = (T)(to_f(*o) + s);
  }
}

}  // namespace gsv

using namespace gsv;

namespace gsveng {

int require_device() {
  int n = 0;
  GSV_HIP(hipGetDeviceCount(&n));
  return GSV_OK;
}

int stage_tensor(Ctx* h, const char* name, const float* data, int64_t numel) {
  GSV_REQUIRE(h && name && data && numel > 0, "%s_load_tensor: bad argument", h ? h->who : "gsv");
  GSV_REQUIRE(!h->finalized, "%s_load_tensor: handle already finalized", h->who);
  h->staged[name].assign(data, data + numel);
  return GSV_OK;
}

int dalloc(Ctx* h, void** p, size_t bytes) {
  GSV_HIP(hipMalloc(p, bytes ? bytes : 16));
  h->allocs.push_back(*p);
  return GSV_OK;
}

int up_f32(Ctx* h, const float* v, size_t n, float** out) {
  GSV_RC(dalloc(h, (void**)out, n * 4));
  GSV_HIP(hipMemcpy(*out, v, n * 4, hipMemcpyHostToDevice));
  return GSV_OK;
}

int up_t(Ctx* h, const std::vector<float>& v, void** out) {
  if (h->dtype == GSV_F32) return up_f32(h, v.data(), v.size(), (float**)out);
  std::vector<_Float16> tmp(v.size());
  for (size_t i = 0; i < v.size(); ++i) tmp[i] = (_Float16)v[i];
  GSV_RC(dalloc(h, out, tmp.size() * 2));
  GSV_HIP(hipMemcpy(*out, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
  return GSV_OK;
}

// fetch a (possibly weight-normed) tensor as fp32 host vector
bool fetch(Ctx* h, const std::string& name, size_t n, int dim0, std::vector<float>& out) {
  auto it = h->staged.find(name);
  if (it != h->staged.end()) {
    if (it->second.size() != n) { set_error("%s: tensor '%s' has %zu elements, expected %zu", h->who, name.c_str(), it->second.size(), n); return false; }
    out = it->second;
    return true;
  }
  // weight norm: name ends with ".weight" -> weight_g / weight_v (torch.nn.utils.weight_norm, dim=0)
  if (name.size() > 7 && name.compare(name.size() - 7, 7, ".weight") == 0) {
    auto ig = h->staged.find(name + "_g"), iv = h->staged.find(name + "_v");
    if (ig != h->staged.end() && iv != h->staged.end()) {
      if (iv->second.size() != n || (int)ig->second.size() != dim0) { set_error("%s: bad weight-norm pair for '%s'", h->who, name.c_str()); return false; }
      out.resize(n);
      const size_t per = n / dim0;
      for (int r = 0; r < dim0; ++r) {
        double ss = 0.0;
        const float* v = iv->second.data() + (size_t)r * per;
        for (size_t i = 0; i < per; ++i) ss += (double)v[i] * v[i];
        const float sc = ig->second[r] / (float)sqrt(ss);
        for (size_t i = 0; i < per; ++i) out[(size_t)r * per + i] = v[i] * sc;
      }
      return true;
    }
  }
  set_error("%s: missing tensor '%s'", h->who, name.c_str());
  return false;
}

// torch Conv1d weight [cout][cin][k] (+bias) -> Conv, the input channels zero-padded to cin_pad (make_conv: cin_pad = cin)
int make_conv_padded(Ctx* h, const std::string& name, int cout, int cin, int cin_pad, int k, bool bias, Conv* c) {
  std::vector<float> w, b;
  if (!fetch(h, name + ".weight", (size_t)cout * cin * k, cout, w)) return GSV_ERR_ARG;
  std::vector<float> p((size_t)cout * k * cin_pad, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i)
      for (int j = 0; j < k; ++j) p[((size_t)o * k + j) * cin_pad + i] = w[((size_t)o * cin + i) * k + j];
  GSV_RC(up_t(h, p, &c->w));
  if (bias) {
    if (!fetch(h, name + ".bias", cout, cout, b)) return GSV_ERR_ARG;
    GSV_RC(up_f32(h, b.data(), b.size(), &c->b));
  }
  c->cin = cin_pad; c->cout = cout; c->taps = k;
  return GSV_OK;
}

// several 1x1 convs / Linears stacked along the output dim
int make_stacked(Ctx* h, const std::vector<std::string>& names, int cout_each, int cin, Conv* c) {
  std::vector<float> W, B;
  for (auto& n : names) {
    std::vector<float> w, b;
    if (!fetch(h, n + ".weight", (size_t)cout_each * cin, cout_each, w)) return GSV_ERR_ARG;
    if (!fetch(h, n + ".bias", cout_each, cout_each, b)) return GSV_ERR_ARG;
    W.insert(W.end(), w.begin(), w.end());
    B.insert(B.end(), b.begin(), b.end());
  }
  GSV_RC(up_t(h, W, &c->w));
  GSV_RC(up_f32(h, B.data(), B.size(), &c->b));
  c->cin = cin; c->cout = cout_each * (int)names.size(); c->taps = 1;
  return GSV_OK;
}

// ConvTranspose1d weight [cin][cout][k], stride u, padding (k-u)/2 -> polyphase conv with
// ceil(k/u) taps producing u*cout virtual channels (row p*cout+co), input x[s - q]
int make_ups(Ctx* h, const std::string& name, int cin, int cout, int k, int u, Conv* c) {
  std::vector<float> w, b;
  if (!fetch(h, name + ".weight", (size_t)cin * cout * k, cin, w)) return GSV_ERR_ARG;
  if (!fetch(h, name + ".bias", cout, cout, b)) return GSV_ERR_ARG;
  const int taps = (k + u - 1) / u;
  std::vector<float> p((size_t)u * cout * taps * cin, 0.f);
  for (int ph = 0; ph < u; ++ph)
    for (int q = 0; q < taps; ++q) {
      const int j = q * u + ph;
      if (j >= k) continue;
      for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
          p[(((size_t)ph * cout + co) * taps + q) * cin + ci] = w[((size_t)ci * cout + co) * k + j];
    }
  GSV_RC(up_t(h, p, &c->w));
  GSV_RC(up_f32(h, b.data(), b.size(), &c->b));
  c->cin = cin; c->cout = u * cout; c->taps = taps; c->ups_u = u; c->ups_pad = (k - u) / 2; c->ups_cout = cout;
  return GSV_OK;
}

int make_vec(Ctx* h, const std::string& name, size_t n, float** out) {
  std::vector<float> v;
  if (!fetch(h, name, n, (int)n, v)) return GSV_ERR_ARG;
  return up_f32(h, v.data(), n, out);
}

int make_mat(Ctx* h, const std::string& name, size_t n, void** out) {
  std::vector<float> v;
  if (!fetch(h, name, n, (int)n, v)) return GSV_ERR_ARG;
  return up_t(h, v, out);
}

int need(Ctx* h, const char* name, size_t bytes, void** out) {
  Buf& b = h->bufs[name];
  if (b.cap < bytes) {
    if (b.p) { GSV_HIP(hipDeviceSynchronize()); GSV_HIP(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t cap = bytes + bytes / 8 + 256;
    GSV_HIP(hipMalloc(&b.p, cap));
    b.cap = cap;
  }
  *out = b.p;
  return GSV_OK;
}

int conv(Ctx* h, hipStream_t s, const Conv& c, const void* x, int ldx, int T_in, void* y, int T_out, const ConvOpt& o) {
  ConvArgs a;
  a.x = x; a.y = y; a.res = o.res;
  const int cout = o.cout >= 0 ? o.cout : c.cout;
  a.w = (const char*)c.w + (size_t)o.w_row0 * c.taps * c.cin * esz(h);
  a.bias = o.no_bias ? nullptr : (o.bias_override ? o.bias_override : (c.b ? c.b + (c.ups_u ? 0 : o.w_row0) : nullptr));
  a.gate = o.gate; a.gate_rows = o.gate_rows; a.gate_ld = o.gate_ld;
  a.w_nt = o.w_nt;
  a.T_in = T_in; a.T_out = T_out; a.Cin = c.cin; a.Cout = cout; a.taps = c.taps;
  a.stride = o.stride; a.dil = o.dil;
  a.pad = o.pad >= 0 ? o.pad : (c.taps * o.dil - o.dil) / 2;
  a.ldx = ldx; a.ldw = c.taps * c.cin;
  a.pre_act = o.pre_act; a.pre_slope = o.pre_slope; a.post_act = o.post_act; a.scale = o.scale;
  a.accumulate = o.accumulate; a.out_f32 = o.out_f32; a.res_f32 = o.res_f32;
  if (c.ups_u > 0) {
    a.ups_u = c.ups_u; a.ups_pad = c.ups_pad; a.ups_cout = c.ups_cout;
    a.dil = -1; a.pad = 0; a.stride = 1;
    a.T_virt = T_in + c.taps - 1;
    a.ldy = o.ldy ? o.ldy : c.ups_cout;
  } else {
    a.T_virt = T_out;
    a.ldy = o.ldy ? o.ldy : cout;
  }
  a.ldr = o.ldr ? o.ldr : a.ldy;
  a.y_col0 = o.y_col0;
  a.row_seg = o.row_seg;
  return launch_conv_gemm(h->dtype, a, s);
}

// materialised multi-head attention: scores GEMM -> row softmax -> P V GEMM (-> relative-value term)
template <typename T>
static int attention_mat(Ctx* h, hipStream_t s, const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0,
                         int Tq, int Tk, int nh, int kc, float scale, const float* rel_k, const float* rel_v, void* out, int ldo,
                         const int* kr) {
  const size_t es = sizeof(T);
  const int G = es == 2 ? 8 : 4;
  const int ldp = (Tk + G - 1) / G * G;
  void *scores, *P, *Vt, *band;
  GSV_RC(need(h, "att_scores", (size_t)nh * Tq * Tk * 4, &scores));
  GSV_RC(need(h, "att_P", (size_t)nh * Tq * ldp * es, &P));
  GSV_RC(need(h, "att_Vt", (size_t)nh * kc * ldp * es, &Vt));
  GSV_RC(need(h, "att_band", (size_t)nh * Tq * 9 * 4 + 64, &band));
  set_attn_route(ATTN_MAT, 0);
  ConvArgs a;
  a.x = (const char*)q + (size_t)qcol0 * es; a.w = (const char*)kv + (size_t)kcol0 * es; a.y = scores;
  a.T_in = Tq; a.T_out = Tq; a.T_virt = Tq; a.Cin = kc; a.Cout = Tk; a.taps = 1;
  a.ldx = ldq; a.ldw = ldkv; a.ldy = Tk; a.out_f32 = 1; a.scale = scale;
  a.Z = nh; a.xz = kc; a.wz = kc; a.yz = (long long)Tq * Tk;
  GSV_RC(launch_conv_gemm(h->dtype, a, s));
  const int w = rel_k ? 4 : 0;
  GSV_LAUNCH(softmax_rows_kernel<T>, dim3(Tq, nh), dim3(256), Tk <= 12288 ? (size_t)Tk * 4 : 0, s, (const float*)scores, Tq, Tk, ldp, (T*)P,
             (const T*)q + qcol0, ldq, kc, rel_k, w, scale, (float*)band, kr);
  GSV_LAUNCH(transpose_v_kernel<T>, dim3(cdiv(ldp, 32), cdiv(kc, 32), nh), dim3(256), 0, s, (const T*)kv, ldkv, vcol0, kc, Tk, ldp, (T*)Vt);
  ConvArgs b;
  b.x = P; b.w = Vt; b.y = out;
  b.T_in = Tq; b.T_out = Tq; b.T_virt = Tq; b.Cin = ldp; b.Cout = kc; b.taps = 1;
  b.ldx = ldp; b.ldw = ldp; b.ldy = ldo;
  b.Z = nh; b.xz = (long long)Tq * ldp; b.wz = (long long)kc * ldp; b.yz = kc;
  GSV_RC(launch_conv_gemm(h->dtype, b, s));
  if (rel_v) GSV_LAUNCH(relv_add_kernel<T>, dim3(Tq), dim3(256), 0, s, (const float*)band, rel_v, Tq, kc, nh, 4, (T*)out, ldo);
  return GSV_OK;
}

// attention()'s choice: the fused fp16 kernel where it applies (the static switch is read once per process)
bool attention_is_fused(const Ctx* h, const void* q, int ldq, const void* kv, int ldkv, int Tq, int Tk, int kc, const float* rel_k,
                        const float* rel_v) {
  static const bool no_flash = getenv("GSV_MATERIALIZED_ENC_ATTN") != nullptr;    // A/B switch
  return !no_flash && h->dtype == GSV_F16 && kc == 96 && rel_k && rel_v && Tq == Tk && q == kv && ldq == ldkv;
}

// multi-head attention: q [Tq][ldq] cols qcol0.., k/v [Tk][ldkv] cols kcol0/vcol0.. -> out [Tq][ldo] (heads concatenated).
// rel_k/rel_v non-null: window-4 relative positions.  Called with the handle's runtime dtype (also from cfm.hip and bwe.hip):
// the fused fp16 kernel where it applies, else the materialised path in the handle's element type.
int attention(Ctx* h, hipStream_t s, const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0,
              int Tq, int Tk, int nh, int kc, float scale, const float* rel_k, const float* rel_v, void* out, int ldo, const int* kr) {
  return attention_routed(h, s, q, ldq, qcol0, kv, ldkv, kcol0, vcol0, Tq, Tk, nh, kc, scale, rel_k, rel_v, out, ldo, kr,
                          attention_is_fused(h, q, ldq, kv, ldkv, Tq, Tk, kc, rel_k, rel_v));
}

// the two routes of attention(): what the engines (through the wrapper above) and gsv_op_attention (the test hook) launch through
int attention_routed(Ctx* h, hipStream_t s, const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0,
                     int Tq, int Tk, int nh, int kc, float scale, const float* rel_k, const float* rel_v, void* out, int ldo, const int* kr,
                     bool fused) {
  if (fused) {
    void* vtb;
    GSV_RC(need(h, "att_vt96", (size_t)nh * 96 * ((Tk + 31) / 32 * 32) * 2, &vtb));
    return launch_flash_rel96_f16((const _Float16*)q + qcol0, ldq, (const _Float16*)kv + kcol0, ldkv, (const _Float16*)kv + vcol0, ldkv,
                                  vtb, Tq, nh, scale, rel_k, rel_v, out, ldo, s, kr);
  }
  return GSV_WITH_T(h, attention_mat<T>(h, s, q, ldq, qcol0, kv, ldkv, kcol0, vcol0, Tq, Tk, nh, kc, scale, rel_k, rel_v, out, ldo, kr));
}

template <typename T>
static int cf_to_cl_t(hipStream_t s, const float* src, int Tn, int C, void* dst, int ldd = 0) {
  GSV_LAUNCH(cf_to_cl_kernel<T>, dim3(cdiv(Tn, 32), cdiv(C, 32)), dim3(256), 0, s, src, Tn, C, (T*)dst, ldd);
  return GSV_OK;
}
int cf_to_cl(Ctx* h, hipStream_t s, const float* src, int Tn, int C, void* dst, int ldd) {
  return GSV_WITH_T(h, cf_to_cl_t<T>(s, src, Tn, C, dst, ldd));
}

int launch_expand_seg(hipStream_t s, const int* seg, int up, long long n, int* out) {
  GSV_LAUNCH(expand_seg_kernel, dim3(nblk(n)), dim3(256), 0, s, seg, up, n, out);
  return GSV_OK;
}
int launch_compact_wav(hipStream_t s, const float* src, const int* seg_f, int up, long long gap, long long n, float* wav) {
  GSV_LAUNCH(compact_wav_kernel, dim3(nblk(n)), dim3(256), 0, s, src, seg_f, up, gap, n, wav);
  return GSV_OK;
}

int seg_upload_begin(SegUpload* u) {
  if (!u->ev) GSV_HIP(hipEventCreateWithFlags(&u->ev, hipEventDisableTiming));
  GSV_HIP(hipEventSynchronize(u->ev));
  return GSV_OK;
}

// the library context of the current device (engine.h)
static int lib_ctx(LibCtx** out) {
  static std::mutex mu;
  static std::map<int, LibCtx*> ctxs;
  int dev = 0;
  GSV_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  LibCtx*& c = ctxs[dev];
  if (!c) {
    LibCtx* n = new LibCtx;
    n->image.resize((size_t)4 * kSegTableMax);
    for (SegSlot& sl : n->slot) {
      GSV_HIP(hipHostMalloc((void**)&sl.host, (size_t)16 * kSegTableMax, hipHostMallocDefault));
      GSV_HIP(hipMalloc((void**)&sl.dev, (size_t)16 * kSegTableMax));
      GSV_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    }
    c = n;
  }
  *out = c;
  return GSV_OK;
}

int seg_table_begin(SegTable* t) {
  GSV_RC(lib_ctx(&t->ctx));
  t->lock = std::unique_lock<std::mutex>(t->ctx->mu);
  t->image = t->ctx->image.data();
  return GSV_OK;
}

int seg_table_upload(SegTable* t, int n_seg, hipStream_t s) {
  LibCtx* c = t->ctx;
  const size_t bytes = (size_t)16 * n_seg;
  SegSlot* sl = &c->slot[c->cur];
  if (!(sl->n == n_seg && sl->stream == s && memcmp(sl->host, t->image, bytes) == 0)) {
    c->cur = (c->cur + 1) % kSegSlots;
    sl = &c->slot[c->cur];
    sl->n = 0;
    GSV_HIP(hipEventSynchronize(sl->ev));             // the launches that read this slot, kSegSlots tables ago
    memcpy(sl->host, t->image, bytes);
    GSV_HIP(hipMemcpyAsync(sl->dev, sl->host, bytes, hipMemcpyHostToDevice, s));
    sl->n = n_seg; sl->stream = s;
  }
  t->dev = sl->dev;
  return GSV_OK;
}

int seg_table_end(SegTable* t, hipStream_t s) {
  GSV_HIP(hipEventRecord(t->ctx->slot[t->ctx->cur].ev, s));
  return GSV_OK;
}

void free_ctx(Ctx* h) {
  for (void* p : h->allocs) (void)hipFree(p);
  for (auto& b : h->bufs) if (b.second.p) (void)hipFree(b.second.p);
  h->allocs.clear();
  h->bufs.clear();
}

}  // namespace gsveng
