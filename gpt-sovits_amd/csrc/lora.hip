// Per-row low-rank (LoRA) correction of the DiT's two adapted GEMM sites (cfm.hip), gfx950.
//
// A flow-matching pass holds DB rows of Tn frames back to back; row b may carry an adapter slot s = slot[b] (-1: the base
// model).  For the rows that do,
//     y[rows of b] += gate (.) ((x[rows of b] . A_s^T) . B_s^T)
// with A_s [n_proj * rp][K] (the n_proj lora_A matrices stacked) and B_s [N][rp] (the lora_B matrices stacked; output
// column c belongs to projection p = c / (N / n_proj) and contracts with columns [p * rp, (p + 1) * rp) of the intermediate,
// i.e. B is block-diagonal).  rp is the slot's own rank padded to a multiple of 16 with zero rows / columns, lora_alpha / r
// is folded into B_s when the adapter is stored.  A workgroup whose row has no slot returns at once: base rows cost
// nothing and are not touched.
//
// fp16: one workgroup = 64 frames of one row.  Phase 1 forms the 64 x (n_proj * rp) intermediate with
// mfma_f32_16x16x32_f16 (wave w owns frames 16w .. 16w + 15, fp32 accumulation) and parks it in LDS as fp16, at most
// 64 x (384 + 8) x 2 B = 49 KB.  Phase 2 walks the 16-column tiles of y, transposed (B_s as the MFMA's A operand) so that a
// lane ends up with 4 consecutive columns of one frame: one 8-byte read-modify-write.  Frames >= Tn of the last tile are
// masked on the load and on the store.
// fp32 (the parity dtype): plain FMA loops, 16 frames per workgroup, the intermediate stays fp32.
#include <algorithm>
#include <vector>

#include "common.h"

namespace gsv {

__device__ __forceinline__ f4 lora_mma16(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// The kernels' bodies are written once; the __global__ entries below differ in where row b finds its gate vector: the one
// vector of the launch, or (the *_rows entries of a flow-matching session, where every row has its own time) gate + b * gate_ld.
__device__ __forceinline__ void lora_delta_f16_body(const _Float16* __restrict__ x, _Float16* __restrict__ y, int Tn, int K, int N,
                                                    int n_proj, const int* __restrict__ slot, int slot_stride,
                                                    const LoraSlot* __restrict__ tab, long long coef_a, long long coef_b,
                                                    const float* __restrict__ gate) {
  extern __shared__ __attribute__((aligned(16))) _Float16 lora_u16[];   // [64][R + 8]
  const int b = blockIdx.y;
  const int sl = slot[(long long)b * slot_stride];
  if (sl < 0) return;
  const LoraSlot e = tab[sl];
  const int rp = e.rp, R = n_proj * rp, LDU = R + 8;
  const _Float16* A = (const _Float16*)e.base + coef_a * rp;
  const _Float16* Bm = (const _Float16*)e.base + coef_b * rp;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int t0 = blockIdx.x * 64;
  const long long row0 = (long long)b * Tn;
  const h8 zero = (h8){0, 0, 0, 0, 0, 0, 0, 0};
  {  // ---- phase 1: u[64][R] = x . A^T, 8 column tiles at a time
    const int t = t0 + 16 * w + r16;
    const bool ok = t < Tn;
    const _Float16* xr = x + (row0 + (ok ? t : 0)) * K + 8 * g;
    const int ntile = R >> 4;
    for (int j0 = 0; j0 < ntile; j0 += 8) {
      const int nj = min(8, ntile - j0);
      f4 acc[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) acc[jj] = (f4){0.f, 0.f, 0.f, 0.f};
      const _Float16* ar = A + (long long)(j0 * 16 + r16) * K + 8 * g;
      for (int k = 0; k < K; k += 32) {
        const h8 a = ok ? *(const h8*)(xr + k) : zero;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
          if (jj < nj) acc[jj] = lora_mma16(a, *(const h8*)(ar + (long long)jj * 16 * K + k), acc[jj]);
      }
#pragma unroll
      for (int jj = 0; jj < 8; ++jj)
        if (jj < nj) {
#pragma unroll
          for (int i = 0; i < 4; ++i) lora_u16[(16 * w + 4 * g + i) * LDU + (j0 + jj) * 16 + r16] = (_Float16)acc[jj][i];
        }
    }
  }
  __syncthreads();
  // ---- phase 2: y^T tile [16 columns][16 frames] = B_s[16 columns][rp] . u^T, k in steps of 32 (the upper half of an odd
  // last step is zero on both operands)
  const int npc = N / n_proj;
  const int ksteps = (rp + 31) >> 5;
  for (int ct = w; ct < (N >> 4); ct += 4) {
    const int c0 = ct << 4;
    const int ucol = (c0 / npc) * rp;
    h8 bw[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int q = kk * 32 + 8 * g;
      bw[kk] = (kk < ksteps && q < rp) ? *(const h8*)(Bm + (long long)(c0 + r16) * rp + q) : zero;
    }
    float gt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gt[i] = gate ? gate[c0 + 4 * g + i] : 1.f;
    for (int rt = 0; rt < 4; ++rt) {
      if (t0 + 16 * rt >= Tn) break;
      f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        if (kk < ksteps) {
          const int q = kk * 32 + 8 * g;
          const h8 uf = q < rp ? *(const h8*)(lora_u16 + (16 * rt + r16) * LDU + ucol + q) : zero;
          acc = lora_mma16(bw[kk], uf, acc);
        }
      const int t = t0 + 16 * rt + r16;
      if (t < Tn) {
        h4* yp = (h4*)(y + (row0 + t) * N + c0 + 4 * g);
        const h4 old = *yp;
        h4 nw;
#pragma unroll
        for (int i = 0; i < 4; ++i) nw[i] = (_Float16)((float)old[i] + gt[i] * acc[i]);
        *yp = nw;
      }
    }
  }
}

__global__ __launch_bounds__(256) void lora_delta_f16_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int Tn, int K, int N,
                                                             int n_proj, const int* __restrict__ slot, int slot_stride,
                                                             const LoraSlot* __restrict__ tab, long long coef_a, long long coef_b,
                                                             const float* __restrict__ gate) {
  lora_delta_f16_body(x, y, Tn, K, N, n_proj, slot, slot_stride, tab, coef_a, coef_b, gate);
}
__global__ __launch_bounds__(256) void lora_delta_f16_rows_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int Tn, int K, int N,
                                                                  int n_proj, const int* __restrict__ slot, int slot_stride,
                                                                  const LoraSlot* __restrict__ tab, long long coef_a, long long coef_b,
                                                                  const float* __restrict__ gate, int gate_ld) {
  lora_delta_f16_body(x, y, Tn, K, N, n_proj, slot, slot_stride, tab, coef_a, coef_b, gate + (long long)blockIdx.y * gate_ld);
}

__device__ __forceinline__ void lora_delta_f32_body(const float* __restrict__ x, float* __restrict__ y, int Tn, int K, int N,
                                                    int n_proj, const int* __restrict__ slot, int slot_stride,
                                                    const LoraSlot* __restrict__ tab, long long coef_a, long long coef_b,
                                                    const float* __restrict__ gate) {
  extern __shared__ __attribute__((aligned(16))) float lora_u32[];   // [16][R]
  const int b = blockIdx.y;
  const int sl = slot[(long long)b * slot_stride];
  if (sl < 0) return;
  const LoraSlot e = tab[sl];
  const int rp = e.rp, R = n_proj * rp;
  const float* A = (const float*)e.base + coef_a * rp;
  const float* Bm = (const float*)e.base + coef_b * rp;
  const int t0 = blockIdx.x * 16;
  const long long row0 = (long long)b * Tn;
  for (int i = threadIdx.x; i < 16 * R; i += 256) {
    const int r = i / R, j = i - r * R, t = t0 + r;
    float acc = 0.f;
    if (t < Tn) {
      const float* xr = x + (row0 + t) * K;
      const float* ar = A + (long long)j * K;
      for (int k = 0; k < K; ++k) acc = fmaf(xr[k], ar[k], acc);
    }
    lora_u32[i] = acc;
  }
  __syncthreads();
  const int npc = N / n_proj;
  for (int i = threadIdx.x; i < 16 * N; i += 256) {
    const int r = i / N, c = i - r * N, t = t0 + r;
    if (t >= Tn) continue;
    const float* ur = lora_u32 + r * R + (c / npc) * rp;
    const float* br = Bm + (long long)c * rp;
    float acc = 0.f;
    for (int q = 0; q < rp; ++q) acc = fmaf(ur[q], br[q], acc);
    y[(row0 + t) * N + c] += (gate ? gate[c] : 1.f) * acc;
  }
}

__global__ __launch_bounds__(256) void lora_delta_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int Tn, int K, int N,
                                                             int n_proj, const int* __restrict__ slot, int slot_stride,
                                                             const LoraSlot* __restrict__ tab, long long coef_a, long long coef_b,
                                                             const float* __restrict__ gate) {
  lora_delta_f32_body(x, y, Tn, K, N, n_proj, slot, slot_stride, tab, coef_a, coef_b, gate);
}
__global__ __launch_bounds__(256) void lora_delta_f32_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int Tn, int K, int N,
                                                                  int n_proj, const int* __restrict__ slot, int slot_stride,
                                                                  const LoraSlot* __restrict__ tab, long long coef_a, long long coef_b,
                                                                  const float* __restrict__ gate, int gate_ld) {
  lora_delta_f32_body(x, y, Tn, K, N, n_proj, slot, slot_stride, tab, coef_a, coef_b, gate + (long long)blockIdx.y * gate_ld);
}

int launch_lora_delta(int dtype, const void* x, void* y, int Tn, int DB, int K, int N, int n_proj, const int* slot, int slot_stride,
                      const LoraSlot* tab, int max_rp, long long coef_a, long long coef_b, const float* gate, hipStream_t s, int gate_ld) {
  GSV_REQUIRE(gate_ld == 0 || (gate && gate_ld >= N), "lora_delta: per-row gates need a gate table with gate_ld >= N");
  GSV_REQUIRE(x && y && slot && tab && Tn > 0 && DB > 0 && DB <= 65535, "lora_delta: bad argument");
  GSV_REQUIRE(n_proj >= 1 && n_proj <= 3 && N > 0 && N % (16 * n_proj) == 0, "lora_delta: N=%d must be a multiple of 16 per projection (%d)", N,
              n_proj);
  GSV_REQUIRE(K > 0 && K % 32 == 0, "lora_delta: K=%d must be a multiple of 32", K);
  GSV_REQUIRE(max_rp >= 16 && max_rp <= GSV_LORA_MAX_RANK && max_rp % 16 == 0, "lora_delta: padded rank %d is not a multiple of 16 in [16, %d]",
              max_rp, GSV_LORA_MAX_RANK);
  const int R = n_proj * max_rp;
  if (gate_ld) {   // per-row gates: the same bodies, the same geometry
    if (dtype == GSV_F16)
      GSV_LAUNCH(lora_delta_f16_rows_kernel, dim3(cdiv(Tn, 64), DB), dim3(256), (size_t)64 * (R + 8) * 2, s, (const _Float16*)x, (_Float16*)y, Tn, K,
                 N, n_proj, slot, slot_stride, tab, coef_a, coef_b, gate, gate_ld);
    else
      GSV_LAUNCH(lora_delta_f32_rows_kernel, dim3(cdiv(Tn, 16), DB), dim3(256), (size_t)16 * R * 4, s, (const float*)x, (float*)y, Tn, K, N, n_proj,
                 slot, slot_stride, tab, coef_a, coef_b, gate, gate_ld);
    return GSV_OK;
  }
  if (dtype == GSV_F16) {
    GSV_LAUNCH(lora_delta_f16_kernel, dim3(cdiv(Tn, 64), DB), dim3(256), (size_t)64 * (R + 8) * 2, s, (const _Float16*)x, (_Float16*)y, Tn, K, N,
               n_proj, slot, slot_stride, tab, coef_a, coef_b, gate);
  } else {
    GSV_LAUNCH(lora_delta_f32_kernel, dim3(cdiv(Tn, 16), DB), dim3(256), (size_t)16 * R * 4, s, (const float*)x, (float*)y, Tn, K, N, n_proj,
               slot, slot_stride, tab, coef_a, coef_b, gate);
  }
  return GSV_OK;
}

}  // namespace gsv

extern "C" int gsv_op_lora_delta(const void* x, void* y, int Tn, int DB, int K, int N, int n_proj, const int* slots, int n_slots,
                                 const void* const* blocks, const int* rp, const float* gate, int dtype, gsv_stream_t stream) {
  using namespace gsv;
  GSV_REQUIRE(x && y && slots && blocks && rp && n_slots > 0 && n_slots <= GSV_CFM_MAX_ADAPTERS && DB > 0, "op_lora_delta: bad argument");
  GSV_REQUIRE(dtype == GSV_F16 || dtype == GSV_F32, "op_lora_delta: bad dtype");
  std::vector<LoraSlot> tab(n_slots);
  int max_rp = 0;
  for (int i = 0; i < n_slots; ++i) {
    GSV_REQUIRE(blocks[i] && rp[i] >= 16 && rp[i] <= GSV_LORA_MAX_RANK && rp[i] % 16 == 0, "op_lora_delta: slot %d: bad block or padded rank %d", i,
                rp[i]);
    tab[i] = LoraSlot{blocks[i], rp[i], 0};
    max_rp = std::max(max_rp, rp[i]);
  }
  for (int b = 0; b < DB; ++b) GSV_REQUIRE(slots[b] >= -1 && slots[b] < n_slots, "op_lora_delta: row %d: slot %d out of range", b, slots[b]);
  hipStream_t s = (hipStream_t)stream;
  LoraSlot* dtab = nullptr;
  int* dslot = nullptr;
  GSV_HIP(hipMalloc((void**)&dtab, tab.size() * sizeof(LoraSlot)));
  hipError_t e = hipMalloc((void**)&dslot, (size_t)DB * sizeof(int));
  int rc = GSV_OK;
  if (e != hipSuccess) { set_error("op_lora_delta: hipMalloc -> %s", hipGetErrorString(e)); rc = GSV_ERR_HIP; }
  if (!rc && (hipMemcpy(dtab, tab.data(), tab.size() * sizeof(LoraSlot), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(dslot, slots, (size_t)DB * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)) {
    set_error("op_lora_delta: upload of the tables failed");
    rc = GSV_ERR_HIP;
  }
  // the block of slot i is A [n_proj * rp][K] followed by B [N][rp]: offsets 0 and n_proj * K, in units of rp elements
  if (!rc) rc = launch_lora_delta(dtype, x, y, Tn, DB, K, N, n_proj, dslot, 1, dtab, max_rp, 0, (long long)n_proj * K, gate, s);
  if (!rc && hipStreamSynchronize(s) != hipSuccess) { set_error("op_lora_delta: the kernel failed"); rc = GSV_ERR_HIP; }
  (void)hipFree(dtab);
  (void)hipFree(dslot);
  return rc;
}
