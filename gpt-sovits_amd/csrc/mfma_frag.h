// MFMA operand fragments of the LDS-staged kernels (conv_lds.hip, gemm_lds.hip, conv_narrow.hip): one 16-byte chunk per lane,
// 8 halfs or 4 floats, the 32 x 32 MFMA of each and the activations applied to a chunk while it is staged.
#pragma once
#include "common.h"

namespace gsv {

template <typename T> struct FragL;
template <> struct FragL<_Float16> { typedef h8 type; };
template <> struct FragL<float> { typedef f4 type; };

__device__ __forceinline__ void mma32l(f16v& acc, const h8& a, const h8& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma32l(f16v& acc, const f4& a, const f4& b) {
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
}

template <typename F> __device__ __forceinline__ F zfrag() {
  F z;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(F) / sizeof(z[0])); ++i) z[i] = 0;
  return z;
}
__device__ __forceinline__ h8 lrelu_l(h8 v, float s) { h8 t = v * (_Float16)s; return __builtin_elementwise_max(v, t); }
__device__ __forceinline__ f4 lrelu_l(f4 v, float s) { f4 t = v * s; return __builtin_elementwise_max(v, t); }
__device__ __forceinline__ h8 relu_l(h8 v) { return __builtin_elementwise_max(v, zfrag<h8>()); }
__device__ __forceinline__ f4 relu_l(f4 v) { return __builtin_elementwise_max(v, zfrag<f4>()); }

}  // namespace gsv
