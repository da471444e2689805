// The tile geometry that the polyphase resampling kernels share: gsv_op_resample_poly_seg (resample.hip) and
// gsv_postprocess_groups_rate (sola.hip).
#pragma once

namespace gsv {

constexpr int kRsTile = 1024;                // consecutive outputs of one segment per workgroup (256 threads, 4 outputs each)
constexpr int kRsLdsFloats = 16384;          // 64 KiB of LDS per workgroup: the input window, and the filter where it still fits
constexpr int kRsMaxFilter = 65535;          // the largest h_len (a filter that does not fit in LDS is read through L2)

// the input window of `tile` consecutive outputs is at most this many samples
static inline long long rs_window(int tile, int up, int down, int L) {
  return ((long long)(tile - 1) * down + (L - 1)) / up + 2;
}

}  // namespace gsv
