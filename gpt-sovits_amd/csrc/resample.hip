// gsv_op_resample_poly_seg: rational polyphase FIR resampling of many audios that lie back to back in one fp32 stream (the
// reference-audio front-end of TTS.make_voices(device_frontend=True)).  The arithmetic is
// scipy.signal.resample_poly(x, up, down, padtype="constant") with the filter handed in:
//   y_s[i] = sum_j h[i * down + half - j * up] * x_s[j],  j in [0, n_s) with the filter index in [0, L),  L = 2 * half + 1.
#include "common.h"
#include "engine.h"
#include "resample.h"

namespace gsv {

// the segment that owns workgroup `tile`: the last one whose first tile (tab[].w) is <= tile
__device__ __forceinline__ int rs_find(const int4* __restrict__ tab, int n_seg, int tile) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].w <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// tab: int4 per segment (first input sample, input samples, first output sample, first tile).  One thread owns one output: one
// fp32 accumulator over its taps in ascending input index, so an output's bits depend on its segment's samples alone, not on the
// tile it falls in or on where the segment lies.  HLDS: the filter is staged in LDS behind the window.
// LDS reads (ds_read_b32: 32 banks, conflicts inside a 32-lane half): lane i reads h[top_i - t * up] with top_i = L - 1 -
// ((half - i * down) mod up); up and down are coprime, so for up <= 32 the lanes' addresses are `up` distinct consecutive words
// (broadcast, no conflict) and for larger up they step by -down mod up, which spreads them over the banks (DESIGN.md 4m counts
// them); the window reads step by down / up words per lane.
template <bool HLDS>
__global__ __launch_bounds__(256) void resample_poly_seg_kernel(const float* __restrict__ x, const float* __restrict__ h, int L, int up,
                                                                int down, const int4* __restrict__ tab, int n_seg,
                                                                float* __restrict__ y, unsigned* __restrict__ peak, int win_cap) {
  extern __shared__ float rs_lds[];
  float* xs = rs_lds;
  const float* hs = HLDS ? rs_lds + win_cap : h;
  const int tid = threadIdx.x;
  const int s = rs_find(tab, n_seg, blockIdx.x);
  const int4 sg = tab[s];
  const int n = sg.y, half = L >> 1;
  const int m = (int)(((long long)n * up + down - 1) / down);
  const int o0 = ((int)blockIdx.x - sg.w) * kRsTile, o1 = min(m, o0 + kRsTile);
  if (o0 >= o1) return;                        // the host launches no such tile
  // the window [w0, w0 + wn) of the segment that outputs [o0, o1) read
  const long long a0 = (long long)o0 * down + half - (L - 1);
  const long long w0 = a0 <= 0 ? 0 : (a0 + up - 1) / up;
  const long long wl = min((long long)n - 1, ((long long)(o1 - 1) * down + half) / up);
  const int wn = (int)min((long long)win_cap, max(0LL, wl - w0 + 1));
  const float* xg = x + (long long)sg.x + w0;
  for (int i = tid; i < wn; i += 256) xs[i] = xg[i];
  if (HLDS) for (int i = tid; i < L; i += 256) rs_lds[win_cap + i] = h[i];
  __syncthreads();
  float pk = 0.f;
  for (int o = o0 + tid; o < o1; o += 256) {
    const long long c = (long long)o * down + half;
    const long long a = c - (L - 1);
    const long long ja = a <= 0 ? 0 : (a + up - 1) / up;
    const long long jb = min((long long)n - 1, c / up);
    int k = (int)(c - ja * up);                // filter index of the first tap, in [0, L)
    const int q0 = (int)(ja - w0), q1 = min((int)(jb - w0), wn - 1);
    float acc = 0.f;
    for (int q = q0; q <= q1; ++q, k -= up) acc = fmaf(hs[k], xs[q], acc);
    y[(long long)sg.z + o] = acc;
    pk = fmaxf(pk, fabsf(acc));
  }
  if (peak) {
    pk = wave_max(pk);
    // |y| >= 0: the bits of non-negative floats order as unsigned integers; the maximum does not depend on the order
    if ((tid & 63) == 0) atomicMax(peak + s, __float_as_uint(pk));
  }
}

}  // namespace gsv

extern "C" {

int gsv_op_resample_poly_seg(const float* x, int n_x, const float* h, int h_len, int up, int down, int n_seg, const int32_t* in_start,
                             const int32_t* in_len, const int32_t* out_start, float* y, int n_y, float* peak, gsv_stream_t stream) {
  GSV_REQUIRE(x && h && y && in_start && in_len && out_start && n_x > 0 && n_y > 0, "op_resample_poly_seg: bad argument");
  GSV_REQUIRE(up >= 1 && down >= 1, "op_resample_poly_seg: up = %d, down = %d (both >= 1)", up, down);
  GSV_REQUIRE(h_len >= 1 && (h_len & 1), "op_resample_poly_seg: h_len = %d must be odd (the filter is centred)", h_len);
  GSV_REQUIRE(h_len <= gsv::kRsMaxFilter, "op_resample_poly_seg: h_len = %d, the kernel takes filters up to %d taps", h_len, gsv::kRsMaxFilter);
  GSV_REQUIRE(n_seg >= 1 && n_seg <= gsveng::kSegTableMax, "op_resample_poly_seg: %d segments (1 .. %d)", n_seg, gsveng::kSegTableMax);
  const long long win = gsv::rs_window(gsv::kRsTile, up, down, h_len);
  GSV_REQUIRE(win <= gsv::kRsLdsFloats, "op_resample_poly_seg: %d -> %d with %d taps needs an input window of %lld samples per tile, "
              "the kernel holds %d", down, up, h_len, win, gsv::kRsLdsFloats);
  long long in_end = 0, out_end = 0, tiles = 0;
  for (int i = 0; i < n_seg; ++i) {
    GSV_REQUIRE(in_len[i] >= 1, "op_resample_poly_seg: segment %d has length %d", i, in_len[i]);
    GSV_REQUIRE(in_start[i] >= in_end, "op_resample_poly_seg: segment %d starts at input sample %d, before %lld where the one before it "
                "ends (ranges are disjoint and ascending)", i, in_start[i], in_end);
    in_end = (long long)in_start[i] + in_len[i];
    GSV_REQUIRE(in_end <= n_x, "op_resample_poly_seg: segment %d ends at input sample %lld of %d", i, in_end, n_x);
    const long long m = ((long long)in_len[i] * up + down - 1) / down;
    GSV_REQUIRE(out_start[i] >= out_end, "op_resample_poly_seg: segment %d starts at output sample %d, before %lld where the one before "
                "it ends (ranges are disjoint and ascending)", i, out_start[i], out_end);
    out_end = (long long)out_start[i] + m;
    GSV_REQUIRE(out_end <= n_y, "op_resample_poly_seg: segment %d ends at output sample %lld of %d", i, out_end, n_y);
    tiles += (m + gsv::kRsTile - 1) / gsv::kRsTile;
  }
  GSV_REQUIRE(tiles <= 0x7fffffffLL, "op_resample_poly_seg: %lld tiles are too many for one launch", tiles);
  gsveng::SegTable tb;                              // holds the library context until it goes out of scope
  GSV_RC(gsveng::seg_table_begin(&tb));
  int tile0 = 0;
  for (int i = 0; i < n_seg; ++i) {
    const long long m = ((long long)in_len[i] * up + down - 1) / down;
    tb.image[4 * i] = in_start[i]; tb.image[4 * i + 1] = in_len[i]; tb.image[4 * i + 2] = out_start[i]; tb.image[4 * i + 3] = tile0;
    tile0 += (int)((m + gsv::kRsTile - 1) / gsv::kRsTile);
  }
  hipStream_t s = (hipStream_t)stream;
  GSV_RC(gsveng::seg_table_upload(&tb, n_seg, s));
  if (peak) GSV_HIP(hipMemsetAsync(peak, 0, sizeof(float) * (size_t)n_seg, s));
  const int win_cap = (int)win;
  const bool hlds = win + h_len <= gsv::kRsLdsFloats;
  const size_t lds = sizeof(float) * (size_t)(win_cap + (hlds ? h_len : 0));
  if (hlds)
    GSV_LAUNCH(gsv::resample_poly_seg_kernel<true>, dim3((unsigned)tiles), dim3(256), lds, s, x, h, h_len, up, down, (const int4*)tb.dev, n_seg,
               y, (unsigned*)peak, win_cap);
  else
    GSV_LAUNCH(gsv::resample_poly_seg_kernel<false>, dim3((unsigned)tiles), dim3(256), lds, s, x, h, h_len, up, down, (const int4*)tb.dev, n_seg,
               y, (unsigned*)peak, win_cap);
  return gsveng::seg_table_end(&tb, s);
}

}
