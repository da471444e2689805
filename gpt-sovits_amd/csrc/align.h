// Monotonic alignment launches (align.hip), as the SoVITS engine calls them after the MRTE attention.
#pragma once
#include "common.h"

namespace gsv {

enum { ALIGN_MAX_PHONES = 1024,    // phonemes of a span the search takes (16 per lane); more take the proportional fallback
       ALIGN_MAX_HEADS = 8, ALIGN_MAX_SPANS = 4096,
       ALIGN_LP_BLOCKS = 8,        // workgroups per span of the log-probability launch: 32 sentences fill the 256 CUs in one round
       ALIGN_LDS_WORDS = 8192 };   // decision bits up to 32 KB stay in the LDS of the span's wave

// 4-byte words of workspace span (nf, nl) takes: 0 where the search is not run
long long align_span_words(int nf, int nl);
int launch_align_logp(int dtype, const void* q, int ldq, const void* k, int ldk, int heads, int head_dim, float scale,
                      const gsv_align_span_t* tab, int n, void* ws, long long ws_bytes, hipStream_t s);
int launch_align_path(const gsv_align_span_t* tab, int n, void* ws, long long ws_bytes, int32_t* ends, float* score, hipStream_t s);

}  // namespace gsv
