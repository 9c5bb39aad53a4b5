// The two-stream online softmax state of the attention kernels and its merge, shared by attention.hip (fp32 MFMA products)
// and attention_bf.hip (bf16 x 6 products): both reduce a query row the same way, so both have the same batch / ragged /
// kernel-shape invariances and agree bit for bit wherever their products are exact.
#pragma once
#include "fh_common.h"

// Every query row is reduced as TWO interleaved online-softmax streams -- stream 0 takes the even 32-key tiles,
// stream 1 the odd ones -- merged once at the end by merge_streams().  The two kernel shapes differ only in who
// runs the streams, never in the arithmetic, so a clip gives the same bits whatever else is in the batch:
//   SPLIT = 2 (small grids): 64 queries per block, the two waves of a 32-query tile take one stream each -- twice
//                            the waves and half the dependent MFMA chain per wave when there are fewer query tiles
//                            than SIMDs (B = 1, n = 1000: 512 tiles, 1024 SIMDs);
//   SPLIT = 1 (large grids): 128 queries per block, every wave runs both streams of its tile one after the other
//                            (half the K / V staging traffic per query).
struct Stream {
  f32x16 o0, o1;
  float m, l;
};

__device__ __forceinline__ void merge_streams(Stream& a, const float (&b0)[16], const float (&b1)[16], float mb, float lb) {
  const float m = fmaxf(a.m, mb);                          // (maxima are in the base-2 domain of the tile loop)
  const float c0 = __builtin_amdgcn_exp2f(a.m - m), c1 = __builtin_amdgcn_exp2f(mb - m);      // exp2(-inf) = 0: a stream that saw no key contributes nothing
  a.l = __fmaf_rn(lb, c1, __fmul_rn(a.l, c0));
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    a.o0[r] = __fmaf_rn(b0[r], c1, __fmul_rn(a.o0[r], c0));
    a.o1[r] = __fmaf_rn(b1[r], c1, __fmul_rn(a.o1[r], c0));
  }
}
