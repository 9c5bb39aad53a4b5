// Streaming-softmax attention with both products in the bf16 x 6 form (dim_head = 64): attn_form = 'bf16x6'.
//
// Replaces the same call site as attention.hip: Attend.forward of the reference, models/attend.py:102-139
//   sim = einsum(q, k) * scale ; attn = softmax(sim) ; out = einsum(attn, v)
// fp32 in / out / accumulate; S^T = K Q^T and O^T = V^T P^T are six v_mfma_f32_32x32x16_bf16 per k-step over exact three-piece
// splits (bf16x6.h), pair order kBf16x6SmallFirst with the pair read as (K piece, Q piece) and (V piece, P piece).
//
// Everything beside the two products is the frame attention.hip has too, attention_softmax.h: block placement, 32-key tiles, two
// interleaved online-softmax streams per query row and their merge, base-2 exponent, the masking of the last tile, the output,
// the SPLIT = 1 / 2 kernel shapes and the rule that picks one.  Where both products are exact in both forms the two kernels give
// the same bits.
//
// Every operand is split once:
//   K   by the block that stages the tile, on the way into LDS: 16-byte units of 8 consecutive d, [piece][tile][d-octet][key];
//       A operand of S^T (row = key, k = d), read with ds_read_b128 (gemm_bf.hip's layout).
//   V   likewise, and transposed while staged: a staging item is 4 consecutive keys of one d, so a split yields the two packed
//       words of half a fragment; units [piece][tile][k-step s][lane half h][d], element j = key 16 s + 8 (j >> 2) + 4 h + (j & 3)
//       of the tile, which is the k order of the S^T accumulator.  A operand of O^T (row = d, k = key), ds_read_b128.
//   Q   once per wave into 48 registers: B operand of S^T for the whole kernel.
//   P   in the S^T accumulator the lane's query is the column, so registers 8 s .. 8 s + 7 are the B fragment of k-step s of
//       O^T with no lane movement: split in registers, the only split arithmetic inside the loop.
// LDS: K 3 x 2 x 8 x 34 + V 3 x 2 x 4 x 64 units = 50 688 bytes per block.
#include "attention_bf_kernel.h"

extern "C" int fh_attention_bf16x6_f32(const float* qkv, float* out, int batch, int n, int heads, float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && batch > 0 && n > 0 && heads > 0, "fh_attention_bf16x6_f32: bad args");
  FH_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "fh_attention_bf16x6_f32: qkv / out must be 16-byte aligned");
  launch_attention(attention_bf_kernel<4, 1>, attention_bf_kernel<4, 2>, qkv, out, nullptr, batch, n, heads, scale, stream);
  FH_CHECK_LAUNCH("fh_attention_bf16x6_f32");
  return FH_OK;
}

extern "C" int fh_attention_bf16x6_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads,
                                           float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && seg && n_seg > 0 && max_n > 0 && heads > 0, "fh_attention_bf16x6_seg_f32: bad args");
  FH_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "fh_attention_bf16x6_seg_f32: qkv / out must be 16-byte aligned");
  launch_attention(attention_bf_kernel<4, 1>, attention_bf_kernel<4, 2>, qkv, out, seg, n_seg, max_n, heads, scale, stream);
  FH_CHECK_LAUNCH("fh_attention_bf16x6_seg_f32");
  return FH_OK;
}
