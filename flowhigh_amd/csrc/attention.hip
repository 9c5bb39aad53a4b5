// Streaming-softmax attention in fp32 on the gfx950 matrix cores (dim_head = 64).
//
// Replaces Attend.forward, /root/reference/src/flowhigh/models/attend.py:102-139
//   sim = einsum(q, k) * scale ; attn = softmax(sim) ; out = einsum(attn, v)
// which materialises [B, 16, n, n] three times (64 MB per clip at n = 1000); here the scores
// live only in MFMA accumulators.
//
// Per wave: 32 queries; per block (4 waves): 128 queries of one (batch, head); key/value tiles of
// 32 keys are staged in LDS and shared by the 4 waves.
//   S^T = K Q^T  (M = key, N = query, K = d):  A = K tile from LDS (ds_read_b128, 4 k-steps each),
//                 B = Q fragments held in 32 VGPRs for the whole kernel.
//   The accumulator then holds, for the lane's query (col = lane & 31), 16 keys per lane half:
//   the row softmax is 16 in-register ops + one exchange with lane ^ 32, and the probabilities are
//   already the B operand of the next product (no LDS round trip, no conversion):
//   O^T = V^T P^T (M = d, N = query, K = key): k-step r pairs keys (r&3)+8(r>>2) and that + 4,
//                 A = V^T read from the LDS V tile with the same key order.
// The frame around the products -- block placement, the two online-softmax streams per query row, their merge, the output and the
// launch rule -- is attention_softmax.h's, shared with attention_bf.hip.
#include "attention_kernel.h"

extern "C" int fh_attention_f32(const float* qkv, float* out, int batch, int n, int heads,
                                float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && batch > 0 && n > 0 && heads > 0, "fh_attention_f32: bad args");
  launch_attention(attention_kernel<4, 1>, attention_kernel<4, 2>, qkv, out, nullptr, batch, n, heads, scale, stream);
  FH_CHECK_LAUNCH("fh_attention_f32");
  return FH_OK;
}

extern "C" int fh_attention_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads,
                                    float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && seg && n_seg > 0 && max_n > 0 && heads > 0, "fh_attention_seg_f32: bad args");
  launch_attention(attention_kernel<4, 1>, attention_kernel<4, 2>, qkv, out, seg, n_seg, max_n, heads, scale, stream);
  FH_CHECK_LAUNCH("fh_attention_seg_f32");
  return FH_OK;
}
