// The banded forms of fh_attention_bf16x6_f32 / fh_attention_bf16x6_seg_f32 (attn_window=): query i of a clip reads the keys j of that clip with
// |i - j| <= radius.  The kernel is attention_bf.hip's (attention_bf_kernel.h) with BAND on, the launch rule is the same, the two online-softmax streams
// are the same: a radius that spans the clip gives the full entry's bits, and a clip gives the same bits alone, in a batch on either
// side of the SPLIT threshold, and in the segment form (attention_softmax.h: AttnBand).
#include "attention_bf_kernel.h"

extern "C" int fh_attention_bf16x6_band_f32(const float* qkv, float* out, int batch, int n, int heads, int radius, float scale,
                                            void* stream) {
  FH_CHECK_ARG(qkv && out && batch > 0 && n > 0 && heads > 0, "fh_attention_bf16x6_band_f32: bad args");
  FH_CHECK_ARG(radius >= 0, "fh_attention_bf16x6_band_f32: radius must be >= 0");
  FH_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "fh_attention_bf16x6_band_f32: qkv / out must be 16-byte aligned");
  launch_attention(attention_bf_kernel<4, 1, true, int>, attention_bf_kernel<4, 2, true, int>, qkv, out, nullptr, batch, n, heads, scale, stream,
                   attn_clamp_radius(radius, n));
  FH_CHECK_LAUNCH("fh_attention_bf16x6_band_f32");
  return FH_OK;
}

extern "C" int fh_attention_bf16x6_band_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads,
                                                int radius, float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && seg && n_seg > 0 && max_n > 0 && heads > 0, "fh_attention_bf16x6_band_seg_f32: bad args");
  FH_CHECK_ARG(radius >= 0, "fh_attention_bf16x6_band_seg_f32: radius must be >= 0");
  FH_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "fh_attention_bf16x6_band_seg_f32: qkv / out must be 16-byte aligned");
  launch_attention(attention_bf_kernel<4, 1, true, int>, attention_bf_kernel<4, 2, true, int>, qkv, out, seg, n_seg, max_n, heads, scale, stream,
                   attn_clamp_radius(radius, max_n));
  FH_CHECK_LAUNCH("fh_attention_bf16x6_band_seg_f32");
  return FH_OK;
}
