// The sampler's prior eps ~ N(0, 1) drawn on the device (cfm_superresolution.py:219-236: `torch.randn_like(cond)`).
//   fh_prior_normal_f32    : counter-based Philox4x32-10 + Box-Muller, one thread per quad of four consecutive elements.
//   fh_prior_normal_at_f32 : the same draw with clip b's rows counted from first_frames[b] instead of 0 (streaming sessions: a
//                            window that starts at absolute frame f0 gets rows f0 .. f0 + n of its session's stream)
// The stream is this project's own (flowhigh_amd/prior.py restates it in numpy): element e = f * d + m of a clip is lane e & 3 of the
// Philox block with counter (e >> 2, stream) under the key `seed`, so a value depends on (seed, stream, row within its clip, column, d)
// only -- not on the batch, the launch or the clip's length.  No state, no atomics, no LDS; keys are read from device memory, so a
// captured launch draws whatever keys are there when it is replayed.
#include "fh_common.h"
#include "philox.h"

namespace {

// (ra, rb) -> two normals: u1 = ((ra >> 8) + 1) 2^-24 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1), both exact in fp32;
// sqrt(-2 ln u1) (cos, sin)(2 pi u2).  The angle goes to sincospi as 2 u2 (exact), so no 2 pi is rounded and no argument is reduced.
__device__ __forceinline__ void box_muller(unsigned ra, unsigned rb, float& z0, float& z1) {
  const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f;
  const float rad = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif((float)(rb >> 8) * 0x1p-23f, &s, &c);
  z0 = rad * c;
  z1 = rad * s;
}

// grid (ceil(n d / 4 / 256), n_seg): thread = quad q of clip blockIdx.y
__global__ __launch_bounds__(256) void prior_normal_kernel(float* __restrict__ out, const unsigned long long* __restrict__ keys,
                                                           const long long* __restrict__ first_frames,
                                                           const int* __restrict__ seg, int n, int d) {
  const int b = blockIdx.y;
  size_t row0 = (size_t)b * n;
  int rows = n;
  if (seg) {             // ragged batch: clip b = rows [seg[2b], + seg[2b+1])
    row0 = (size_t)seg[2 * b];
    rows = seg[2 * b + 1];
  }
  const unsigned long long q = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (q * 4 >= (unsigned long long)rows * d) return;
  const unsigned long long seed = keys[2 * b], strm = keys[2 * b + 1];
  // the clip's first row is row first_frames[b] of its stream: d % 4 == 0, so that row starts at quad first_frames[b] * (d / 4)
  const unsigned long long c = q + (first_frames ? (unsigned long long)first_frames[b] * (unsigned)(d / 4) : 0ull);
  const u32x4 ctr = {(unsigned)c, (unsigned)(c >> 32), (unsigned)strm, (unsigned)(strm >> 32)};
  const u32x4 r = philox4x32_10(ctr, (unsigned)seed, (unsigned)(seed >> 32));
  f32x4 z;
  float a0, a1;
  box_muller(r[0], r[1], a0, a1);
  z[0] = a0;
  z[1] = a1;
  box_muller(r[2], r[3], a0, a1);
  z[2] = a0;
  z[3] = a1;
  *reinterpret_cast<f32x4*>(out + row0 * d + 4 * q) = z;
}

}  // namespace

namespace {

// both entries: the argument checks under the entry's own name, then the one kernel (first_frames NULL: every clip counts from 0)
int prior_normal_launch(const char* name, float* out, const uint64_t* keys, const int64_t* first_frames, const int32_t* seg, int n_seg,
                        int n, int d, void* stream) {
  FH_CHECK_ARG(out && keys, "%s: null pointer (out %p, keys %p)", name, (void*)out, (const void*)keys);
  FH_CHECK_ARG(n_seg > 0 && n_seg <= 65535 && n > 0 && d > 0, "%s: n_seg %d (1 .. 65535) / n %d / d %d unsupported", name, n_seg, n, d);
  FH_CHECK_ARG(d % 4 == 0, "%s: d %d is not a multiple of 4", name, d);
  FH_CHECK_ARG(((uintptr_t)out & 15) == 0, "%s: out is not 16-byte aligned", name);
  const long long quads = (long long)n * d / 4;
  FH_CHECK_ARG(quads < (1ll << 31), "%s: %lld quads per clip (n %d x d %d) do not fit one grid", name, quads, n, d);
  hipLaunchKernelGGL(prior_normal_kernel, dim3(fh_cdiv(quads, 256), n_seg), dim3(256), 0, (hipStream_t)stream, out,
                     (const unsigned long long*)keys, (const long long*)first_frames, (const int*)seg, n, d);
  FH_CHECK_LAUNCH(name);
  return FH_OK;
}

}  // namespace

extern "C" int fh_prior_normal_f32(float* out, const uint64_t* keys, const int32_t* seg, int n_seg, int n, int d, void* stream) {
  return prior_normal_launch("fh_prior_normal_f32", out, keys, nullptr, seg, n_seg, n, d, stream);
}

extern "C" int fh_prior_normal_at_f32(float* out, const uint64_t* keys, const int64_t* first_frames, const int32_t* seg, int n_seg, int n,
                                      int d, void* stream) {
  FH_CHECK_ARG(first_frames, "fh_prior_normal_at_f32: null pointer (first_frames)");
  return prior_normal_launch("fh_prior_normal_at_f32", out, keys, first_frames, seg, n_seg, n, d, stream);
}
