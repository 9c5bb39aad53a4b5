// Streaming sessions (FlowHighSR.stream / stream_push; flowhigh_amd/stream.py is the definition): the seam between two
// consecutive windows of a stream.
//   fh_xfade_seg_f32   head[u] = fmaf(w_in[u], head[u], fl(w_out[u] * tail[u])) over the o48 samples two windows share, in place in
//                      the newer window, for every seam of every session of a push in one launch
// A term whose weight is exactly 0 is skipped, not multiplied (as fh_rk_combine_f32 skips a zero weight): where a ramp's guard
// gives one window the weight 0, the result is the other window's bits and nothing of the first (a NaN either) gets through.
// Jobs do not depend on each other: 2 * overlap <= window keeps a window's head (written) and tail (read) apart, so job k may read
// the tail of the row whose head job k - 1 writes.  No LDS, no atomics, nothing syncs.
#include "fh_common.h"

namespace {

constexpr uint32_t ABS_MASK = 0x7fffffffu;

// (the zero tests are on the bits of the table's value, whatever the denormal mode of a compare)
__device__ __forceinline__ bool is_zero(float w) { return (__float_as_uint(w) & ABS_MASK) == 0; }

__device__ __forceinline__ float xfade_one(float wi, float wo, float cur, float prev) {
  if (is_zero(wo)) return is_zero(wi) ? 0.0f : __fmul_rn(wi, cur);
  const float s = __fmul_rn(wo, prev);
  return is_zero(wi) ? s : fmaf(wi, cur, s);
}

// four floats from any 4-byte aligned address: one 16-byte load where the address allows it
__device__ __forceinline__ f32x4 load4(const float* p) {
  if ((((size_t)p) & 15) == 0) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

// grid (slots of o48 samples at any alignment, n_jobs).  Slot s is the 16-byte word s of the head's memory counted from the aligned
// address at or below `head` (level.hip: row_gain_body): a slot wholly inside the overlap is one 16-byte load and store of the
// head, the (at most two) slots that overlap an end go element by element.  The tail and the tables have alignments of their own.
__global__ __launch_bounds__(256) void xfade_seg_kernel(const fh_xfade_job* __restrict__ jobs, const float* __restrict__ w_in,
                                                        const float* __restrict__ w_out, int o48) {
  const fh_xfade_job J = jobs[blockIdx.y];
  float* head = J.head;
  const float* tail = J.tail;
  const int lead = (int)(((size_t)head >> 2) & 3);                   // elements between the aligned address and the head
  const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 - lead;      // the slot's first element in the overlap
  if (first >= o48) return;
  if (first >= 0 && first + 4 <= o48) {
    f32x4* p = reinterpret_cast<f32x4*>(head + first);
    const f32x4 cur = *p, prev = load4(tail + first), wi = load4(w_in + first), wo = load4(w_out + first);
    *p = f32x4{xfade_one(wi.x, wo.x, cur.x, prev.x), xfade_one(wi.y, wo.y, cur.y, prev.y), xfade_one(wi.z, wo.z, cur.z, prev.z),
               xfade_one(wi.w, wo.w, cur.w, prev.w)};
    return;
  }
  for (int k = 0; k < 4; ++k) {
    const long long u = first + k;
    if (u >= 0 && u < o48) head[u] = xfade_one(w_in[u], w_out[u], head[u], tail[u]);
  }
}

}  // namespace

extern "C" int fh_sizeof_xfade_job(void) { return (int)sizeof(fh_xfade_job); }

extern "C" int fh_xfade_seg_f32(const fh_xfade_job* jobs, int n_jobs, const float* w_in, const float* w_out, int o48, void* stream) {
  FH_CHECK_ARG(jobs && w_in && w_out, "fh_xfade_seg_f32: null pointer (jobs %p, w_in %p, w_out %p)", (const void*)jobs, (const void*)w_in,
               (const void*)w_out);
  FH_CHECK_ARG(n_jobs > 0 && n_jobs < 65536, "fh_xfade_seg_f32: %d jobs (1 .. 65535)", n_jobs);
  FH_CHECK_ARG(o48 > 0, "fh_xfade_seg_f32: o48 %d must be positive", o48);
  FH_CHECK_ARG(((((size_t)w_in) | ((size_t)w_out)) & 3) == 0, "fh_xfade_seg_f32: w_in and w_out must be 4-byte aligned");
  hipLaunchKernelGGL(xfade_seg_kernel, dim3(fh_cdiv(((long long)o48 + 3) / 4 + 1, 256), n_jobs), dim3(256), 0, (hipStream_t)stream, jobs,
                     w_in, w_out, o48);
  FH_CHECK_LAUNCH("fh_xfade_seg_f32");
  return FH_OK;
}
