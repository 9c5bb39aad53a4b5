// Element-wise sums of fp32 tensors in a fixed order of addition: the mean over the AMP blocks of a vocoder stage, the merge of
// split-K partial outputs, and a batch of such sums in one launch.  16-byte accesses: 4 elements per thread.
#include "fh_common.h"

namespace {

// out = ((a + b) + c) * scale, 4 elements per thread (the reference's xs += ...; xs / n order)
__global__ __launch_bounds__(256) void mean_kernel(const f32x4* __restrict__ a, const f32x4* __restrict__ b,
                                                   const f32x4* __restrict__ c, f32x4* __restrict__ out,
                                                   long long n4, float scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = a[i] + b[i];
  if (c) v += c[i];
  out[i] = v * scale;
}

}  // namespace

extern "C" int fh_mean_f32(const float* a, const float* b, const float* c, float* out, long long n, float scale,
                           void* stream) {
  FH_CHECK_ARG(a && b && out && n > 0 && n % 4 == 0, "fh_mean_f32: bad args (n must be a multiple of 4)");
  FH_CHECK_ARG(((((size_t)a) | ((size_t)b) | ((size_t)c) | ((size_t)out)) & 15) == 0, "fh_mean_f32: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(mean_kernel, dim3(fh_cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const f32x4*)a, (const f32x4*)b, (const f32x4*)c, (f32x4*)out, n / 4, scale);
  FH_CHECK_LAUNCH("fh_mean_f32");
  return FH_OK;
}

// out = (((p0 + p1) + p2) + ...) * scale over up to 12 tensors (split-K partial outputs: fixed order of addition)
namespace {
struct SumArgs {
  const f32x4* p[12];
  int n;
};
__global__ __launch_bounds__(256) void sum_kernel(SumArgs a, f32x4* __restrict__ out, long long n4, float scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = a.p[0][i];
#pragma unroll
  for (int k = 1; k < 12; ++k)
    if (k < a.n) v += a.p[k][i];
  out[i] = v * scale;
}
}  // namespace

extern "C" int fh_sum_f32(const float* const* srcs, int n_srcs, float* out, long long n, float scale, void* stream) {
  FH_CHECK_ARG(srcs && n_srcs >= 1 && n_srcs <= 12 && out && n > 0 && n % 4 == 0,
               "fh_sum_f32: bad args (1..12 sources, n a multiple of 4)");
  SumArgs a;
  a.n = n_srcs;
  for (int k = 0; k < 12; ++k) {
    a.p[k] = (const f32x4*)(k < n_srcs ? srcs[k] : srcs[0]);
    FH_CHECK_ARG(a.p[k] && (((size_t)a.p[k]) & 15) == 0, "fh_sum_f32: source %d is null or not 16-byte aligned", k);
  }
  FH_CHECK_ARG((((size_t)out) & 15) == 0, "fh_sum_f32: out must be 16-byte aligned");
  hipLaunchKernelGGL(sum_kernel, dim3(fh_cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, a, (f32x4*)out, n / 4,
                     scale);
  FH_CHECK_LAUNCH("fh_sum_f32");
  return FH_OK;
}

namespace {
__global__ __launch_bounds__(256) void sum_multi_kernel(const fh_sum_job* __restrict__ jobs) {
  const fh_sum_job& J = jobs[blockIdx.y];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= J.n / 4) return;
  f32x4 v = reinterpret_cast<const f32x4*>(J.src[0])[i];
  for (int k = 1; k < J.n_src; ++k) v += reinterpret_cast<const f32x4*>(J.src[k])[i];
  reinterpret_cast<f32x4*>(J.out)[i] = v * J.scale;
}
}  // namespace

extern "C" int fh_sizeof_sum_job(void) { return (int)sizeof(fh_sum_job); }

extern "C" int fh_sum_multi_f32(const fh_sum_job* jobs, int n_jobs, long long max_n, void* stream) {
  FH_CHECK_ARG(jobs && n_jobs > 0 && n_jobs < 65536 && max_n > 0 && max_n % 4 == 0, "fh_sum_multi_f32: bad args");
  hipLaunchKernelGGL(sum_multi_kernel, dim3(fh_cdiv(max_n / 4, 256), n_jobs), dim3(256), 0, (hipStream_t)stream, jobs);
  FH_CHECK_LAUNCH("fh_sum_multi_f32");
  return FH_OK;
}
