// Stage arithmetic of the sampler's explicit Runge-Kutta methods (flowhigh_amd/ode.py): out = y + h * sum_j w_j k_j over up to
// four stage fields, for one or two weight rows in one pass (the next stage's input and the last stage's base read the same
// k's).  16-byte accesses: 4 elements per thread.  Nothing depends on rows or clips: the batched and the ragged layout are
// the same call.
#include "fh_common.h"

namespace {

constexpr int RK_MAX_K = 4;

struct RkArgs {
  const f32x4* k[RK_MAX_K];
  float wa[RK_MAX_K];
  float wb[RK_MAX_K];
  int n;
};

__device__ __forceinline__ f32x4 fma4(float w, f32x4 k, f32x4 s) {
  return f32x4{fmaf(w, k.x, s.x), fmaf(w, k.y, s.y), fmaf(w, k.z, s.z), fmaf(w, k.w, s.w)};
}

// one weight row: s = w_j0 k_j0 for the first non-zero weight, then s = fma(w_j, k_j, s) in rising j; a zero weight is skipped,
// not multiplied (an infinite k of weight 0 does not reach s).  The weights are kernel arguments: every branch is uniform.
__device__ __forceinline__ void rk_term(float w, const f32x4& kv, f32x4& s, bool& started) {
  if (w == 0.0f) return;
  s = started ? fma4(w, kv, s) : kv * w;
  started = true;
}

// No __restrict__: an output may be y or one of the k's.  Every load of an element comes before the stores of that element, and
// no thread touches another's.
template <bool TWO>
__global__ __launch_bounds__(256) void rk_combine_kernel(const f32x4* y, RkArgs a, float h, f32x4* out_a, f32x4* out_b,
                                                         long long n4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4 yv = y[i];
  f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
  bool has_a = false, has_b = false;
#pragma unroll
  for (int j = 0; j < RK_MAX_K; ++j) {
    if (j >= a.n || (a.wa[j] == 0.0f && (!TWO || a.wb[j] == 0.0f))) continue;
    const f32x4 kv = a.k[j][i];          // read once for both rows
    rk_term(a.wa[j], kv, sa, has_a);
    if (TWO) rk_term(a.wb[j], kv, sb, has_b);
  }
  const f32x4 ra = fma4(h, sa, yv);
  if (TWO) {
    const f32x4 rb = fma4(h, sb, yv);
    out_b[i] = rb;
  }
  out_a[i] = ra;
}

}  // namespace

extern "C" int fh_rk_combine_f32(const float* y, const float* const* ks, int n_k, float h, const float* wa, float* out_a,
                                 const float* wb, float* out_b, long long n, void* stream) {
  FH_CHECK_ARG(n_k >= 1 && n_k <= RK_MAX_K, "fh_rk_combine_f32: n_k %d (1..%d stage fields)", n_k, RK_MAX_K);
  FH_CHECK_ARG(y && ks && wa && out_a, "fh_rk_combine_f32: y, ks, wa and out_a must be given");
  FH_CHECK_ARG((wb != nullptr) == (out_b != nullptr), "fh_rk_combine_f32: wb and out_b go together (both null, or both given)");
  FH_CHECK_ARG(n > 0 && n % 4 == 0, "fh_rk_combine_f32: n %lld must be a positive multiple of 4", n);
  FH_CHECK_ARG(((((size_t)y) | ((size_t)out_a) | ((size_t)out_b)) & 15) == 0,
               "fh_rk_combine_f32: y, out_a and out_b must be 16-byte aligned");
  FH_CHECK_ARG(out_a != out_b, "fh_rk_combine_f32: out_a and out_b are the same buffer");
  RkArgs a;
  a.n = n_k;
  bool any_a = false, any_b = false;
  for (int j = 0; j < RK_MAX_K; ++j) {
    a.k[j] = (const f32x4*)(j < n_k ? ks[j] : ks[0]);
    a.wa[j] = j < n_k ? wa[j] : 0.0f;
    a.wb[j] = j < n_k && wb ? wb[j] : 0.0f;
    FH_CHECK_ARG(a.k[j] && (((size_t)a.k[j]) & 15) == 0, "fh_rk_combine_f32: stage field %d is null or not 16-byte aligned", j);
    any_a |= a.wa[j] != 0.0f;
    any_b |= a.wb[j] != 0.0f;
  }
  FH_CHECK_ARG(any_a && (any_b || !wb), "fh_rk_combine_f32: a weight row is all zero (that output would be y: pass y instead)");
  const dim3 grid(fh_cdiv(n / 4, 256)), block(256);
  if (wb)
    hipLaunchKernelGGL(rk_combine_kernel<true>, grid, block, 0, (hipStream_t)stream, (const f32x4*)y, a, h, (f32x4*)out_a,
                       (f32x4*)out_b, n / 4);
  else
    hipLaunchKernelGGL(rk_combine_kernel<false>, grid, block, 0, (hipStream_t)stream, (const f32x4*)y, a, h, (f32x4*)out_a,
                       (f32x4*)nullptr, n / 4);
  FH_CHECK_LAUNCH("fh_rk_combine_f32");
  return FH_OK;
}
