// Stage arithmetic of the sampler's explicit Runge-Kutta methods (flowhigh_amd/ode.py): out = y + h * sum_j w_j k_j over up to
// four stage fields, for one or two weight rows in one pass (the next stage's input and the last stage's base read the same
// k's).  16-byte accesses: 4 elements per thread.  Nothing depends on rows or clips: the batched and the ragged layout are
// the same call.  fh_rk_combine_groups_f32 is the same element arithmetic (rk_element) with a step size per group of rows, for
// clips of different step counts in one sequence (row_groups.h): a row of group g has the bits of the one-time entry called
// with that group's h because both kernels run that one body.
#include "row_groups.h"

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

// One 16-byte element i of one or two weight rows.  No __restrict__: an output may be y or one of the k's.  Every load of an
// element comes before the stores of that element, and no thread touches another's.
template <bool TWO>
__device__ __forceinline__ void rk_element(const f32x4* y, const RkArgs& a, float h, f32x4* out_a, f32x4* out_b, size_t i) {
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

// one h: a thread per element, n4 is not tied to rows
template <bool TWO>
__global__ __launch_bounds__(256) void rk_combine_kernel(const f32x4* y, RkArgs a, float h, f32x4* out_a, f32x4* out_b,
                                                         long long n4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  rk_element<TWO>(y, a, h, out_a, out_b, (size_t)i);
}

// an h per group of rows: a wave per row
template <bool TWO>
__global__ __launch_bounds__(256) void rk_combine_groups_kernel(const f32x4* y, RkArgs a, GroupVals hs, f32x4* out_a, f32x4* out_b,
                                                                int rows, int dim4, fh_row_groups grp) {
  const int row = wave_row();
  if (row >= rows) return;
  const float h = pick(hs, group_of(grp, row));
  const size_t base = (size_t)row * dim4;
  for (int c = threadIdx.x & 63; c < dim4; c += 64) rk_element<TWO>(y, a, h, out_a, out_b, base + c);
}

// The checks both entries share and the argument block, in the order of the checks: `entry` is the caller's name in the
// messages, h_name is "h, " where h is a pointer that must be given, shape() holds the entry's own checks of n or rows / dim / groups.
template <class Shape>
int rk_args(const char* entry, const float* y, const float* const* ks, int n_k, bool given, const char* h_name, const float* wa,
            float* out_a, const float* wb, float* out_b, Shape shape, RkArgs& a) {
  FH_CHECK_ARG(n_k >= 1 && n_k <= RK_MAX_K, "%s: n_k %d (1..%d stage fields)", entry, n_k, RK_MAX_K);
  FH_CHECK_ARG(given, "%s: y, ks, %swa and out_a must be given", entry, h_name);
  FH_CHECK_ARG((wb != nullptr) == (out_b != nullptr), "%s: wb and out_b go together (both null, or both given)", entry);
  if (const int e = shape()) return e;
  FH_CHECK_ARG(((((size_t)y) | ((size_t)out_a) | ((size_t)out_b)) & 15) == 0, "%s: y, out_a and out_b must be 16-byte aligned", entry);
  FH_CHECK_ARG(out_a != out_b, "%s: out_a and out_b are the same buffer", entry);
  a.n = n_k;
  bool any_a = false, any_b = false;
  for (int j = 0; j < RK_MAX_K; ++j) {
    a.k[j] = (const f32x4*)(j < n_k ? ks[j] : ks[0]);
    a.wa[j] = j < n_k ? wa[j] : 0.0f;
    a.wb[j] = j < n_k && wb ? wb[j] : 0.0f;
    FH_CHECK_ARG(a.k[j] && (((size_t)a.k[j]) & 15) == 0, "%s: stage field %d is null or not 16-byte aligned", entry, j);
    any_a |= a.wa[j] != 0.0f;
    any_b |= a.wb[j] != 0.0f;
  }
  FH_CHECK_ARG(any_a && (any_b || !wb), "%s: a weight row is all zero (that output would be y: pass y instead)", entry);
  return FH_OK;
}

}  // namespace

extern "C" int fh_rk_combine_f32(const float* y, const float* const* ks, int n_k, float h, const float* wa, float* out_a,
                                 const float* wb, float* out_b, long long n, void* stream) {
  RkArgs a;
  const auto shape = [&]() -> int {
    FH_CHECK_ARG(n > 0 && n % 4 == 0, "fh_rk_combine_f32: n %lld must be a positive multiple of 4", n);
    return FH_OK;
  };
  if (const int e = rk_args("fh_rk_combine_f32", y, ks, n_k, y && ks && wa && out_a, "", wa, out_a, wb, out_b, shape, a)) return e;
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

extern "C" int fh_rk_combine_groups_f32(const float* y, const float* const* ks, int n_k, const float* h, const float* wa, float* out_a,
                                        const float* wb, float* out_b, int rows, int dim, const fh_row_groups* groups, void* stream) {
  RkArgs a;
  const auto shape = [&]() -> int {
    FH_CHECK_ARG(rows > 0 && dim > 0 && dim % 4 == 0, "fh_rk_combine_groups_f32: rows %d must be positive, dim %d a positive multiple of 4",
                 rows, dim);
    FH_CHECK_GROUPS("fh_rk_combine_groups_f32", groups, rows);
    return FH_OK;
  };
  if (const int e = rk_args("fh_rk_combine_groups_f32", y, ks, n_k, y && ks && h && wa && out_a, "h, ", wa, out_a, wb, out_b, shape, a))
    return e;
  const dim3 grid(fh_cdiv(rows, 4)), block(256);
  const GroupVals hs = vals_arg(h, groups->n);
  if (wb)
    hipLaunchKernelGGL(rk_combine_groups_kernel<true>, grid, block, 0, (hipStream_t)stream, (const f32x4*)y, a, hs, (f32x4*)out_a,
                       (f32x4*)out_b, rows, dim / 4, groups_arg(groups));
  else
    hipLaunchKernelGGL(rk_combine_groups_kernel<false>, grid, block, 0, (hipStream_t)stream, (const f32x4*)y, a, hs, (f32x4*)out_a,
                       (f32x4*)nullptr, rows, dim / 4, groups_arg(groups));
  FH_CHECK_LAUNCH("fh_rk_combine_groups_f32");
  return FH_OK;
}
