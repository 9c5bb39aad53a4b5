// The sampler's small kernels that take one scalar, or a scalar per group of rows: the time embedding, the GEMV behind it and the
// grouped field update.  A time and a step size per clip (flowhigh_amd/ode.py: mixed_schedule) make the clips of one step count
// a group of rows (row_groups.h).  The one-time entry and the grouped entry of an operator launch ONE kernel body, the one-time
// one as the case of a single group or a single vector, so a row of group g has the bits of the one-time entry called with that
// group's scalar by construction: here fh_time_fourier(_groups)_f32 and fh_gemv(_rows)_f32, in flow_ops.hip the two RMS norm
// entries, in ode.hip the two RK combine entries.  fh_axpy_groups_f32 restates the linear GEMM epilogue's alpha / R update
// (gemm_common.h); tests/test_hip_mixed_steps.py holds it to that.
#include "row_groups.h"

namespace {

// ---- time embedding, a time per group; grid.y = group (fh_time_fourier_f32: one group) -------------------------------------------
__global__ __launch_bounds__(256) void time_fourier_groups_kernel(const float* __restrict__ w, GroupVals ts, float* __restrict__ out,
                                                                  int half) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= half) return;
  const float t = pick(ts, (int)blockIdx.y);
  float* o = out + (size_t)blockIdx.y * 2 * half;
  // pos_emb.py:24: freqs = x * weights * 2 * math.pi, evaluated left to right in fp32
  float f = t * w[i];
  f = f * 2.0f;
  f = f * 3.14159265358979323846f;
  o[i] = sinf(f);
  o[half + i] = cosf(f);
}

// ---- Y[j] = act(W X[j] + b) for T vectors, one wave per row of W, the row read once (fh_gemv_f32: T = 1) ---------------------------
template <int T>
__global__ __launch_bounds__(256) void gemv_rows_kernel(const float* __restrict__ W, const float* __restrict__ X, int ldx,
                                                        const float* __restrict__ bias, float* __restrict__ Y, int ldy, int N,
                                                        int K, int act) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* w = W + (size_t)row * K;
  float s[T];
#pragma unroll
  for (int j = 0; j < T; ++j) s[j] = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(X + (size_t)j * ldx + k);
      s[j] = fmaf(wv[0], xv[0], s[j]);
      s[j] = fmaf(wv[1], xv[1], s[j]);
      s[j] = fmaf(wv[2], xv[2], s[j]);
      s[j] = fmaf(wv[3], xv[3], s[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < T; ++j) s[j] = wave_sum(s[j]);
  if (lane == 0) {
    const float b = bias ? bias[row] : 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      float r = s[j];
      r += b;
      if (act == 1) r = r / (1.f + expf(-r));
      Y[(size_t)j * ldy + row] = r;
    }
  }
}

// ---- out = alpha_g v + res: the linear GEMM epilogue's update.  There `v *= alpha` and `v += R[..]` sit on two sides of the
// `if (R)` branch and compile to v_mul_f32 and v_add_f32, never to one FMA: the same two roundings here, spelled so that no
// contraction can join them.  No __restrict__: out may be v or res (an element depends on its own index alone).
template <bool RES>
__global__ __launch_bounds__(256) void axpy_groups_kernel(const f32x4* v, GroupVals alpha, const f32x4* res, f32x4* out, int rows,
                                                          int dim4, fh_row_groups grp) {
#pragma clang fp contract(off)          // (the product is rounded before the add: __fmul_rn / __fadd_rn are still contracted)
  const int row = wave_row();
  if (row >= rows) return;
  const float a = pick(alpha, group_of(grp, row));
  const size_t base = (size_t)row * dim4;
  for (int c = threadIdx.x & 63; c < dim4; c += 64) {
    f32x4 o = v[base + c] * a;
    if (RES) o = o + res[base + c];
    out[base + c] = o;
  }
}

}  // namespace

extern "C" int fh_sizeof_row_groups(void) { return (int)sizeof(fh_row_groups); }

extern "C" int fh_time_fourier_f32(const float* w, float t, float* out, int half_dim, void* stream) {
  FH_CHECK_ARG(w && out && half_dim > 0, "fh_time_fourier_f32: bad args");
  hipLaunchKernelGGL(time_fourier_groups_kernel, dim3(fh_cdiv(half_dim, 256), 1), dim3(256), 0, (hipStream_t)stream, w, vals_arg(&t, 1),
                     out, half_dim);
  FH_CHECK_LAUNCH("fh_time_fourier_f32");
  return FH_OK;
}

extern "C" int fh_time_fourier_groups_f32(const float* w, const float* t, float* out, int half_dim, int n_groups, void* stream) {
  FH_CHECK_ARG(n_groups >= 1 && n_groups <= FH_MAX_GROUPS, "fh_time_fourier_groups_f32: %d groups (1..%d)", n_groups, FH_MAX_GROUPS);
  FH_CHECK_ARG(w && t && out && half_dim > 0, "fh_time_fourier_groups_f32: bad args");
  hipLaunchKernelGGL(time_fourier_groups_kernel, dim3(fh_cdiv(half_dim, 256), n_groups), dim3(256), 0, (hipStream_t)stream, w,
                     vals_arg(t, n_groups), out, half_dim);
  FH_CHECK_LAUNCH("fh_time_fourier_groups_f32");
  return FH_OK;
}

extern "C" int fh_gemv_f32(const float* W, const float* x, const float* bias, float* y, int N, int K, int act, void* stream) {
  FH_CHECK_ARG(W && x && y && N > 0 && K > 0 && K % 4 == 0, "fh_gemv_f32: bad args");
  hipLaunchKernelGGL(gemv_rows_kernel<1>, dim3(fh_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, W, x, K, bias, y, N, N, K, act);
  FH_CHECK_LAUNCH("fh_gemv_f32");
  return FH_OK;
}

extern "C" int fh_gemv_rows_f32(const float* W, const float* X, int ldx, const float* bias, float* Y, int ldy, int N, int K, int T,
                                int act, void* stream) {
  FH_CHECK_ARG(T >= 1 && T <= FH_MAX_GROUPS, "fh_gemv_rows_f32: %d vectors (1..%d)", T, FH_MAX_GROUPS);
  FH_CHECK_ARG(W && X && Y && N > 0 && K > 0 && K % 4 == 0, "fh_gemv_rows_f32: bad args");
  FH_CHECK_ARG(ldx >= K && ldx % 4 == 0 && ldy >= N, "fh_gemv_rows_f32: ldx %d (>= K = %d, a multiple of 4) / ldy %d (>= N = %d)", ldx,
               K, ldy, N);
  FH_CHECK_ARG(((((size_t)W) | ((size_t)X)) & 15) == 0, "fh_gemv_rows_f32: W and X must be 16-byte aligned");
  FH_CHECK_ARG(act == 0 || act == 1, "fh_gemv_rows_f32: act %d (0 none, 1 SiLU)", act);
  const dim3 grid(fh_cdiv(N, 4)), block(256);
#define FH_GEMV_ROWS(T_)                                                                                                      \
  case T_:                                                                                                                    \
    hipLaunchKernelGGL(gemv_rows_kernel<T_>, grid, block, 0, (hipStream_t)stream, W, X, ldx, bias, Y, ldy, N, K, act);        \
    break;
  switch (T) {
    FH_GEMV_ROWS(1) FH_GEMV_ROWS(2) FH_GEMV_ROWS(3) FH_GEMV_ROWS(4) FH_GEMV_ROWS(5) FH_GEMV_ROWS(6) FH_GEMV_ROWS(7) FH_GEMV_ROWS(8)
  }
#undef FH_GEMV_ROWS
  FH_CHECK_LAUNCH("fh_gemv_rows_f32");
  return FH_OK;
}

extern "C" int fh_axpy_groups_f32(const float* v, const float* alpha, const float* res, float* out, int rows, int dim,
                                  const fh_row_groups* groups, void* stream) {
  FH_CHECK_ARG(v && alpha && out && rows > 0, "fh_axpy_groups_f32: v, alpha and out must be given, rows positive");
  FH_CHECK_ARG(dim > 0 && dim % 4 == 0, "fh_axpy_groups_f32: dim %d must be a positive multiple of 4", dim);
  FH_CHECK_GROUPS("fh_axpy_groups_f32", groups, rows);
  FH_CHECK_ARG(((((size_t)v) | ((size_t)res) | ((size_t)out)) & 15) == 0, "fh_axpy_groups_f32: v, res and out must be 16-byte aligned");
  const dim3 grid(fh_cdiv(rows, 4)), block(256);
  const GroupVals a = vals_arg(alpha, groups->n);
  if (res)
    hipLaunchKernelGGL(axpy_groups_kernel<true>, grid, block, 0, (hipStream_t)stream, (const f32x4*)v, a, (const f32x4*)res,
                       (f32x4*)out, rows, dim / 4, groups_arg(groups));
  else
    hipLaunchKernelGGL(axpy_groups_kernel<false>, grid, block, 0, (hipStream_t)stream, (const f32x4*)v, a, (const f32x4*)nullptr,
                       (f32x4*)out, rows, dim / 4, groups_arg(groups));
  FH_CHECK_LAUNCH("fh_axpy_groups_f32");
  return FH_OK;
}
