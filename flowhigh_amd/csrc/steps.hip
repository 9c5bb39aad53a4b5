// A time and a step size per clip: the grouped twins of the sampler's small kernels (flowhigh_amd/ode.py: mixed_schedule).
// The clips of a ragged sequence are sorted by step count, so the clips of one count are one contiguous range of rows, a group
// (fh_row_groups).  The groups and every per-group scalar travel BY VALUE as kernel arguments: no device table, no upload, no
// sync, and a captured graph holds them.  A wave works on one row: it finds the row's group by scalar compares against the
// row ends and selects its scalar by scalar selects (no dynamic index into the argument block, which would go through scratch).
//
// Every kernel restates the arithmetic of its one-time twin term by term (gemm_mfma.hip: gemv_kernel, time_fourier_kernel;
// flow_ops.hip: rmsnorm_kernel; ode.hip: rk_combine_kernel; gemm_common.h: the linear epilogue's alpha / R update), so a row of
// group g has the bits of the twin called with that group's scalar.  tests/test_hip_mixed_steps.py holds them to that.
#include "fh_common.h"

namespace {

struct GroupVals {
  float v[FH_MAX_GROUPS];
};

// group of a wave-uniform row: the number of row ends at or below it (the last end is the row count: not compared)
__device__ __forceinline__ int group_of(const fh_row_groups& g, int row) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < FH_MAX_GROUPS - 1; ++i) k += (i < g.n - 1 && row >= g.row_end[i]) ? 1 : 0;
  return k;
}

__device__ __forceinline__ float pick(const GroupVals& s, int k) {
  float r = s.v[0];
#pragma unroll
  for (int i = 1; i < FH_MAX_GROUPS; ++i) r = k == i ? s.v[i] : r;
  return r;
}

// the row of this wave, in an SGPR (threadIdx.x >> 6 is uniform in a wave, which the compiler cannot see)
__device__ __forceinline__ int wave_row() { return uni((int)(blockIdx.x * 4 + (threadIdx.x >> 6))); }

// ---- time embedding: time_fourier_kernel per group; grid.y = group ------------------------------------------------------------
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

// ---- Y[j] = act(W X[j] + b) for T vectors, one wave per row of W, the row read once ------------------------------------------------
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

// ---- rmsnorm_kernel with the row's group choosing gamma / beta; one wave per row ---------------------------------------------------
__global__ __launch_bounds__(256) void rmsnorm_groups_kernel(const float* __restrict__ x, const float* __restrict__ gamma0,
                                                             const float* __restrict__ beta0, long long g_stride,
                                                             float* __restrict__ y, int rows, int dim, float scale,
                                                             fh_row_groups grp) {
  const int row = wave_row();
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int gi = group_of(grp, row);
  const float* gamma = gamma0 + (size_t)gi * g_stride;
  const float* beta = beta0 ? beta0 + (size_t)gi * g_stride : nullptr;
  const float* xr = x + (size_t)row * dim;
  float* yr = y + (size_t)row * dim;
  f32x4 v[16];
  const int nv = dim >> 8;   // float4 per lane
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < nv) {
      v[i] = *reinterpret_cast<const f32x4*>(xr + (i * 64 + lane) * 4);
      ss += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
  }
  ss = wave_sum(ss);
  const float inv = scale / fmaxf(sqrtf(ss), 1e-12f);     // F.normalize eps
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < nv) {
      const int c = (i * 64 + lane) * 4;
      f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
      f32x4 o;
      if (beta) {
        f32x4 bt = *reinterpret_cast<const f32x4*>(beta + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[i][e] * inv * g[e] + bt[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[i][e] * inv * g[e];
      }
      *reinterpret_cast<f32x4*>(yr + c) = o;
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

// ---- rk_combine_kernel (ode.hip) with the row's group choosing h ----------------------------------------------------------------
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

__device__ __forceinline__ void rk_term(float w, const f32x4& kv, f32x4& s, bool& started) {
  if (w == 0.0f) return;
  s = started ? fma4(w, kv, s) : kv * w;
  started = true;
}

// No __restrict__: an output may be y or one of the k's.  Every load of an element comes before the stores of that element.
template <bool TWO>
__global__ __launch_bounds__(256) void rk_combine_groups_kernel(const f32x4* y, RkArgs a, GroupVals hs, f32x4* out_a, f32x4* out_b,
                                                                int rows, int dim4, fh_row_groups grp) {
  const int row = wave_row();
  if (row >= rows) return;
  const float h = pick(hs, group_of(grp, row));
  const size_t base = (size_t)row * dim4;
  for (int c = threadIdx.x & 63; c < dim4; c += 64) {
    const size_t i = base + c;
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
}

bool groups_ok(const fh_row_groups* g) {
  if (!g || g->n < 1 || g->n > FH_MAX_GROUPS) return false;
  int prev = 0;
  for (int i = 0; i < g->n; ++i) {
    if (g->row_end[i] <= prev) return false;
    prev = g->row_end[i];
  }
  return true;
}

// the groups as a kernel argument: the entries behind n filled with the last end (never compared)
fh_row_groups groups_arg(const fh_row_groups* g) {
  fh_row_groups a;
  a.n = g->n;
  for (int i = 0; i < FH_MAX_GROUPS; ++i) a.row_end[i] = g->row_end[i < g->n ? i : g->n - 1];
  return a;
}

GroupVals vals_arg(const float* v, int n) {
  GroupVals a;
  for (int i = 0; i < FH_MAX_GROUPS; ++i) a.v[i] = v[i < n ? i : n - 1];
  return a;
}

}  // namespace

#define FH_CHECK_GROUPS(entry, g, rows)                                                                                    \
  do {                                                                                                                     \
    FH_CHECK_ARG((g) != nullptr, entry ": the groups must be given");                                                      \
    FH_CHECK_ARG((g)->n >= 1 && (g)->n <= FH_MAX_GROUPS, entry ": %d groups (1..%d)", (g)->n, FH_MAX_GROUPS);              \
    FH_CHECK_ARG(groups_ok(g), entry ": the groups' row ends must be positive and strictly increasing");                   \
    FH_CHECK_ARG((g)->row_end[(g)->n - 1] == (rows), entry ": the last group ends at row %d, the call has %d rows",       \
                 (g)->row_end[(g)->n - 1], (rows));                                                                        \
  } while (0)

extern "C" int fh_sizeof_row_groups(void) { return (int)sizeof(fh_row_groups); }

extern "C" int fh_time_fourier_groups_f32(const float* w, const float* t, float* out, int half_dim, int n_groups, void* stream) {
  FH_CHECK_ARG(n_groups >= 1 && n_groups <= FH_MAX_GROUPS, "fh_time_fourier_groups_f32: %d groups (1..%d)", n_groups, FH_MAX_GROUPS);
  FH_CHECK_ARG(w && t && out && half_dim > 0, "fh_time_fourier_groups_f32: bad args");
  hipLaunchKernelGGL(time_fourier_groups_kernel, dim3(fh_cdiv(half_dim, 256), n_groups), dim3(256), 0, (hipStream_t)stream, w,
                     vals_arg(t, n_groups), out, half_dim);
  FH_CHECK_LAUNCH("fh_time_fourier_groups_f32");
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

extern "C" int fh_rmsnorm_groups_f32(const float* x, const float* gamma, const float* beta, long long g_stride, float* y, int rows,
                                     int dim, const fh_row_groups* groups, void* stream) {
  FH_CHECK_ARG(x && gamma && y && rows > 0, "fh_rmsnorm_groups_f32: bad args");
  FH_CHECK_ARG(dim % 256 == 0 && dim > 0 && dim <= 4096, "fh_rmsnorm_groups_f32: dim %d unsupported", dim);
  FH_CHECK_GROUPS("fh_rmsnorm_groups_f32", groups, rows);
  FH_CHECK_ARG(g_stride >= 0 && g_stride % 4 == 0, "fh_rmsnorm_groups_f32: g_stride %lld must be a non-negative multiple of 4", g_stride);
  FH_CHECK_ARG(((((size_t)x) | ((size_t)gamma) | ((size_t)beta) | ((size_t)y)) & 15) == 0,
               "fh_rmsnorm_groups_f32: x, gamma, beta and y must be 16-byte aligned");
  hipLaunchKernelGGL(rmsnorm_groups_kernel, dim3(fh_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, g_stride, y,
                     rows, dim, sqrtf((float)dim), groups_arg(groups));
  FH_CHECK_LAUNCH("fh_rmsnorm_groups_f32");
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

extern "C" int fh_rk_combine_groups_f32(const float* y, const float* const* ks, int n_k, const float* h, const float* wa, float* out_a,
                                        const float* wb, float* out_b, int rows, int dim, const fh_row_groups* groups, void* stream) {
  FH_CHECK_ARG(n_k >= 1 && n_k <= RK_MAX_K, "fh_rk_combine_groups_f32: n_k %d (1..%d stage fields)", n_k, RK_MAX_K);
  FH_CHECK_ARG(y && ks && h && wa && out_a, "fh_rk_combine_groups_f32: y, ks, h, wa and out_a must be given");
  FH_CHECK_ARG((wb != nullptr) == (out_b != nullptr), "fh_rk_combine_groups_f32: wb and out_b go together (both null, or both given)");
  FH_CHECK_ARG(rows > 0 && dim > 0 && dim % 4 == 0, "fh_rk_combine_groups_f32: rows %d must be positive, dim %d a positive multiple of 4",
               rows, dim);
  FH_CHECK_GROUPS("fh_rk_combine_groups_f32", groups, rows);
  FH_CHECK_ARG(((((size_t)y) | ((size_t)out_a) | ((size_t)out_b)) & 15) == 0,
               "fh_rk_combine_groups_f32: y, out_a and out_b must be 16-byte aligned");
  FH_CHECK_ARG(out_a != out_b, "fh_rk_combine_groups_f32: out_a and out_b are the same buffer");
  RkArgs a;
  a.n = n_k;
  bool any_a = false, any_b = false;
  for (int j = 0; j < RK_MAX_K; ++j) {
    a.k[j] = (const f32x4*)(j < n_k ? ks[j] : ks[0]);
    a.wa[j] = j < n_k ? wa[j] : 0.0f;
    a.wb[j] = j < n_k && wb ? wb[j] : 0.0f;
    FH_CHECK_ARG(a.k[j] && (((size_t)a.k[j]) & 15) == 0, "fh_rk_combine_groups_f32: stage field %d is null or not 16-byte aligned", j);
    any_a |= a.wa[j] != 0.0f;
    any_b |= a.wb[j] != 0.0f;
  }
  FH_CHECK_ARG(any_a && (any_b || !wb), "fh_rk_combine_groups_f32: a weight row is all zero (that output would be y: pass y instead)");
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
