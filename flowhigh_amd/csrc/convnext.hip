// The two operators of the ConvNeXt vector field (FLowHigh(architecture='convnext')) that nothing else in csrc/ covers.
//
// Replaces, in the reference (paths under its src/flowhigh/):
//   fh_dwconv_ln_f32   ConvNeXtBlock: dwconv (Conv1d k = 7, pad 3, groups = dim) + AdaLayerNorm   models/convnext.py:44-52,87-93
//                      and, with w == NULL, the plain nn.LayerNorm behind the blocks               models/flow.py:253
//   fh_gelu_f32        nn.GELU between the two pointwise linears                                   models/convnext.py:54
//
// Rows are token-major [B*n, dim].  ONE kernel body with a clip locator as template parameter, as in frontend.hip: the batched
// entry (equal-length clips, clip b at row b * n) and the segment form (clips of different lengths, the table of
// fh_dwconv_gelu_res_seg_f32) are two instantiations of it.
//
// Block = dim / 4 threads (dim / 256 waves), lane = 4 consecutive channels: every access is one 16-byte vector.  A block owns
// LN_ROWS consecutive rows of one clip and reads 3 halo rows a side; the window of LN_GROUP + 6 input rows slides down the
// clip in registers, so an input row is loaded once per block.  Rows are normalised LN_GROUP at a time (two barriers per group).
//
// Row statistics: corrected two-pass over values that never leave the registers.  Pass 1 sums u, m = sum / dim.  Pass 2 sums
// d = u - m AND d * d: mean(d) takes the rounding of m out of d (it matters for rows with |mean| >> std: without it a row of
// equal values comes out as its rounding error times 1 / sqrt(eps)), the variance is that of the centred values -- never
// E[u^2] - mean^2.  Every sum is: the lane's 4 values, a 64-lane butterfly, then the waves' partials added in wave order out of
// LDS.  None of it depends on where the row sits in its block, its clip or the launch: a row's bits are a function of its own
// 7 input rows (zeros beyond the clip's ends), the same alone, in any batch and in the segment form.
#include "fh_common.h"

namespace {

constexpr int LN_ROWS = 16;        // rows a block owns (flowhigh_amd/convnext.py: DWLN_ROWS)
constexpr int LN_GROUP = 4;        // rows normalised between two pairs of barriers
constexpr int LN_HALO = 3;         // (7 - 1) / 2: shorter kernels are centred in the 7-tap window with zero taps around them
constexpr int LN_TAPS = 2 * LN_HALO + 1;
constexpr int LN_MAX_WAVES = 16;   // dim <= 4096
static_assert(LN_ROWS % LN_GROUP == 0, "a block's rows are whole groups");

struct BatchedRows {       // equal-length clips back to back
  static constexpr bool kExact = true;
  int n;
  __device__ void operator()(int b, int& row0, int& rows) const {
    row0 = b * n;
    rows = n;
  }
};
struct SegRows {           // device int32 [n_seg][2] = (first row, rows)
  static constexpr bool kExact = false;
  const int32_t* seg;
  __device__ void operator()(int b, int& row0, int& rows) const {
    row0 = seg[2 * b];
    rows = seg[2 * b + 1];
  }
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// LN_GROUP sums at once: per wave by butterfly, then the waves' partials in wave order.  `part` is [LN_GROUP][LN_MAX_WAVES];
// the caller alternates between two such arrays, so one barrier per call is enough.
__device__ __forceinline__ void block_sums(float (&v)[LN_GROUP], float* part, int wave, int lane, int n_waves) {
#pragma unroll
  for (int g = 0; g < LN_GROUP; ++g) v[g] = wave_sum(v[g]);
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < LN_GROUP; ++g) part[g * LN_MAX_WAVES + wave] = v[g];
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < LN_GROUP; ++g) {
    float tot = part[g * LN_MAX_WAVES];
    for (int w = 1; w < n_waves; ++w) tot += part[g * LN_MAX_WAVES + w];
    v[g] = tot;
  }
}

template <class Loc, bool CONV>
__global__ __launch_bounds__(1024) void dwconv_ln_kernel(Loc loc, const float* __restrict__ x, const float* __restrict__ wt,
                                                         const float* __restrict__ bias, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, float* __restrict__ y, int dim,
                                                         int ksz, float eps) {
#pragma clang fp contract(off)      // (every fused multiply-add below is spelled out: the same roundings in every instantiation)
  __shared__ float part[3][LN_GROUP * LN_MAX_WAVES];
  int row0, n;
  loc(blockIdx.y, row0, n);
  const int t0 = blockIdx.x * LN_ROWS;
  if (!Loc::kExact && t0 >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const int c = 4 * tid;
  const float* xb = x + (size_t)row0 * dim + c;
  float* yb = y + (size_t)row0 * dim + c;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  auto row = [&](int t) -> f32x4 { return (t >= 0 && t < n) ? ld4(xb + (size_t)t * dim) : zero; };

  f32x4 w[LN_TAPS], bv = zero;
  f32x4 win[LN_GROUP + 2 * LN_HALO];             // rows t - 3 .. t + LN_GROUP + 2 of the group at t
  if (CONV) {
    const int lo = LN_HALO - ksz / 2;            // tap j of the kernel sits at window tap lo + j
#pragma unroll
    for (int j = 0; j < LN_TAPS; ++j) w[j] = (j >= lo && j < lo + ksz) ? ld4(wt + (size_t)(j - lo) * dim + c) : zero;
    bv = ld4(bias + c);
#pragma unroll
    for (int i = 0; i < 2 * LN_HALO; ++i) win[LN_GROUP + i] = row(t0 - LN_HALO + i);
  }
  const f32x4 sc = ld4(scale + c), sh = ld4(shift + c);

  for (int t = t0; t < t0 + LN_ROWS && t < n; t += LN_GROUP) {
    f32x4 u[LN_GROUP];
    if (CONV) {
#pragma unroll
      for (int i = 0; i < 2 * LN_HALO; ++i) win[i] = win[LN_GROUP + i];
#pragma unroll
      for (int g = 0; g < LN_GROUP; ++g) win[2 * LN_HALO + g] = row(t + LN_HALO + g);
#pragma unroll
      for (int g = 0; g < LN_GROUP; ++g) {
        f32x4 acc = bv;
#pragma unroll
        for (int j = 0; j < LN_TAPS; ++j) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(w[j][e], win[g + j][e], acc[e]);
        }
        u[g] = acc;
      }
    } else {
#pragma unroll
      for (int g = 0; g < LN_GROUP; ++g) u[g] = row(t + g);
    }
    // pass 1: the mean
    float s[LN_GROUP];
#pragma unroll
    for (int g = 0; g < LN_GROUP; ++g) s[g] = (u[g][0] + u[g][1]) + (u[g][2] + u[g][3]);
    block_sums(s, part[0], wave, lane, n_waves);
    // pass 2: the centred values, their mean (what rounding left in pass 1's) and their sum of squares
    float s1[LN_GROUP], s2[LN_GROUP];
#pragma unroll
    for (int g = 0; g < LN_GROUP; ++g) {
      const float m = s[g] / (float)dim;
#pragma unroll
      for (int e = 0; e < 4; ++e) u[g][e] = u[g][e] - m;
      s1[g] = (u[g][0] + u[g][1]) + (u[g][2] + u[g][3]);
      s2[g] = fmaf(u[g][3], u[g][3], fmaf(u[g][2], u[g][2], fmaf(u[g][1], u[g][1], u[g][0] * u[g][0])));
    }
    // (both sums behind ONE barrier: s1 goes through part[1], s2 through part[2]; the next group's pass 1 writes part[0] again
    // only after this barrier, behind which nobody reads part[0] any more)
#pragma unroll
    for (int g = 0; g < LN_GROUP; ++g) {
      s1[g] = wave_sum(s1[g]);
      s2[g] = wave_sum(s2[g]);
    }
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < LN_GROUP; ++g) {
        part[1][g * LN_MAX_WAVES + wave] = s1[g];
        part[2][g * LN_MAX_WAVES + wave] = s2[g];
      }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < LN_GROUP; ++g) {
      float t1 = part[1][g * LN_MAX_WAVES], t2 = part[2][g * LN_MAX_WAVES];
      for (int wv = 1; wv < n_waves; ++wv) {
        t1 += part[1][g * LN_MAX_WAVES + wv];
        t2 += part[2][g * LN_MAX_WAVES + wv];
      }
      if (t + g < n) {
        const float dm = t1 / (float)dim;
        float var = t2 / (float)dim - dm * dm;          // (dm is a rounding error: no cancellation here)
        var = fmaxf(var, 0.f);
        const float rstd = 1.0f / sqrtf(var + eps);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf((u[g][e] - dm) * rstd, sc[e], sh[e]);
        *reinterpret_cast<f32x4*>(yb + (size_t)(t + g) * dim) = o;
      }
    }
    // (the next group's first barrier separates these reads of part[1] / part[2] from the next writes to them)
  }
}

// y = gelu_erf(x); 4 elements per thread, one 16-byte access where both pointers allow it
__global__ __launch_bounds__(256) void gelu_kernel(const float* x, float* y, long long n, int vec) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (vec && i + 4 <= n) {
    const f32x4 v = ld4(x + i);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = gelu_erf(v[e]);
    *reinterpret_cast<f32x4*>(y + i) = o;
  } else {
    for (long long k = i; k < i + 4 && k < n; ++k) y[k] = gelu_erf(x[k]);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <class Loc>
int launch_dwconv_ln(const char* name, Loc loc, const float* x, const float* w, const float* bias, const float* scale,
                     const float* shift, float* y, int n_clips, int max_n, int dim, int ksz, float eps, void* stream) {
  const dim3 grid(fh_cdiv(max_n, LN_ROWS), n_clips), block(dim / 4);
  if (w)
    hipLaunchKernelGGL((dwconv_ln_kernel<Loc, true>), grid, block, 0, (hipStream_t)stream, loc, x, w, bias, scale, shift, y, dim,
                       ksz, eps);
  else
    hipLaunchKernelGGL((dwconv_ln_kernel<Loc, false>), grid, block, 0, (hipStream_t)stream, loc, x, w, bias, scale, shift, y,
                       dim, ksz, eps);
  FH_CHECK_LAUNCH(name);
  return FH_OK;
}

}  // namespace

#define FH_CHECK_DWLN(name)                                                                                                  \
  FH_CHECK_ARG(dim > 0 && dim % 256 == 0 && dim <= 256 * LN_MAX_WAVES, name ": dim %d unsupported (a multiple of 256, <= %d)", \
               dim, 256 * LN_MAX_WAVES);                                                                                     \
  FH_CHECK_ARG(!w || (bias && (ksz & 1) && ksz >= 1 && ksz <= LN_TAPS), name ": ksz %d unsupported (odd, <= %d, with a bias)", \
               ksz, LN_TAPS);                                                                                                \
  FH_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(w) && aligned16(bias) && aligned16(scale) && aligned16(shift),      \
               name ": pointers must be 16-byte aligned");                                                                   \
  FH_CHECK_ARG(eps > 0.f, name ": eps must be positive")

extern "C" int fh_dwconv_ln_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                                float* y, int batch, int n, int dim, int ksz, float eps, void* stream) {
  FH_CHECK_ARG(x && scale && shift && y && batch > 0 && batch < 65536 && n > 0 && (long long)batch * n < (1ll << 31),
               "fh_dwconv_ln_f32: bad args");
  FH_CHECK_DWLN("fh_dwconv_ln_f32");
  return launch_dwconv_ln("fh_dwconv_ln_f32", BatchedRows{n}, x, w, bias, scale, shift, y, batch, n, dim, ksz, eps, stream);
}

extern "C" int fh_dwconv_ln_seg_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                                    float* y, const int* seg, int n_seg, int max_n, int dim, int ksz, float eps, void* stream) {
  FH_CHECK_ARG(x && scale && shift && y && seg && n_seg > 0 && n_seg < 65536 && max_n > 0, "fh_dwconv_ln_seg_f32: bad args");
  FH_CHECK_DWLN("fh_dwconv_ln_seg_f32");
  return launch_dwconv_ln("fh_dwconv_ln_seg_f32", SegRows{seg}, x, w, bias, scale, shift, y, n_seg, max_n, dim, ksz, eps, stream);
}

extern "C" int fh_gelu_f32(const float* x, float* y, long long n, void* stream) {
  FH_CHECK_ARG(x && y && n > 0 && n < (1ll << 40), "fh_gelu_f32: bad args");
  hipLaunchKernelGGL(gelu_kernel, dim3(fh_cdiv(n, 1024)), dim3(256), 0, (hipStream_t)stream, x, y, n,
                     (int)(aligned16(x) && aligned16(y)));
  FH_CHECK_LAUNCH("fh_gelu_f32");
  return FH_OK;
}
