// The 2048-point complex FFT in LDS that the kernels of fft.hip and quality.hip share: radix-2 decimation in time on two double
// arrays of 2048 (32 KB), bit-reversed load, 11 butterfly stages, one barrier each, 4 butterflies per thread and stage, 256
// threads.  Twiddles W^k = exp(-2 pi i k / 2048), k < 1024, come from a table computed in float64 on the host
// (tables.fft_twiddles).
#pragma once
#include "fh_common.h"

namespace {

constexpr int FFT_N = 2048;
constexpr int FFT_LOG = 11;
constexpr int FFT_BINS = 1025;

__device__ __forceinline__ int bitrev11(int n) { return (int)(__brev((unsigned)n) >> 21); }

// 11 in-place butterfly stages over re[], im[] (bit-reversed order in, natural order out)
__device__ __forceinline__ void fft2048_stages(double* re, double* im, const double2* __restrict__ tw, int tid) {
#pragma unroll 1
  for (int s = 1; s <= FFT_LOG; ++s) {
    const int half = 1 << (s - 1);
    const int tstep = FFT_N >> s;               // twiddle index stride: W_m^pos = W_2048^(pos * 2048 / m)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = tid + 256 * q;
      const int pos = j & (half - 1);
      const int i0 = ((j >> (s - 1)) << s) + pos, i1 = i0 + half;
      const double2 w = tw[pos * tstep];
      const double xr = re[i1], xi = im[i1];
      const double tr = w.x * xr - w.y * xi, ti = w.x * xi + w.y * xr;
      const double ar = re[i0], ai = im[i0];
      re[i0] = ar + tr;
      im[i0] = ai + ti;
      re[i1] = ar - tr;
      im[i1] = ai - ti;
    }
  }
  __syncthreads();
}

}  // namespace
