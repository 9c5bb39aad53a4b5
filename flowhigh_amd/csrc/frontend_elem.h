// Per-element arithmetic of the front / back end kernels, shared by the batched entries (frontend.hip: equal-length clips,
// clip b at b * len) and their segment forms (frontend_seg.hip: clips of different lengths, one descriptor per clip).
// One copy of every expression, so that a clip gets the same bits whichever entry runs it: the callers only differ in
// how a block finds its clip's pointers and lengths.
#pragma once
#include "fh_common.h"

constexpr int FE_P_BLOCKS = 33;                  // 33 * 32 = 1056 >= 1025 bins
constexpr int FE_P_WIDTH = FE_P_BLOCKS * 64;     // 2112 floats per frame (P-layout)
constexpr int FE_SE_LANES = 32;                  // frame lanes of the spectral energy sum

// frames[t, k] = pad(a)[hop t + k] * window[k]; pad_mode 0: reflect (no edge repeat; pad < len), 1: zero
__device__ __forceinline__ float fe_frame_value(const float* __restrict__ a, const float* __restrict__ window, int len,
                                                int t, int k, int hop, int pad, int pad_mode) {
  int i = hop * t + k - pad;
  float v;
  if (pad_mode == 0) {
    if (i < 0) i = -i;
    if (i >= len) i = 2 * (len - 1) - i;
    v = a[i];
  } else {
    v = (i >= 0 && i < len) ? a[i] : 0.f;
  }
  return v * window[k];
}

// One block of 32 * FE_SE_LANES threads: energy[bin] = sum_t |S[t, bin]| for the 32 bins of P-block `blk` over the n_frames
// rows at `spec` (the clip's first row).  thread -> (bin i = tid & 31, frame lane = tid >> 5); every lane sums its frames
// t = fl, fl + 64, ... and t = fl + 32, fl + 96, ... as two independent chains in double, lanes are added in lane order.
__device__ __forceinline__ void fe_spec_energy_block(const float* __restrict__ spec, float* __restrict__ energy, int n_frames,
                                                     int blk) {
  __shared__ double part[FE_SE_LANES][32];
  const int i = threadIdx.x & 31, fl = threadIdx.x >> 5;
  const float* s = spec + blk * 64;
  double acc = 0.0, acc2 = 0.0;
  for (int t = fl; t < n_frames; t += 2 * FE_SE_LANES) {
    float re = s[(size_t)t * FE_P_WIDTH + i], im = s[(size_t)t * FE_P_WIDTH + 32 + i];
    acc += (double)sqrtf(re * re + im * im);
    const int t2 = t + FE_SE_LANES;
    if (t2 < n_frames) {
      re = s[(size_t)t2 * FE_P_WIDTH + i], im = s[(size_t)t2 * FE_P_WIDTH + 32 + i];
      acc2 += (double)sqrtf(re * re + im * im);
    }
  }
  part[fl][i] = acc + acc2;
  __syncthreads();
  if (fl == 0) {
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < FE_SE_LANES; ++q) tot += part[q][i];
    int bin = blk * 32 + i;
    if (bin < 1025) energy[bin] = (float)tot;
  }
}

// frequency bin of column `col` of a P-layout row (re at 64 b + i, im at 64 b + 32 + i, bin = 32 b + i)
__device__ __forceinline__ int fe_p_bin(int col) { return (col >> 6) * 32 + (col & 31); }

// sample j of the inverse STFT's overlap-add over the clip's n_frames rows at `fb`: sum_t w f / sum_t w^2 over the frames
// that cover j, zero past the OLA signal's end (torch.istft zero-fills there)
__device__ __forceinline__ float fe_istft_ola_value(const float* __restrict__ fb, const float* __restrict__ window, int j,
                                                    int n_frames, int nfft, int hop) {
  const int avail = hop * (n_frames - 1) + nfft / 2;
  if (j >= avail) return 0.f;
  const int p = j + nfft / 2;
  int t_hi = p / hop;
  if (t_hi > n_frames - 1) t_hi = n_frames - 1;
  int t_lo = (p - nfft + hop) / hop;          // ceil((p - nfft + 1) / hop) for p - nfft + 1 > 0
  if (p - nfft + 1 <= 0) t_lo = 0;
  float num = 0.f, den = 0.f;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int k = p - hop * t;
    const float w = window[k];
    num = fmaf(w, fb[(size_t)t * nfft + k], num);
    den = fmaf(w, w, den);
  }
  return num / den;
}

// max over a 256-thread block of m >= 0 into *peak_bits (non-negative float bits order as integers: order-independent)
__device__ __forceinline__ void fe_block_peak(float m, uint32_t* __restrict__ peak_bits) {
  __shared__ float red[4];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(peak_bits, __float_as_uint(m));
  }
}

// same order as the reference: (y / peak) * 0.99
__device__ __forceinline__ float fe_peak_scale_value(float y, float peak, float target) {
  float v = y / peak;
  return v * target;
}

// out[i] = sum_j x[j] * h[(i + pre) * down - j * up],  h zero outside [0, n_taps)
__device__ __forceinline__ float fe_resample_value(const float* __restrict__ xb, const float* __restrict__ h, int i,
                                                   int len_in, int up, int down, int n_taps, int pre) {
  const long long pos = (long long)(i + pre) * down;
  long long j_hi = pos / up;
  if (j_hi > len_in - 1) j_hi = len_in - 1;
  float acc = 0.f;
  // ascending j == descending tap index; scipy's upfirdn walks the taps in ascending order,
  // so accumulate from the smallest tap index (largest j) down to match its summation order.
  for (long long j = j_hi; j >= 0; --j) {
    long long k = pos - j * up;
    if (k >= n_taps) break;
    acc = fmaf(xb[j], h[k], acc);
  }
  return acc;
}
