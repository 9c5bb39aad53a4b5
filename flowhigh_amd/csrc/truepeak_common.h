// The pieces the true-peak kernels of clips (truepeak.hip) and of streams (stream_delivery.hip) share, so that both give the
// same bits: the tile's constants, the 4x oversampling's phases and a sample's peak, the limiter's gain over a tile and its last
// step.  flowhigh_amd/truepeak.py is the definition.
#pragma once
#include "fh_common.h"

namespace tp {

constexpr int THREADS = 256;
constexpr int TILE = 1024;                      // frames (outputs) per workgroup
constexpr int PER = TILE / THREADS;
constexpr int HALO = 10;                        // input samples either side of n that x4[4 n + p] reads (truepeak.HALF)
constexpr int PHASE_TAPS = 2 * HALO + 1;        // phase 0; the others have one fewer
constexpr int PLAN_TAPS = 8 * HALO + 2;         // tables.resample_poly_plan(4, 1): one leading pad, then the 81 taps
constexpr int MAX_H = 512;                      // the limiter's largest half window (truepeak.MAX_H)
constexpr int LIM_N = TILE + 4 * MAX_H;         // r over a tile +- 2 H

// hs[p][i] = h[p + 4 i], h = taps + 1 (the plan's taps behind its leading pad); phases 1 .. 3 have 20 taps
__device__ __forceinline__ void load_taps(const float* __restrict__ taps, float (*hs)[PHASE_TAPS]) {
  const int t = threadIdx.x;
  if (t < 4 * PHASE_TAPS) {
    const int p = t / PHASE_TAPS, i = t % PHASE_TAPS, j = p + 4 * i;
    hs[p][i] = j < PLAN_TAPS - 1 ? taps[1 + j] : 0.f;
  }
}

template <int P>
__device__ __forceinline__ float tp_phase(const float* __restrict__ xs, const float (*hs)[PHASE_TAPS], int i) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < (P == 0 ? PHASE_TAPS : PHASE_TAPS - 1); ++k) acc = fmaf(hs[P][k], xs[i + 2 * HALO - k], acc);
  return fabsf(acc);
}

// max(|x[n]|, |x4[4 n + p]|, p = 0 .. 3) of the sample staged at xs[j + HALO]
__device__ __forceinline__ float peak_at(const float* __restrict__ xs, const float (*hs)[PHASE_TAPS], int j) {
  float mv = fabsf(xs[j + HALO]);
  mv = fmaxf(mv, tp_phase<0>(xs, hs, j));
  mv = fmaxf(mv, tp_phase<1>(xs, hs, j));
  mv = fmaxf(mv, tp_phase<2>(xs, hs, j));
  mv = fmaxf(mv, tp_phase<3>(xs, hs, j));
  return mv;
}

// a[0][j] = r[tile0 - 2 H + j], j < N = TILE + 4 H, and ws[k] = w[k], k < 2 H + 1 (both behind a barrier) -> acc[k] =
// g[tile0 + t + k THREADS] in float64: the sliding minimum over 2 H + 1 by doubling (a[j] = min r[j .. j + P), P the largest
// power of two <= 2 H + 1, then two overlapping windows) and the Hann sum in ascending k
__device__ __forceinline__ void gain_tile(float (*a)[LIM_N], const double* __restrict__ ws, int H, double (&acc)[PER]) {
  const int t = threadIdx.x, W = 2 * H + 1, N = TILE + 4 * H;
  int cur = 0, P = 1;
  for (; 2 * P <= W; P *= 2) {                                      // a[cur][j] = min r[j .. j + P) -> ... + 2 P)
    for (int j = t; j < N; j += THREADS) a[cur ^ 1][j] = j + P < N ? fminf(a[cur][j], a[cur][j + P]) : a[cur][j];
    cur ^= 1;
    __syncthreads();
  }
  // q[i] = min r[i .. i + W): the frame tile0 - H + i, i < TILE + 2 H (i + W - 1 <= N - 1)
  float* __restrict__ q = a[cur ^ 1];
  for (int i = t; i < TILE + 2 * H; i += THREADS) q[i] = fminf(a[cur][i], a[cur][i + W - P]);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) acc[k] = 0.0;
  for (int kk = 0; kk < W; ++kk) {                                  // g[tile0 + i] = sum_kk w[kk] q[i + kk], ascending
    const double wv = ws[kk];
#pragma unroll
    for (int k = 0; k < PER; ++k) acc[k] = fma(wv, (double)q[t + k * THREADS + kk], acc[k]);
  }
}

__device__ __forceinline__ float limit_sample(float x, float g, float c32) {
  return fminf(fmaxf(__fmul_rn(x, g), -c32), c32);
}

}  // namespace tp
