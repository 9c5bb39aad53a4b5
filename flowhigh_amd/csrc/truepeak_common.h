// The pieces the true-peak kernels of clips (truepeak.hip) and of streams (stream_delivery.hip) share, so that both give the
// same bits: the 4x oversampling's phases and the limiter's last step.  flowhigh_amd/truepeak.py is the definition.
#pragma once
#include "fh_common.h"

namespace tp {

constexpr int HALO = 10;                        // input samples either side of n that x4[4 n + p] reads (truepeak.HALF)
constexpr int PHASE_TAPS = 2 * HALO + 1;        // phase 0; the others have one fewer
constexpr int PLAN_TAPS = 8 * HALO + 2;         // tables.resample_poly_plan(4, 1): one leading pad, then the 81 taps
constexpr int MAX_H = 512;                      // the limiter's largest half window (truepeak.MAX_H)

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

__device__ __forceinline__ float limit_sample(float x, float g, float c32) {
  return fminf(fmaxf(__fmul_rn(x, g), -c32), c32);
}

}  // namespace tp
