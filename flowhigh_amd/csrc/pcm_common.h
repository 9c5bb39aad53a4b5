// The sample encoder and the dither of the int16 encoders (pcm.hip: clips, stream_delivery.hip: blocks of a stream), one
// statement for both: flowhigh_amd/pcm.py is the definition.
#pragma once
#include "fh_common.h"
#include "philox.h"

namespace {

constexpr int RUN = 8;                          // samples per thread = one 16-byte store of int16
constexpr unsigned KEY_TAG = 0x50434D31u;       // 'PCM1': keeps the dither's blocks apart from the prior's under the same key

typedef short i16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ short encode(float x, float d) {
  float v = __fmul_rn(x, 32768.f);
  v = __fadd_rn(v, d);
  float q = rintf(v);
  q = fminf(fmaxf(q, -32768.f), 32767.f);
  return (v != v) ? (short)0 : (short)(int)q;
}

// d[k] = the dither of sample first + k of channel ch under the key (seed, strm).  A run of 8 samples touches 4 Philox blocks
// when it starts on an even sample, 5 when on an odd one; with first < 0 the run's samples before t = 0 are never stored.
__device__ __forceinline__ void dither_run(unsigned long long seed, unsigned long long strm, int ch, long long first,
                                           float (&d)[RUN]) {
  const unsigned k0 = (unsigned)seed ^ KEY_TAG, k1 = (unsigned)(seed >> 32) ^ (unsigned)ch;
  const long long t0 = first < 0 ? 0 : first;
  const long long q0 = t0 >> 1;
  u32x4 r[RUN / 2 + 1];
#pragma unroll
  for (int j = 0; j <= RUN / 2; ++j) {
    const unsigned long long q = (unsigned long long)(q0 + j);
    if (j < RUN / 2 || (first & 1))
      r[j] = philox4x32_10(u32x4{(unsigned)q, (unsigned)(q >> 32), (unsigned)strm, (unsigned)(strm >> 32)}, k0, k1);
    else
      r[j] = u32x4{0u, 0u, 0u, 0u};
  }
  const int odd = (int)(first & 1);            // (first may be negative: & 1 is its parity all the same)
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long t = first + k;              // sample t lies in block (t >> 1) - q0
    const int j = (int)((t >> 1) - q0);
    u32x4 rr = r[0];
#pragma unroll
    for (int m = 1; m <= RUN / 2; ++m) rr = (j == m) ? r[m] : rr;
    const bool hi = ((k + odd) & 1) != 0;
    const unsigned ra = hi ? rr[2] : rr[0], rb = hi ? rr[3] : rr[1];
    d[k] = (float)((int)(ra >> 8) - (int)(rb >> 8)) * 0x1p-24f;
  }
}

}  // namespace
