// The sample encoders and the dither of the PCM encoders (pcm.hip: clips, stream_delivery.hip: blocks of a stream), one
// statement for both: flowhigh_amd/pcm.py is the definition.  int16: encode(); 24-bit ('s24' packed in 3 bytes, 's24in32' in an
// int32): encode24(), and the stores of a run of 8 such samples (lead24, store_run24).
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

// The 24-bit sample: v = x * 2^23 in float64 (exact, so contraction cannot change it), ONE float64 add of the dither (a float32
// add would round it away: x * 2^23 fills the float32 significand), rint to even, clamp to [-2^23, 2^23 - 1]; NaN -> 0.
__device__ __forceinline__ int encode24(float x, float d) {
  double v = __dmul_rn((double)x, 8388608.0);
  v = __dadd_rn(v, (double)d);
  double q = rint(v);
  q = fmin(fmax(q, -8388608.0), 8388607.0);
  return (v != v) ? 0 : (int)q;
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

// The dither of ONE sample t >= 0 of channel ch: dither_run's value for it (one Philox block per sample; the flat interleaved
// runs of the 24-bit encoders, whose 8 samples lie in up to 8 channels).
__device__ __forceinline__ float dither_at(unsigned long long seed, unsigned long long strm, int ch, long long t) {
  const unsigned k0 = (unsigned)seed ^ KEY_TAG, k1 = (unsigned)(seed >> 32) ^ (unsigned)ch;
  const unsigned long long q = (unsigned long long)t >> 1;
  const u32x4 r = philox4x32_10(u32x4{(unsigned)q, (unsigned)(q >> 32), (unsigned)strm, (unsigned)(strm >> 32)}, k0, k1);
  const bool hi = (t & 1) != 0;
  const unsigned ra = hi ? r[2] : r[0], rb = hi ? r[3] : r[1];
  return (float)((int)(ra >> 8) - (int)(rb >> 8)) * 0x1p-24f;
}

// ---- the stores of the 24-bit encoders -------------------------------------------------------------------------------------
// A row is N samples of `container` bytes (3: the low three bytes, least significant first; 4: the int32) from the byte address
// `row` on.  A thread owns a run of 8 samples = 24 or 32 contiguous bytes; run r starts at sample 8 r - lead, and lead24 puts that
// at an 8-byte (packed) or 32-byte (int32, row 4-byte aligned) boundary: 3 lead = row (mod 8) has the solution lead = 3 row, and
// 24 is a multiple of 8, so every run of the row is aligned alike.  A run wholly inside the row is three 8-byte stores (two
// 16-byte ones for int32); the at most two runs over a row end go byte by byte (sample by sample for int32).  Nothing outside
// [row, row + container * N) is read or written, and no word is shared: neighbours that abut at any byte address stay intact.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int lead24(const unsigned char* row, int container) {
  return container == 3 ? (int)((3 * ((size_t)row & 7)) & 7) : (int)(((size_t)row >> 2) & (RUN - 1));
}

__device__ __forceinline__ void store_run24(unsigned char* __restrict__ row, long long first, long long N, const int (&q)[RUN],
                                            int container) {
  const bool whole = first >= 0 && first + RUN <= N;
  if (container == 4) {
    int* __restrict__ out = reinterpret_cast<int*>(row);
    if (whole) {
      *reinterpret_cast<i32x4*>(out + first) = i32x4{q[0], q[1], q[2], q[3]};
      *reinterpret_cast<i32x4*>(out + first + 4) = i32x4{q[4], q[5], q[6], q[7]};
      return;
    }
#pragma unroll
    for (int k = 0; k < RUN; ++k)
      if (first + k >= 0 && first + k < N) out[first + k] = q[k];
    return;
  }
  if (whole) {
    unsigned w[6];
#pragma unroll
    for (int h = 0; h < 2; ++h) {             // 4 samples = 12 bytes = 3 words
      const unsigned a = (unsigned)q[4 * h] & 0xFFFFFFu, b = (unsigned)q[4 * h + 1] & 0xFFFFFFu,
                     c = (unsigned)q[4 * h + 2] & 0xFFFFFFu, e = (unsigned)q[4 * h + 3] & 0xFFFFFFu;
      w[3 * h] = a | (b << 24);
      w[3 * h + 1] = (b >> 8) | (c << 16);
      w[3 * h + 2] = (c >> 16) | (e << 8);
    }
    u32x2* __restrict__ out = reinterpret_cast<u32x2*>(row + 3 * first);
    out[0] = u32x2{w[0], w[1]};
    out[1] = u32x2{w[2], w[3]};
    out[2] = u32x2{w[4], w[5]};
    return;
  }
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const long long s = first + k;
    if (s < 0 || s >= N) continue;
    const unsigned u = (unsigned)q[k];
    row[3 * s] = (unsigned char)u;
    row[3 * s + 1] = (unsigned char)(u >> 8);
    row[3 * s + 2] = (unsigned char)(u >> 16);
  }
}

}  // namespace
