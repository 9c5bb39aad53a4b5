// Philox4x32-10 (Salmon et al., SC'11; Random123), the counter-based generator behind the device prior (prior.hip) and the
// dither of the int16 encoder (pcm.hip).  flowhigh_amd/prior.py restates it in numpy.
#pragma once
#include "fh_common.h"

namespace {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;        // multipliers
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;        // Weyl increments of the key

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
    const unsigned hi1 = __umulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
    c = u32x4{hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return c;
}

}  // namespace
