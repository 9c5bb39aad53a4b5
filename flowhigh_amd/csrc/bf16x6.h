// The bf16 x 6 form of fp32 products on the bf16 matrix cores (conv_form = 'bf16x6'): the device split of fp32 operands into
// bf16 pieces and the orders in which the piece pairs are multiplied.  Shared by conv_wino.hip (BF), conv_wino54_kernel.h (BF),
// narrow_bf.hip, conv_mfma_bf.hip and gemm_bf.hip.  Further down: the two-piece, three-pair form of the two direct conv kernels
// (conv_form = 'direct_bf16x3').
//
// Every fp32 operand is split EXACTLY into three pieces, x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)
// (round to nearest even; both subtractions are exact in fp32): 3 x 8 significant bits.  Pieces are numbered h = 0, m = 1,
// l = 2.  A product a b is the sum of the six piece pairs (i, j) with i + j <= 2 -- h h, h m, m h, h l, l h, m m -- one bf16
// MFMA each, all into the SAME fp32 accumulator; the dropped pairs (m l, l m, l l) are <= 2^-24 |a b|, below the rounding of
// the fp32 accumulation itself (tools/micro/bf16x6.hip: a 32 x 32 x 1024 product against float64: 4.17e-7 of sum |a b| for
// this form, 4.19e-7 for v_mfma_f32_32x32x2_f32).  Weights are split on the host (packing.split_pieces), activations on the
// device by bf16x6_split.
#pragma once
#include "fh_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned bf16_pack(float a, float b) {          // v_cvt_pk_bf16_f32 (round to nearest even)
  const bf16x2 v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, v);
}
// the low / high bf16 of a pair as a float.  (The low half by v_perm_b32: from `p << 16` the combiner makes a SECOND v_cvt_pk
// of (a, 0) and then the shift)
__device__ __forceinline__ float bf16_lo(unsigned p) { return __uint_as_float(__builtin_amdgcn_perm(0u, p, 0x01000c0cu)); }
__device__ __forceinline__ float bf16_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }

// 8 floats -> their three pieces, 8 bf16 (16 bytes) each; value e is bf16 e of each piece.  (The pieces are made as scalars and
// put into the vectors at the end: element writes into h / m / l give the two conv kernels another instruction schedule.)
__device__ __forceinline__ void bf16x6_split(const float (&v)[8], u32x4& h, u32x4& m, u32x4& l) {
  unsigned hp[4], mp[4], lp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = v[2 * i], b = v[2 * i + 1];
    hp[i] = bf16_pack(a, b);
    const float ra = a - bf16_lo(hp[i]), rb = b - bf16_hi(hp[i]);
    mp[i] = bf16_pack(ra, rb);
    lp[i] = bf16_pack(ra - bf16_lo(mp[i]), rb - bf16_hi(mp[i]));
  }
  h = (u32x4){hp[0], hp[1], hp[2], hp[3]};
  m = (u32x4){mp[0], mp[1], mp[2], mp[3]};
  l = (u32x4){lp[0], lp[1], lp[2], lp[3]};
}

// 8 floats -> the first two pieces only (conv_form = 'direct_bf16x3'): the h and m of bf16x6_split, bit for bit, without the third
// pack and the second pair of subtractions.
__device__ __forceinline__ void bf16x3_split(const float (&v)[8], u32x4& h, u32x4& m) {
  unsigned hp[4], mp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = v[2 * i], b = v[2 * i + 1];
    hp[i] = bf16_pack(a, b);
    mp[i] = bf16_pack(a - bf16_lo(hp[i]), b - bf16_hi(hp[i]));
  }
  h = (u32x4){hp[0], hp[1], hp[2], hp[3]};
  m = (u32x4){mp[0], mp[1], mp[2], mp[3]};
}

// Pair schedules: the six MFMAs of a product in the order they accumulate, as (piece of the first MFMA operand, piece of the
// second).  The order is part of a kernel's bits.
struct Bf16x6Pair {
  int a, b;
};
// small terms first: (l h) (h l) (m m) (m h) (h m) (h h) -- conv_wino.hip, narrow_bf.hip, gemm_bf.hip
constexpr Bf16x6Pair kBf16x6SmallFirst[6] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};
// first operand's piece major: (h h) (h m) (h l) (m h) (m m) (l h) -- conv_wino54_kernel.h, whose weight refill follows it
constexpr Bf16x6Pair kBf16x6AMajor[6] = {{0, 0}, {0, 1}, {0, 2}, {1, 0}, {1, 1}, {2, 0}};

// every pair (i, j) with i, j >= 0 and i + j <= 2 exactly once
constexpr bool bf16x6_is_schedule(const Bf16x6Pair (&s)[6]) {
  for (int k = 0; k < 6; ++k) {
    if (s[k].a < 0 || s[k].b < 0 || s[k].a + s[k].b > 2) return false;
    for (int j = 0; j < k; ++j)
      if (s[j].a == s[k].a && s[j].b == s[k].b) return false;
  }
  return true;
}
static_assert(bf16x6_is_schedule(kBf16x6SmallFirst) && bf16x6_is_schedule(kBf16x6AMajor),
              "a bf16 x 6 schedule is the six pairs with i + j <= 2");

// The bf16 x 3 form (conv_form = 'direct_bf16x3'; conv_mfma_bf.hip and narrow_bf.hip with two pieces): x ~ h + m, the first two pieces
// of the split above, and the three pairs with i + j <= 1.  bf16 rounds to 8 significant bits: |m| <= 2^-8 |x| and
// |x - h - m| <= 2^-16 |x|, so the dropped terms (a_m b_m and the two operands' remainders) are at most 3 2^-16 |a b| in the worst
// case -- eight bits short of the six-pair form, eight bits better than plain bf16; on random operands a sum of products sits at
// 0.04 .. 0.2 of 2^-16 sum |a b| (tests/test_direct_bf3_cpu.py).
// small terms first: (m h) (h m) (h h)
constexpr Bf16x6Pair kBf16x3SmallFirst[3] = {{1, 0}, {0, 1}, {0, 0}};

// every pair (i, j) with i, j >= 0 and i + j <= 1 exactly once
constexpr bool bf16x3_is_schedule(const Bf16x6Pair (&s)[3]) {
  for (int k = 0; k < 3; ++k) {
    if (s[k].a < 0 || s[k].b < 0 || s[k].a + s[k].b > 1) return false;
    for (int j = 0; j < k; ++j)
      if (s[j].a == s[k].a && s[j].b == s[k].b) return false;
  }
  return true;
}
static_assert(bf16x3_is_schedule(kBf16x3SmallFirst), "a bf16 x 3 schedule is the three pairs with i + j <= 1");

// the small-terms-first schedule of a product of NP-piece operands (NP = 3: six pairs, NP = 2: three) and its k-th pair
template <int NP>
constexpr int bf16_n_pairs() {
  static_assert(NP == 2 || NP == 3, "two or three pieces per operand");
  return NP == 3 ? 6 : 3;
}
template <int NP>
constexpr Bf16x6Pair bf16_small_first(int k) {
  return NP == 3 ? kBf16x6SmallFirst[k] : kBf16x3SmallFirst[k];
}

// the last index of schedule s whose first operand is piece p: behind it, that piece's registers are free
constexpr int bf16x6_last_use(const Bf16x6Pair (&s)[6], int p) {
  int last = -1;
  for (int k = 0; k < 6; ++k)
    if (s[k].a == p) last = k;
  return last;
}
