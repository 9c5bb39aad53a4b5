// The frame of the two attention kernels, attention.hip (fp32 MFMA products) and attention_bf.hip (bf16 x 6 products): everything
// beside the staging of K / V and the two products.  Both kernels place a block, reduce a query row, merge its streams, write
// it out and are launched by this one copy, so both have the same batch / ragged / kernel-shape invariances and agree bit for
// bit wherever their products are exact.  A kernel reads: attn_prologue, its Q fragments, init_streams, its staging loop with
// per tile (S^T product, softmax_step, O^T product), attn_finish.
#pragma once
#include <float.h>
#include <math.h>

#include "fh_common.h"

// Every query row is reduced as TWO interleaved online-softmax streams -- stream 0 takes the even 32-key tiles,
// stream 1 the odd ones -- merged once at the end by merge_streams().  The two kernel shapes differ only in who
// runs the streams, never in the arithmetic, so a clip gives the same bits whatever else is in the batch:
//   SPLIT = 2 (small grids): 64 queries per block, the two waves of a 32-query tile take one stream each -- twice
//                            the waves and half the dependent MFMA chain per wave when there are fewer query tiles
//                            than SIMDs (B = 1, n = 1000: 512 tiles, 1024 SIMDs);
//   SPLIT = 1 (large grids): 128 queries per block, every wave runs both streams of its tile one after the other
//                            (half the K / V staging traffic per query).
struct Stream {
  f32x16 o0, o1;
  float m, l;
};

// Where a thread stands: block = (query block, head, clip), wave = (query tile qt, stream sp), lane = query qi of the tile
// (column l31 of the MFMA tiles, lane half lh).
struct AttnBlock {
  bool live;               // false: a ragged clip ends before this block's first query
  int h, tid, lane, l31, lh;
  int inner;               // heads * 64: row pitch of out, offset of K (and 2 x: of V) in a qkv row
  size_t ld;               // row pitch of qkv
  size_t row0;             // the clip's first row of the token-major tensors
  int n;                   // its rows = its keys
  const float* base;       // Q of that row, this head
  int qt, sp, qi;
};

template <int WAVES, int SPLIT>
__device__ __forceinline__ AttnBlock attn_prologue(const float* __restrict__ qkv, int n, int heads, const int* __restrict__ seg) {
  AttnBlock c;
  const int b = blockIdx.z;
  c.h = blockIdx.y;
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  const int wave = c.tid >> 6;
  c.l31 = c.lane & 31;
  c.lh = c.lane >> 5;
  c.inner = heads * 64;
  c.ld = (size_t)3 * c.inner;
  // ragged batch (the _seg_ entries): clip b is rows [seg[2b], seg[2b] + seg[2b+1]) of the token-major tensors;
  // its keys are its own rows only (the reference's key mask, attend.py:127-128, for clips packed without padding)
  c.row0 = (size_t)b * n;
  c.n = n;
  c.live = true;
  if (seg) {
    c.row0 = (size_t)__builtin_amdgcn_readfirstlane(seg[2 * b]);
    c.n = __builtin_amdgcn_readfirstlane(seg[2 * b + 1]);
    c.live = (int)blockIdx.x * (32 * WAVES / SPLIT) < c.n;          // (block-uniform: the kernel returns before any barrier)
  }
  c.base = qkv + c.row0 * c.ld + c.h * 64;
  c.qt = wave / SPLIT;                     // query tile of the block
  c.sp = wave % SPLIT;                     // stream of this wave (SPLIT = 2)
  c.qi = blockIdx.x * (32 * WAVES / SPLIT) + c.qt * 32 + c.l31;
  return c;
}

// The band of the banded kernels (BAND): query i reads the keys j with |i - j| <= radius.  Two things follow from it.
//   The keys [lo, hi) a block's staging loop walks, in 64-key iterations from lo: all of the clip's, or (BAND) the iterations that
//   hold a key within `radius` of one of the block's `qb` queries.  lo is a multiple of 64, so a tile keeps its absolute index and
//   with it its stream, (k0 / 32) & 1, whatever the band and the kernel shape; the range is block-uniform (the barriers of the loop
//   stay outside any divergence, every wave runs the same trip count).
//   The key mask of softmax_step.  A tile of the range that is out of a query's band is an exact no-op for that query, so a row's
//   bits depend on its valid keys alone: not on the batch, the kernel shape or the form (batched / segment) of the launch.
// The full kernels hold the empty AttnBand<false>: their code is what it was before there was a band.
template <bool BAND>
struct AttnBand;

template <>
struct AttnBand<false> {
  __device__ __forceinline__ AttnBand(const AttnBlock&, int) {}
  __device__ __forceinline__ int lo() const { return 0; }
  __device__ __forceinline__ int hi(int n) const { return n; }
};

template <>
struct AttnBand<true> {
  int radius;              // <= the longest clip's rows (clamped by the entry): query + radius cannot overflow
  int k_lo, k_hi;
  int q_lo, q_hi;          // the lane's valid keys are [q_lo, q_hi] (and < n)
  int w_lo, w_hi;          // a tile [k0, k0 + 32) with w_lo <= k0 <= w_hi is inside the band of all 32 queries of the wave's tile
  __device__ __forceinline__ AttnBand(const AttnBlock& c, int qb, int r) : radius(r) {
    const int q0 = blockIdx.x * qb;
    const int first = q0 - r, end = q0 + qb + r;
    k_lo = (first > 0 ? first : 0) / 64 * 64;
    k_hi = end < c.n ? end : c.n;
    q_lo = c.qi - r;
    q_hi = c.qi + r;
    const int qw0 = __builtin_amdgcn_readfirstlane(c.qi - c.l31);        // first query of the wave's tile (wave-uniform)
    w_lo = qw0 + 31 - r;
    w_hi = qw0 + r - 31;
  }
  __device__ __forceinline__ int lo() const { return k_lo; }
  __device__ __forceinline__ int hi(int) const { return k_hi; }
};

template <int NS>
__device__ __forceinline__ void init_streams(Stream (&st)[NS]) {
#pragma unroll
  for (int i = 0; i < NS; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { st[i].o0[r] = 0.f; st[i].o1[r] = 0.f; }
    st[i].m = -INFINITY;
    st[i].l = 0.f;
  }
}

// One 32-key tile of scores s (the S^T accumulator: this lane's query, key of reg r = k0 + (r&3) + 8 (r>>2) + 4 lh) into
// stream S: s becomes the probabilities, S.o0 / S.o1 are rescaled for the O^T product that follows.
// Online softmax in base 2 (scores arrive multiplied by scale * log2(e): one v_exp_f32 per probability instead of the libm
// expf's ~10 instructions -- matrix and vector instructions share the fp32 ALUs, so every one of the ~420 vector instructions
// per tile cost matrix time: round 6).
// BAND: a key is valid for the lane's query iff key < n and it is within the band.  A tile inside the band of all 32 queries of
// the wave and below n takes the unmasked path (wave-uniform).  A lane may meet a tile -- its first one too -- in which none of its
// keys is valid: that tile leaves m and l as they are, gives p = 0 and multiplies o by exactly 1 (by 0 while m is still -inf: o is
// still 0 then).
template <bool BAND>
__device__ __forceinline__ void softmax_step(Stream& S, f32x16& s, int k0, int n, int lh, float scale, const AttnBand<BAND>& band) {
  float mx = -INFINITY;
  bool whole;
  if constexpr (BAND) whole = k0 + 32 <= n && k0 >= band.w_lo && k0 <= band.w_hi;
  else whole = k0 + 32 <= n;
  if (whole) {                                     // (whole tile: no key mask -- wave-uniform)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = __fmul_rn(s[r], scale);
      mx = fmaxf(mx, s[r]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      bool valid;
      if constexpr (BAND) valid = key < n && key >= band.q_lo && key <= band.q_hi;
      else valid = key < n;
      const float v = valid ? __fmul_rn(s[r], scale) : -INFINITY;
      s[r] = v;
      mx = fmaxf(mx, v);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(S.m, mx);            // finite: every tile has >= 1 valid key (BAND: per lane it may have none)
  // (BAND, no valid key so far: exp2(-inf - -inf) would be NaN; against a finite number every exponent below is exp2(-inf) = 0)
  const float m_ref = BAND ? fmaxf(m_new, -FLT_MAX) : m_new;
  const float corr = __builtin_amdgcn_exp2f(S.m - m_ref);        // exp2(-inf) = 0 on the first tile
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float p = __builtin_amdgcn_exp2f(s[r] - m_ref);
    s[r] = p;
    psum += p;
  }
  psum += __shfl_xor(psum, 32, 64);
  S.l = __fmaf_rn(S.l, corr, psum);
  S.m = m_new;
  // (the running maximum settles after a few tiles: when no lane's changed, the 32 multiplications by 1 are skipped --
  // x * 1 is exact, so the bits are those of the multiplied form)
  if (__builtin_amdgcn_ballot_w64(corr != 1.f) != 0ull) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { S.o0[r] *= corr; S.o1[r] *= corr; }
  }
}

__device__ __forceinline__ void merge_streams(Stream& a, const float (&b0)[16], const float (&b1)[16], float mb, float lb) {
  const float m = fmaxf(a.m, mb);                          // (maxima are in the base-2 domain of the tile loop)
  const float c0 = __builtin_amdgcn_exp2f(a.m - m), c1 = __builtin_amdgcn_exp2f(mb - m);      // exp2(-inf) = 0: a stream that saw no key contributes nothing
  a.l = __fmaf_rn(lb, c1, __fmul_rn(a.l, c0));
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    a.o0[r] = __fmaf_rn(b0[r], c1, __fmul_rn(a.o0[r], c0));
    a.o1[r] = __fmaf_rn(b1[r], c1, __fmul_rn(a.o1[r], c0));
  }
}

// Floats of LDS attn_finish uses at xch: with SPLIT = 2, per query tile 32 O values + m + l per lane; none with SPLIT = 1.
// The kernel asserts that the array it passes holds them.
template <int WAVES, int SPLIT>
constexpr int kAttnExchangeFloats = SPLIT == 2 ? (WAVES / SPLIT) * 34 * 64 : 0;

// The end of a kernel, after its last tile: stream 1 joins stream 0 (SPLIT = 2: through xch, which may be the K / V tiles' LDS
// -- the first barrier ends their use; the sp == 1 waves are done after it), the row is divided by its sum and written.
template <int WAVES, int SPLIT>
__device__ __forceinline__ void attn_finish(Stream (&st)[3 - SPLIT], const AttnBlock& c, float* xch, float* __restrict__ out) {
  if constexpr (SPLIT == 2) {
    __syncthreads();
    float* X = xch + c.qt * (34 * 64);
    if (c.sp == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { X[r * 64 + c.lane] = st[0].o0[r]; X[(16 + r) * 64 + c.lane] = st[0].o1[r]; }
      X[32 * 64 + c.lane] = st[0].m;
      X[33 * 64 + c.lane] = st[0].l;
    }
    __syncthreads();
    if (c.sp != 0) return;
    float b0[16], b1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { b0[r] = X[r * 64 + c.lane]; b1[r] = X[(16 + r) * 64 + c.lane]; }
    merge_streams(st[0], b0, b1, X[32 * 64 + c.lane], X[33 * 64 + c.lane]);
  } else {
    float b0[16], b1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { b0[r] = st[1].o0[r]; b1[r] = st[1].o1[r]; }
    merge_streams(st[0], b0, b1, st[1].m, st[1].l);
  }
  if (c.qi < c.n) {
    const float inv = 1.f / st[0].l;
    float* orow = out + (c.row0 + c.qi) * c.inner + c.h * 64;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // regs 4g..4g+3 -> d = 8 g + 4 lh + (0..3)
      f32x4 a = {st[0].o0[4 * g] * inv, st[0].o0[4 * g + 1] * inv, st[0].o0[4 * g + 2] * inv, st[0].o0[4 * g + 3] * inv};
      f32x4 e = {st[0].o1[4 * g] * inv, st[0].o1[4 * g + 1] * inv, st[0].o1[4 * g + 2] * inv, st[0].o1[4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(orow + 8 * g + 4 * c.lh) = a;
      *reinterpret_cast<f32x4*>(orow + 32 + 8 * g + 4 * c.lh) = e;
    }
  }
}

// The launch both forms share: the base-2 scale and the rule that picks the kernel shape (4 waves per block either way).  The banded
// kernels take one argument more, the radius (`band`): same grid, same threshold.
using AttnKernel = void (*)(const float* qkv, float* out, int n, int heads, float scale, const int* seg);

template <typename Kernel, typename... Band>
static inline void launch_attention(Kernel split1, Kernel split2, const float* qkv, float* out, const int* seg, int batch,
                                    int n, int heads, float scale, void* stream, Band... band) {
  scale *= 1.44269504088896340736f;        // the kernel's softmax runs in base 2: exp(x) = exp2(x log2(e))
  const bool large = (long long)fh_cdiv(n, 128) * heads * batch >= 512;
  const dim3 grid(fh_cdiv(n, large ? 128 : 64), heads, batch);      // queries per block: 32 WAVES / SPLIT
  const Kernel kernel = large ? split1 : split2;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, qkv, out, n, heads, scale, seg, band...);
}

// The banded entries' radius as the kernels take it: clamped to the (longest) clip's rows -- every key is within n - 1 of every
// query, so the band is the same, and query + radius stays far from INT_MAX.
static inline int attn_clamp_radius(int radius, int n) { return radius < n ? radius : n; }
