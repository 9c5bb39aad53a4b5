// The kernel of attention_bf.hip (the full entries) and attention_bf_band.hip (the banded ones), described at the top of attention_bf.hip.
// The two sets of entries are translation units of their own so that the full kernels compile to exactly what they compiled to before
// there was a band: instantiated beside the banded ones in one module, their SPLIT = 2 shapes came out in another instruction order.
#pragma once
#include <math.h>

#include "attention_softmax.h"
#include "bf16x6.h"
#include "fh_common.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int KPB = 34;                    // pitch (units) of a (piece, tile, d-octet) plane of K: a staging pass's 16 lanes are 2 keys x
                                           // 8 d-octets, 2 mod 16 puts them in 16 different bank groups
constexpr int K_UNITS = 3 * 2 * 8 * KPB;
constexpr int V_UNITS = 3 * 2 * 4 * 64;

__device__ __forceinline__ bf16x8 as_bf(const u32x4& v) { return __builtin_bit_cast(bf16x8, v); }

// BAND (the banded entries): query i reads the keys j with |i - j| <= radius, the one argument the banded instantiations take
// beside the full ones' (Radius = int; the full instantiations have none and are what they were before there was a band): the
// staging loop walks only the 64-key iterations of the block's band (attention_softmax.h: AttnBand), softmax_step masks by key.
template <int WAVES, int SPLIT, bool BAND = false, typename... Radius>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void attention_bf_kernel(const float* __restrict__ qkv,
                                                               float* __restrict__ out, int n_max, int heads,
                                                               float scale, const int* __restrict__ seg, Radius... radius) {
  static_assert(sizeof...(Radius) == (BAND ? 1 : 0), "the banded kernels take the radius, the full ones nothing");
  constexpr int NT = 64 * WAVES;           // threads
  constexpr int NKI = 512 / NT;            // (key, d-octet) items of K staged per thread and iteration (64 keys)
  constexpr int NVI = 1024 / NT;           // (4 keys, d) items of V
  static_assert(NVI % 2 == 0, "V items are split in pairs");
  __shared__ __attribute__((aligned(16))) u32x4 smem[K_UNITS + V_UNITS];
  u32x4* const Ks = smem;
  u32x4* const Vs = smem + K_UNITS;
  const AttnBlock blk = attn_prologue<WAVES, SPLIT>(qkv, n_max, heads, seg);
  if (!blk.live) return;
  const int tid = blk.tid, l31 = blk.l31, lh = blk.lh, sp = blk.sp;
  const int n = blk.n;                     // this clip's keys (n_max: the longest clip's)

  // Q pieces: element j of qp[piece][ks] = piece of Q[qi][16 ks + 8 lh + j]
  u32x4 qp[3][4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (blk.qi < n) {
      const float* p = blk.base + (size_t)blk.qi * blk.ld + 16 * ks + 8 * lh;
      v0 = *reinterpret_cast<const f32x4*>(p);
      v1 = *reinterpret_cast<const f32x4*>(p + 4);
    }
    const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    bf16x6_split(v, qp[0][ks], qp[1][ks], qp[2][ks]);
  }

  constexpr int NS = 3 - SPLIT;            // streams this wave runs: 2 (SPLIT = 1) or 1 (SPLIT = 2)
  Stream st[NS];
  init_streams(st);
  const AttnBand<BAND> band(blk, 32 * WAVES / SPLIT, radius...);

  // one 32-key tile (tile t of the staged 64 keys) into one stream
  auto tile = [&](Stream& S, int k0, int t) {
    // S^T tile
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 kf[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) kf[p] = as_bf(Ks[((p * 2 + t) * 8 + 2 * ks + lh) * KPB + l31]);
#pragma unroll
      for (int pp = 0; pp < 6; ++pp) {
        const Bf16x6Pair c = kBf16x6SmallFirst[pp];                  // (K piece, Q piece)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[c.a], as_bf(qp[c.b][ks]), s, 0, 0, 0);
      }
    }
    softmax_step(S, s, k0, n, lh, scale, band);
    // O^T += V^T P^T: registers 8 s2 .. 8 s2 + 7 are k-step s2 of the B operand
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const float pv[8] = {s[8 * s2], s[8 * s2 + 1], s[8 * s2 + 2], s[8 * s2 + 3], s[8 * s2 + 4], s[8 * s2 + 5], s[8 * s2 + 6], s[8 * s2 + 7]};
      u32x4 pq[3];
      bf16x6_split(pv, pq[0], pq[1], pq[2]);
      bf16x8 v0[3], v1[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const u32x4* plane = Vs + ((p * 2 + t) * 4 + 2 * s2 + lh) * 64;
        v0[p] = as_bf(plane[l31]);
        v1[p] = as_bf(plane[32 + l31]);
      }
#pragma unroll
      for (int pp = 0; pp < 6; ++pp) {
        const Bf16x6Pair c = kBf16x6SmallFirst[pp];                  // (V piece, P piece)
        S.o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0[c.a], as_bf(pq[c.b]), S.o0, 0, 0, 0);
        S.o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1[c.a], as_bf(pq[c.b]), S.o1, 0, 0, 0);
      }
    }
  };

  // K / V of the next 64 keys go global -> registers one iteration ahead, registers -> split -> LDS at the top of their own
  // iteration.  K item: key = item >> 3, d-octet = item & 7 (2 float4).  V item: d = item & 63, keys 4 (item >> 6) .. + 3 (4 floats;
  // a wave's 64 lanes read one row's 256 bytes per load).
  f32x4 kreg[NKI][2];
  float vreg[NVI][4];
  auto load_kv = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
      const int item = tid + NT * i, key = item >> 3, oct = item & 7;
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
      if (k0 + key < n) {
        const float* rowp = blk.base + (size_t)(k0 + key) * blk.ld + blk.inner + 8 * oct;
        a = *reinterpret_cast<const f32x4*>(rowp);
        c = *reinterpret_cast<const f32x4*>(rowp + 4);
      }
      kreg[i][0] = a;
      kreg[i][1] = c;
    }
#pragma unroll
    for (int i = 0; i < NVI; ++i) {
      const int item = tid + NT * i, d = item & 63, key = 4 * (item >> 6);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        vreg[i][e] = k0 + key + e < n ? blk.base[(size_t)(k0 + key + e) * blk.ld + 2 * blk.inner + d] : 0.f;
    }
  };
  auto store_kv = [&]() {
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
      const int item = tid + NT * i, key = item >> 3, oct = item & 7;
      const f32x4 &a = kreg[i][0], &c = kreg[i][1];
      const float v[8] = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
      u32x4 pc[3];
      bf16x6_split(v, pc[0], pc[1], pc[2]);
#pragma unroll
      for (int p = 0; p < 3; ++p) Ks[((p * 2 + (key >> 5)) * 8 + oct) * KPB + (key & 31)] = pc[p];
    }
#pragma unroll
    for (int i = 0; i < NVI; i += 2) {
      const float v[8] = {vreg[i][0], vreg[i][1], vreg[i][2], vreg[i][3], vreg[i + 1][0], vreg[i + 1][1], vreg[i + 1][2], vreg[i + 1][3]};
      u32x4 pc[3];
      bf16x6_split(v, pc[0], pc[1], pc[2]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // key-quad kq of the 64 keys -> tile kq >> 3, k-step (kq >> 2) & 1, 8-byte half (kq >> 1) & 1, lane half kq & 1
        const int item = tid + NT * (i + j), d = item & 63, kq = item >> 6;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          u32x2* unit = reinterpret_cast<u32x2*>(Vs + ((p * 2 + (kq >> 3)) * 4 + 2 * ((kq >> 2) & 1) + (kq & 1)) * 64 + d);
          unit[(kq >> 1) & 1] = (u32x2){pc[p][2 * j], pc[p][2 * j + 1]};
        }
      }
    }
  };
  load_kv(band.lo());
  for (int kb = band.lo(); kb < band.hi(n); kb += 64) {
    __syncthreads();
    store_kv();
    __syncthreads();
    if (kb + 64 < band.hi(n)) load_kv(kb + 64);
    if constexpr (SPLIT == 2) {
      const int k0 = kb + 32 * sp;               // this wave's key tile of the iteration
      if (k0 < band.hi(n)) tile(st[0], k0, sp);       // (wave-uniform; the barriers are outside)
    } else {
      tile(st[0], kb, 0);
      if (kb + 32 < band.hi(n)) tile(st[1], kb + 32, 1);
    }
  }

  static_assert(kAttnExchangeFloats<WAVES, SPLIT> <= 4 * (K_UNITS + V_UNITS), "exchange area: all of smem");
  attn_finish<WAVES, SPLIT>(st, blk, reinterpret_cast<float*>(smem), out);
}

}  // namespace
