// The kernel of attention.hip (the full entries) and attention_band.hip (the banded ones), described at the top of attention.hip.
// The two sets of entries are translation units of their own so that the full kernels compile to exactly what they compiled to before
// there was a band: instantiated beside the banded ones in one module, their SPLIT = 2 shapes came out in another instruction order.
#pragma once
#include <math.h>

#include "attention_softmax.h"
#include "fh_common.h"

namespace {

constexpr int KP = 68;   // K tile pitch (floats): b128 reads conflict free
constexpr int VP = 64;

// BAND (the banded entries): query i reads the keys j with |i - j| <= radius, the one argument the banded instantiations take
// beside the full ones' (Radius = int; the full instantiations have none and are what they were before there was a band): the
// staging loop walks only the 64-key iterations of the block's band (attention_softmax.h: AttnBand), softmax_step masks by key.
template <int WAVES, int SPLIT, bool BAND = false, typename... Radius>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void attention_kernel(const float* __restrict__ qkv,
                                                               float* __restrict__ out, int n_max, int heads,
                                                               float scale, const int* __restrict__ seg, Radius... radius) {
  static_assert(sizeof...(Radius) == (BAND ? 1 : 0), "the banded kernels take the radius, the full ones nothing");
  constexpr int NT = 64 * WAVES;           // threads
  constexpr int NLD = 1024 / NT;           // float4 of K (and of V) staged per thread and iteration (64 keys)
  constexpr int KT = 32 * KP, VT = 32 * VP;
  __shared__ __attribute__((aligned(16))) float Ks[2 * KT];
  __shared__ __attribute__((aligned(16))) float Vs[2 * VT];
  const AttnBlock blk = attn_prologue<WAVES, SPLIT>(qkv, n_max, heads, seg);
  if (!blk.live) return;
  const int tid = blk.tid, l31 = blk.l31, lh = blk.lh, sp = blk.sp;
  const int n = blk.n;                       // this clip's keys (n_max: the longest clip's)

  // Q fragments: qf[q'][e] = Q[qi][8 q' + 4 lh + e]
  f32x4 qf[8];
#pragma unroll
  for (int qq = 0; qq < 8; ++qq) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (blk.qi < n) v = *reinterpret_cast<const f32x4*>(blk.base + (size_t)blk.qi * blk.ld + 4 * (2 * qq + lh));
    qf[qq] = v;
  }

  constexpr int NS = 3 - SPLIT;            // streams this wave runs: 2 (SPLIT = 1) or 1 (SPLIT = 2)
  Stream st[NS];
  init_streams(st);
  const AttnBand<BAND> band(blk, 32 * WAVES / SPLIT, radius...);

  // one 32-key tile into one stream
  auto tile = [&](Stream& S, int k0, const float* Kt, const float* Vt) {
    // S^T tile
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) {
      f32x4 kf = *reinterpret_cast<const f32x4*>(Kt + l31 * KP + 4 * (2 * qq + lh));
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[qq][e], s, 0, 0, 0);
    }
    softmax_step(S, s, k0, n, lh, scale, band);
    // O^T += V^T P^T
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float v0 = Vt[key * VP + l31];
      const float v1 = Vt[key * VP + 32 + l31];
      S.o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, s[r], S.o0, 0, 0, 0);
      S.o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, s[r], S.o1, 0, 0, 0);
    }
  };

  // K / V tiles (2 x 512 float4 each) go global -> registers one iteration ahead, registers -> LDS at the top
  // of their own iteration: the loads of the next 64 keys are in flight while these are on the matrix cores
  f32x4 kreg[NLD], vreg[NLD];
  auto load_kv = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int f = tid + NT * i, key = f >> 4, c4 = f & 15;        // key < 64
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (k0 + key < n) {
        const float* rowp = blk.base + (size_t)(k0 + key) * blk.ld + 4 * c4;
        kv = *reinterpret_cast<const f32x4*>(rowp + blk.inner);
        vv = *reinterpret_cast<const f32x4*>(rowp + 2 * blk.inner);
      }
      kreg[i] = kv;
      vreg[i] = vv;
    }
  };
  load_kv(band.lo());
  for (int kb = band.lo(); kb < band.hi(n); kb += 64) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int f = tid + NT * i, key = f >> 4, c4 = f & 15;
      *reinterpret_cast<f32x4*>(Ks + key * KP + 4 * c4) = kreg[i];
      *reinterpret_cast<f32x4*>(Vs + key * VP + 4 * c4) = vreg[i];
    }
    __syncthreads();
    if (kb + 64 < band.hi(n)) load_kv(kb + 64);
    if constexpr (SPLIT == 2) {
      const int k0 = kb + 32 * sp;               // this wave's key tile of the iteration
      if (k0 < band.hi(n)) tile(st[0], k0, Ks + sp * KT, Vs + sp * VT);     // (wave-uniform; the barriers are outside)
    } else {
      tile(st[0], kb, Ks, Vs);
      if (kb + 32 < band.hi(n)) tile(st[1], kb + 32, Ks + KT, Vs + VT);
    }
  }

  static_assert(kAttnExchangeFloats<WAVES, SPLIT> <= 2 * KT, "exchange area: the K tiles");
  attn_finish<WAVES, SPLIT>(st, blk, Ks, out);
}

}  // namespace
