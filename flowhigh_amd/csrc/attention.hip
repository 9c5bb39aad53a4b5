// Streaming-softmax attention in fp32 on the gfx950 matrix cores (dim_head = 64).
//
// Replaces Attend.forward, /root/reference/src/flowhigh/models/attend.py:102-139
//   sim = einsum(q, k) * scale ; attn = softmax(sim) ; out = einsum(attn, v)
// which materialises [B, 16, n, n] three times (64 MB per clip at n = 1000); here the scores
// live only in MFMA accumulators.
//
// Per wave: 32 queries; per block (4 waves): 128 queries of one (batch, head); key/value tiles of
// 32 keys are staged in LDS and shared by the 4 waves.
//   S^T = K Q^T  (M = key, N = query, K = d):  A = K tile from LDS (ds_read_b128, 4 k-steps each),
//                 B = Q fragments held in 32 VGPRs for the whole kernel.
//   The accumulator then holds, for the lane's query (col = lane & 31), 16 keys per lane half:
//   the row softmax is 16 in-register ops + one exchange with lane ^ 32, and the probabilities are
//   already the B operand of the next product (no LDS round trip, no conversion):
//   O^T = V^T P^T (M = d, N = query, K = key): k-step r pairs keys (r&3)+8(r>>2) and that + 4,
//                 A = V^T read from the LDS V tile with the same key order.
// The frame around the products -- block placement, the two online-softmax streams per query row, their merge, the output and the
// launch rule -- is attention_softmax.h's, shared with attention_bf.hip.
#include <math.h>

#include "attention_softmax.h"
#include "fh_common.h"

namespace {

constexpr int KP = 68;   // K tile pitch (floats): b128 reads conflict free
constexpr int VP = 64;

template <int WAVES, int SPLIT>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void attention_kernel(const float* __restrict__ qkv,
                                                               float* __restrict__ out, int n_max, int heads,
                                                               float scale, const int* __restrict__ seg) {
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
    softmax_step(S, s, k0, n, lh, scale);
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
  load_kv(0);
  for (int kb = 0; kb < n; kb += 64) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int f = tid + NT * i, key = f >> 4, c4 = f & 15;
      *reinterpret_cast<f32x4*>(Ks + key * KP + 4 * c4) = kreg[i];
      *reinterpret_cast<f32x4*>(Vs + key * VP + 4 * c4) = vreg[i];
    }
    __syncthreads();
    if (kb + 64 < n) load_kv(kb + 64);
    if constexpr (SPLIT == 2) {
      const int k0 = kb + 32 * sp;               // this wave's key tile of the iteration
      if (k0 < n) tile(st[0], k0, Ks + sp * KT, Vs + sp * VT);     // (wave-uniform; the barriers are outside)
    } else {
      tile(st[0], kb, Ks, Vs);
      if (kb + 32 < n) tile(st[1], kb + 32, Ks + KT, Vs + VT);
    }
  }

  static_assert(kAttnExchangeFloats<WAVES, SPLIT> <= 2 * KT, "exchange area: the K tiles");
  attn_finish<WAVES, SPLIT>(st, blk, Ks, out);
}

}  // namespace

extern "C" int fh_attention_f32(const float* qkv, float* out, int batch, int n, int heads,
                                float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && batch > 0 && n > 0 && heads > 0, "fh_attention_f32: bad args");
  launch_attention(attention_kernel<4, 1>, attention_kernel<4, 2>, qkv, out, nullptr, batch, n, heads, scale, stream);
  FH_CHECK_LAUNCH("fh_attention_f32");
  return FH_OK;
}

extern "C" int fh_attention_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads,
                                    float scale, void* stream) {
  FH_CHECK_ARG(qkv && out && seg && n_seg > 0 && max_n > 0 && heads > 0, "fh_attention_seg_f32: bad args");
  launch_attention(attention_kernel<4, 1>, attention_kernel<4, 2>, qkv, out, seg, n_seg, max_n, heads, scale, stream);
  FH_CHECK_LAUNCH("fh_attention_seg_f32");
  return FH_OK;
}
