// GEMM in the bf16 x 6 form:  C[M, N] = epilogue(A[M, K] * W[N, K]^T) with fp32 in / out / accumulate and every product as six
// v_mfma_f32_32x32x16_bf16 over exact three-piece splits (bf16x6.h, small terms first): the transformer's linears of a
// conv_form = 'bf16x6' model.
//
// Replaces the same nn.Linear call sites as gemm_mfma.hip (/root/reference/src/flowhigh/models/flow.py:239,261; attend.py:170-171,
// 176,189; transformer.py:98-104) and shares its frame, gemm_common.h: the epilogues (bias, alpha, residual; GEGLU pairs), the
// tile variants, the block order, the argument checks and the launch.
//
// The recipe of narrow_bf.hip: an operand is split ONCE, on its way into LDS (A: by the block that stages the tile, 11 vector
// instructions per pair of values; W: on the host, packing.pack_gemm_bf_weight), and the K loop is ds_read_b128 + MFMA with no
// vector arithmetic.  LDS tile of an operand: 16-byte units (8 consecutive k as bf16) [piece][k-octet 0..3][row]: the fragment of a
// 32-row tile, one k-step (16) and one piece is 2 x 32 consecutive units -- conflict-free ds_read_b128.  BK = 32 = two k-steps;
// global loads of stage i + 1 are in registers before the MFMAs of stage i; LDS single-buffered, two barriers per stage.
// W in memory: [64-row granule][k stage][piece][k-octet][64 rows][8 bf16] (12 KB per granule and stage: a stage's W tile is a
// straight copy of 1-2 granules).
#include "bf16x6.h"
#include "gemm_common.h"

namespace {

constexpr int GB_BK = 32;
constexpr int GB_GRAN = 3 * 4 * 64;        // 16-byte units of one (64-row granule, k stage) of packed W

template <int MT, int NT>   // wave tile = (32 MT) x (32 NT), block tile = (64 MT) x (64 NT)
__global__ __launch_bounds__(256) void gemm_bf_kernel(const float* __restrict__ A, int lda, const u32x4* __restrict__ Wp,
                                                      const float* __restrict__ bias, const float* __restrict__ R, int ldr,
                                                      float* __restrict__ C, int ldc, int M, int N, int K, float alpha, int mode,
                                                      int m_tiles) {
  constexpr int BM = 64 * MT, BN = 64 * NT;
  constexpr int AIT = MT;          // (row, k-octet) items of the A tile per thread: BM x 4 / 256
  constexpr int WIT = 3 * NT;      // 16-byte units of the W tile per thread: NT granules x 768 / 256
  constexpr int AP = BM + 4;       // pitch of a (piece, k-octet) plane of the A tile: a staging pass's 16 lanes are 4 rows x 4 k-octets,
                                   // 4 mod 16 puts them in 16 different bank groups (pitch BM: 4 to a group)
  __shared__ __attribute__((aligned(16))) u32x4 As[3 * 4 * AP];
  __shared__ __attribute__((aligned(16))) u32x4 Ws[3 * 4 * BN];

  const GemmBlock g = gemm_block<MT, NT>(m_tiles);
  const int m0 = g.m0, n0 = g.n0;
  if (n0 >= N) return;
  const int tid = g.tid, wm = g.wm, wn = g.wn, l31 = g.l31, lh = g.lh;
  const int kstages = K / GB_BK;

  f32x16 acc[MT][NT];
  zero_acc(acc);

  f32x4 areg[AIT][2];
  u32x4 wreg[WIT];
  auto gload = [&](int ks) {
#pragma unroll
    for (int i = 0; i < AIT; ++i) {
      const int item = tid + 256 * i, row = item >> 2, ko = item & 3;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (m0 + row < M) {
        const float* p = A + (size_t)(m0 + row) * lda + ks * GB_BK + 8 * ko;
        v0 = *reinterpret_cast<const f32x4*>(p);
        v1 = *reinterpret_cast<const f32x4*>(p + 4);
      }
      areg[i][0] = v0;
      areg[i][1] = v1;
    }
#pragma unroll
    for (int i = 0; i < WIT; ++i) {
      const int u = tid + 256 * i, g = u / GB_GRAN, r = u - g * GB_GRAN;
      wreg[i] = Wp[((size_t)((n0 >> 6) + g) * kstages + ks) * GB_GRAN + r];
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < AIT; ++i) {
      const int item = tid + 256 * i, row = item >> 2, ko = item & 3;
      const f32x4 &v0 = areg[i][0], &v1 = areg[i][1];
      const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      u32x4 h, m, l;
      bf16x6_split(v, h, m, l);
      As[(0 * 4 + ko) * AP + row] = h;
      As[(1 * 4 + ko) * AP + row] = m;
      As[(2 * 4 + ko) * AP + row] = l;
    }
#pragma unroll
    for (int i = 0; i < WIT; ++i) {
      const int u = tid + 256 * i, g = u / GB_GRAN, r = u - g * GB_GRAN;
      Ws[(r >> 6) * BN + g * 64 + (r & 63)] = wreg[i];          // r >> 6 = piece * 4 + k-octet
    }
  };

  gload(0);
  for (int ks = 0; ks < kstages; ++ks) {
    __syncthreads();          // previous stage's fragment reads are done
    lstore();
    __syncthreads();
    if (ks + 1 < kstages) gload(ks + 1);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bf16x8 a[MT][3], b[NT][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt][p] = __builtin_bit_cast(bf16x8, As[(p * 4 + 2 * q + lh) * AP + (wm * MT + mt) * 32 + l31]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt][p] = __builtin_bit_cast(bf16x8, Ws[(p * 4 + 2 * q + lh) * BN + (wn * NT + nt) * 32 + l31]);
      }
#pragma unroll
      for (int pp = 0; pp < 6; ++pp) {
        const Bf16x6Pair s = kBf16x6SmallFirst[pp];                  // (A piece, W piece)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt][s.a], b[nt][s.b], acc[mt][nt], 0, 0, 0);
      }
    }
  }

  gemm_epilogue(acc, g, bias, R, ldr, C, ldc, M, N, alpha, mode);
}

}  // namespace

extern "C" int fh_gemm_bf16x6_f32(const float* A, int lda, const float* Wp, const float* bias, const float* R, int ldr, float* C,
                                  int ldc, int M, int N, int K, float alpha, int epilogue, void* stream) {
  return launch_gemm<u32x4>("fh_gemm_bf16x6_f32", GB_BK, gemm_bf_kernel<1, 1>, gemm_bf_kernel<1, 2>, gemm_bf_kernel<2, 2>, A, lda, Wp,
                            bias, R, ldr, C, ldc, M, N, K, alpha, epilogue, stream);
}
