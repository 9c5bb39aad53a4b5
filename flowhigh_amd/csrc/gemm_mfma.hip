// fp32 GEMM on the gfx950 matrix cores:  C[M, N] = epilogue(A[M, K] * W[N, K]^T).
//
// Replaces the nn.Linear call sites of the FLowHigh transformer
// (/root/reference/src/flowhigh/models/flow.py:239,261; attend.py:170-171,176,189;
// transformer.py:98-104), and, used as DFT-by-GEMM, torch.stft / torch.istft
// (melvoco.py:78-79; postprocessing.py:22-23,39) and the mel projection (melvoco.py:83).
//
// v_mfma_f32_32x32x2_f32 (exact fp32 fma chain).  Block = 4 waves (2 x 2), BK = 32.
// Both operands are K-contiguous row tiles; rows are padded to 36 floats in LDS so that one
// ds_read_b128 per lane is conflict free (start bank 4 (9 i mod 16)) and feeds four k-steps; the K
// order inside a 32-wide tile is permuted identically for A and W (k-step (q, e) pairs columns
// 8q + e and 8q + 4 + e).  Global loads of tile i+1 are issued into registers before the MFMAs of
// tile i (register prefetch), LDS is single buffered, two barriers per tile.
//
// The frame around the products -- tile variants, block order, epilogues, argument checks and the launch -- is gemm_common.h's,
// shared with gemm_bf.hip.  W is padded to a multiple of 128 rows.
#include "gemm_common.h"

namespace {

constexpr int BK = 32;
constexpr int LP = BK + 4;   // LDS row pitch, floats

template <int MT, int NT>   // wave tile = (32 MT) x (32 NT), block tile = (64 MT) x (64 NT)
__global__ __launch_bounds__(256) void gemm_kernel(const float* __restrict__ A, int lda,
                                                   const float* __restrict__ W,
                                                   const float* __restrict__ bias,
                                                   const float* __restrict__ R, int ldr,
                                                   float* __restrict__ C, int ldc, int M, int N,
                                                   int K, float alpha, int mode, int m_tiles) {
  constexpr int BM = 64 * MT, BN = 64 * NT;
  constexpr int AREG = BM * 8 / 256;   // float4 per thread for the A tile
  constexpr int WREGS = BN * 8 / 256;  // float4 per thread for the W tile
  __shared__ __attribute__((aligned(16))) float As[BM * LP];
  __shared__ __attribute__((aligned(16))) float Ws[BN * LP];

  const GemmBlock g = gemm_block<MT, NT>(m_tiles);
  const int m0 = g.m0, n0 = g.n0;
  if (n0 >= N) return;
  const int tid = g.tid, wm = g.wm, wn = g.wn, l31 = g.l31, lh = g.lh;

  f32x16 acc[MT][NT];
  zero_acc(acc);

  f32x4 areg[AREG], wreg[WREGS];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AREG; ++i) {
      int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m0 + row < M) v = *reinterpret_cast<const f32x4*>(A + (size_t)(m0 + row) * lda + k0 + 4 * c4);
      areg[i] = v;
    }
#pragma unroll
    for (int i = 0; i < WREGS; ++i) {
      int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
      wreg[i] = *reinterpret_cast<const f32x4*>(W + (size_t)(n0 + row) * K + k0 + 4 * c4);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < AREG; ++i) {
      int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
      *reinterpret_cast<f32x4*>(As + row * LP + 4 * c4) = areg[i];
    }
#pragma unroll
    for (int i = 0; i < WREGS; ++i) {
      int f = tid + 256 * i, row = f >> 3, c4 = f & 7;
      *reinterpret_cast<f32x4*>(Ws + row * LP + 4 * c4) = wreg[i];
    }
  };

  gload(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();          // previous tile's fragment reads are done
    lstore();
    __syncthreads();
    if (k0 + BK < K) gload(k0 + BK);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 a[MT], bfr[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        a[mt] = *reinterpret_cast<const f32x4*>(As + ((wm * MT + mt) * 32 + l31) * LP + 4 * (2 * q + lh));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        bfr[nt] = *reinterpret_cast<const f32x4*>(Ws + ((wn * NT + nt) * 32 + l31) * LP + 4 * (2 * q + lh));
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][e], bfr[nt][e], acc[mt][nt], 0, 0, 0);
    }
  }

  gemm_epilogue(acc, g, bias, R, ldr, C, ldc, M, N, alpha, mode);
}

}  // namespace

extern "C" int fh_gemm_f32(const float* A, int lda, const float* W, const float* bias,
                           const float* R, int ldr, float* C, int ldc, int M, int N, int K,
                           float alpha, int epilogue, void* stream) {
  return launch_gemm<float>("fh_gemm_f32", BK, gemm_kernel<1, 1>, gemm_kernel<1, 2>, gemm_kernel<2, 2>, A, lda, W, bias, R, ldr, C,
                            ldc, M, N, K, alpha, epilogue, stream);
}
