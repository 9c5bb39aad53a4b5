// The frame of the two GEMM kernels, gemm_mfma.hip (fp32 MFMA products) and gemm_bf.hip (bf16 x 6 products): everything
// beside the staging of A / W and the products.  Both kernels place a block, hold their accumulators, write C = epilogue(acc)
// and are launched -- argument checks, tile variant, grid -- by this one copy.  A kernel reads: gemm_block, zero_acc, its
// staging loop with the products, gemm_epilogue.
//
// Block = 4 waves (2 x 2); a wave's tile is (32 MT) x (32 NT), the block's (64 MT) x (64 NT).  Tile variants: 128 x 128
// (MT, NT = 2, 2), 64 x 128 (1, 2) and 64 x 64 (1, 1) -- the smaller ones keep more CUs busy at M = N_frames ~ 1000.
#pragma once
#include "fh_common.h"

// Where a thread stands: the block's tile starts at (m0, n0), the wave's is tile (wm, wn) of its 2 x 2, the lane is column
// l31 of a 32 x 32 MFMA tile, lane half lh.
struct GemmBlock {
  int m0, n0;
  int tid, wm, wn, l31, lh;
};

template <int MT, int NT>
__device__ __forceinline__ GemmBlock gemm_block(int m_tiles) {
  GemmBlock g;
  // XCD-aware order: the m-tiles of one n-tile (sharing the W panel) go to one XCD
  const int bid = blockIdx.x;
  const int per_xcd = gridDim.x >> 3;              // grid is a multiple of 8
  const int work = (bid & 7) * per_xcd + (bid >> 3);
  g.n0 = (work / m_tiles) * (64 * NT);             // (>= N in the blocks that round the grid up: the kernel returns)
  g.m0 = (work % m_tiles) * (64 * MT);
  g.tid = threadIdx.x;
  const int lane = g.tid & 63, wave = g.tid >> 6;
  g.wm = wave >> 1;
  g.wn = wave & 1;
  g.l31 = lane & 31;
  g.lh = lane >> 5;
  return g;
}

template <int MT, int NT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MT][NT]) {
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

__device__ __forceinline__ float epi_pair(float first, float second, int mode) {
  if (mode == FH_EPI_GEGLU) return gelu_erf(second) * first;
  return sqrtf(first * first + second * second + 1e-9f);
}

// s_waitcnt vmcnt(0) (gfx9 encoding; the other counters at their maxima).  The epilogue waits for its bias values once, before
// the rows: left to the compiler, the wait can land in every row's bounds-guarded block, where it also waits for the previous
// row's store -- 32 serialised stores per lane, 2-4 % of a K = 1024 launch.
__device__ __forceinline__ void wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0f70); }

// D reg r of lane l: row = (r&3) + 8 (r>>2) + 4 lh, col = l31.
// The MFMA computed D[i][j] = sum_k A[i][k] W[j][k] with i = A row (m), j = W row (n).
template <int MT, int NT>
__device__ __forceinline__ void gemm_epilogue(const f32x16 (&acc)[MT][NT], const GemmBlock& g, const float* __restrict__ bias,
                                              const float* __restrict__ R, int ldr, float* __restrict__ C, int ldc, int M, int N,
                                              float alpha, int mode) {
  const int m0 = g.m0, n0 = g.n0, wm = g.wm, wn = g.wn, l31 = g.l31, lh = g.lh;
  if (mode == FH_EPI_LINEAR || mode == FH_EPI_LOGCLAMP) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + (wn * NT + nt) * 32 + l31;
        if (n >= N) continue;
        const float bv = bias ? bias[n] : 0.f;
        wait_vmem();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + (wm * MT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m >= M) continue;
          float v = acc[mt][nt][r] + bv;
          if (mode == FH_EPI_LOGCLAMP) {
            v = logf(fmaxf(v, 1e-5f));
          } else {
            v *= alpha;
            if (R) v += R[(size_t)m * ldr + n];
          }
          C[(size_t)m * ldc + n] = v;
        }
      }
  } else {
    // pair modes: the wave's two 32-column tiles are (first, second) of one packed 64 block
    const int blk = (n0 >> 6) + wn;                 // packed block index
    const int n_out = blk * 32 + l31;
    const int n_first = n0 + wn * 64 + l31;         // packed column of `first`
    if (NT == 2 && n_first < N) {
      const float b1 = bias ? bias[n_first] : 0.f;
      const float b2 = bias ? bias[n_first + 32] : 0.f;
      wait_vmem();
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + (wm * MT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m >= M) continue;
          C[(size_t)m * ldc + n_out] = epi_pair(acc[mt][0][r] + b1, acc[mt][NT - 1][r] + b2, mode);
        }
    }
  }
}

// The launch both forms share (entry: the C entry's name for its messages; bk: the kernel's K stage; WT: the element type the
// kernel reads W as).  W is padded to a multiple of 128 rows.
template <typename WT>
using GemmKernel = void (*)(const float* A, int lda, const WT* W, const float* bias, const float* R, int ldr, float* C, int ldc,
                            int M, int N, int K, float alpha, int mode, int m_tiles);

template <typename WT>
static int launch_gemm(const char* entry, int bk, GemmKernel<WT> k64x64, GemmKernel<WT> k64x128, GemmKernel<WT> k128x128,
                       const float* A, int lda, const float* W, const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N, int K,
                float alpha, int epilogue, void* stream) {
  FH_CHECK_ARG(A && W && C && M > 0 && N > 0 && K > 0, "%s: bad args", entry);
  FH_CHECK_ARG(K % bk == 0, "%s: K=%d must be a multiple of %d", entry, K, bk);
  FH_CHECK_ARG(lda % 4 == 0 && (((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0,
               "%s: A/W must be 16-byte aligned with lda %% 4 == 0", entry);
  FH_CHECK_ARG(epilogue >= 0 && epilogue <= 3, "%s: unknown epilogue %d", entry, epilogue);
  if (epilogue == FH_EPI_GEGLU || epilogue == FH_EPI_MAG)
    FH_CHECK_ARG(N % 64 == 0, "%s: pair epilogue needs N %% 64 == 0", entry);
  const bool plain = epilogue == FH_EPI_LINEAR || epilogue == FH_EPI_LOGCLAMP;
  const long long t128 = (long long)fh_cdiv(M, 128) * fh_cdiv(N, 128);
  const long long t64x128 = (long long)fh_cdiv(M, 64) * fh_cdiv(N, 128);
  GemmKernel<WT> kernel = k128x128;
  int bm = 128, bn = 128;
  if (plain && t64x128 < 200) {
    // few tiles (M = frames ~ 1000, N = 1024): 64 x 64 tiles put a block on every CU (the pair epilogues need NT = 2)
    kernel = k64x64;
    bm = 64, bn = 64;
  } else if (t128 < 512) {
    kernel = k64x128;
    bm = 64;
  }
  const int m_tiles = fh_cdiv(M, bm);
  const int blocks = fh_cdiv((long long)m_tiles * fh_cdiv(N, bn), 8) * 8;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A, lda, reinterpret_cast<const WT*>(W), bias, R,
                     ldr, C, ldc, M, N, K, alpha, epilogue, m_tiles);
  FH_CHECK_LAUNCH(entry);
  return FH_OK;
}
