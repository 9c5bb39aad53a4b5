// What the two grouped implicit-GEMM conv kernels share (conv_mfma.hip: fp32 MFMA; conv_mfma_bf.hip: the bf16 x 6 form): the
// tile table behind tile_cfg, the block -> (group, batch item, co tile, n tile) mapping; the epilogue is conv_mfma_epilogue.h.  Both kernels use
// 4-wave blocks of WM x WN waves, each wave MT x NT accumulator tiles of 32 x 32 (v_mfma_*_32x32x*: D reg r of lane l =
// D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31]), so everything behind the K loop is the same code.
#pragma once
#include "fh_common.h"

namespace {

constexpr int NT_RUN = 8;       // n-tiles of a panel that run together on one XCD

struct TileInfo { int bm, bn; };
constexpr TileInfo kTiles[] = {{128, 128}, {192, 128}, {96, 256}, {64, 256}, {32, 512}, {128, 64}, {96, 128}};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);

// the launch's grid for a tile of BM x BN (0: too large); co_tiles / n_tiles are the kernel's arguments
static inline long long conv_grid_blocks(int n_groups, int batch, int cout_pad, int n_len, int bm, int bn, int* co_tiles, int* n_tiles) {
  *co_tiles = cout_pad / bm;
  *n_tiles = fh_cdiv(n_len, bn);
  const long long panels = (long long)n_groups * batch * *co_tiles;
  const long long runs = panels * fh_cdiv(*n_tiles, NT_RUN);
  return (long long)fh_cdiv(runs, 8) * 8 * NT_RUN;
}

// ---- block -> (panel, n tile); panels = (group, batch, co tile), heavy groups first ----
// Block -> work mapping is XCD aware: blocks with equal (id mod 8) share an L2; the n-tiles of one (group, batch, co-tile) panel
// are dealt to one XCD in runs of 8, so the weight tiles they share are fetched into that L2 once.  The statement sequence of a
// kernel's first lines (a macro: its early returns are the kernel's): defines cot, b, ntile and G; a block without work returns.
#define FH_CONV_BLOCK_MAP(groups, n_groups, batch, co_tiles, n_tiles)                              \
  const int panels = n_groups * batch * co_tiles;                                                  \
  const int runs_per_panel = (n_tiles + NT_RUN - 1) / NT_RUN;                                      \
  const int total_runs = panels * runs_per_panel;                                                  \
  const int bid = blockIdx.x;                                                                      \
  const int slot = bid >> 3;                                                                       \
  const int run = (slot / NT_RUN) * 8 + (bid & 7);                                                 \
  if (run >= total_runs) return;                                                                   \
  /* (runtime integer divisions are done on the VALU: pin the results back to SGPRs) */            \
  const int panel = uni(run / runs_per_panel);                                                     \
  const int ntile = uni((run % runs_per_panel) * NT_RUN + (slot % NT_RUN));                        \
  if (ntile >= n_tiles) return;                                                                    \
  const int cot = uni(panel % co_tiles);                                                           \
  const int gb = uni(panel / co_tiles);                                                            \
  const int b = uni(gb % batch);                                                                   \
  const fh_conv_group* __restrict__ G = groups + uni(gb / batch)

}  // namespace
