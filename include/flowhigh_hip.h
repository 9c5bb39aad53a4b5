/* flowhigh_hip.h -- C ABI of libflowhigh_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the FlowHighSR.generate() hot path of resemble-ai/flowhigh.
 * The reference has no FFI layer: its path is stock PyTorch aten ops called from
 * Python.  Each entry point below names the reference call
 * site (file:line under /root/reference/src/flowhigh/) whose arithmetic it replaces.
 * The Python host class `flowhigh_amd.FlowHighSR` binds these through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch-allocated); the
 *     library never allocates, frees, or synchronises; every call only enqueues work
 *     on `stream` (a hipStream_t passed as void*), so calls are graph-capturable;
 *   - all tensors are float32, dense, layouts stated per function;
 *   - return value: 0 = ok, negative = FH_E_* ; fh_last_error() gives the message
 *     (thread-local, valid until the next failing call on the same thread).
 */
#ifndef FLOWHIGH_HIP_H
#define FLOWHIGH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FH_OK 0
#define FH_E_ARG (-1)     /* bad argument / unsupported shape */
#define FH_E_LAUNCH (-2)  /* HIP launch error */

#define FH_ABI_VERSION 6

int fh_abi_version(void);
const char* fh_last_error(void);

/* ------------------------------------------------------------------------------------
 * Grouped implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces: Conv1d / ConvTranspose1d call sites of BigVGAN,
 *   models/bigvgan/models.py:172-194 (conv_pre, ups[i], and the convs1/convs2 of
 *   AMPBlock1 :63-72), including "+ x" (:70) and the "xs / num_kernels" average (:187).
 *
 * One launch runs `n_groups` independent groups (e.g. the three AMP blocks of a stage,
 * or the `u` output phases of a transposed conv).  A group sums `nseg` K-segments, each
 * a (input tensor, packed weight slab, tap list) triple, into one accumulator tile:
 *     out[b, co, n*out_stride + out_phase] =
 *         scale * ( bias[co] + sum_r res[r][b, co, .] +
 *                   sum_seg sum_tap sum_ci  w_seg[tap, ci, co] * x_seg[b, ci, n + tap_off[tap]] )
 * with x read as 0 outside [0, lin).
 *
 * Packed weights: float [cin/ck][ntaps][cout_pad][ck], ck = channel chunk (16, or 8 when some
 * cin % 16 != 0), cout_pad = cout rounded up to the tile height of `tile_cfg` (fh_conv_tile_m),
 * zero padded.  cin % ck == 0 for every segment.
 * --------------------------------------------------------------------------------- */
#define FH_CONV_MAX_TAPS 16
#define FH_CONV_MAX_SEG 3
#define FH_CONV_MAX_HALO 64

typedef struct {
  const float* x;      /* [B, cin, lin] */
  const float* w;      /* packed, see above */
  int32_t cin;
  int32_t ntaps;
  int32_t off_min;     /* min(tap_off) */
  int32_t off_max;     /* max(tap_off); off_max - off_min <= FH_CONV_MAX_HALO */
  int32_t tap_off[FH_CONV_MAX_TAPS];
} fh_conv_seg;

typedef struct {
  fh_conv_seg seg[FH_CONV_MAX_SEG];
  const float* bias;                 /* [cout] or NULL */
  const float* res[FH_CONV_MAX_SEG]; /* each [B, cout, lout] or NULL */
  float* out;                        /* [B, cout, lout] */
  int32_t nseg;
  int32_t nres;
  int32_t cout;
  int32_t cout_pad;
  int32_t lin;
  int32_t lout;
  int32_t n_len;        /* number of n positions (= lout for a plain conv, lin for a transposed-conv phase) */
  int32_t out_stride;
  int32_t out_phase;
  float scale;
} fh_conv_group;

int fh_sizeof_conv_group(void);
/* tile_cfg: 0 = 128x128, 1 = 192x128, 2 = 96x256, 3 = 64x256, 4 = 32x512, 5 = 128x64, 6 = 96x128 (co x n) */
int fh_conv_tile_m(int tile_cfg);
int fh_conv_tile_n(int tile_cfg);
/* groups: device array of n_groups descriptors; all groups share cout_pad and n_len. */
int fh_conv_grouped_f32(const fh_conv_group* groups, int n_groups, int batch, int cout_pad,
                        int n_len, int tile_cfg, int ck, void* stream);

/* ConvTranspose1d(k, stride u, padding (k - u) / 2) with u = `phases` in {2, 3} and k - u even (models/bigvgan/models.py:141-146,179)
 * with ALL output phases of a (co tile, time tile) computed by one block: every group has nseg == phases segments -- segment p =
 * output phase p: the same x, that phase's taps and packed weights (as the per-phase groups of fh_conv_grouped_f32 would have
 * them), an EVEN number of (16-channel chunk, tap) steps -- out_stride == phases, out_phase == 0, n_len input positions, no
 * residuals.  out[b, co, phases * n + p] = scale * (bias[co] + phase p's sum).  Same bits as `phases` groups with strided stores;
 * the block writes phases consecutive floats per position (whole lines).  tile_cfg 3, 4 or 6; channel chunk 16. */
int fh_conv_transpose_fused_f32(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len,
                                int tile_cfg, int phases, void* stream);

/* fh_conv_grouped_f32 in the bf16 x 6 form (conv_mfma_bf.hip; conv_form = 'direct_bf16x6'): the same call sites
 * (models/bigvgan/models.py:63-72 AMPBlock1 convs, :141-146 ConvTranspose1d as phase groups, :172-194 conv_pre / forward), the same
 * descriptors (1 .. 3 K segments, tap lists, bias, residuals, scale, out_stride / out_phase, groups of different n_len), the same
 * tile_cfg ids and cout_pad, the same block -> work mapping.  Every product w x is the six piece-pair v_mfma_f32_32x32x16_bf16
 * of exact three-piece splits (h h, h m, m h, h l, l h, m m; small terms first) into one fp32 accumulator: fp32-grade sums at
 * 6 / 16 of the fp32 instruction's matrix-pipe time.  Steps run in (segment, 16-channel chunk, tap) order, so the bits of an
 * output depend on its (group, channel, position) only, not on tile_cfg, the batch size or the launch it is part of.
 * Differences: every segment has cin % 16 == 0 (no ck argument), and seg.w points at three-piece weights, bf16 bit patterns
 * [cin/16][ntaps][cout_pad][piece h, m, l][16] (packing.pack_conv_bf_weight: the fp32 layout with ck = 16, each row of 16
 * channels split; 6 bytes per weight); x is split on the device.  A descriptor array in pinned host memory is checked by the
 * launcher (segments, taps, cin % 16); one in device memory is the caller's to get right, as for fh_conv_grouped_f32. */
int fh_conv_grouped_bf16x6_f32(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len, int tile_cfg,
                               void* stream);

/* fh_conv_grouped_bf16x6_f32 in the bf16 x 3 form (conv_form = 'direct_bf16x3'; the same kernel body with two pieces per operand):
 * the same call sites, descriptors, tile_cfg ids, cout_pad, block mapping, step order and argument checks.  Every operand keeps
 * the first two pieces of the exact split, h = bf16(x) and m = bf16(x - h), and a product w x is the three piece-pair MFMAs
 * (m h), (h m), (h h) -- small terms first -- into one fp32 accumulator: half the MFMAs and two thirds of the slab, LDS reads and
 * weight bytes of the six-pair form.  The dropped terms (w_m x_m and both remainders) are <= 3 2^-16 |w x| per product (bf16x6.h):
 * NOT fp32-grade, ~2-3e-5 on the waveform (profiles/direct_bf16x3.md).  seg.w points at two-piece weights, bf16 bit patterns
 * [cin/16][ntaps][cout_pad][piece h, m][16] (packing.pack_conv_bf3_weight: the first two pieces of pack_conv_bf_weight's rows;
 * 64-byte rows, 4 bytes per weight); x is split on the device. */
int fh_conv_grouped_bf16x3_f32(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len, int tile_cfg,
                               void* stream);

/* ------------------------------------------------------------------------------------
 * The same Conv1d call sites (models/bigvgan/models.py:63-72, "same"-padded, stride 1, square
 * cin x cout residual-stack convs) evaluated with the Winograd minimal-filtering identity
 * F(4,3): the k taps are walked in groups of 3 and every group of 4 outputs costs 6 instead of
 * 12 multiply-adds per (cin, cout) pair.  Exact in exact arithmetic; in fp32 the end-to-end
 * difference to the direct form is ~1e-6 (tests/tools/winograd_numerics.py).
 *   out[b, co, n] = scale * (bias[co] + sum_res res[b, co, n]
 *                            + sum_seg sum_ci sum_{j<k} w[co, ci, j] * x[b, ci, n + (j - center) * dilation])
 * u = host-transformed weights (flowhigh_amd/vocoder.py: pack_wino_weight):
 *   [cin/16][ngrp][6][cout_pad][16], u[., g, xi, co, .] = sum_j G[xi][j] * w[co, ., 3g + j]
 *   (taps past k are zero), cout_pad % (64 or 96, see tile_cfg) == 0, cin % 16 == 0.
 * cin need not equal cout.  With out_stride = u > 1 a group is one output phase of ConvTranspose1d(k, stride u,
 * padding (k - u) / 2) (models/bigvgan/models.py:131-140,179): its taps j = r + p (mod u), ordered by input offset,
 * form a stride-1 correlation with `center` = minus the smallest offset (flowhigh_amd/vocoder.py:
 * transposed_conv_phases), and its outputs interleave with the other phases'.
 */
typedef struct {
  const float* x;      /* [B, cin, len] */
  const float* u;
  int32_t cin;
  int32_t ngrp;        /* ceil(k / 3) */
  int32_t center;      /* (k - 1) / 2 */
  int32_t xlen;        /* 0: x rows are `len` samples long (the group's len).  > 0: x is [B, cin, xlen] and reads past
                          xlen are zero -- a transposed-conv phase whose rows are shorter than its output count, below
                          (plain layout, dilation 1; rows not 16-byte aligned need FH_WINO_NOVL) */
} fh_wino_seg;

typedef struct {
  fh_wino_seg seg[FH_CONV_MAX_SEG];
  const float* bias;                 /* [cout] or NULL */
  const float* res[FH_CONV_MAX_SEG]; /* each [B, cout, len] or NULL */
  float* out;                        /* [B, cout, len] */
  int32_t nseg;
  int32_t nres;
  int32_t cout;
  int32_t cout_pad;
  int32_t len;
  float scale;
  int32_t out_stride;   /* 0 or 1: out[b, co, n]; u > 1: one output phase of a transposed conv (models.py:179),   */
  int32_t out_phase;    /*   out [B, cout, u * len] written at u * n + out_phase (dilation 1, plain layout, no res)  */
  int32_t out_len;      /* 0, or the row length of out when it is not out_stride * len: ConvTranspose1d(k, u, padding
                           (k - u) / 2) with k - u ODD returns u * L + 1 samples (models.py:141-146): its phase groups have
                           len = L + 1 output positions, seg.xlen = L, out_len = u * L + 1; positions u * n + out_phase >=
                           out_len are not written */
  int32_t pad_;
} fh_wino_group;

int fh_sizeof_wino_group(void);
/* tile_cfg: 0 = 64 co x 512 outputs per block, 1 = 96 co x 256 outputs (cout_pad % fh_wino_tile_m == 0);
 * 4 = 64 co x 256 outputs (short rows: less padding of the last block of a dilation phase);
 * 5 = 32 co x 256 outputs (short clips: more, shorter blocks); 6 = 128 co x 256 outputs.  Every shape gives the
 * same bits (same accumulation order); which one is fastest depends on the block count (vocoder.choose_wino_cfg). */
int fh_wino_tile_m(int tile_cfg);
/* Phase-major layout of a [B, C, len] tensor for dilation d: every (batch, channel) row holds its d decimated
 * phases one after the other, x[b, c, p + d u] at row + p * fh_phase_len(len, d) + u, row pitch
 * d * fh_phase_len(len, d) floats.  A dilated conv then reads and writes contiguous runs. */
int fh_phase_len(int len, int dilation);
/* groups: device array; all groups share cout_pad, len and the dilation.  phase_major != 0: x, res and out of
 * every group are phase-major for this dilation (see above), else plain [B, C, len]. */
/* tile_cfg | FH_WINO_BF16X6: the groups' `u` pointers name THREE-PIECE bf16 weights
 * ([C_in/16][tap group][6][cout_pad][3 pieces][16 channels] bf16 = 96 bytes per row and chunk; every fp32 value
 * x = h + m + l, h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)) and the contraction runs on the BF16 matrix cores as
 * six v_mfma_f32_32x32x16_bf16 per 16-channel k-block (pairs hh, hm, mh, mm, hl, lh; fp32 accumulation): fp32-grade
 * products (dropped terms <= 2^-24 |a b|) at 0.375 of the matrix-pipe cycles.  Inputs, outputs and accumulation stay
 * float32; results differ from the fp32-MFMA form by rounding only. */
#define FH_WINO_BF16X6 16
/* tile_cfg | FH_WINO_XCD_RANGES: block -> work mapping by TIME instead of by weight panel: XCD x (block id mod 8) works on
 * the x-th eighth of the time axis of every (group, batch, co tile) panel, the co tiles of the same time tiles next to
 * each other in dispatch order.  The co tiles of a group then read their common input through one L2 while it is
 * resident; every XCD fetches every weight panel.  For launches whose transformed weights are
 * small beside their activations (C <= 384 at batch 1): less HBM traffic, same bits.  Ignored by the ragged entry. */
#define FH_WINO_XCD_RANGES 32
/* tile_cfg | FH_WINO_NOVL: some tensor row of the launch is not 16-byte aligned although `len` % 4 == 0 (a segment with
 * xlen % 4 != 0): the slab loader must not use 16-byte loads.  Same bits. */
#define FH_WINO_NOVL 64
/* tile_cfg | FH_WINO_BF16X6 | FH_WINO_FRAG_ORDER (fh_conv_wino54_f32 and its ragged entry only): the three-piece weights lie
 * in FRAGMENT order, [C_in/16][tap group][8][cout_pad/32 granules][3 pieces][64 lanes][8 bf16]: lane 32 h + r of granule q,
 * piece p holds channels 8 h .. 8 h + 7 of row 32 q + r of that piece, the order in which the lanes of
 * v_mfma_f32_32x32x16_bf16 take the A operand (flowhigh_amd/packing.py: pack_wino54_weight_frag).  A wave's 16-byte load then
 * reads 1 KB contiguous (8 cache lines) where the 96-byte rows make it 32 segments over 24 lines.  Same values, same MFMA
 * order: same bits.  Without FH_WINO_BF16X6, or on fh_conv_wino_f32, the bit is an argument error. */
#define FH_WINO_FRAG_ORDER 128
int fh_conv_wino_f32(const fh_wino_group* groups, int n_groups, int batch, int cout_pad, int len,
                     int dilation, int phase_major, int tile_cfg, void* stream);
/* Ragged form (clips of different lengths, one group per clip and AMP block, batch 1): the grid is laid out for
 * max_len; a "run" is fh_wino_run_len(n_tiles) consecutive output tiles of one (group, co tile) panel
 * (n_tiles = ceil(ceil(max_len / dilation) / fh_wino_tile_n(tile_cfg)) * dilation), run id = panel * runs_per_panel +
 * run-in-panel with panel = group * co_tiles + co tile.  run_map (device int32 [n_runs]) lists the runs that hold
 * real tiles, in launch order (heavy groups first): they are dealt round-robin to the 8 XCDs.
 * layout_flags (0..3): bit 0 = the groups' tensors are phase-major (as phase_major != 0 above); bit 1 = some group's
 * rows are not 16-byte aligned (a len that is not a multiple of 4 in a plain-layout launch): no vector loads. */
int fh_wino_tile_n(int tile_cfg);
int fh_wino_run_len(int n_tiles);
int fh_conv_wino_ragged_f32(const fh_wino_group* groups, int n_groups, int cout_pad, int max_len, int dilation,
                            int layout_flags, int tile_cfg, const int* run_map, int n_runs, void* stream);

/* The same Conv1d call sites in the minimal-filtering form F(5,4) (8 points 0, +-1, +-2, +-1/2, inf; taps walked in
 * groups of 4: 1.6 ceil(k/4) multiply-adds per output and channel pair, 20 % fewer than F(4,3) over k = 3 / 7 / 11), for
 * the wide stages.  Same descriptors with ngrp = ceil(k / 4) and
 *   u = [cin/16][ngrp][8][cout_pad][16], u[., g, xi, co, .] = sum_j G8[xi][j] * w[co, ., 4g + j]
 * (flowhigh_amd/vocoder.py: pack_wino54_weight); ngrp <= 3 (k <= 12), out_stride <= 1, xlen = 0, out_len = 0 (longer
 * kernels run on fh_conv_grouped_f32, transposed-conv phases on fh_conv_wino_f32; the descriptors live in device memory, so
 * the library cannot check this on the host: flowhigh_amd/planner.py does when it builds a descriptor, and the kernel traps
 * on a segment it cannot walk).  Any dilation and any
 * len < 2^24 - 4096 (16.7 M samples = 5.8 min at 48 kHz per row; FH_E_ARG beyond: the kernel finds a sample's phase in fp32): rows
 * that are not 16-byte aligned are read and written with 4-byte accesses, same arithmetic.  tile_cfg: 0 = 128 co x 320 outputs per block,
 * 1 = 96 x 320, 2 = 64 x 320, 3 = 48 x 320 (three 16-row tiles of v_mfma_f32_16x16x4_f32: it sums a chunk's channels in another
 * order than the others, so a caller keeps ONE of {0, 1, 2} / 3 per weight tensor) (cout_pad % fh_wino54_tile_m(tile_cfg) == 0).  Results differ from the F(4,3) form by
 * rounding: 0.8-1.1e-5 per conv against float64 on unit-scale data (F(4,3) 0.6-1.1e-5, direct 4e-7), kernel-fuzz worst cases about a
 * third above F(4,3)'s (tests/tools/winograd_numerics.py, wino_fuzz.py; headroom against the weights' gain: profiles/r05_regime_sweep.txt). */
int fh_wino54_tile_m(int tile_cfg);
int fh_wino54_tile_n(void);
int fh_conv_wino54_f32(const fh_wino_group* groups, int n_groups, int batch, int cout_pad, int len,
                       int dilation, int phase_major, int tile_cfg, void* stream);
/* Ragged form, as fh_conv_wino_ragged_f32: runs of fh_wino54_run_len(n_tiles) consecutive 320-output tiles,
 * n_tiles = fh_wino54_n_tiles(max_len, dilation, phase-major?): in the plain layout ceil(ceil(len / dilation) / 320) tiles per
 * phase, tile index = block-in-phase * dilation + phase; in the phase-major layout the d phases are tiled as ONE sequence
 * (every phase owns ceil(n / 5) + >= 3 five-output tile slots, rounded up to a multiple of 4; a tile is 64 consecutive slots), a
 * group's real tiles are 0 .. fh_wino54_n_tiles(its len, ...) - 1.  layout_flags bit 0 = phase-major, bit 1 = some group's
 * plain rows are not 16-byte aligned. */
int fh_wino54_n_tiles(int len, int dilation, int phase_major);   /* 320-output blocks per (group, batch, co tile) panel */
int fh_wino54_run_len(int n_tiles);
int fh_conv_wino54_ragged_f32(const fh_wino_group* groups, int n_groups, int cout_pad, int max_len, int dilation,
                              int layout_flags, int tile_cfg, const int* run_map, int n_runs, void* stream);

/* out = ((a + b) + c) * scale over n floats (c may be NULL; n % 4 == 0, 16-byte aligned pointers): the
 * `xs += resblock(x); x = xs / num_kernels` of BigVGAN.forward (models/bigvgan/models.py:183-188) for the
 * stages whose closing conv is not fused (too few blocks to fill the chip at batch 1). */
int fh_mean_f32(const float* a, const float* b, const float* c, float* out, long long n, float scale,
                void* stream);
/* out = (((srcs[0] + srcs[1]) + ...) + srcs[n_srcs-1]) * scale, n floats each (n % 4 == 0, 16-byte aligned); srcs is a
 * HOST array of 1..12 device pointers.  Adds the partial outputs of a conv whose input channels were cut into
 * slices (one fh_wino_group per slice; short clips, vocoder.wino_split_k) in a fixed order; out may be srcs[0]. */
int fh_sum_f32(const float* const* srcs, int n_srcs, float* out, long long n, float scale, void* stream);

/* out = scale * (((p0 + p1) + p2) + ...) for several independent jobs in one launch (the averaging / partial-sum
 * passes of a ragged batch: one job per clip; same order of additions as fh_sum_f32 / fh_mean_f32). */
typedef struct {
  const float* src[12];
  float* out;
  int64_t n;             /* floats, % 4 == 0 */
  int32_t n_src;
  float scale;
} fh_sum_job;
int fh_sizeof_sum_job(void);
int fh_sum_multi_f32(const fh_sum_job* jobs, int n_jobs, long long max_n, void* stream);

/* conv_post + tanh (models/bigvgan/models.py:190-192): x [B, cin, L], w [cin, ksz], bias[1]
 * -> out [B, L] = tanh(bias + sum_ci sum_j w[ci,j] * x[b, ci, t + j - ksz/2]).  ksz odd <= 15. */
int fh_conv_post_tanh_f32(const float* x, const float* w, const float* bias, float* out,
                          int batch, int cin, int len, int ksz, void* stream);

/* ------------------------------------------------------------------------------------
 * Anti-aliased periodic activation, fused: 2x kaiser-sinc upsample -> Snake/SnakeBeta ->
 * 2x low-pass downsample, one read and one write of the tensor.
 * Replaces: Activation1d.forward, models/bigvgan/alias_free_torch/act.py:23-28
 *   (UpSample1d resample.py:25-33, SnakeBeta activations.py:107-120 / Snake :48-59,
 *    DownSample1d -> LowPassFilter1d filter.py:86-95).
 * Grouped like the conv: group g maps x[g] -> y[g] with its own per-channel parameters.
 *   alpha, inv_beta: [channels] already exponentiated if log-scale;
 *   inv_beta = 1 / (beta + 1e-9)  (or 1 / (alpha + 1e-9) for Snake).
 *   up_taps / down_taps: the 12 filter taps stored in the checkpoint.
 * --------------------------------------------------------------------------------- */
typedef struct {
  const float* x;        /* [B, C, L] */
  float* y;              /* [B, C, L] */
  const float* alpha;    /* [C] */
  const float* inv_beta; /* [C] */
  float up_taps[12];
  float down_taps[12];
  int32_t len;           /* fh_act1d_ragged_f32 only: L of THIS group (batch 1) */
  int32_t tile_base;     /* fh_act1d_ragged_f32 only: C * sum over the groups before of ceil(len / fh_act_tile_len()) */
} fh_act_group;

int fh_sizeof_act_group(void);
int fh_act1d_grouped_f32(const fh_act_group* groups, int n_groups, int batch, int channels,
                         int len, void* stream);
/* Same with phase-major tensors (fh_phase_len below): din / dout = dilation (1 .. 16) whose phase-major layout x / y
 * use, 1 = plain [B, C, len].  Used on both sides of a dilated Winograd conv. */
int fh_act1d_grouped_pm_f32(const fh_act_group* groups, int n_groups, int batch, int channels, int len,
                            int din, int dout, void* stream);
/* Ragged batches (clips of different lengths in ONE launch): group g = one clip's [C, groups[g].len] tensor,
 * total_tiles = groups[n-1].tile_base + C * ceil(groups[n-1].len / fh_act_tile_len()).  Same arithmetic per
 * sample as the launches above (replicate padding at each clip's own ends).  all_len_mult4: every group's len is a
 * multiple of 4 (rows 16-byte aligned: vector accesses). */
int fh_act_tile_len(void);
int fh_act1d_ragged_f32(const fh_act_group* groups, int n_groups, int channels, int din, int dout,
                        long long total_tiles, int all_len_mult4, void* stream);
/* Occupancy cap of the activation launches on the CURRENT device: at most `blocks` (2 .. 5) 4-wave blocks per CU, 0 = no cap
 * (7, the default).  A tuning knob, not a semantic one (results are the same bits): on some MI355X boxes the uncapped launch
 * draws enough power that the shader clock drops for the duration of the NEXT launch (a Winograd conv then takes 14 % longer);
 * 3 blocks per CU avoid most of that (the step is 5-7 % faster there) and cost the activation 25 % on boxes without the effect.  No
 * reference counterpart; the host calibrates it once per device (flowhigh_amd/vocoder.py: calibrate_act_occupancy,
 * FH_ACT_BLOCKS). */
int fh_act_set_blocks_per_cu(int blocks);
int fh_act_get_blocks_per_cu(void);

/* ------------------------------------------------------------------------------------
 * Narrow stages (C <= 48 channels): the Conv1d of an AMP block behind its Activation1d, shaped for few channels.
 * Replaces the `xt = conv(xt)` half of one `xt = self.activations[i](x); xt = conv(xt)` pair of an AMP block,
 *   models/bigvgan/models.py:63-72 (AMPBlock1: convs1[dilated] and convs2 "+ x") and :108-117 (AMPBlock2), incl. the
 *   "xs / num_kernels" average of the stage's blocks (:181-187) as K segments of one group:
 *     out[b, co, t] = scale * ( bias[co] + sum_r res[r][b, co, t]
 *                               + sum_seg sum_ci sum_{j<k} w_seg[co, ci, j] * x_seg[b, ci, t + (j - center) * dilation] )
 *   with x_seg read as 0 outside [0, len) (the conv's zero padding).  All tensors are plain [B, C, len] whatever the
 *   dilation.  The conv is evaluated in the Winograd F(5,4) form (fh_conv_wino54_f32): k <= 12 odd,
 *   dilation <= 6, (max_center - center) + 4 ngrp + 3 <= 16 for every segment.
 *   (ABI 3 also had the form with the Activation1d inside the launch -- flags bit 1 clear, activation parameters in the segment:
 *   measured slower than the pair of launches, it left the library with ABI 4.)
 * u = host-transformed weights (flowhigh_amd/packing.py: pack_amp_weight), float
 *   [C/8 chunks][ngrp][ blockA: [8 points][64 lanes][4]  (ceil(C/16) >= 2)  |  blockB: [8 points][64 lanes][2]  (ceil(C/16) odd) ]
 *   lane l = 16 kq + r: blockA[xi][l][2 m + s] = U[g][xi][co = 16 m + r][ci = 8 chunk + 2 kq + s] for the row tiles m = 0, 1,
 *   blockB[xi][l][s] the same for the last row tile of an odd count; U[g][xi] = sum_j G8[xi][j] w[:, :, 4 g + j] (float64 on
 *   the host, taps past k and rows past C zero): 1024 ceil(C/16) floats per (chunk, tap group) stage.
 * Groups may have different `len` (ragged batches).  The work list is a device array of `total_tiles` fh_amp_tile entries, one
 * per (group, batch item, tile of fh_amp_tile_len(dilation) outputs starting at t0), heavy groups first; a group's batch items
 * are [batch, C, len] tensors behind its pointers.
 * max_center: the largest `center` of any segment of the launch (<= 5): it places the samples in the kernel's LDS slabs, the same
 *        for every block.  The launch runs 2 x (CUs of the device) persistent blocks that walk the tile list with stride gridDim.
 * flags: bit 0 = every row of every group is 16-byte aligned (len % 4 == 0: vector accesses; same bits without);
 *        bit 1 = must be set (the conv alone; FH_E_ARG otherwise).
 * --------------------------------------------------------------------------------- */
typedef struct {
  const float* x;        /* [B, C, len]: the conv's input */
  const float* u;        /* transformed weights, layout above */
  int32_t ngrp;          /* ceil(k / 4) */
  int32_t center;        /* (k - 1) / 2 */
} fh_amp_seg;

typedef struct {
  fh_amp_seg seg[FH_CONV_MAX_SEG];
  const float* bias;                 /* [C] or NULL */
  const float* res[FH_CONV_MAX_SEG]; /* each [B, C, len] or NULL */
  float* out;                        /* [B, C, len] */
  int32_t nseg;
  int32_t nres;
  int32_t len;
  int32_t pad0_;
  float scale;
  int32_t pad1_;
} fh_amp_group;

typedef struct {
  int32_t group;       /* index into the launch's groups */
  int32_t batch_item;
  int32_t t0;          /* first output of the tile: a multiple of fh_amp_tile_len(dilation) */
  int32_t len;         /* = groups[group].len */
} fh_amp_tile;

int fh_sizeof_amp_group(void);
int fh_sizeof_amp_tile(void);
int fh_amp_tile_len(int dilation);     /* outputs per block and row: 320, 320, 300, 320, 300, 240 for dilation 1 .. 6; -1 beyond */
int fh_amp_max_channels(void);         /* 48 */
int fh_amp_actconv_f32(const fh_amp_group* groups, int n_groups, const fh_amp_tile* tiles, int total_tiles, int channels,
                       int dilation, int max_center, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * The same launches in the bf16 x 6 form (conv_form = 'bf16x6'; narrow_bf.hip): the narrow stages' residual-stack convs as a
 * DIRECT implicit GEMM on v_mfma_f32_16x16x32_bf16 -- every input sample is split once into three bf16 pieces (exact), a
 * product is six MFMAs with fp32 accumulation (dropped terms <= 2^-24 |a b|), no Winograd transforms.  Replaces the same
 * reference lines as fh_amp_actconv_f32 (bigvgan/models.py:63-72, :108-117, :181-187).  Same descriptors, read differently:
 *   fh_amp_seg.ngrp = k (taps, 1 .. 11), fh_amp_seg.center = zero-padding on the left in taps (<= 5; "same": (k - 1) / 2);
 *   fh_amp_seg.u = packing.pack_narrow_bf_weight: the channels' octets (8 channels) in slabs of at most three (24 channels: one
 *     slab; 48: two of three octets; balanced otherwise); per slab ceil(k og / 4) k-blocks of 32 = four (tap, octet) pairs,
 *     pair index q = tap og + octet; per k-block [N tile = 16 output channels][piece h, m, l][lane][8 bf16]: lane l holds
 *     w[co = 16 n + (l & 15)][ci = 8 (slab's first octet + octet of pair 4 kb + (l >> 4))  + 0 .. 7][tap of that pair], zero past
 *     the last pair / channel: ceil(C / 16) x 3 KB per k-block;
 *   tiles: t0 a multiple of fh_narrow_tile_len() = 256 outputs per block and row, any dilation 1 .. 6.
 * flags: bit 0 = every row of every group is 16-byte aligned (len % 4 == 0: vector accesses; same bits without).
 * A sample's bits depend on its position in the row only (fixed K order): alone, batched, ragged and chunked runs agree.
 * --------------------------------------------------------------------------------- */
int fh_narrow_tile_len(void);          /* 256 */
int fh_narrow_conv_bf16x6_f32(const fh_amp_group* groups, int n_groups, const fh_amp_tile* tiles, int total_tiles, int channels,
                              int dilation, int flags, void* stream);
/* ... and in the bf16 x 3 form (conv_form = 'direct_bf16x3'; the same kernel body with two pieces per operand: h and m of the
 * split, the three pairs (m h), (h m), (h h), dropped terms <= 3 2^-16 |a b|).  Same descriptors, tiles, flags and
 * argument checks; fh_amp_seg.u = packing.pack_narrow_bf3_weight: the layout above with two pieces per N tile,
 * [k-block][N tile][piece h, m][lane][8 bf16], ceil(C / 16) x 2 KB per k-block. */
int fh_narrow_conv_bf16x3_f32(const fh_amp_group* groups, int n_groups, const fh_amp_tile* tiles, int total_tiles, int channels,
                              int dilation, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * fp32 MFMA GEMM:  C[M, N] = epilogue( A[M, K] * W[N, K]^T )
 * Replaces every nn.Linear on the path (models/flow.py:239,261; attend.py:170-171;
 * transformer.py:98-104), torch.stft / torch.istft as DFT-by-GEMM
 * (melvoco.py:78-79; postprocessing.py:22-23,39) and the mel projection (melvoco.py:83).
 *   A row-major, row stride lda (floats, % 4 == 0); W row-major [n_pad, K] with
 *   n_pad = N rounded up to 128 (rows >= N zero); K % 32 == 0.
 * epilogue (v = acc + bias[n]):
 *   FH_EPI_LINEAR : C[m, n] = alpha * v + (R ? R[m, n] : 0)              (ldc, ldr strides)
 *   FH_EPI_GEGLU  : packed pairs: columns come in blocks of 64 = 32 "value" + 32 "gate";
 *                   C[m, 32*blk + i] = gelu_erf(gate) * value            (transformer.py:92-95)
 *   FH_EPI_MAG    : pairs (re, im): C = sqrt(re^2 + im^2 + 1e-9)         (melvoco.py:80-81)
 *   FH_EPI_LOGCLAMP: C = log(max(v, 1e-5))                               (modules.py:31-36)
 * --------------------------------------------------------------------------------- */
#define FH_EPI_LINEAR 0
#define FH_EPI_GEGLU 1
#define FH_EPI_MAG 2
#define FH_EPI_LOGCLAMP 3

int fh_gemm_f32(const float* A, int lda, const float* W, const float* bias, const float* R,
                int ldr, float* C, int ldc, int M, int N, int K, float alpha, int epilogue,
                void* stream);

/* The same GEMM in the bf16 x 6 form (gemm_bf.hip; the transformer's linears of a conv_form = 'bf16x6' model): fp32 in / out /
 * accumulate, every product as six v_mfma_f32_32x32x16_bf16 over exact three-piece bf16 splits (dropped terms <= 2^-24 |a b|).
 * A is split by the kernel on its way into LDS; Wp = packing.pack_gemm_bf_weight(W [n_pad, K]): bf16 bit patterns
 * [n_pad / 64][K / 32][piece h, m, l][k-octet 0..3][64 rows][8 bf16] (6 bytes per weight).  Same arguments, epilogues and
 * restrictions as fh_gemm_f32 (flow.py:239,261; attend.py:170-171; transformer.py:98-104). */
int fh_gemm_bf16x6_f32(const float* A, int lda, const float* Wp, const float* bias, const float* R,
                       int ldr, float* C, int ldc, int M, int N, int K, float alpha, int epilogue,
                       void* stream);

/* y[n] = act(bias[n] + sum_k W[n, k] * x[k]),  act: 0 none, 1 SiLU.  One vector (the time
 * embedding is the same for every clip: flow.py:208-211,242; transformer.py:81-83). */
int fh_gemv_f32(const float* W, const float* x, const float* bias, float* y, int N, int K,
                int act, void* stream);

/* LearnedSinusoidalPosEmb (models/pos_emb.py:22-26): out[0:h] = sin(t*w*2pi), out[h:2h] = cos. */
int fh_time_fourier_f32(const float* w, float t, float* out, int half_dim, void* stream);

/* ------------------------------------------------------------------------------------
 * Transformer pointwise / reduction kernels.
 * --------------------------------------------------------------------------------- */
/* ConvPositionEmbed + residual (models/transformer.py:16-46, flow.py:240):
 * y[b,n,c] = x[b,n,c] + gelu_erf(bias[c] + sum_j w[c,j] * x[b, n + j - ksz/2, c]), zero padded.
 * w is passed TRANSPOSED, [ksz, dim] (tap-major), dim % 128 == 0. */
int fh_dwconv_gelu_res_f32(const float* x, const float* w, const float* bias, float* y,
                           int batch, int n, int dim, int ksz, void* stream);

/* AdaptiveRMSNorm / RMSNorm (transformer.py:49-88):
 * y = x / max(||x||, 1e-12) * sqrt(dim) * gamma[c] + (beta ? beta[c] : 0); rows of `dim`. */
int fh_rmsnorm_f32(const float* x, const float* gamma, const float* beta, float* y, int rows,
                   int dim, void* stream);

/* MultiheadRMSNorm on q,k + rotary embedding, in place on the fused qkv buffer
 * (attend.py:144-151,179-184; pos_emb.py:53-59).  qkv [rows = B*n, 3*heads*64];
 * gq, gk [heads, 64]; cos_t, sin_t [n, 32] (angle table, one half).  dim_head must be 64. */
int fh_qknorm_rope_f32(float* qkv, const float* gq, const float* gk, const float* cos_t,
                       const float* sin_t, int batch, int n, int heads, void* stream);

/* softmax(q k^T * scale) v without materialising the score matrix (attend.py:102-139).
 * qkv as above (q | k | v along the feature axis), out [B*n, heads*64].  dim_head 64. */
int fh_attention_f32(const float* qkv, float* out, int batch, int n, int heads, float scale,
                     void* stream);
/* The same (attend.py:102-139) with both products in the bf16 x 6 form: six bf16 MFMAs per product over exact three-piece
 * splits, fp32 in / out / accumulate; the softmax is fh_attention_f32's, instruction for instruction (attn_form = 'bf16x6').
 * qkv and out must be 16-byte aligned. */
int fh_attention_bf16x6_f32(const float* qkv, float* out, int batch, int n, int heads, float scale, void* stream);

/* Ragged batches: clips of DIFFERENT lengths packed back to back in the token-major tensors, no padding rows.
 * seg: device int32 [n_seg][2] = (first row, rows) of every clip; max_n = the longest clip.  These are the
 * reference's mask paths -- the key mask of Attend (attend.py:127-128), the mask of ConvPositionEmbed
 * (transformer.py:35-44) -- for the layout in which masked positions simply do not exist; rotary positions
 * restart at 0 in every clip (pos_emb.py:47-51).  Every clip gets the bits it gets alone.
 * cos_t / sin_t must cover max_n positions. */
int fh_attention_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads,
                         float scale, void* stream);
/* fh_attention_seg_f32 in the bf16 x 6 form (the key mask of attend.py:127-128). */
int fh_attention_bf16x6_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads,
                                float scale, void* stream);
/* Banded attention (attn_window = radius, in frames): the four entries above with a band.  Query i of a clip of n rows reads
 * the keys j with 0 <= j < n and |i - j| <= radius; in the seg form i and j count from the clip's first row.  radius >= 0; any
 * radius >= n - 1 (INT_MAX too) is full attention and gives the bits of the full entry of the same form.  Cost O(n radius): a block
 * walks only the 64-key iterations that hold a key of its queries' bands.  A clip gives the same bits alone, inside any batch, and
 * in the seg form.  Arguments and checks of the full entries otherwise; qkv and out must be 16-byte aligned in both forms.
 * (The reference has no band: this is the mask sim.masked_fill(|i - j| > radius, -max) before the softmax of attend.py:131.) */
int fh_attention_band_f32(const float* qkv, float* out, int batch, int n, int heads, int radius, float scale, void* stream);
int fh_attention_band_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads, int radius,
                              float scale, void* stream);
int fh_attention_bf16x6_band_f32(const float* qkv, float* out, int batch, int n, int heads, int radius, float scale, void* stream);
int fh_attention_bf16x6_band_seg_f32(const float* qkv, float* out, const int* seg, int n_seg, int max_n, int heads, int radius,
                                     float scale, void* stream);
int fh_dwconv_gelu_res_seg_f32(const float* x, const float* w, const float* bias, float* y, const int* seg,
                               int n_seg, int max_n, int dim, int ksz, void* stream);
int fh_qknorm_rope_seg_f32(float* qkv, const float* gq, const float* gk, const float* cos_t,
                           const float* sin_t, const int* seg, int n_seg, int max_n, int heads, void* stream);

/* ------------------------------------------------------------------------------------
 * ConvNeXt vector field (models/convnext.py:9-93, flow.py:247-253): csrc/convnext.hip.
 * --------------------------------------------------------------------------------- */
/* Depthwise conv + time-conditioned LayerNorm of a ConvNeXtBlock, rows [batch * n, dim] token-major:
 *   u[r, c] = bias[c] + sum_{j < ksz} w[j, c] * x[r + j - ksz / 2, c]     zero padded at the CLIP's ends
 *   y[r, c] = (u[r, c] - mean_c u[r]) / sqrt(var_c u[r] + eps) * scale[c] + shift[c]     biased variance over the dim channels
 * w is tap-major [ksz, dim] as for fh_dwconv_gelu_res_f32, ksz odd and <= 7.  w == NULL: no conv, u = x (bias and ksz are not
 * read): a plain LayerNorm with scale = its weight and shift = its bias.  dim % 256 == 0, dim <= 4096; every pointer 16-byte
 * aligned; y must not overlap x.  FH_E_ARG otherwise, before anything is launched.  A block owns 16 consecutive rows of one clip.
 * The statistics are two passes over values kept in registers (the mean, then the centred values' mean and sum of squares),
 * summed in an order that does not depend on the row's place: a row's bits are a function of its own ksz input rows, the
 * same alone, in any batch and in the segment form (seg: the table of fh_dwconv_gelu_res_seg_f32, int32 [n_seg][2] =
 * (first row, rows); max_n = the longest clip's rows). */
int fh_dwconv_ln_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                     float* y, int batch, int n, int dim, int ksz, float eps, void* stream);
int fh_dwconv_ln_seg_f32(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                         float* y, const int* seg, int n_seg, int max_n, int dim, int ksz, float eps, void* stream);
/* y[i] = 0.5 x[i] (1 + erf(x[i] / sqrt 2)), i < n: nn.GELU as the GEGLU epilogue of the GEMMs evaluates it.  y may be x. */
int fh_gelu_f32(const float* x, float* y, long long n, void* stream);

/* ------------------------------------------------------------------------------------
 * STFT framing, post-processing (postprocessing.py:5-41) and peak normalisation.
 * Packed spectrum layout ("P-layout") used between the DFT GEMMs: per frame 33 blocks of
 * 64 floats = 32 real parts then 32 imaginary parts of bins 32*blk .. 32*blk+31 (bins >= 1025
 * are zero): width 2112.
 * --------------------------------------------------------------------------------- */
/* frames[b*nf + t, k] = pad(audio[b])[hop*t + k] * window[k], k < nfft.
 * pad_mode 0: reflect (melvoco.py:74), 1: zero (torch.stft center=True, pad_mode='constant'). */
int fh_frame_f32(const float* audio, const float* window, float* frames, int batch, int len,
                 int n_frames, int nfft, int hop, int pad, int pad_mode, void* stream);

/* energy[b, f] = sum_t |S[b, t, f]| over the first n_frames frames, f < 1025 (P-layout in). */
int fh_spec_energy_f32(const float* spec, float* energy, int batch, int n_frames, void* stream);

/* get_cutoff_index (postprocessing.py:10-16) / find_cutoff (cfm_superresolution.py:135-140):
 * cr[b] = max{ j in [1, nbins-1] : cumsum(energy[b])[j] < thr * total } or 0; energy [B, nbins]. */
int fh_cutoff_index_f32(const float* energy, int32_t* cr, int batch, int nbins, float thr,
                        void* stream);

/* 2048-point real FFT of framed audio and its inverse (the DFT halves of torch.stft / torch.istft,
 * models/melvoco.py:56-86, postprocessing.py:5-9,39): frames [rows, 2048] ->
 *   mode 0: packed complex spectrum [rows, 2112] (33 blocks of 32 Re + 32 Im, bins >= 1025 zero),
 *   mode 1: magnitudes sqrt(re^2 + im^2 + 1e-9) [rows, 1056] (melvoco.py:81, the input of the mel projection);
 * fh_irfft2048_f32: packed spectrum -> frames (C2R, imaginary parts of DC / Nyquist ignored, 1/N).
 * The butterflies run in float64 (see csrc/fft.hip).
 * twiddles: [1024, 2] DOUBLE = (cos, -sin)(2 pi k / 2048), flowhigh_amd/tables.py: fft_twiddles. */
int fh_rfft2048_f32(const float* frames, const double* twiddles, float* out, int rows, int mode, void* stream);
int fh_irfft2048_f32(const float* spec, const double* twiddles, float* frames, int rows, void* stream);

/* Sampler options of cfm_superresolution.py: mel-domain cutoff energy (:134-159, input to
 * fh_cutoff_index_f32 with thr 0.9995), low-band replacement mel_replace_ops (:146-152), and the
 * independent_cfm_* prior cond * std_1 + eps * std_2 (:226-236).  mel tensors are [B, n, d]. */
int fh_mel_energy_f32(const float* mel, float* energy, int batch, int n, int d, void* stream);
int fh_mel_splice_f32(const float* low, const float* high, const int32_t* cut, float* out, int batch,
                      int n, int d, void* stream);
/* Same for clips of different lengths packed back to back (the reference's masked batches, cfm:162-175,278-279):
 * seg = device int32 [n_seg][2] = (first row, rows) of every clip, mel tensors [sum rows, d], energy [n_seg, d],
 * cut [n_seg]; every clip gets the bits of a call on that clip alone. */
int fh_mel_energy_seg_f32(const float* mel, float* energy, const int32_t* seg, int n_seg, int d, void* stream);
int fh_mel_splice_seg_f32(const float* low, const float* high, const int32_t* cut, float* out,
                          const int32_t* seg, int n_seg, int max_n, int d, void* stream);
int fh_axpby_f32(const float* x, float a, const float* y, float b, float* out, long long n,
                 void* stream);

/* Stage arithmetic of the explicit Runge-Kutta methods of the sampler (flowhigh_amd/ode.py; heun2, heun3, rk4):
 *   out_a = y + h * sum_j wa[j] ks[j]     and, where wb and out_b are given (both, or neither),     out_b = y + h * sum_j wb[j] ks[j]
 * over n floats (n % 4 == 0, every pointer 16-byte aligned); every k and y is read once for both outputs.  ks, wa, wb are HOST
 * arrays of n_k = 1..4 entries, read at call time into kernel arguments (graph-capturable).  Per element and output:
 * s = w_j0 k_j0 for the first non-zero weight, then s = fmaf(w_j, k_j, s) in rising j, then out = fmaf(h, s, y); a term whose
 * weight is exactly 0 is skipped, not multiplied; a row of zeros only is an error.  out_a / out_b may be y or one of ks (an
 * element depends on its own index alone); out_a == out_b is an error.  No rows, no segment table: the batched and the ragged
 * layout are the same call. */
int fh_rk_combine_f32(const float* y, const float* const* ks, int n_k, float h, const float* wa, float* out_a,
                      const float* wb, float* out_b, long long n, void* stream);

/* A time and a step size per clip (flowhigh_amd/ode.py: mixed_schedule; csrc/row_groups.h): the clips of a ragged sequence are
 * sorted by step count, so the clips of one count are one contiguous range of rows, a GROUP.  Group g is the rows
 * row_end[g - 1] .. row_end[g] - 1 (row_end[-1] = 0); n = 1 .. FH_MAX_GROUPS, row_end strictly increasing from a first entry >= 1.
 * Every entry below reads the groups and its per-group scalars (HOST pointers, n entries) at call time into kernel
 * arguments: no device table, no upload, graph-capturable; a wave finds its row's group by at most eight scalar compares.
 * An entry that takes rows refuses row_end[n - 1] != rows.  Each grouped entry launches the kernel body of its one-time entry (the
 * one-time entry is the case of one group, or one vector), which is why a group's rows have that entry's bits. */
#define FH_MAX_GROUPS 8
typedef struct {
  int32_t n;
  int32_t row_end[FH_MAX_GROUPS];
} fh_row_groups;
int fh_sizeof_row_groups(void);
/* fh_time_fourier_f32 for n_groups times: out [n_groups][2 half_dim], row g the embedding of t[g]: the one-time entry is this
 * kernel with one group. */
int fh_time_fourier_groups_f32(const float* w, const float* t, float* out, int half_dim, int n_groups, void* stream);
/* Y[j] = act(W X[j] + bias) for T = 1 .. 8 vectors X[j] = X + j ldx (K floats each), Y[j] = Y + j ldy (N floats each); K % 4 == 0,
 * ldx % 4 == 0, W and X 16-byte aligned.  One wave per row of W, which is read once for all T; fh_gemv_f32 is this kernel at
 * T = 1, ldx = K, ldy = N, so every Y[j] has that entry's bits. */
int fh_gemv_rows_f32(const float* W, const float* X, int ldx, const float* bias, float* Y, int ldy, int N, int K, int T, int act,
                     void* stream);
/* fh_rmsnorm_f32 with a gamma / beta per group: a row of group g reads gamma + g g_stride and beta + g g_stride (beta may be
 * NULL); g_stride % 4 == 0.  dim % 256 == 0, dim <= 4096; one kernel body with fh_rmsnorm_f32 (which is group 0
 * for every row), hence its bits on the group's rows with its vectors. */
int fh_rmsnorm_groups_f32(const float* x, const float* gamma, const float* beta, long long g_stride, float* y, int rows, int dim,
                          const fh_row_groups* groups, void* stream);
/* out = alpha[g] v + res over [rows, dim] floats (res may be NULL: out = alpha[g] v), dim % 4 == 0, 16-byte aligned pointers: the
 * update of the linear GEMM epilogue (alpha, R) applied to a field that was written raw, with that epilogue's bits -- a
 * rounded multiply, then a rounded add of res (the epilogue's multiply and add sit on two sides of a branch and are never
 * fused).  out may be v or res. */
int fh_axpy_groups_f32(const float* v, const float* alpha, const float* res, float* out, int rows, int dim,
                       const fh_row_groups* groups, void* stream);
/* fh_rk_combine_f32 with a step h[g] per group over [rows, dim] floats (dim % 4 == 0): the same term order, skipped zero weights,
 * one- and two-output forms and aliasing rules, because both kernels run one element body; a row of group g has the bits of
 * that entry called with h[g]. */
int fh_rk_combine_groups_f32(const float* y, const float* const* ks, int n_k, const float* h, const float* wa, float* out_a,
                             const float* wb, float* out_b, int rows, int dim, const fh_row_groups* groups, void* stream);

/* eps ~ N(0,1) for the sampler's prior (cfm_superresolution.py:219-236), drawn on the device: counter-based Philox4x32-10 +
 * Box-Muller.  out [rows, d] token-major.  keys: DEVICE uint64 [n_seg][2] = (seed, stream) of every clip.
 * seg NULL: n_seg clips of n rows each; seg = device int32 [n_seg][2] = (first row, rows) as in the *_seg entries, n = longest clip.
 * d % 4 == 0, out 16-byte aligned.  An element's value depends on (seed, stream, row within its clip, column, d) only.
 * Element (f, m) of a clip: e = f d + m, quad q = e >> 2, lane e & 3; (r0 .. r3) = Philox4x32-10 of the counter
 * (q & 0xffffffff, q >> 32, stream & 0xffffffff, stream >> 32) under the key (seed & 0xffffffff, seed >> 32); with
 * u1 = ((r >> 8) + 1) 2^-24 and u2 = (r' >> 8) 2^-24, lanes 0, 1 = sqrt(-2 ln u1) (cos, sin)(2 pi u2) of (r0, r1), lanes 2, 3 the same
 * of (r2, r3); within 1e-5 of the float64 evaluation (flowhigh_amd/prior.py: prior_normal_host).  n_seg <= 65535, n d < 2^33. */
int fh_prior_normal_f32(float* out, const uint64_t* keys, const int32_t* seg, int n_seg, int n, int d, void* stream);
/* The same draw with clip b's rows counted from first_frames[b] (DEVICE int64 [n_seg], non-negative; a captured launch reads what
 * is there): quad q of clip b takes the counter first_frames[b] * d / 4 + q in 64 bits, so its n rows are rows first_frames[b] ..
 * first_frames[b] + n of a draw from 0 under the same key, bit for bit (the windows of a streaming session: flowhigh_amd/stream.py).
 * One kernel body with fh_prior_normal_f32, which is the case of no first_frames. */
int fh_prior_normal_at_f32(float* out, const uint64_t* keys, const int64_t* first_frames, const int32_t* seg, int n_seg, int n, int d,
                           void* stream);

/* out[b,t,:] = bins < cr[b] ? src : pred  (P-layout, postprocessing.py:36-37). */
int fh_spec_splice_f32(const float* pred, const float* src, const int32_t* cr, float* out,
                       int batch, int n_frames, void* stream);

/* Overlap-add of windowed inverse-DFT frames with window-envelope division, centre trim,
 * zero fill (torch.istft semantics, postprocessing.py:39); also atomically tracks
 * max|y| per clip in peak_bits[b] (float bits as uint32, must be zeroed by the caller). */
int fh_istft_ola_f32(const float* frames, const float* window, float* y, uint32_t* peak_bits,
                     int batch, int n_frames, int len, int nfft, int hop, void* stream);

/* y[b, :] *= target / peak[b]   (postprocessing.py:40; flowhighsr.py:69). */
int fh_peak_scale_f32(float* y, const uint32_t* peak_bits, int batch, int len, float target,
                      void* stream);

/* peak_bits[b] = bits(max_t |x[b,t]|) (caller zeroes peak_bits first). */
int fh_peak_abs_f32(const float* x, uint32_t* peak_bits, int batch, int len, void* stream);

/* ------------------------------------------------------------------------------------
 * Host pre-step on device: scipy.signal.resample_poly(x, up, down) with zero padding
 * (flowhighsr.py:68).  taps: the scipy FIR (already multiplied by `up`), n_taps odd-centred as
 * scipy pads it; y[b, i] = sum_j taps[j*up + (i*down + pre) % up ...] -- see resample_poly_kernel in
 * flowhigh_amd/csrc/frontend.hip.
 * --------------------------------------------------------------------------------- */
int fh_resample_poly_f32(const float* x, const float* taps, float* y, int batch, int len_in,
                         int len_out, int up, int down, int n_taps, int n_pre_remove,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * Segment forms of the entries above (flowhigh_amd/csrc/frontend.hip as well): clips of DIFFERENT lengths in one
 * launch, the front and back end of a ragged call (generate_many(ends='ragged')).  Every clip gets the bits of the
 * batched entry called on that clip alone (both are instantiations of one kernel body, which differ in the clip locator).
 *
 * A clip is described by the device int32 [n][2] table (first row, rows) of fh_mel_energy_seg_f32 where only packed
 * rows are involved, or by one fh_clip where it has a pointer or a sample range of its own.  An entry reads only
 * the fields its comment names; the others may hold anything.  n_clips <= 65535; the max_* / min_* arguments are the
 * largest / smallest value of that field over the table (the table lives on the device: the host that builds it
 * knows them and checks every clip; the entries check what they are given).
 * --------------------------------------------------------------------------------- */
typedef struct {
  const float* src;    /* the clip's input samples */
  float* dst;          /* the clip's output */
  int32_t len_in;      /* samples at src */
  int32_t len_out;     /* samples (elements) at dst */
  int32_t row0;        /* first of the clip's rows in the packed row buffer of the call */
  int32_t rows;
} fh_clip;
int fh_sizeof_clip(void);

/* dst[0 .. len_out) = resample_poly(src[0 .. len_in)) with one up, down, taps and n_pre_remove for the call; clips of
 * different input rates go through fh_resample_poly_rates_seg_f32 below.
 * taps == NULL (up == down == 1, equal rates): dst = src, len_in == len_out. */
int fh_resample_poly_seg_f32(const fh_clip* clips, int n_clips, int max_len_out, const float* taps, int up, int down,
                             int n_taps, int n_pre_remove, void* stream);
/* The same with a polyphase filter per clip: clip c is resampled by row rate_of[c] of `rates` (device int32 [n_clips],
 * device fh_rate [n_rates]), whose taps are tap_bank[taps_off .. taps_off + n_taps) of the device bank of bank_len floats
 * that holds the filters of all rates back to back.  Bits per clip: fh_resample_poly_f32 on that clip with that row.
 * The tables live on the device, so the kernel checks a row before it uses it: a clip whose rate_of is outside
 * [0, n_rates), or whose row has up <= 0, down <= 0, a negative field or taps_off + n_taps > bank_len, is left unwritten. */
typedef struct {
  int32_t taps_off;     /* first tap of this rate's filter in the tap bank (floats) */
  int32_t n_taps;       /* 0: equal rates, dst = src (len_in == len_out) */
  int32_t up, down;     /* reduced by their gcd */
  int32_t n_pre_remove;
} fh_rate;
int fh_sizeof_rate(void);
int fh_resample_poly_rates_seg_f32(const fh_clip* clips, const int32_t* rate_of, int n_clips, int max_len_out,
                                   const fh_rate* rates, int n_rates, const float* tap_bank, int bank_len, void* stream);
/* peak_bits[c] = bits(max |dst[0 .. len_out)|) (caller zeroes peak_bits first); dst[j] = (dst[j] / peak[c]) * target. */
int fh_peak_abs_seg_f32(const fh_clip* clips, int n_clips, int max_len, uint32_t* peak_bits, void* stream);
int fh_peak_scale_seg_f32(const fh_clip* clips, int n_clips, int max_len, const uint32_t* peak_bits, float target,
                          void* stream);
/* frames[row0 + t, k] = pad(src[0 .. len_in))[hop t + k] * window[k] for t < rows; pad modes as fh_frame_f32.
 * min_len: the shortest len_in (reflect: pad < min_len); hop (rows - 1) + nfft <= len_in + 2 pad for every clip. */
int fh_frame_seg_f32(const fh_clip* clips, int n_clips, int max_rows, int min_len, const float* window, float* frames,
                     int nfft, int hop, int pad, int pad_mode, void* stream);
/* energy [n_seg, 1025] over each clip's own rows of the packed P-layout spectrum; fh_cutoff_index_f32 takes it as it is. */
int fh_spec_energy_seg_f32(const float* spec, float* energy, const int32_t* seg, int n_seg, void* stream);
/* fh_spec_splice_f32 with clip c's cr[c] on its rows. */
int fh_spec_splice_seg_f32(const float* pred, const float* src, const int32_t* cr, float* out, const int32_t* seg,
                           int n_seg, int max_rows, void* stream);
/* fh_istft_ola_f32 per clip: dst[0 .. len_out) from the clip's rows [row0, row0 + rows) of frames, peak_bits[c]. */
int fh_istft_ola_seg_f32(const float* frames, const float* window, const fh_clip* clips, int n_clips, int max_len,
                         uint32_t* peak_bits, int nfft, int hop, void* stream);
/* dst[ch * rows + n] = mel[(row0 + n) * d + ch]: the packed token-major rows of a ragged batch into every clip's own
 * channel-major [d, rows] buffer (the vocoder's input), a plain copy. */
int fh_rows_to_channels_seg_f32(const float* mel, const fh_clip* clips, int n_clips, int max_rows, int d, void* stream);

/* -----------------------------------------------------------------------------------
 * Level-true output and multichannel clips (csrc/level.hip; FlowHighSR.generate*(channels=, level=)).  A row is one
 * channel of a clip run as a mono clip; its gain is the peak p its 48 kHz input was divided by.  Peak slots hold
 * non-negative float bits, as fh_peak_abs_f32 and fh_istft_ola_f32 leave them.
 * --------------------------------------------------------------------------------- */
/* gains[i] = the float in peak_bits[i]; a slot that holds +-0 becomes the bits of 1.0f (a silent row: the
 * fh_peak_scale_f32 that follows leaves its zeros as they are).  It goes between fh_peak_abs_f32 and fh_peak_scale_f32, or
 * between their segment forms. */
int fh_channel_peaks_f32(uint32_t* peak_bits, float* gains, int n, void* stream);
/* q_bits[i] = bits(max over the rows r of i's group, gains[r] != 0, of fl(q[r] * gains[r])); a maximum of 0 (every row
 * silent) becomes 1.0f.  group: device int32 [n], non-decreasing (rows of a group are adjacent).  One thread walks a
 * group: meant for a clip's channels, not for thousands of rows per group. */
int fh_group_peak_f32(uint32_t* q_bits, const float* gains, const int32_t* group, int n, void* stream);
/* y[b, :] *= gains[b] (one float32 multiply per sample), y [batch, len] at any 4-byte alignment; batch <= 65535. */
int fh_row_gain_f32(float* y, const float* gains, int batch, int len, void* stream);
/* The same over dst[0 .. len_out) of every clip (the table fh_peak_scale_seg_f32 takes); max_len: the longest len_out. */
int fh_row_gain_seg_f32(const fh_clip* clips, int n_clips, int max_len, const float* gains, void* stream);

/* -----------------------------------------------------------------------------------
 * int16 PCM on the device (csrc/pcm.hip; FlowHighSR.generate*(pcm='int16', dither=, interleaved=)): the last step of
 * delivery.  flowhigh_amd/pcm.py is the definition, the entries give its bits.
 *   sample x -> v = fl(x * 32768) (exact) -> v = fl(v + d) when dithering -> rint, ties to even -> clamp to
 *   [-32768, 32767]; NaN -> 0, +-inf saturates.
 *   d of channel c, sample t under the clip's key (seed, stream): (r0 .. r3) = Philox4x32-10 of the counter
 *   (q & 0xffffffff, q >> 32, stream & 0xffffffff, stream >> 32), q = t >> 1, under the key ((seed & 0xffffffff) ^ 0x50434D31,
 *   (seed >> 32) ^ c); even t takes (ra, rb) = (r0, r1), odd t (r2, r3); d = (ra >> 8) 2^-24 - (rb >> 8) 2^-24: triangular on
 *   (-1, 1) LSB, exact in fp32, a function of (key, c, t) only.
 * keys: DEVICE uint64 [n_clips][2] = (seed, stream) of every clip, or NULL: no dither.
 * interleaved 0: clip b's output is [channels][len] (planar, as its input); 1: [len][channels], written in that order.
 * --------------------------------------------------------------------------------- */
/* x [n_clips][channels][len] float32 (4-byte aligned) -> y, n_clips * channels * len int16 at any 2-byte alignment.
 * channels 1 .. 8, n_clips <= 65535. */
int fh_pcm_i16_f32(const float* x, int16_t* y, const uint64_t* keys, int n_clips, int channels, int len, int interleaved,
                   void* stream);
/* The same for clips of different shapes in one launch; clip c gets the bits of fh_pcm_i16_f32 on that clip alone with
 * keys[c].  Rows are read where they are: row r of a clip starts at src + r * pitch. */
typedef struct {
  const float* src;    /* the clip's first row */
  int16_t* dst;        /* channels * len int16, any 2-byte alignment */
  int64_t pitch;       /* floats from one row of the clip to the next */
  int32_t channels;    /* 1 .. 8 (a clip outside that range, or with len < 1, is left unwritten) */
  int32_t len;         /* samples per row */
} fh_pcm_clip;
int fh_sizeof_pcm_clip(void);
/* max_channels, max_len: the largest channels / len of the table. */
int fh_pcm_i16_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_channels, int max_len, const uint64_t* keys,
                       int interleaved, void* stream);
/* 24-bit PCM (pcm='s24', pcm='s24in32'; pcm.py: quantize24, pack24):
 *   sample x -> v = double(x) * 2^23 (exact) -> v = v + double(d) when dithering, ONE float64 add (a float32 add would round
 *   the dither away: x * 2^23 fills the float32 significand) -> rint, ties to even -> clamp to [-8388608, 8388607]; NaN -> 0,
 *   +-inf saturates.  d is the dither above, unchanged (one LSB is 256 times smaller).
 * container 3: a sample is its low three bytes, least significant first (pcm_s24le), y at ANY byte address; rows, clips and
 *   blocks may abut anywhere: no byte outside y[0 .. 3 n_clips channels len) is read or written.
 * container 4: the integer sign-extended in an int32; y 4-byte aligned (refused otherwise).  Any other container is refused.
 * Layouts, keys and limits as fh_pcm_i16_f32. */
int fh_pcm_s24_f32(const float* x, void* y, const uint64_t* keys, int n_clips, int channels, int len, int interleaved,
                   int container, void* stream);
/* The same over a table of clips: fh_pcm_clip with dst read as a BYTE address (container 4: a clip whose dst is not 4-byte
 * aligned is left unwritten).  Clip c gets the bits of fh_pcm_s24_f32 on that clip alone with keys[c]. */
int fh_pcm_s24_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_channels, int max_len, const uint64_t* keys,
                       int interleaved, int container, void* stream);

/* -----------------------------------------------------------------------------------
 * Integrated loudness on the device (csrc/loudness.hip; FlowHighSR.generate*(loudness=L), FlowHighSR.measure_loudness): ITU-R
 * BS.1770-4 as flowhigh_amd/loudness.py defines it -- K-weighting, 100 ms sub-block energies, 400 ms blocks at 75 % overlap,
 * the absolute gate at -70 LUFS and the relative gate 10 LU below the absolute-gated mean, both strict.  Everything behind the
 * float32 load is float64.  A clip shorter than one block is one block of its whole length; every channel weight is 1.0.
 * --------------------------------------------------------------------------------- */
/* Samples per span of the K-weighting recursion: one workgroup walks the spans of a row in order (tests stand either side). */
int fh_loudness_span_len(void);
/* energies[r, i] = sum over n in [i hop, min((i + 1) hop, len)) of y[r, n]^2, i < n_sub = ceil(len / hop), y = the K-weighted
 * row r of x [rows, len] (float32, 4-byte aligned); energies: DEVICE double [rows, n_sub].
 * coef: HOST double [10] = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (a0 = 1), read before the call returns.
 * hop >= 16 (a rate of 155 Hz or more); rows <= 65535; len <= 2^30.  A row's result depends on that row alone. */
int fh_kweight_energy_f32(const float* x, const double* coef, double* energies, int rows, int len, int hop, void* stream);
/* The same over clips read where they are: row r is channel r - (first row of its clip) of clip group[r] of the table (src,
 * pitch, channels, len are read; dst is not).  group: device int32 [rows], non-decreasing, with values in [0, n_clips).
 * energies: DEVICE double [rows, ceil(max_len / hop)], row r written up to its own ceil(len / hop); max_len: the largest len
 * of the table (a clip longer than that, or with len < 1, is left unwritten).  Row r gets the bits of
 * fh_kweight_energy_f32 on that row alone. */
int fh_kweight_energy_seg_f32(const fh_pcm_clip* clips, const int32_t* group, int n_clips, int rows, int max_len,
                              const double* coef, double* energies, int hop, void* stream);
/* One workgroup per clip: lufs[c] = the gated loudness of clip c (float32; -inf when no block passes a gate), whose rows are
 * those r with group[r] == c (group as above; every row of a clip has the clip's length lens[r]); energies: DEVICE double
 * [rows, n_sub] as the entries above leave it.  gains[r] = the clip's gain in each of its rows:
 *   fl32(min(10^((target - lufs[c]) / 20), 0.99 / peak)), peak = the largest of the rows' peak_bits (non-negative float bits, as
 *   fh_peak_abs_f32 leaves them); 1 when lufs[c] is not finite or the peak is 0 or not finite.
 * The gain is a function of the float32 lufs[c] that is written.  target: -70 .. 0 LUFS, or NaN: measure only, every gain 1.
 * Double arithmetic, blocks summed in ascending order. */
int fh_loudness_gate_f32(const double* energies, int n_sub, const int32_t* lens, const int32_t* group, int rows, int n_clips,
                         int hop, double target, const uint32_t* peak_bits, float* lufs, float* gains, void* stream);

/* -----------------------------------------------------------------------------------
 * Loudness meter (csrc/loudness.hip; FlowHighSR.measure_loudness_report, FlowHighSR.loudness_meter, delivery_stream(meter=True)):
 * EBU R128's figures as flowhigh_amd/meter.py defines them -- the integrated loudness above, the momentary series (the 400 ms
 * blocks), the short-term series (3 s windows of 30 sub-blocks at 100 ms hop) and the loudness range of EBU Tech 3342 (absolute
 * gate at -70 LUFS, relative gate 20 LU below the absolute-gated mean, both strict; the 10th and 95th percentile of the survivors
 * by the nearest-rank rule in integers).
 * --------------------------------------------------------------------------------- */
/* One workgroup per clip over the energies the two energy entries leave; energies, n_sub (the pitch), lens, group, rows, n_clips
 * and hop as fh_loudness_gate_f32 takes them, and n_sub <= 2^20.  report: DEVICE float [n_clips][6] =
 *   I        the integrated loudness: the bits of fh_loudness_gate_f32's lufs on the same energies
 *   M_max    the largest momentary loudness -0.691 + 10 log10(z[j]) over the clip's 400 ms blocks (a clip shorter than one
 *            block is one block of its whole length)
 *   S_max    the largest short-term loudness over the windows zs[j] = (s[j] + ... + s[j + 29]) / (30 hop), j < K - 29,
 *            s[i] = the sum over the clip's rows of energies[r, i], K = len / hop the complete sub-blocks
 *   LRA      10 log10(hi / lo) in LU: of the n windows with zs > ZA and zs > 0.01 mean(zs over those with zs > ZA), sorted
 *            ascending, lo is number (10 (n - 1) + 50) / 100 and hi number (95 (n - 1) + 50) / 100 (integer division); 0 when n = 0
 *   M_last, S_last   the last value of either series
 * in LUFS / LU; -inf for an empty series or a block of energy 0.  Double arithmetic, every window's 30 terms added in ascending
 * order; the percentiles are an exact selection over the windows' bit patterns (8 passes of 8 bits, both at once), the windows
 * made again from the energies on every pass: nothing is sorted or stored. */
int fh_loudness_report_f32(const double* energies, int n_sub, const int32_t* lens, const int32_t* group, int rows, int n_clips,
                           int hop, float* report, void* stream);
/* The K-weighting of a stream, block by block, with the bits of fh_kweight_energy_f32 on the whole stream: one job per row (one
 * channel of one stream) and launch.  A job's source is two runs read as one: the n_kept samples the row kept (fewer than a
 * span), then the n_fresh new ones; `base` is the absolute index of the first of them, a multiple of the span length, so span
 * boundaries stay where fh_kweight_energy_f32 has them.  The job starts from its record, walks every whole span of the source
 * -- with `ended` also the partial one behind them, and the stream ends there --, writes every sub-block sum that it finishes, and
 * the running sum of the one in progress, to log[] at the sub-block's absolute index (an index of log_len or more is not
 * written), stores the record back and copies the samples behind the last whole span to keep[] (a buffer that is neither run).
 * Nothing is read back: what was walked follows from the lengths alone. */
typedef struct {
  double s1, s2, t1, t2;   /* the filter's state behind the last sample walked */
  double acc;              /* the running sum of the sub-block in progress */
} fh_meter_state;
typedef struct {
  const float* kept;       /* n_kept float32 */
  const float* fresh;      /* n_fresh float32 */
  float* keep;             /* (n_kept + n_fresh) % span samples, when the stream has not ended */
  fh_meter_state* state;   /* the row's record: all zero for a new stream */
  double* log;             /* the row of the stream's energy log, log_len doubles */
  int64_t base;            /* absolute index of the first source sample: a multiple of fh_loudness_span_len() */
  int32_t n_kept, n_fresh;
  int32_t log_len;         /* <= 2^20 */
  int32_t ended;
} fh_meter_job;
int fh_sizeof_meter_state(void);
int fh_sizeof_meter_job(void);
/* jobs: DEVICE array; check: the same table on the HOST, read before the call returns: a job with a null pointer to something
 * it would use, a negative count, n_kept of a span or more, n_fresh > 2^30 - 2 spans, log_len > 2^20 or a base that is negative or no
 * multiple of the span length is refused here (FH_E_ARG), and the kernel leaves a job of the device table that fails the same
 * checks unwritten.  coef and hop as fh_kweight_energy_f32 takes them; n_jobs <= 65535. */
int fh_stream_kweight_energy_f32(const fh_meter_job* jobs, const fh_meter_job* check, int n_jobs, const double* coef, int hop,
                                 void* stream);

/* -----------------------------------------------------------------------------------
 * True peak and the look-ahead limiter on the device (csrc/truepeak.hip; FlowHighSR.generate*(true_peak=, limiter=),
 * FlowHighSR.measure_true_peak): ITU-R BS.1770-4 Annex 2 as flowhigh_amd/truepeak.py defines it.  Oversampling is by 4 at every
 * rate with the 81 taps of scipy.signal.resample_poly(x, 4, 1), zeros outside the clip, in float32 FMA chains in ascending tap order:
 *   x4[4 n + p] = sum_i h[p + 4 i] x[n + 10 - i]   (21 taps at p = 0, 20 at p = 1 .. 3)
 * taps: DEVICE float [82], the polyphase plan of (4, 1) as fh_resample_poly_f32 takes it: one leading zero, then h[0 .. 81).
 * A batched entry and its segment form give a clip the same bits; tiles are counted from the clip's sample 0.
 * --------------------------------------------------------------------------------- */
/* Frames per workgroup of the true-peak and envelope entries (tests stand either side). */
int fh_tp_tile_len(void);
/* peak_bits[r] = max(peak_bits[r], bits(max_n max(|x[r, n]|, |x4[r, 4 n + p]|, p = 0 .. 3))) over x [rows, len] float32 (4-byte
 * aligned): an integer atomic maximum of non-negative float bits into slots the caller zeroes, as fh_peak_abs_f32.
 * rows <= 65535; len <= 2^30. */
int fh_true_peak_f32(const float* x, const float* taps, uint32_t* peak_bits, int rows, int len, void* stream);
/* The same over clips read where they are: row r is channel r - (first row of its clip) of clip group[r] of the table (src, pitch,
 * channels, len are read; dst is not), group as fh_kweight_energy_seg_f32 takes it; max_len: the largest len of the table. */
int fh_true_peak_seg_f32(const fh_pcm_clip* clips, const int32_t* group, int n_clips, int rows, int max_len, const float* taps,
                         uint32_t* peak_bits, void* stream);
/* m[b, n] = max over the channels c of clip b of max(|x[b, c, n]|, |x4[b, c, 4 n + p]|): x [n_clips][channels][len], m [n_clips][len]
 * float32.  channels 1 .. 8, n_clips <= 65535. */
int fh_tp_envelope_f32(const float* x, const float* taps, float* m, int n_clips, int channels, int len, void* stream);
/* The same over a table of clips (src, pitch, channels, len are read); m [n_clips][max_len], clip b written up to its len. */
int fh_tp_envelope_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_len, const float* taps, float* m, void* stream);
/* The look-ahead limiter with half window H (1 .. 512) under the ceiling c (float32, 0 < c <= 1), from the clip's envelope m:
 *   r[n] = c / m[n] where m[n] > c, else 1; 1 outside [0, len)        (float32 division, correctly rounded)
 *   q[n] = min r[n - H .. n + H]
 *   g[n] = fl32(sum_k w[k] q[n - H + k], k = 0 .. 2 H ascending, in float64)     w: DEVICE double [2 H + 1]
 *   y[b, c, n] = clamp(fl32(x[b, c, n] g[n]), -c, c)
 * x, y [n_clips][channels][len] at any 4-byte alignment, y == x: in place; m [n_clips][len]; gain: NULL, or [n_clips][len], g is
 * written there as well.  Grid (tiles of 1024 frames, clips). */
int fh_limit_f32(const float* x, float* y, const float* m, const double* w, float* gain, int n_clips, int channels, int len, int H,
                 float ceiling, void* stream);
/* The same over a table of clips: dst NULL: the clip's rows are limited in place; else dst is the clip's output, FLOAT32
 * [channels][len] behind the table's int16_t*.  m and gain [n_clips][max_len]. */
int fh_limit_seg_f32(const fh_pcm_clip* clips, int n_clips, int max_len, const float* m, const double* w, float* gain, int H,
                     float ceiling, void* stream);
/* The gain of a delivery in every row of every clip (group as above), joint over the clip's rows:
 *   g_L = 1 when target is NaN, else from the clip's float32 loudness lufs[c]:
 *         uncapped 0: fl32(min(10^((target - lufs[c]) / 20), 0.99 / peak)), peak the largest of the rows' peak_bits (fh_loudness_gate_f32's gain)
 *         uncapped 1: fl32(10^((target - lufs[c]) / 20))                    (what a limiter follows)
 *         1 when lufs[c] is not finite (capped: or the peak is 0)
 *   gains[r] = g_L, or with uncapped 0 and tp_bits: fl32(min(g_L, ceiling / TP)), TP the largest of the rows' tp_bits (as
 *         fh_true_peak_f32 leaves them); g_L when TP is 0.  ceiling: linear, 0 < c <= 1.
 *   dbtp[c] = fl32(20 log10(TP)), -inf for TP = 0 (NULL: not written; gains may be NULL then).
 * lufs, peak_bits, tp_bits may be NULL where the rule does not read them.  Double arithmetic. */
int fh_delivery_gain_f32(const float* lufs, double target, const uint32_t* peak_bits, const uint32_t* tp_bits,
                         const int32_t* group, int rows, int n_clips, double ceiling, int uncapped, float* gains, float* dbtp,
                         void* stream);

/* ---- streaming sessions (csrc/stream.hip; flowhigh_amd/stream.py is the definition) ---- */
/* The seam between two consecutive windows of a stream, for every seam of a push in one launch.  Job j blends the first o48
 * samples of the newer window (head, in place) with the last o48 of the older one (tail):
 *   head[u] = fmaf(w_in[u], head[u], fl(w_out[u] * tail[u]))            float32, u = 0 .. o48 - 1
 * a term whose weight is exactly 0 is skipped, not multiplied (w_out[u] == 0: fl(w_in[u] * head[u]); w_in[u] == 0: fl(w_out[u] *
 * tail[u]); both: 0), so behind a weight 0 nothing is read into the result.  jobs: DEVICE array; w_in, w_out: DEVICE float32
 * [o48]; heads and tails at any 4-byte alignment.  No job's head may overlap any job's tail or another head (2 * overlap <=
 * window); the jobs are then independent and one session's consecutive seams go in one launch.  n_jobs <= 65535. */
typedef struct {
  float* head;
  const float* tail;
} fh_xfade_job;
int fh_sizeof_xfade_job(void);
int fh_xfade_seg_f32(const fh_xfade_job* jobs, int n_jobs, const float* w_in, const float* w_out, int o48, void* stream);

/* -----------------------------------------------------------------------------------
 * Streaming delivery (csrc/stream_delivery.hip; FlowHighSR.stream(delivery=), FlowHighSR.delivery_stream): the resampler, the
 * look-ahead limiter and the int16 encoder of delivery run block by block over a stream, with the bits of the one-shot entries on
 * the whole stream (flowhigh_amd/stream_delivery.py is the schedule and the definition).  One job per stream and launch, jobs:
 * DEVICE array.  A job's source is two spans read as one run of float32 samples -- the carry the stream kept, then the fresh
 * block -- whose first sample has the absolute index `base`; a sample outside the spans reads as 0.  The job writes the outputs
 * with the absolute indices [first, first + n_out) to dst[0 .. n_out) and copies the last n_keep source samples to
 * carry_out[0 .. n_keep) (a buffer that is neither span: a stream's two carry buffers take turns).  A job with a negative count,
 * a negative base or first, n_keep > n_carry + n_fresh, a null pointer to something it would use or (fh_stream_pcm_i16_f32) a dst
 * at an odd address is left unwritten; no job
 * reads outside its spans or writes outside dst[0 .. n_out) and carry_out[0 .. n_keep).  n_jobs <= 65535; max_out: the largest
 * n_out of the table (0: only carries move). */
typedef struct {
  const void* carry;   /* n_carry float32: the carried samples */
  const void* fresh;   /* n_fresh float32: the new block */
  void* dst;           /* n_out outputs: float32, int16 for fh_stream_pcm_i16_f32 */
  void* carry_out;     /* n_keep float32 (fh_stream_pcm_i16_f32 keeps nothing and does not read it) */
  int64_t base;        /* absolute index of carry[0] (of fresh[0] when n_carry is 0) */
  int64_t first;       /* absolute index of dst[0] */
  int32_t n_carry, n_fresh, n_out, n_keep;
  int32_t ended;       /* NOT READ BY THE KERNELS: the host's record that the stream ends at base + n_carry + n_fresh.  What lies
                          past the spans reads as the zeros (and r = 1) past a clip's end whether it is set or not; it is the
                          schedule that asks for outputs that read there only when the stream has ended */
  int32_t pad_;
} fh_stream_job;
int fh_sizeof_stream_job(void);
/* out[i] = sum_j x[j] taps[(i + pre) down - j up], fh_resample_poly_f32's loop and order with 64-bit indices; j runs down from
 * min((i + pre) down / up, the source's last sample). */
int fh_stream_resample_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const float* taps, int up, int down, int n_taps,
                           int pre, void* stream);
/* fh_tp_envelope_f32 + fh_limit_f32 of a mono stream in one launch: y[n] for n in [first, first + n_out) from the samples
 * n - 2 H - 10 .. n + 2 H + 10, zeros and r = 1 before sample 0 and past the source's end.  taps4: fh_tp_envelope_f32's taps;
 * w: DEVICE double [2 H + 1]; H 1 .. 512; 0 < ceiling <= 1.  Grid (tiles of 1024 outputs + 1, jobs). */
int fh_stream_limit_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const float* taps4, const double* w, int H,
                        float ceiling, void* stream);
/* fh_pcm_i16_f32's encoding of one channel: output o of a job encodes the source's sample first + o with the dither of channel 0
 * at the 64-bit sample index first + o under the job's key.  keys: DEVICE uint64 [n_jobs][2], NULL: no dither. */
int fh_stream_pcm_i16_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const uint64_t* keys, void* stream);
/* Streams of channels.  A stream of C channels (1 .. 8) is C consecutive jobs, one per channel row, each with its own carry,
 * fresh, dst and carry_out and all with equal base, first, n_carry, n_fresh, n_out and n_keep (fh_stream_resample_f32 runs them
 * as they are: a row per job).  groups: DEVICE int32 [n_groups + 1], group g = the jobs groups[g] .. groups[g + 1] of the table;
 * n_groups <= 65535.  A group that does not lie in the table, whose size is not 1 .. 8, whose jobs differ in a counter or one of
 * whose jobs would be left unwritten on its own (above) is left unwritten as a whole, and so is a job that no group holds.
 *
 * fh_stream_limit_f32, channel-linked: one envelope m[n] = the maximum over the group's channels (folded in
 * fh_tp_envelope_f32's order) and one gain for all of them: the bits of fh_tp_envelope_f32 + fh_limit_f32 on the whole
 * [C, T] stream, and of fh_stream_limit_f32 for C = 1.  Grid (tiles of 1024 outputs + 1, groups). */
int fh_stream_limit_linked_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out,
                               const float* taps4, const double* w, int H, float ceiling, void* stream);
/* fh_pcm_i16_f32's encoding of a stream of channels: output o of the group's job c encodes its source's sample first + o with the
 * dither of channel c at the 64-bit sample index first + o under the GROUP's key.  keys: DEVICE uint64 [n_groups][2], NULL: no
 * dither.  Planar (interleaved 0): every job writes its own dst[0 .. n_out); a group with a dst at an odd address is left
 * unwritten.  Interleaved: the dst of the group's FIRST job is the frame buffer int16 [n_out, C] (the other jobs' dst are
 * checked for null like any and not written); at an odd address the group is left unwritten.  The bits of fh_pcm_i16_f32 on
 * the whole [C, T] stream under the same key, and of fh_stream_pcm_i16_f32 for C = 1 planar. */
int fh_stream_pcm_i16_rows_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out,
                               const uint64_t* keys, int interleaved, void* stream);
/* The 24-bit twin (fh_pcm_s24_f32's encoding and containers): dst is container * n_out bytes per job, or the frame buffer of
 * container * n_out * C bytes behind the group's first job.  A mono stream is a group of one job.  container 3: dst at any byte
 * address; container 4: a group with a dst (interleaved: its first dst) that is not 4-byte aligned is left unwritten.  The bits
 * of fh_pcm_s24_f32 on the whole [C, T] stream under the same key. */
int fh_stream_pcm_s24_rows_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out,
                               const uint64_t* keys, int interleaved, int container, void* stream);

/* -----------------------------------------------------------------------------------
 * Spectral quality report on the device (csrc/quality.hip; FlowHighSR.measure_quality): the log-spectral distance of an estimate
 * e from a reference r, over all bins and below / above a cutoff bin, and their SNR, as flowhigh_amd/quality.py defines them.
 *   STFT: n_fft 2048, hop 480, the float32 Hann window (`window`, 2048 floats) taken as double, 1024 zeros either side:
 *   F = 1 + len / 480 frames, bins k = 0 .. 1024, P[t, k] = |X[t, k]|^2;  d = log10(max(P_r, 1e-8)) - log10(max(P_e, 1e-8));
 *   kc = the first bin of the high band: low = [0, kc), high = [kc, 1025), kc = -1: no cutoff;
 *   l_band[t] = sqrt(mean over the band's bins of d[t, k]^2): NaN for an empty band, and for low and high without a cutoff.
 * Both spectra of a frame come from ONE complex transform of e + i r (the LDS FFT of fh_rfft2048_f32; `twiddles` as that entry
 * takes them), separated as X_e[k] = (Z[k] + conj Z[2048 - k]) / 2, X_r[k] = (Z[k] - conj Z[2048 - k]) / (2 i).  Everything
 * behind the float32 loads is float64; no frame or spectrum is stored.  No floating-point atomics: every sum is a fixed tree.
 * --------------------------------------------------------------------------------- */
/* One workgroup per frame of every row pair of est, ref [rows, len] (float32).  frames: DEVICE double [rows][F][5], 8-byte
 * aligned; frame t of row r gets
 *   l_full[t], l_low[t], l_high[t]                                    (above)
 *   sum of r[n]^2 and sum of (r[n] - e[n])^2 over the samples n in [480 t, min(480 t + 480, len)) that the frame owns, the
 *   difference formed per sample in double
 * and nothing else is written.  1 <= len <= 2^30, rows <= 65535, -1 <= kc <= 1025.  A frame's five values depend on the row pair,
 * t and kc alone. */
int fh_quality_frames_f32(const float* est, const float* ref, const float* window, const double* twiddles, double* frames, int rows,
                          int len, int kc, void* stream);
/* The same over clips of different lengths and channel counts read where they are; a row gets the bits of
 * fh_quality_frames_f32 on that row pair alone with the clip's kc. */
typedef struct {
  const float* est;    /* the estimate's first row */
  const float* ref;    /* the reference's first row */
  int64_t est_pitch;   /* floats from one row of est to the next */
  int64_t ref_pitch;   /* the same for ref */
  int32_t channels;    /* rows of the clip, >= 1 */
  int32_t len;         /* samples per row, >= 1 */
  int32_t kc;          /* -1 .. 1025 */
  int32_t pad_;
} fh_quality_clip;
int fh_sizeof_quality_clip(void);
/* clips: DEVICE array; check: the same table on the HOST, read before the call returns (a clip with a null pointer, channels < 1,
 * len outside 1 .. max_len or kc outside -1 .. 1025 is refused; the kernel checks its own copy again and leaves such a clip
 * unwritten).  group: DEVICE int32 [rows], non-decreasing, values in [0, n_clips): row r is channel r - (first row of its clip)
 * of clip group[r].  frames: DEVICE double [rows][1 + max_len / 480][5], row r written up to its own 1 + len / 480 frames;
 * max_len: the largest len of the table. */
int fh_quality_frames_seg_f32(const fh_quality_clip* clips, const fh_quality_clip* check, const int32_t* group, int n_clips,
                              int rows, int max_len, const float* window, const double* twiddles, double* frames, void* stream);
/* One workgroup per clip over the frames either entry leaves (f_pitch: the frames per row of the buffer): the clip's rows are
 * those r with group[r] == c, every one of lens[r] samples (lens, group: DEVICE int32 [rows]).  report: DEVICE float
 * [n_clips][4] =
 *   lsd, lsd_low, lsd_high   the mean of l_band[t] over the C F frames of the clip's C rows
 *   snr_db                   10 log10(sum r^2 / sum (r - e)^2) over all of its samples: +inf for identical rows, -inf for a
 *                            silent reference beside another estimate, NaN for 0 / 0
 * each computed in double and rounded once.  Thread t adds the values of the frames i = t, t + 256, ... of the clip (i = channel
 * * F + frame) in ascending order, the 256 partial sums are added in a fixed tree: the order depends on the clip's (C, F)
 * alone, so a clip has the same bits whatever it is packed with.  A clip with no row, or whose frames do not fit f_pitch, reads
 * nothing and reports NaN. */
int fh_quality_report_f32(const double* frames, int f_pitch, const int32_t* lens, const int32_t* group, int rows, int n_clips,
                          float* report, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWHIGH_HIP_H */
