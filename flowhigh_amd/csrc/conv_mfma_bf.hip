// Grouped implicit-GEMM 1-D convolution in the bf16 x 6 form (conv_form = 'direct_bf16x6'): conv_mfma.hip's contract -- the same
// descriptors, K segments, tap lists, epilogue, tiles and block mapping -- on v_mfma_f32_32x32x16_bf16.
//
// Replaces the Conv1d / ConvTranspose1d call sites of BigVGAN
// (/root/reference/src/flowhigh/models/bigvgan/models.py:63-72 AMPBlock1 convs, :141-146 ConvTranspose1d, :172-194 forward).
//
// GEMM view per group:  D[co, n] = sum_{seg} sum_{chunk} sum_{tap} sum_{ci < 16} W[chunk, tap, co, ci] * X[16 chunk + ci, n + off(tap)]
//   M = output channels (A operand: weights), N = time positions (B operand: samples), one K step = (16-channel chunk, tap).
// v_mfma_f32_32x32x16_bf16: A lane l = A[row l & 31][k = 8 (l >> 5) + j], B lane l = B[k = 8 (l >> 5) + j][col l & 31], j = 0..7
// (one 16-byte vector each); D as the fp32 instruction's.  A product is the six piece-pair MFMAs of bf16x6.h, small terms first,
// into ONE fp32 accumulator; steps run in (segment, chunk, tap) order, so an output's bits depend on its (group, channel,
// position) only -- not on the tile shape, the batch size or the block that computes it.
//
// Block = 4 waves, tile BM x BN = (32 MT WM) x (32 NT WN), as conv_mfma.hip:
//   * the slab of a chunk -- BN + halo samples of 16 channels -- is split ONCE (bf16x6_split) on its way into LDS and stored as
//     [piece][octet 0, 1][sample] in 16-byte units (8 channels x bf16), narrow_bf.hip's layout: the B fragment of a tap for 32
//     consecutive positions is 32 consecutive units of the lane half's octet, one conflict-free ds_read_b128 per piece at a shifted
//     sample index, any tap offset.  Samples are fetched with range-checked buffer loads (out of range -> 0: the conv's padding);
//     the slab is double buffered: chunk i + 1 is requested during chunk i's first tap and split + written during its second
//     (behind that step's first 3 MT NT MFMAs; the compiler's wait there is vmcnt(0), so once per chunk the next step's weight
//     fragments are waited for as well), so there is ONE barrier per chunk;
//   * the weights [cin/16][tap][cout_pad][piece h, m, l][16] bf16 (packing.pack_conv_bf_weight) are the A fragments as they lie
//     in memory: lane (row, half) loads the 8 channels of a piece as one 16-byte vector straight from L2 / L1, one K step ahead
//     (two register sets, requested unconditionally -- past the last step through a 0-byte descriptor -- so that every step's
//     wait is a counted vmcnt that leaves the next step's 3 MT loads in flight); no LDS, no barrier for them;
//   * a K step of a wave is 3 NT ds_read_b128 + 3 MT 16-byte loads for 6 MT NT MFMAs.
//
// The body is a template over the pieces per operand, NP.  NP = 3 is the form above.  NP = 2 (conv_form = 'direct_bf16x3',
// fh_conv_grouped_bf16x3_f32) keeps h and m only and multiplies the three pairs of kBf16x3SmallFirst -- (m h) (h m) (h h); the
// dropped terms are <= 3 2^-16 |a b| -- on two piece planes per slab and 64-byte weight rows [piece h, m][16]
// (packing.pack_conv_bf3_weight): a K step of a wave is 2 NT ds_read_b128 + 2 MT 16-byte loads for 3 MT NT MFMAs, and the next
// chunk's slab is written behind the FIRST pair's MFMAs.  Everything else -- descriptors, step order, epilogue, tiles, block
// mapping -- is the same code.
#include "bf16x6.h"
#include "conv_mfma_common.h"
#include "fh_common.h"

namespace {

// NP: pieces per operand -- 3: the six-pair form (fh_conv_grouped_bf16x6_f32), 2: the three-pair form (fh_conv_grouped_bf16x3_f32)
template <int NP, int MT, int NT, int WM, int WN>
struct ConvBfCfg {
  static_assert(NP == 2 || NP == 3, "two or three pieces per operand");
  static constexpr int BM = 32 * MT * WM;
  static constexpr int BN = 32 * NT * WN;
  static constexpr int XW = BN + FH_CONV_MAX_HALO;       // staged samples per octet
  static constexpr int ITEMS = 2 * XW;                   // (octet, sample) items of a chunk: 8 floats -> NP 16-byte units
  static constexpr int XR = (ITEMS + 255) / 256;         // items per thread
  static constexpr int PLANE = 2 * XW;                   // units of a piece plane
  static constexpr int SLAB = NP * PLANE;                // units of a slab
  static constexpr int TOFF = FH_CONV_MAX_SEG * FH_CONV_MAX_TAPS / 4;      // units of the tap shift table
  static constexpr int LDS_BYTES = 16 * (2 * SLAB + TOFF);                 // two slabs and the table
  // blocks per CU the launch bounds promise: as many as fit the CU's 160 KB of LDS, at most 2 (three pieces: 2, except the 32 x 512
  // tile, whose two slabs -- 108 KB -- leave room for one; two pieces: that tile's 72 KB fit twice as well)
  static constexpr int BLOCKS_PER_CU = 2 * LDS_BYTES <= 160 * 1024 ? 2 : 1;
};

template <int NP, int MT, int NT, int WM, int WN>
__global__ __launch_bounds__(256, (ConvBfCfg<NP, MT, NT, WM, WN>::BLOCKS_PER_CU)) void conv_mfma_bf_kernel(const fh_conv_group* __restrict__ groups, int n_groups, int batch, int co_tiles,
                                                              int n_tiles) {
  using Cfg = ConvBfCfg<NP, MT, NT, WM, WN>;
  constexpr int BM = Cfg::BM, BN = Cfg::BN, XW = Cfg::XW, XR = Cfg::XR, PLANE = Cfg::PLANE, SLAB = Cfg::SLAB;
  constexpr int PH = 1;
  constexpr unsigned ROW_BYTES = 32 * NP;                  // a weight row: NP pieces x 16 bf16
  constexpr int NPAIRS = bf16_n_pairs<NP>();
  constexpr int STAGE_PAIR = NP == 3 ? 2 : 0;              // the pair behind whose MFMAs the next chunk's slab is written
  __shared__ __attribute__((aligned(16))) u32x4 lds[2 * SLAB + Cfg::TOFF];
  int* toff = reinterpret_cast<int*>(lds + 2 * SLAB);    // [seg][tap] sample shift of each tap

  FH_CONV_BLOCK_MAP(groups, n_groups, batch, co_tiles, n_tiles);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, lh = lane >> 5;
  const int co0 = cot * BM;
  const int n0 = ntile * BN;
  const int lin = uni(G->lin), cout_pad = uni(G->cout_pad), nseg = uni(G->nseg);
  // (ragged launches: a block past its group's last column has nothing to do)
  if (n0 >= uni(G->n_len)) return;

  f32x16 acc[PH][MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][i][j][r] = 0.f;

  int nsteps = 0;
  for (int s = 0; s < nseg; ++s) nsteps += uni((G->seg[s].cin / 16) * G->seg[s].ntaps);

  if (tid < FH_CONV_MAX_SEG * FH_CONV_MAX_TAPS) {
    const fh_conv_seg* sg = &G->seg[tid / FH_CONV_MAX_TAPS];
    toff[tid] = (tid / FH_CONV_MAX_TAPS) < nseg ? sg->tap_off[tid % FH_CONV_MAX_TAPS] - sg->off_min : 0;
  }

  // ---- cursors (conv_mfma.hip's): K the step that computes, W the step whose weights are requested (one ahead), X the chunk whose
  // slab is requested (one ahead) ---------------------------------------------------------------------------------------------------
  struct Cur { int s, j, nt, cl; };          // segment, tap, taps per chunk, chunks left in the segment (this one included)
  Cur K = {0, 0, uni(G->seg[0].ntaps), uni(G->seg[0].cin) / 16};
  const unsigned wstep = (unsigned)cout_pad * ROW_BYTES;                   // bytes of one (chunk, tap) of weights
  int w_seg = -1, w_left = 0;
  unsigned w_soff = 0;
  __amdgpu_buffer_rsrc_t w_r = make_rsrc(nullptr, 0);
  auto w_enter = [&]() {
    ++w_seg;
    const fh_conv_seg* sg = &G->seg[w_seg < nseg ? w_seg : nseg - 1];
    w_left = w_seg < nseg ? (uni(sg->cin) / 16) * uni(sg->ntaps) : 0x7fffffff;
    w_r = make_rsrc(reinterpret_cast<const char*>(uni(sg->w)) + (size_t)co0 * ROW_BYTES,
                    w_seg < nseg ? (unsigned)w_left * wstep - (unsigned)co0 * ROW_BYTES : 0u);
    w_soff = 0;
  };
  unsigned avoff[MT];                          // lane (row, half): the half's 8 channels of piece 0 of the row
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) avoff[mt] = (unsigned)((wm * MT + mt) * 32 + l31) * ROW_BYTES + (unsigned)lh * 16u;
  auto load_a = [&](u32x4 (&a)[MT][NP]) {       // the W cursor's fragments, then on to the next step
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int p = 0; p < NP; ++p) a[mt][p] = __builtin_amdgcn_raw_buffer_load_b128(w_r, avoff[mt] + 32u * p, w_soff, 0);
    w_soff += wstep;
    if (--w_left == 0) w_enter();
  };

  int x_seg = -1, x_left = 0, x_t0 = 0;
  const float* x_chunk = nullptr;              // first row of the X cursor's chunk
  auto x_enter = [&]() {
    ++x_seg;
    const fh_conv_seg* sg = &G->seg[x_seg < nseg ? x_seg : nseg - 1];
    const int cin = uni(sg->cin);
    x_left = x_seg < nseg ? cin / 16 : 0x7fffffff;
    x_chunk = uni(sg->x) + (size_t)b * cin * lin;
    x_t0 = n0 + uni(sg->off_min);
  };
  // item = (octet o, slab sample s): the 8 channels 8 o .. 8 o + 7 at t = x_t0 + s; t outside [0, lin) reads 0
  unsigned xreg[XR][8];
  int xo[XR], xs_[XR];
#pragma unroll
  for (int r = 0; r < XR; ++r) {
    const int item = tid + 256 * r;
    xo[r] = item >= XW ? 1 : 0;
    xs_[r] = item - xo[r] * XW;
  }
  auto load_x = [&]() {                        // the X cursor's chunk, then on to the next one
    const __amdgpu_buffer_rsrc_t r16 = make_rsrc(x_chunk, 16u * (unsigned)lin * 4u);
    const unsigned row = (unsigned)lin * 4u;
#pragma unroll
    for (int r = 0; r < XR; ++r) {
      const int t = x_t0 + xs_[r];
      const bool in = (unsigned)t < (unsigned)lin && tid + 256 * r < Cfg::ITEMS;
      const unsigned off = in ? (unsigned)(xo[r] * 8 * lin + t) * 4u : 0x80000000u;
#pragma unroll
      for (int c = 0; c < 8; ++c) xreg[r][c] = __builtin_amdgcn_raw_buffer_load_b32(r16, off, row * c, 0);
    }
    x_chunk += (size_t)16 * lin;
    if (--x_left == 0) x_enter();
  };
  auto store_x = [&](int buf) {                // split the requested chunk into the slab `buf`
#pragma unroll
    for (int r = 0; r < XR; ++r) {
      if (tid + 256 * r < Cfg::ITEMS) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = __uint_as_float(xreg[r][c]);
        if constexpr (NP == 3) {
          u32x4 h, m, l;
          bf16x6_split(v, h, m, l);
          u32x4* const dst = lds + buf * SLAB + xo[r] * XW + xs_[r];
          dst[0] = h;
          dst[PLANE] = m;
          dst[2 * PLANE] = l;
        } else {
          u32x4 h, m;
          bf16x3_split(v, h, m);
          u32x4* const dst = lds + buf * SLAB + xo[r] * XW + xs_[r];
          dst[0] = h;
          dst[PLANE] = m;
        }
      }
    }
  };

  // ---- prologue -----------------------------------------------------------------------------------------------------------
  u32x4 aA[MT][NP], aB[MT][NP];
  int xbuf = 0;
  w_enter();
  x_enter();
  load_a(aA);
  load_x();
  store_x(0);
  __syncthreads();

  // One K step: CUR holds this step's weight fragments, NXT receives the next step's.  The next chunk's slab is requested at a
  // chunk's first tap and split into the other buffer behind the first three pair MFMAs (two pieces: the first pair's) of its second tap
  // (of its only tap when it has one): the barrier at the chunk's end is the only one.
  int xoff_cur = toff[0];
  auto step = [&](int it, const u32x4 (&CUR)[MT][NP], u32x4 (&NXT)[MT][NP]) {
    const bool last_tap = K.j == K.nt - 1;
    const bool more_chunks = K.cl > 1 || K.s + 1 < nseg;
    const bool flip_x = last_tap && more_chunks;
    const bool stage = more_chunks && K.j == (K.nt > 1 ? 1 : 0);
    const int j1 = last_tap ? 0 : K.j + 1;
    const int s1 = (last_tap && K.cl == 1 && K.s + 1 < nseg) ? K.s + 1 : K.s;
    load_a(NXT);                                 // (past the last step: a 0-byte descriptor, nothing is fetched)
    if (K.j == 0 && more_chunks) load_x();
    const u32x4* const xsb = lds + xbuf * SLAB + lh * XW + xoff_cur + wn * NT * 32 + l31;
    bf16x8 bfr[NT][NP];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int p = 0; p < NP; ++p) bfr[nt][p] = __builtin_bit_cast(bf16x8, xsb[p * PLANE + nt * 32]);
    const int xoff_next = toff[s1 * FH_CONV_MAX_TAPS + j1];
#pragma unroll
    for (int pp = 0; pp < NPAIRS; ++pp) {
      const Bf16x6Pair s = bf16_small_first<NP>(pp);         // (weight piece, sample piece)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[0][mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, CUR[mt][s.a]), bfr[nt][s.b], acc[0][mt][nt], 0, 0, 0);
      if (pp == STAGE_PAIR && stage) store_x(xbuf ^ 1);
    }
    if (flip_x) {
      __syncthreads();
      xbuf ^= 1;
    }
    xoff_cur = xoff_next;
    if (last_tap) {
      K.j = 0;
      if (--K.cl == 0 && K.s + 1 < nseg) {
        ++K.s;
        K.nt = uni(G->seg[K.s].ntaps);
        K.cl = uni(G->seg[K.s].cin) / 16;
      }
    } else {
      ++K.j;
    }
  };

  for (int it = 0; it < nsteps; it += 2) {
    step(it, aA, aB);
    if (it + 1 < nsteps) step(it + 1, aB, aA);
  }

  // (kernel body fragment: reads PH, MT, NT, acc, G, b, co0, n0, wm, wn, l31, lh of this scope -- see the header's static_asserts)
#include "conv_mfma_epilogue.h"
}

// the entry's name, for its messages
template <int NP>
constexpr const char* conv_bf_name() {
  return NP == 3 ? "fh_conv_grouped_bf16x6_f32" : "fh_conv_grouped_bf16x3_f32";
}

template <int NP, int MT, int NT, int WM, int WN>
int launch_conv_bf(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len, hipStream_t stream) {
  using Cfg = ConvBfCfg<NP, MT, NT, WM, WN>;
  int co_tiles, n_tiles;
  const long long blocks = conv_grid_blocks(n_groups, batch, cout_pad, n_len, Cfg::BM, Cfg::BN, &co_tiles, &n_tiles);
  FH_CHECK_ARG(blocks > 0 && blocks < (1ll << 31), "%s: grid too large", conv_bf_name<NP>());
  hipLaunchKernelGGL((conv_mfma_bf_kernel<NP, MT, NT, WM, WN>), dim3((unsigned)blocks), dim3(256), 0, stream, groups, n_groups, batch, co_tiles,
                     n_tiles);
  FH_CHECK_LAUNCH(conv_bf_name<NP>());
  return FH_OK;
}

// The descriptors of a launch normally live in device memory, where the launcher cannot see them (the host plan checks the shapes
// it builds them from).  An array in pinned host memory -- which the kernel reads just as well -- is checked here.
int check_host_groups(const char* name, const fh_conv_group* groups, int n_groups) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, groups) != hipSuccess) {
    (void)hipGetLastError();
    return FH_OK;
  }
  if (at.type != hipMemoryTypeHost || !at.hostPointer) return FH_OK;
  const fh_conv_group* g = static_cast<const fh_conv_group*>(at.hostPointer);
  for (int i = 0; i < n_groups; ++i) {
    FH_CHECK_ARG(g[i].nseg >= 1 && g[i].nseg <= FH_CONV_MAX_SEG && g[i].nres >= 0 && g[i].nres <= FH_CONV_MAX_SEG,
                 "%s: group %d has %d segments, %d residuals (1 .. %d, 0 .. %d)", name, i, g[i].nseg, g[i].nres,
                 FH_CONV_MAX_SEG, FH_CONV_MAX_SEG);
    for (int s = 0; s < g[i].nseg; ++s) {
      const fh_conv_seg& sg = g[i].seg[s];
      FH_CHECK_ARG(sg.cin > 0 && sg.cin % 16 == 0, "%s: group %d segment %d has %d input channels (a multiple of 16)", name,
                   i, s, sg.cin);
      FH_CHECK_ARG(sg.ntaps >= 1 && sg.ntaps <= FH_CONV_MAX_TAPS && sg.off_max - sg.off_min <= FH_CONV_MAX_HALO && sg.off_max >= sg.off_min,
                   "%s: group %d segment %d: %d taps over %d samples (at most %d over %d)", name, i, s, sg.ntaps,
                   sg.off_max - sg.off_min, FH_CONV_MAX_TAPS, FH_CONV_MAX_HALO);
    }
  }
  return FH_OK;
}

template <int NP>
int conv_grouped_bf(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len, int tile_cfg, void* stream) {
  constexpr const char* name = conv_bf_name<NP>();
  FH_CHECK_ARG(groups && n_groups > 0 && batch > 0 && n_len > 0, "%s: bad sizes", name);
  const int bm = fh_conv_tile_m(tile_cfg);
  FH_CHECK_ARG(bm > 0, "%s: unknown tile_cfg %d", name, tile_cfg);
  FH_CHECK_ARG(cout_pad % bm == 0, "%s: cout_pad %d not a multiple of tile %d", name, cout_pad, bm);
  if (const int rc = check_host_groups(name, groups, n_groups)) return rc;
  // per-clip tensors are addressed with 32-bit byte offsets (buffer descriptors): cout * lout * 4 < 2^31 and 16 * lin * 4 < 2^32
  // are checked by the host plan (flowhigh_amd/planner.py) where the shapes are known.
  hipStream_t st = (hipStream_t)stream;
#define FH_CONV_BF_CASE(id, MT, NT, WM, WN) \
  case id:                                  \
    return launch_conv_bf<NP, MT, NT, WM, WN>(groups, n_groups, batch, cout_pad, n_len, st);
  switch (tile_cfg) {          // (conv_mfma.hip's shapes: the planner's tile choice and cout_pad carry over)
    FH_CONV_BF_CASE(0, 2, 2, 2, 2)
    FH_CONV_BF_CASE(1, 3, 2, 2, 2)
    FH_CONV_BF_CASE(2, 3, 2, 1, 4)
    FH_CONV_BF_CASE(3, 2, 2, 1, 4)
    FH_CONV_BF_CASE(4, 1, 4, 1, 4)
    FH_CONV_BF_CASE(5, 2, 1, 2, 2)
    FH_CONV_BF_CASE(6, 3, 1, 1, 4)
  }
#undef FH_CONV_BF_CASE
  return FH_E_ARG;
}

}  // namespace

extern "C" int fh_conv_grouped_bf16x6_f32(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len, int tile_cfg,
                                          void* stream) {
  return conv_grouped_bf<3>(groups, n_groups, batch, cout_pad, n_len, tile_cfg, stream);
}

// The same launches with two pieces per operand and the three pairs of kBf16x3SmallFirst (conv_form = 'direct_bf16x3'): weights
// [cin/16][tap][cout_pad][piece h, m][16] bf16 (packing.pack_conv_bf3_weight), 64-byte rows.
extern "C" int fh_conv_grouped_bf16x3_f32(const fh_conv_group* groups, int n_groups, int batch, int cout_pad, int n_len, int tile_cfg,
                                          void* stream) {
  return conv_grouped_bf<2>(groups, n_groups, batch, cout_pad, n_len, tile_cfg, stream);
}
