// What the two Winograd conv kernels share, conv_wino.hip (F(4,3), 6 transform points) and conv_wino54_kernel.h (F(5,4), 8 points):
// everything outside the transforms, the LDS slabs and the MFMA loops -- the segment record, the block -> work mapping, the fp32
// weight loader and the L2 warm-up, the exchange-tile write, the output-side record with its residual / tail-store paths, and
// the host's launch geometry and LDS opt-in.  Template parameters are what really differs: NP = transform points, BM = output
// rows of a block, ROWF = floats per weight row and 16-channel chunk (16 fp32, 24 = three bf16 pieces).
#pragma once
#include "fh_common.h"

namespace {

constexpr int WINO_RUN = 8;          // n-blocks of a panel that run together on one XCD

// ---- one segment of a group: input rows, transformed weights ---------------------------------------------------------
// (xlen > 0: the rows are xlen samples long, not the group's len -- F(4,3) as a transposed conv's phase; the F(5,4) kernel
// never reads the field, so it costs that kernel nothing)
struct WinoSeg {
  const float* x;
  const float* u;
  int cin, ngrp, center, xlen;
};
__device__ __forceinline__ WinoSeg load_wino_seg(const fh_wino_seg* S) {
  WinoSeg w;
  w.x = uni(S->x);
  w.u = uni(S->u);
  w.cin = uni(S->cin);
  w.ngrp = uni(S->ngrp);
  w.center = uni(S->center);
  w.xlen = uni(S->xlen);
  return w;
}

// ---- block -> (panel, n block) -------------------------------------------------------------------------------------
// launch constants the mapping divides by (fh_common.h: fh_fastdiv), made by wino_geometry below
struct WinoDivs {
  fh_fastdiv run_len, runs_per_panel, co_tiles, batch, dil;
};

// Panels = (group, batch item, co tile), heavy groups first.  A panel's n blocks are cut into equal runs of <= WINO_RUN
// (with fixed runs of 8 and 10 blocks per panel, every other XCD would get the 2-block remainders only); run r goes to XCD
// r % 8, the blocks of a run are 8 block ids apart.  False: this block has no work.
// Ragged launches (groups of different lengths, grid sized for the longest): only the runs that hold real tiles are
// launched, listed heavy-first in run_map -- otherwise the empty runs of the short clips, which fall on the same XCDs for
// every panel (run r of a panel -> XCD (panel * runs_per_panel + r) % 8), leave the real work on 2-4 of the 8 XCDs.
__device__ __forceinline__ bool wino_block_work(int bid, const int* __restrict__ run_map, int n_runs, int panels, int run_len,
                                                int n_tiles, const WinoDivs& dv, int& panel, int& ntile) {
  const int total_runs = panels * (int)dv.runs_per_panel.d;
  const int slot = bid >> 3;
  const int slot_run = fh_div(slot, dv.run_len);
  int run = slot_run * 8 + (bid & 7);
  if (run_map) {
    if (run >= n_runs) return false;
    run = uni(run_map[run]);
  }
  if (run >= total_runs) return false;
  panel = fh_div(run, dv.runs_per_panel);
  ntile = fh_mod(run, panel, dv.runs_per_panel) * run_len + fh_mod(slot, slot_run, dv.run_len);
  return ntile < n_tiles;
}
__device__ __forceinline__ void wino_split_panel(int panel, const WinoDivs& dv, int& gi, int& b, int& cot) {
  const int gb = fh_div(panel, dv.co_tiles);
  cot = fh_mod(panel, gb, dv.co_tiles);
  gi = fh_div(gb, dv.batch);
  b = fh_mod(gb, gi, dv.batch);
}

// ---- weights: global -> registers in fragment layout -------------------------------------------------------------------
// where a wave's weight tiles are: U[cin / 16][tap group][NP points][cout_pad][ROWF], rows co0 .. co0 + BM - 1 of point xi
struct WinoWts {
  int xi, co0, cout_pad;
};
template <int NP, int ROWF>
__device__ __forceinline__ const float* wino_a_tile(const WinoSeg& S, int chunk, int g, const WinoWts& w) {
  return uni(S.u + ((size_t)((chunk * S.ngrp + g) * NP + w.xi) * w.cout_pad + w.co0) * ROWF);
}
// Every load is issued unconditionally from straight-line code ("nothing to load" is a zero-sized descriptor: the hardware
// returns 0 without touching memory), so the number of loads in flight at each use is a compile-time constant and the
// s_waitcnt the compiler places are exact.
// fp32 form, half h (k-steps 4 h .. 4 h + 3) of the MA row tiles of ROWS rows: lane (row, half) holds 8 consecutive channels of
// its row, two 16-byte loads; a_lane = the lane's byte offset inside a row tile (the caller's: the 16-row form has its own)
template <int NP, int BM, int MA, int ROWS = 32, int NA>
__device__ __forceinline__ void wino_load_a_half(u32x4 (&areg)[NA][2], int h, const WinoSeg& S, int chunk, int g, bool valid,
                                                 const WinoWts& w, int a_lane) {
  static_assert(MA <= NA, "register set too small");
  const __amdgpu_buffer_rsrc_t r = make_rsrc(wino_a_tile<NP, 16>(S, chunk, g, w), valid ? BM * 16 * 4 : 0);
#pragma unroll
  for (int mt = 0; mt < MA; ++mt) areg[mt][h] = __builtin_amdgcn_raw_buffer_load_b128(r, a_lane + mt * ROWS * 16 * 4 + 16 * h, 0, 0);
}
// (The three-piece loaders of the bf16 x 6 forms stay in the kernels: F(5,4)'s takes a piece mask and keeps its offsets immediates
// through an empty asm; given that form, F(4,3)'s 96-row K loops come out as another instruction sequence: profiles/winograd_kernel_frame.md.)

// L2 warm-up of the A tiles of the NEXT chunk (all its tap groups, this wave's xi): the register prefetch of the K loops is
// only half a step deep, enough for an L2 hit but not for HBM, and the blocks that share a weight panel run in lockstep, so
// without this every tile is a first touch for all of them.  One lane per 128-byte line, lanes 0-31 tap group 2j, lanes
// 32-63 group 2j + 1; the result is never used.  The loads are ordinary builtin loads into two registers that the NEXT
// prefetch "reads" (an empty asm) before it overwrites them: the compiler then knows when they land.  (Until round 6 this
// was an inline-asm load into one register the compiler knew nothing about -- correct only while the allocator happened to
// keep that register for the kernel's whole life: every instantiation that spilled moved it, the late write then hit
// whatever lived there, and the result was garbage that changed from run to run: tools/exp/ragged_bf_debug.py, DESIGN
// section 0.)  A kernel ends with wino_prefetch_done: the last prefetch is waited for, never used.
template <int NP, int BM, int ROWF>
__device__ __forceinline__ void wino_prefetch_a(unsigned (&pf)[2], const WinoSeg& S, int chunk, bool valid, const WinoWts& w,
                                                int l31, int lh) {
  const float* up = wino_a_tile<NP, ROWF>(S, chunk, 0, w);
  const unsigned gstride = (unsigned)NP * (unsigned)w.cout_pad * ROWF * 4u;          // bytes between tap groups
  const __amdgpu_buffer_rsrc_t r = make_rsrc(up, valid ? (unsigned)(S.ngrp - 1) * gstride + BM * ROWF * 4 : 0u);
  asm volatile("" :: "v"(pf[0]), "v"(pf[1]));          // the previous prefetch has landed before its registers are reused
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    // (lanes past the tile's lines: out of range; the 96-byte rows of the three-piece form are 0.75 BM lines, the first
    // 32 lanes' worth of which is touched: enough to start the L2 fill of the tile)
    // (a select of two values, not a branch around the sum: a load under a branch costs the exact wait counts, above)
    const unsigned line = (unsigned)(2 * j + lh) * gstride + (unsigned)l31 * 128u;
    const unsigned off = l31 < BM * ROWF / 32 ? line : 0x80000000u;
    pf[j] = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
  }
}
__device__ __forceinline__ void wino_prefetch_done(const unsigned (&pf)[2]) { asm volatile("" :: "v"(pf[0]), "v"(pf[1])); }

// ---- epilogue ------------------------------------------------------------------------------------------------------------
// A lane's 16 accumulators of a 32 x 32 tile are 4 runs of 4 consecutive rows (8 q + 4 lh + 0..3) of its column l31: four
// ds_write_b128 into a COLUMN-major exchange tile; ew = the lane's column + 4 lh.  (Column pitch 36 floats in both kernels:
// 16-byte aligned, and 36 col mod 64 takes 16 distinct multiples of 4 over 16 lanes: conflict-free b128.)
__device__ __forceinline__ void wino_exchange_write(float* ew, const f32x16& a) {
#pragma unroll
  for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(ew + 8 * q) = (f32x4){a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
}

__device__ __forceinline__ f32x4 wino_as_f32(u32x4 t) {
  return (f32x4){__uint_as_float(t[0]), __uint_as_float(t[1]), __uint_as_float(t[2]), __uint_as_float(t[3])};
}

// The output side of one (group, batch item): out, up to three residuals, bias; out = (y + bias + res...) * scale.
// Store paths: one per WAVE, every access an unconditional buffer operation in straight-line code (nothing to do =
// out-of-range offset 0x80000000, or a zero-sized descriptor for an absent residual / bias).  With a per-lane "whole
// vector?" branch around them the compiler's s_waitcnt in front of each residual use let only 2-3 operations stay in
// flight, and vmcnt counts loads and stores in order -- every sub-tile then waited for the write acknowledge of the one
// before it; with the bias load inside the item loop it put s_waitcnt vmcnt(0) behind every item's loads
// (tools/exp/w54_fixed_cost.py).  So: the bias and the first residual are requested ahead by the kernels, and the
// functions below only branch on the wave-uniform nres.
struct WinoOut {
  __amdgpu_buffer_rsrc_t ro, rr0, rr1, rr2, rbias;
  int nres;
  float scale;
};
// slab = the batch item's first float in out and the residuals, all of cout rows of `pitch` floats
__device__ __forceinline__ WinoOut wino_make_out(const float* out, const float* const (&res)[3], const float* bias, int nres,
                                                 float scale, size_t slab, int cout, int pitch) {
  const unsigned slab_bytes = (unsigned)cout * (unsigned)pitch * 4u;
  WinoOut o;
  o.ro = make_rsrc(out + slab, slab_bytes);
  o.rr0 = make_rsrc(nres > 0 ? res[0] + slab : nullptr, nres > 0 ? slab_bytes : 0u);
  o.rr1 = make_rsrc(nres > 1 ? res[1] + slab : nullptr, nres > 1 ? slab_bytes : 0u);
  o.rr2 = make_rsrc(nres > 2 ? res[2] + slab : nullptr, nres > 2 ? slab_bytes : 0u);
  o.rbias = make_rsrc(bias, bias ? (unsigned)cout * 4u : 0u);
  o.nres = nres;
  o.scale = scale;
  return o;
}
// 16-byte path (nres > 0): rs[i] = first[i] + residual 1 + residual 2 at byte offset off[i]; first = residual 0, requested
// ahead.  All N loads of a residual are issued before the first is used.
template <int N>
__device__ __forceinline__ void wino_add_res16(const WinoOut& O, const u32x4 (&first)[N], const unsigned (&off)[N], f32x4 (&rs)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) rs[i] = wino_as_f32(first[i]);
  if (O.nres > 1) {
    u32x4 t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = __builtin_amdgcn_raw_buffer_load_b128(O.rr1, off[i], 0, 0);
#pragma unroll
    for (int i = 0; i < N; ++i) rs[i] += wino_as_f32(t[i]);
  }
  if (O.nres > 2) {
    u32x4 t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = __builtin_amdgcn_raw_buffer_load_b128(O.rr2, off[i], 0, 0);
#pragma unroll
    for (int i = 0; i < N; ++i) rs[i] += wino_as_f32(t[i]);
  }
}
__device__ __forceinline__ f32x4 wino_add_res16(const WinoOut& O, u32x4 first, unsigned off) {      // ... of one vector
  const u32x4 f[1] = {first};
  const unsigned o[1] = {off};
  f32x4 rs[1];
  wino_add_res16(O, f, o, rs);
  return rs[0];
}
// 4-byte path (a row ends inside the wave's tiles, strided or unaligned rows): four outputs y[0..3] of one row at four
// byte offsets: residuals, bias, scale, store
template <class Y>
__device__ __forceinline__ void wino_store_tail(const WinoOut& O, const unsigned (&off)[4], const Y& y, float bv) {
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
  if (O.nres > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) rs[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(O.rr0, off[q], 0, 0));
    if (O.nres > 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) rs[q] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(O.rr1, off[q], 0, 0));
    }
    if (O.nres > 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) rs[q] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(O.rr2, off[q], 0, 0));
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float o = y[q] + bv;
    if (O.nres > 0) o += rs[q];
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o * O.scale), O.ro, off[q], 0, 0);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline int wino_run_len(int n_tiles) { return fh_cdiv(n_tiles, fh_cdiv(n_tiles, WINO_RUN)); }

// run length, runs and blocks of a launch of `panels` panels of n_tiles n-blocks (run_map: a ragged launch's own list of
// n_runs runs), and the kernel's divisors
struct WinoGeom {
  int run_len;
  long long blocks;
  WinoDivs dv;
};
inline WinoGeom wino_geometry(int n_tiles, long long panels, const int* run_map, int n_runs, int co_tiles, int batch, int dilation) {
  WinoGeom g;
  g.run_len = wino_run_len(n_tiles);
  const long long runs = run_map ? (long long)n_runs : panels * fh_cdiv(n_tiles, g.run_len);
  g.blocks = (long long)fh_cdiv(runs, 8) * 8 * g.run_len;
  g.dv = {fh_make_fastdiv((unsigned)g.run_len), fh_make_fastdiv((unsigned)fh_cdiv(n_tiles, g.run_len)),
          fh_make_fastdiv((unsigned)co_tiles), fh_make_fastdiv((unsigned)batch), fh_make_fastdiv((unsigned)dilation)};
  return g;
}

// > 64 KB of dynamic LDS needs the attribute once per DEVICE (a kernel has one function object per device, and a process
// may hold models on several): one flag per device ordinal and kernel (KERNEL = the instantiation's address).
template <auto KERNEL>
int wino_lds_opt_in(int bytes, const char* entry) {
  static std::atomic<bool> lds_opt_in[FH_MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= FH_MAX_DEVICES) {
    fh_set_error("%s: no current HIP device (or ordinal >= %d)", entry, FH_MAX_DEVICES);
    return FH_E_LAUNCH;
  }
  if (!lds_opt_in[dev].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
      fh_set_error("%s: cannot reserve %d bytes of LDS on device %d: %s", entry, bytes, dev, hipGetErrorString(e));
      return FH_E_LAUNCH;
    }
    lds_opt_in[dev].store(true, std::memory_order_release);
  }
  return FH_OK;
}

}  // namespace
