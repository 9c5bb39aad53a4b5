// The epilogue of the grouped implicit-GEMM conv kernels (conv_mfma.hip, conv_mfma_bf.hip): a fragment of a kernel BODY, included
// as the kernel's last statements (text, not a function: as an inlined function the same lines gave the fp32 kernel another register
// assignment, and that kernel's instruction stream is kept as it was measured).  In scope where it is included:
//   PH, MT, NT (compile-time), f32x16 acc[PH][MT][NT], const fh_conv_group* G, b, co0, n0, wm, wn, l31, lh.
  // (the include site's contract, checked where the compiler can: a renamed or re-shaped accumulator, or a missing index, fails here)
  static_assert(PH >= 1 && sizeof(acc) == sizeof(f32x16) * PH * MT * NT, "conv_mfma_epilogue.h: acc must be f32x16[PH][MT][NT]");
  static_assert(sizeof(b) + sizeof(co0) + sizeof(n0) + sizeof(wm) + sizeof(wn) + sizeof(l31) + sizeof(lh) == 7 * sizeof(int) &&
                    sizeof(G->seg) == sizeof(fh_conv_seg) * FH_CONV_MAX_SEG,
                "conv_mfma_epilogue.h: G (fh_conv_group*), b, co0, n0, wm, wn, l31, lh (int) must be in scope");
  // ---- epilogue: bias + residuals, scale, strided store -------------------------------------
  // One buffer descriptor per tensor spans this batch item's [cout, lout] slab, so rows past
  // cout fall out of range by themselves; columns past n_len get an out-of-range offset.  Every
  // load and store is then unconditional (no exec-mask branches) and can be issued in bulk.
  const int nres = uni(G->nres);
  const float scale = G->scale;
  const int cout = uni(G->cout), lout = uni(G->lout), n_len = uni(G->n_len);
  const int ostride = uni(G->out_stride), ophase = uni(G->out_phase);
  const float* __restrict__ bias = uni(G->bias);
  const size_t slab = (size_t)b * cout * lout;
  const unsigned slab_bytes = (unsigned)cout * (unsigned)lout * 4u;
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(uni((const float*)G->out) + slab, slab_bytes);
  const __amdgpu_buffer_rsrc_t rr0 = make_rsrc(nres > 0 ? uni(G->res[0]) + slab : nullptr, nres > 0 ? slab_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rr1 = make_rsrc(nres > 1 ? uni(G->res[1]) + slab : nullptr, nres > 1 ? slab_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rr2 = make_rsrc(nres > 2 ? uni(G->res[2]) + slab : nullptr, nres > 2 ? slab_bytes : 0u);
  unsigned coloff[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + (wn * NT + nt) * 32 + l31;
    coloff[nt] = n < n_len ? (unsigned)(n * ostride + ophase) * 4u : 0x80000000u;
  }
  if constexpr (PH > 1) {
    // out[co, PH n + p] for p < PH: PH consecutive floats per lane, lanes on consecutive positions: whole lines per wave store
    // (ostride == PH, ophase == 0, no residuals: checked by the launcher / the host)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + (wm * MT + mt) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float bv = (bias && co < cout) ? bias[co] : 0.f;
        const unsigned rowoff = (unsigned)co * (unsigned)lout * 4u;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const unsigned off = (co < cout) ? rowoff + coloff[nt] : 0x80000000u;
          if constexpr (PH == 2) {
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 v = {__float_as_uint((acc[0][mt][nt][r] + bv) * scale), __float_as_uint((acc[1][mt][nt][r] + bv) * scale)};
            __builtin_amdgcn_raw_buffer_store_b64(v, ro, off, 0, 0);
          } else {
            typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
            const u32x3 v = {__float_as_uint((acc[0][mt][nt][r] + bv) * scale), __float_as_uint((acc[1][mt][nt][r] + bv) * scale),
                             __float_as_uint((acc[PH - 1][mt][nt][r] + bv) * scale)};
            __builtin_amdgcn_raw_buffer_store_b96(v, ro, off, 0, 0);
          }
        }
      }
    return;
  }
  auto& acc1 = acc[0];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      float v[4][NT];
      unsigned off[4][NT];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = co0 + (wm * MT + mt) * 32 + q + 8 * g4 + 4 * lh;
        const float bv = (bias && co < cout) ? bias[co] : 0.f;
        const unsigned rowoff = (unsigned)co * (unsigned)lout * 4u;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          off[q][nt] = (co < cout) ? rowoff + coloff[nt] : 0x80000000u;
          v[q][nt] = acc1[mt][nt][4 * g4 + q] + bv;
        }
      }
      if (nres > 0) {
        float t0[4][NT];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            t0[q][nt] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr0, off[q][nt], 0, 0));
        if (nres > 1) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              t0[q][nt] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr1, off[q][nt], 0, 0));
        }
        if (nres > 2) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              t0[q][nt] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr2, off[q][nt], 0, 0));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) v[q][nt] += t0[q][nt];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q][nt] * scale), ro, off[q][nt], 0, 0);
    }
  }
