// bf16 x 6 instantiations of the F(5,4) wide-stage conv (conv_wino54_kernel.h, `BF`): a translation unit of their own because
// they are compiled with -fno-slp-vectorize (flowhigh_amd/build.py): at plain -O3 the SLP vectoriser re-packs the scalar FMAs /
// subtractions of the transform and the split into v_pk_fma_f32 / v_pk_add_f32, which stall the bf16 MFMAs they sit beside.
// The fp32-MFMA instantiations (conv_wino54.hip) keep the default flags and their code.
#include "conv_wino54_kernel.h"

// frag: the weights are in fragment order (FH_WINO_FRAG_ORDER, conv_wino54_kernel.h: FR), else in 96-byte rows
int fh_internal_wino54_bf(const fh_wino_group* groups, int n_groups, int batch, int cout_pad, int len, int dilation, int pm, int mt,
                          bool vl, bool frag, hipStream_t st, const int* run_map, int n_runs) {
#define FH_W54BF_LAUNCH(MT, VL, FR) launch_wino54<MT, VL, false, true, FR>(groups, n_groups, batch, cout_pad, len, dilation, pm, st, run_map, n_runs)
#define FH_W54BF_CASE(MT)                                                                      \
  case MT:                                                                                     \
    if (frag) return vl ? FH_W54BF_LAUNCH(MT, true, true) : FH_W54BF_LAUNCH(MT, false, true);  \
    return vl ? FH_W54BF_LAUNCH(MT, true, false) : FH_W54BF_LAUNCH(MT, false, false);
  switch (mt) {          // (a 128-row block fits with 2 spilled registers and is no faster per row: 3.00 us per K step against
                         // 2.22 us of the 96-row block -- the loop is not bound by the vector work an extra row tile amortises)
    FH_W54BF_CASE(3)
    FH_W54BF_CASE(2)
  }
#undef FH_W54BF_CASE
#undef FH_W54BF_LAUNCH
  fh_set_error("fh_conv_wino54_f32: no bf16 x 6 block of %d row tiles", mt);
  return FH_E_ARG;
}
