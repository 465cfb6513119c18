// Diagnostic / A-B switches of the library (host only: no HIP header, so the conv planner and its host tests can
// include it).
#pragma once

namespace alcm {

// diagnostic / A-B switches, read from ALCM_* environment variables at library load (alcm_knobs.cpp)
struct Knobs {
  int wconv = 8;                 // ALCM_WCONV: > 0 = the wide-layer kernels (alcm_wconv.hip), 0 = opconv_kernel (A/B)
  int wconv3 = -1;               // ALCM_WCONV3: persistent 8-wave 256 x 192 wide conv (alcm_wconv.hip): -1 by shape, 0 off, 1 on
  int wconv3_grid = 0;           // ALCM_WCONV3_GRID: cap on wconv3's persistent workgroups (tests; 0 = one per CU)
  int ups2_grid = 0;             // ALCM_UPS2_GRID: cap on ups2's persistent workgroups (tests; 0 = one or two per CU)
  int nconv = -1;                // ALCM_NCONV: 0 = opconv_kernel for the narrow tail, 2 = nconv for every width
  int opconv_tile = 0;           // ALCM_OPCONV_TILE: narrow-layer tile variant
  bool serial_resblocks = false; // ALCM_SERIAL_RESBLOCKS: default of alcm_model_set_resblock_streams
  bool prof_shapes = false;      // ALCM_PROF_SHAPES: split profile rows per layer shape
  int tconv_ablate = 0;          // ALCM_TCONV_ABLATE: timing-only ablation bits of the tail convs (1 no epilogue,
                                 // 2 no MFMA, 4 no window DMA, 8 no plane stores, 16 no fp32 state stores); selects
                                 // their diagnostics instantiation
  bool tconv_trace = false;      // ALCM_TCONV_TRACE: per-phase shader-clock trace of the tail convs (alcm_debug_tconv_trace;
                                 // diagnostics instantiation)
  int lin1 = -1;                 // ALCM_LIN1: single-plane 1x1 convs on lin_plane_kernel (1: 32-deep 4-stage ring, 2: 64-deep
                                 // double-buffered, -1: 64-deep for plane outputs), 0 = wconv2
  int tconv = 1;                 // ALCM_TCONV: narrow conv for BigVGAN stages 3-5: 1 by shape, 2 streamed weights,
                                 // 3 resident weights, 4 resident with C = 48 as 24-column halves on 128-row tiles (two
                                 // workgroups per CU), 5 = 4 with k = 3 at three per CU (decided by dense_conv_plan,
                                 // alcm_convplan.cpp; kernels in alcm_tconv.hip), 0 = opconv / nconv
  int act_defer = 1;             // ALCM_ACT_DEFER: act_mfma issues a tile's plane stores one tile late, before the next
                                 // prefetch (0 = at the end of the tile)
  int act_mfma = 1;              // ALCM_ACT_MFMA: Activation1d FIRs on MFMA for the wide stages (0 = VALU act_coop)
  int conv1_h16 = 1;             // ALCM_CONV1_H16: wide-stage AMPBlock conv1 writes an fp16 plane for its Activation1d
  int act_x3_mfma = 1;           // ALCM_ACT_X3_MFMA: the wide stages' three first Activation1d in one MFMA-FIR pass (0 = three)
  int nct_cl = 1;                // ALCM_NCT_CL: NCT conv inputs (DiT proj_in, BigVGAN conv_pre) transposed to channels-last
                                 // first (0 = strided gather in the conv)
  int ups_t160 = 1;              // ALCM_UPS_T160: strided (upsampler phase) wconv2 launches may take 160-row tiles
  int gemm_skinny = 1;           // ALCM_GEMM_SKINNY: k = 1 GEMMs of M <= 1024 rows (SK_MAXM) on gemm_skinny_kernel
                                 // (0 = MFMA tiles)
  int wconv_sum = 1;             // ALCM_WCONV_SUM: the wide stages' three chains' last conv2 + residual in one sum-form
                                 // launch writing the next stage's upsampler planes (2 = fp32 output + to_planes,
                                 // 0 = three accumulating launches)
  int ksplit = 1;                // ALCM_KSPLIT: wconv3 K parts on under-filled grids where a workspace is given (0 = never)
  int xp[4] = {0, 0, 0, 0};      // ALCM_XP0..3: scratch switches for an experiment in flight (no default path reads them)
};
const Knobs& knobs();

}  // namespace alcm
