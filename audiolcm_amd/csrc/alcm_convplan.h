// Host-only planner of the operand-plane convs (alcm_opconv / alcm_opconv_sum / alcm_opconv_dense): validates a call
// and decides, once, which kernel instantiation it gets, with which tile, grid, K parts and workgroup order, and under
// which profile name.  No HIP header and no device call: pointers are only tested for null-ness and alignment, never
// dereferenced.  The launchers (alcm_sgemm.hip, alcm_wconv.hip, alcm_nconv.hip, alcm_opconv.hip, alcm_tconv.hip) take
// the plan and only launch.
#pragma once
#include <cstdint>

#include "audiolcm_hip.h"
#include "alcm_knobs.h"

namespace alcm {

// tile geometry the planner shares with the kernels
constexpr int W3_BM = 256, W3_BN = 192;  // wconv3_kernel tile
constexpr int W2_HALO = 64;              // wconv2_kernel: max (k - 1) * dil
constexpr int OC_HALO = 64;              // opconv_kernel: max (k-1)*dil
constexpr int NC_HALO = 64;              // nconv_kernel: max (k-1)*dil
constexpr int SG_BM = 128, SG_BN = 192;  // sgemm_planes / lin_plane tile
constexpr int ACT_EPI_HALO = 8;          // conv tile rows computed beyond each side of the emitted rows

// CK_TCONV / CK_TCONV2: the BigVGAN tail convs of alcm_opconv_dense, tconv_kernel (weights resident in LDS) and
// tconv2_kernel (weights streamed)
enum ConvKernel { CK_LIN_PLANE = 0, CK_WCONV3, CK_WCONV3_SUM, CK_WCONV2, CK_NCONV, CK_OPCONV, CK_TCONV, CK_TCONV2 };
// the tail convs' epilogue forms: Activation1d planes only (an AMPBlock's conv1) | + residual, fp32 state and planes
// (conv2) | + residual into the scaled, accumulated fp32 output, no activation (a resblock's last conv2)
enum TailEpi { TE_CONV1 = 0, TE_CONV2, TE_LAST };

struct ConvPlan {
  int kernel;          // ConvKernel
  int BM, BN;          // tile rows / columns
  int WGM, WGN, TPS;   // opconv_kernel: wave grid, taps per K step
  int kdeep, nstage;   // lin_plane_kernel: K depth of a stage, stages in flight; nconv_kernel: nstage = weight ring depth
  int64_t grid;        // workgroups of the conv launch (a K split's reduction is a second launch)
  int tiles_per_batch, tiles_n;
  int64_t tiles;       // output tiles (grid = tiles * ksplit, or the persistent kernels' workgroups walking them)
  int ksplit;          // 1 = none
  int n_major;         // wconv2 / wconv3 workgroup order: 1 = N-tile major
  bool vec, act, act3, geglu;
  // the tail convs: the template arguments of the instantiation (KMAX: tconv_kernel only, STG: tconv2_kernel only; 0
  // where the family has none), its epilogue form, threads per workgroup, column groups (N / NS) and the 16-B slots of
  // an LDS weight row (odd); BN = NS, tiles = B * tiles_per_batch * ncg
  int C, NS, NPB, R, KMAX, OCC, STG;
  int epi;             // TailEpi
  int block, ncg, wslots;
  char inst[96];       // the template-id in full but for the diagnostics flag, which the launch decides
  double flops, bytes;
  char name[160];      // the profile row: the demangled rocprofv3 name of the instantiation (bench.py joins by it)
  const char* err;     // the message of an ALCM_E_INVALID return
};

// 0 and *p, or ALCM_E_INVALID and p->err
int conv_plan(const alcm_opconv_args& a, int ncu, const Knobs& k, ConvPlan* p);
// the plans of alcm_opconv_sum: one CK_WCONV3_SUM launch, or n launches of conv_sum_term(a, i) in order;
// ALCM_E_INVALID with p[0].err
int conv_sum_plan(const alcm_opconv_args* a, int n, int ncu, const Knobs& k, ConvPlan p[3], int* launches);

// term i of a sum as the accumulating launch it is when the one-launch form does not apply
inline alcm_opconv_args conv_sum_term(const alcm_opconv_args* a, int i) {
  alcm_opconv_args g = a[i];
  g.out = a[0].out;
  g.out_scale = a[0].out_scale;
  g.accumulate = i > 0 ? 1 : a[0].accumulate;
  return g;
}

// alcm_opconv_dense (the BigVGAN stage 3-5 AMPBlock convs on dense K = tap * C + c weights): one CK_TCONV / CK_TCONV2
// launch; ALCM_E_INVALID with p->err
int dense_conv_plan(const alcm_opconv_args& a, int ncu, const Knobs& k, ConvPlan* p);
// whether the tail convs take this shape at this precision (ALCM_TCONV=0: none)
bool tconv_supported(const Knobs& k, int prec, int C, int N, int ksize, int dil);
// whether alcm_opconv can fuse Activation1d into its epilogue for N output channels at this precision
bool opconv_act_supported(int prec, int N, int Cp_in);

// K parts of a conv whose `tiles` fill the chip's `slots` badly: the smallest part count that cuts the rounds of
// items per part by more than 5 %, among the divisors k <= 8 of the `chunks` 64-channel chunks with >= 4 chunks per
// part whose k partial slices of `elems` floats fit the workspace; 1 = no split
int ksplit_parts(int64_t tiles, int64_t slots, int chunks, double elems, double ws_floats);

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the weight plane a single-plane kernel reads: planes of the packed weight are bf16 hi | bf16 lo | fp16 hi | fp16 lo,
// w_lo_off apart
inline const unsigned short* conv_wplane(const alcm_opconv_args& a) {
  const bool f16 = a.prec == ALCM_PREC_F16 || a.prec == ALCM_PREC_F16W2;
  return (const unsigned short*)a.w + (f16 ? 2 * a.w_lo_off : 0);
}

}  // namespace alcm
