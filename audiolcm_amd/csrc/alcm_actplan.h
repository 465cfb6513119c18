// Host-only planner of Activation1d on operand planes (alcm_activation1d_op and its fp16-input and three-set forms):
// validates a call and decides, once, which kernel instantiation of alcm_act.hip it gets, with which grid and kernel
// scalars, and under which profile name.  Same rules as alcm_gemmplan.h: no HIP header and no device call, pointers
// are only tested for null-ness and alignment, never dereferenced.  The launcher (alcm_act.hip, activation1d_planes)
// takes the plan and only launches; the BigVGAN stage planner (alcm_vocplan.cpp) asks act_kernel_for for the same
// choice without pointers.
#pragma once
#include <cstdint>

#include "audiolcm_hip.h"
#include "alcm_knobs.h"

namespace alcm {

// geometry the planner shares with the kernels
constexpr int AC_ELEMS = 2048;  // act_coop_kernel: a tile is NP channel pairs x AC_ELEMS / NP output rows
constexpr int AM_TILE = 64;     // act_mfma_kernel / act_mfma3_kernel: output rows of a wave tile (their TT)
constexpr int AM_STRIP = 8;     // wave tiles per workgroup strip (the tap fragments are built once per strip)

enum ActKernel { AK_COOP = 0, AK_MFMA, AK_MFMA3 };  // act_coop_kernel (VALU FIRs), act_mfma_kernel, act_mfma3_kernel

struct ActPlan {
  int kernel;             // ActKernel
  // template parameters: PREC of the planes written (F16W2 planes are F16 planes); coop: NP channel pairs per tile
  // (16 / 32) and NSET; mfma: DEFER (a tile's stores issued one tile late) and IN16 (x is an fp16 plane)
  int prec, np, nset;
  bool defer, in16;
  int64_t grid;           // workgroups (256 threads each)
  int tiles_t, tiles_c;   // coop: row tiles of a clip; every kernel: channel tiles
  int strips_t;           // mfma / mfma3: strips of AM_STRIP wave tiles of a clip
  int64_t y_lo;           // coop: elements from the hi plane to the lo plane of a SPLIT output
  double flops, bytes;    // algorithmic cost of the launch; 0 unless want_profile
  char name[64];          // the profile row; empty unless want_profile
  const char* err;        // the message of an ALCM_E_INVALID return
};

// The kernel a call of nset parameter sets on C channels (planes Cp wide) at prec gets when its pointers are 16-byte
// aligned: both FIRs on MFMA for fp16 planes of whole 64-channel tiles (ALCM_ACT_MFMA=0: never; the three-set form only
// under ALCM_ACT_X3_MFMA), else the VALU kernel.  -1: an fp16-input call outside the MFMA kernel's shapes (refused)
int act_kernel_for(const Knobs& k, int nset, int C, int Cp, int prec, bool x_is_f16);

// 0 and *p, or ALCM_E_INVALID and p->err.  want_profile: also the cost and the profile row (the hot path formats no
// string)
int act_plan(const alcm_act_args& a, const Knobs& k, bool want_profile, ActPlan* p);

}  // namespace alcm
