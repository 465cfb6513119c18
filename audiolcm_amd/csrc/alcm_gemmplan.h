// Host-only planner of the fp32-operand GEMM / implicit-GEMM conv (alcm_gemm): validates a call and decides, once,
// which kernel instantiation of alcm_gemm.hip it gets, with which tile and grid, and under which profile name.  No HIP
// header and no device call: pointers are only tested for null-ness and alignment, never dereferenced.  The launcher
// (alcm_gemm.hip, launch_gemm) takes the plan and only launches.
#pragma once
#include <cstdint>

#include "audiolcm_hip.h"
#include "alcm_knobs.h"

namespace alcm {

// geometry the planner shares with the kernels
constexpr int BK = 32;        // K step of every kernel: Kpad is a multiple
constexpr int HALO_MAX = 64;  // conv_kernel: max (k - 1) * dil its LDS window holds beside the tile's rows
// gemm_skinny_kernel: columns / rows per workgroup, K and M limits
constexpr int SK_N = 32, SK_M = 32, SK_KMAX = 768, SK_MAXM = 1024;

enum GemmFamily { GF_NONE = 0, GF_WINDOW_CONV, GF_SKINNY, GF_GEMM };  // GF_NONE: M or N <= 0, nothing to launch
enum { BK_W = 0, BK_ACT = 1, BK_ACTT = 2 };                          // the B operand: packed weight, ACT, ACT_T

struct GemmPlan {
  int family;            // GemmFamily
  int BM, BN, WM, WN;    // tile and wave grid of conv_kernel / gemm_kernel (gemm_skinny_kernel: SK_M x SK_N, 0 waves)
  bool avec;             // A rows read as whole 16-byte vectors (gemm_kernel's AVEC)
  bool pro;              // conv_kernel: a prologue (norm / affine / SiLU) on the A operand
  int bkind, prec;       // BK_*, ALCM_PREC_*
  int gx, gy, gz;        // grid (256 threads per workgroup)
  int tpb, T_out, nbatch;  // conv_kernel: row tiles per clip, output rows per clip, clips
  double flops, bytes;   // algorithmic cost of the launch; 0 unless want_profile
  char name[128];        // the profile row: the demangled rocprofv3 name of the instantiation; empty unless want_profile
  const char* err;       // the message of an ALCM_E_INVALID return
};

// 0 and *p, or ALCM_E_INVALID and p->err.  want_profile: also the cost and the profile row (the hot path formats no
// string)
int gemm_plan(const alcm_gemm_args& g, const Knobs& k, bool want_profile, GemmPlan* p);

}  // namespace alcm
