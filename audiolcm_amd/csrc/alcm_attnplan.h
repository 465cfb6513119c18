// Host-only planner of the fused attention (alcm_flash_attention / alcm_flash_attention_ex): validates a call and
// decides, once, which kernel of alcm_attn.hip it gets — the resident-K/V kernel on operand rows or on fp32 rows, or the
// tiled kernel — with which grid, scale and profile name.  Same rules as alcm_gemmplan.h: no HIP header and no device
// call, pointers are only tested for null-ness and alignment, never dereferenced.  The launcher (alcm_attn.hip,
// flash_attention) takes the plan and only launches; the DiT and text forwards ask attn_form_for for the same choice
// without pointers.
#pragma once
#include <cstdint>

#include "audiolcm_hip.h"
#include "alcm_knobs.h"

namespace alcm {

// geometry the planner shares with the kernels
constexpr int FA_Q = 64;          // flash_attn_kernel: queries per workgroup (256 threads)
constexpr int FA_KT = 64;         // keys per tile
constexpr int FR_MAXL = 512;      // flash_attn_res_kernel: most keys (padded to a multiple of FA_KT) its LDS holds
constexpr int FR_MAXDH = 72;      // largest head dim of either kernel
constexpr int FR_THREADS = 1024;  // 16 waves: 4 per SIMD hide the per-tile softmax / LDS latency chain

// resident on operand rows, resident on fp32 rows, tiled; attn_form_for's refusals: a shape no kernel takes (sizes,
// head dim, precision), or one only the resident kernel would take, beyond its length
enum AttnForm { AF_INVALID = -2, AF_NONE = -1, AF_RES_PLANE = 0, AF_RES_F32, AF_TILED };

// The form a call gets by its shape alone: B clips of L positions, H channels in `heads` heads at prec, q / k / v given
// as operand rows (plane) or fp32 rows, with a score bias, with an explicit scale.  The one statement of the rule:
// attn_plan decides through it, and the model forwards (alcm_models.cpp) ask it, without pointers, which stage may
// feed the attention.  A refusal (< 0) leaves its message in *why
int attn_form_for(const Knobs& k, int prec, int B, int L, int H, int heads, bool plane, bool bias, bool scale,
                  const char** why = nullptr);

struct AttnPlan {
  int form;             // AttnForm
  int prec;             // template PREC: ALCM_PREC_F16 or ALCM_PREC_BF16
  bool bias;            // template BIAS (resident kernel)
  int Lp, dh;           // keys padded to a multiple of FA_KT; head dim
  float scale;          // the score scale: the caller's, or dh^-1/2
  int64_t grid;         // workgroups
  int block;            // threads per workgroup
  double flops, bytes;  // algorithmic cost of the launch; 0 unless want_profile
  char name[80];        // the profile row; empty unless want_profile
  const char* err;      // the message of an ALCM_E_INVALID return
};

// 0 and *p, or ALCM_E_INVALID and p->err.  want_profile: also the cost and the profile row
int attn_plan(const alcm_attn_args& a, const Knobs& k, bool want_profile, AttnPlan* p);

}  // namespace alcm
