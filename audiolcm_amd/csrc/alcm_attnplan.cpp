// The fused-attention planner (alcm_attnplan.h): one validator and one kernel choice for alcm_flash_attention(_ex).
// The score bias, an explicit scale and operand-row input are the resident kernel's alone (L <= FR_MAXL).
#include "alcm_attnplan.h"

#include <cmath>
#include <cstdio>

namespace alcm {

namespace {

int fail(AttnPlan* p, const char* msg) {
  p->err = msg;
  return ALCM_E_INVALID;
}

}  // namespace

int attn_plan(const alcm_attn_args& a, const Knobs&, bool want_profile, AttnPlan* p) {  // (no switch bears on it yet)
  *p = AttnPlan{};
  const int B = a.B, L = a.L, H = a.H, nh = a.heads;
  const bool plane = a.qkv_plane != nullptr;
  if ((a.qkv != nullptr) == plane || (!a.out && !a.out_plane) || B <= 0 || L <= 0 || nh <= 0 || H % nh)
    return fail(p, "flash_attention: bad args");
  const int dh = H / nh;
  if (dh > FR_MAXDH || dh % 4 || H % 4) return fail(p, "flash_attention: head dim must be <= 72, % 4");
  if (a.prec != ALCM_PREC_F16 && a.prec != ALCM_PREC_BF16) return fail(p, "flash_attention: F16 or BF16 only");
  if (!plane && (((uintptr_t)a.qkv) & 15)) return fail(p, "flash_attention: qkv must be 16-byte aligned");
  if (plane && (((uintptr_t)a.qkv_plane) & 7)) return fail(p, "flash_attention: qkv_plane must be 8-byte aligned");
  if (a.bias && a.bld < L) return fail(p, "flash_attention: bias pitch < L");
  p->prec = a.prec;
  p->bias = a.bias != nullptr;
  p->dh = dh;
  p->scale = a.scale > 0.f ? a.scale : 1.0f / std::sqrt((float)dh);
  p->Lp = (L + FA_KT - 1) / FA_KT * FA_KT;
  const int64_t heads = (int64_t)B * nh;
  if (p->Lp <= FR_MAXL && heads < (1ll << 31)) {  // one workgroup per (clip, head), its K and V resident in LDS
    p->form = plane ? AF_RES_PLANE : AF_RES_F32;
    p->grid = heads;
    p->block = FR_THREADS;
  } else {
    if (plane) return fail(p, "flash_attention: plane input only for L <= 512");
    if (a.bias || a.scale > 0.f) return fail(p, "flash_attention: score bias / scale only for L <= 512");
    p->form = AF_TILED;
    p->grid = (int64_t)((L + FA_Q - 1) / FA_Q) * heads;
    p->block = 256;
    if (p->grid >= (1ll << 31)) return fail(p, "flash_attention: problem too large");
  }
  if (want_profile) {
    p->flops = (double)heads * 4.0 * L * (double)L * dh;
    p->bytes = plane ? (double)B * L * (3.0 * H * 2.0 + H * 2.0) : (double)B * L * (3.0 * H + H) * 4.0;
    if (p->form == AF_TILED) std::snprintf(p->name, sizeof(p->name), "alcm::flash_attn_kernel<%d>", a.prec);
    else
      std::snprintf(p->name, sizeof(p->name), "alcm::flash_attn_res_kernel<%d, %s, %s>", a.prec,
                    p->bias ? "true" : "false", plane ? "true" : "false");
  }
  return 0;
}

}  // namespace alcm
