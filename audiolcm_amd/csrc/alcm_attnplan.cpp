// The fused-attention planner (alcm_attnplan.h): one validator and one kernel choice for alcm_flash_attention(_ex).
// The score bias, an explicit scale and operand-row input are the resident kernel's alone (L <= FR_MAXL).
#include "alcm_attnplan.h"

#include <cmath>
#include <cstdio>

namespace alcm {

namespace {

const char* const kBadArgs = "flash_attention: bad args";

int fail(AttnPlan* p, const char* msg) {
  p->err = msg;
  return ALCM_E_INVALID;
}

int padded(int L) { return (L + FA_KT - 1) / FA_KT * FA_KT; }

}  // namespace

int attn_form_for(const Knobs&, int prec, int B, int L, int H, int nh, bool plane, bool bias, bool scale,
                  const char** why) {  // (no switch bears on it yet)
  const auto no = [&](int form, const char* msg) {
    if (why) *why = msg;
    return form;
  };
  if (B <= 0 || L <= 0 || nh <= 0 || H % nh) return no(AF_INVALID, kBadArgs);
  const int dh = H / nh;
  if (dh > FR_MAXDH || dh % 4 || H % 4) return no(AF_INVALID, "flash_attention: head dim must be <= 72, % 4");
  if (prec != ALCM_PREC_F16 && prec != ALCM_PREC_BF16) return no(AF_INVALID, "flash_attention: F16 or BF16 only");
  const int64_t heads = (int64_t)B * nh;
  // one workgroup per (clip, head), its K and V resident in LDS
  if (padded(L) <= FR_MAXL && heads < (1ll << 31)) return plane ? AF_RES_PLANE : AF_RES_F32;
  if (plane) return no(AF_NONE, "flash_attention: plane input only for L <= 512");
  if (bias || scale) return no(AF_NONE, "flash_attention: score bias / scale only for L <= 512");
  if ((int64_t)((L + FA_Q - 1) / FA_Q) * heads >= (1ll << 31)) return no(AF_NONE, "flash_attention: problem too large");
  return AF_TILED;
}

int attn_plan(const alcm_attn_args& a, const Knobs& k, bool want_profile, AttnPlan* p) {
  *p = AttnPlan{};
  const int B = a.B, L = a.L, H = a.H, nh = a.heads;
  const bool plane = a.qkv_plane != nullptr;
  if ((a.qkv != nullptr) == plane || (!a.out && !a.out_plane)) return fail(p, kBadArgs);
  const char* why = nullptr;
  const int form = attn_form_for(k, a.prec, B, L, H, nh, plane, a.bias != nullptr, a.scale > 0.f, &why);
  if (form == AF_INVALID) return fail(p, why);
  if (!plane && (((uintptr_t)a.qkv) & 15)) return fail(p, "flash_attention: qkv must be 16-byte aligned");
  if (plane && (((uintptr_t)a.qkv_plane) & 7)) return fail(p, "flash_attention: qkv_plane must be 8-byte aligned");
  if (a.bias && a.bld < L) return fail(p, "flash_attention: bias pitch < L");
  if (form == AF_NONE) return fail(p, why);
  const int dh = H / nh;
  const int64_t heads = (int64_t)B * nh;
  p->form = form;
  p->prec = a.prec;
  p->bias = a.bias != nullptr;
  p->dh = dh;
  p->scale = a.scale > 0.f ? a.scale : 1.0f / std::sqrt((float)dh);
  p->Lp = padded(L);
  p->grid = form == AF_TILED ? (int64_t)((L + FA_Q - 1) / FA_Q) * heads : heads;
  p->block = form == AF_TILED ? 256 : FR_THREADS;
  if (want_profile) {
    p->flops = (double)heads * 4.0 * L * (double)L * dh;
    p->bytes = plane ? (double)B * L * (3.0 * H * 2.0 + H * 2.0) : (double)B * L * (3.0 * H + H) * 4.0;
    if (form == AF_TILED) std::snprintf(p->name, sizeof(p->name), "alcm::flash_attn_kernel<%d>", a.prec);
    else
      std::snprintf(p->name, sizeof(p->name), "alcm::flash_attn_res_kernel<%d, %s, %s>", a.prec,
                    p->bias ? "true" : "false", plane ? "true" : "false");
  }
  return 0;
}

}  // namespace alcm
