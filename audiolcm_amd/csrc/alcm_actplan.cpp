// The Activation1d-on-planes planner (alcm_actplan.h): one validator and one kernel choice for alcm_activation1d_op,
// alcm_activation1d_op_f16in and the three-set form.
#include "alcm_actplan.h"

#include <cstdio>

namespace alcm {

namespace {

constexpr int PREC_BF16 = ALCM_PREC_BF16, PREC_SPLIT = ALCM_PREC_SPLIT, PREC_F16 = ALCM_PREC_F16,
              PREC_F16W2 = ALCM_PREC_F16W2;

int fail(ActPlan* p, const char* msg) {
  p->err = msg;
  return ALCM_E_INVALID;
}

inline bool misaligned(const void* q, int mask) { return (((uintptr_t)q) & mask) != 0; }

// the checks every form shares, in the order of alcm_activation1d_op
const char* validate(const alcm_act_args& a) {
  if (!a.x || (a.nset != 1 && a.nset != 3) || !a.up_filter || !a.down_filter || a.B <= 0 || a.T <= 0 || a.C <= 0)
    return "activation1d_op: bad arguments";
  for (int i = 0; i < a.nset; ++i)
    if (!a.y[i] || !a.alpha_exp[i] || !a.inv_beta[i]) return "activation1d_op: bad arguments";
  if (a.Cp < a.C || a.Cp % 32) return "activation1d_op: Cp must be >= C and a multiple of 32";
  if (a.C % 2) return "activation1d_op: C must be even";
  if (a.prec < PREC_BF16 || a.prec > PREC_F16W2) return "activation1d_op: bad prec";
  // what the VALU kernel's 8-byte loads and 4-byte stores need (the MFMA kernels' 16 bytes: act_plan)
  if (misaligned(a.x, 7)) return "activation1d_op: alignment";
  for (int i = 0; i < a.nset; ++i)
    if (misaligned(a.y[i], 3)) return "activation1d_op: alignment";
  if ((int64_t)a.B * a.T * a.Cp >= (1ll << 40)) return "activation1d_op: problem too large";
  return nullptr;
}

}  // namespace

int act_kernel_for(const Knobs& k, int nset, int C, int Cp, int prec, bool x_is_f16) {
  const bool mfma = k.act_mfma && prec == PREC_F16 && C >= 192 && C % 64 == 0 && Cp == C;
  if (x_is_f16) return mfma && nset == 1 ? AK_MFMA : -1;  // the VALU kernel reads fp32 only
  if (!mfma) return AK_COOP;
  if (nset == 1) return AK_MFMA;
  return k.act_x3_mfma ? AK_MFMA3 : AK_COOP;
}

int act_plan(const alcm_act_args& a, const Knobs& k, bool want_profile, ActPlan* p) {
  *p = ActPlan{};
  if (const char* e = validate(a)) return fail(p, e);
  const int B = a.B, T = a.T, C = a.C, Cp = a.Cp;
  const bool in16 = a.x_is_f16 != 0;
  int kernel = act_kernel_for(k, a.nset, C, Cp, a.prec, in16);
  // the MFMA kernels move whole 16-byte pieces.  An fp32-input call off that alignment takes the VALU kernel (what the
  // public entry has always done; the models' workspace buffers are 256-byte aligned)
  bool al16 = !misaligned(a.x, 15);
  for (int i = 0; i < a.nset; ++i) al16 = al16 && !misaligned(a.y[i], 15);
  if (kernel != AK_COOP && !al16) kernel = in16 ? -1 : AK_COOP;
  if (kernel < 0)
    return fail(p, "activation1d_op_f16in: needs prec F16, C >= 192, C % 64 == 0, Cp == C and 16-byte aligned x / y");
  p->kernel = kernel;
  p->nset = a.nset;
  if (kernel == AK_COOP) {
    // 64-channel tiles (whole 128-B output lines) measured faster at C = 768 (-15 %) and for the two-plane split
    // output (-10 %), slower at C = 384 (+10..15 %), even at C = 192 fp16 (scripts/microbench.py actnp)
    const bool wide = Cp % 64 == 0 && (C >= 768 || a.prec == PREC_SPLIT);
    p->np = wide ? 32 : 16;
    const int tt = AC_ELEMS / p->np;
    p->prec = a.prec == PREC_F16W2 ? PREC_F16 : a.prec;
    p->tiles_t = (T + tt - 1) / tt;
    p->tiles_c = Cp / (2 * p->np);
    p->grid = (int64_t)B * p->tiles_t * p->tiles_c;
    p->y_lo = (int64_t)B * T * Cp;
    if (p->grid >= (1ll << 31)) return fail(p, "activation1d_op: problem too large");
  } else {
    p->prec = PREC_F16;
    p->defer = kernel == AK_MFMA && k.act_defer;  // (the three-set kernel stores each set's tile at once)
    p->in16 = in16;
    p->tiles_c = C / 64;
    p->strips_t = ((T + AM_TILE - 1) / AM_TILE + AM_STRIP - 1) / AM_STRIP;
    p->grid = (int64_t)B * p->strips_t * p->tiles_c;
    if (p->grid >= (1ll << 31) || (int64_t)T * C >= (1ll << 31)) return fail(p, "activation1d_op: problem too large");
  }
  if (want_profile) {
    const double e = (double)B * T;
    p->flops = a.nset * 2.0 * 36.0 * e * C;
    p->bytes = e * ((in16 ? 2.0 : 4.0) * C + a.nset * 2.0 * Cp * (a.prec == PREC_SPLIT ? 2 : 1));
    if (kernel == AK_COOP)
      std::snprintf(p->name, sizeof(p->name), "alcm::act_coop_kernel<%d>%s", p->prec, a.nset == 3 ? ", x3" : "");
    else if (kernel == AK_MFMA3)
      std::snprintf(p->name, sizeof(p->name), "alcm::act_mfma3_kernel<%d>", AM_TILE);
    else
      std::snprintf(p->name, sizeof(p->name), "alcm::act_mfma_kernel<%d, %s, %s>", AM_TILE, p->defer ? "true" : "false",
                    in16 ? "true" : "false");
  }
  return 0;
}

}  // namespace alcm
