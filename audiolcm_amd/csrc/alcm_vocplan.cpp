// The BigVGAN stage planner (alcm_vocplan.h).
#include "alcm_vocplan.h"

#include <cstring>

namespace alcm {

namespace {

constexpr int PREC_BF16 = ALCM_PREC_BF16, PREC_SPLIT = ALCM_PREC_SPLIT, PREC_F16 = ALCM_PREC_F16,
              PREC_F16W2 = ALCM_PREC_F16W2;

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// MFMA precision of the AMPBlock layers of stage si (scripts/precision_emulate.py):
// mixed policy: fp16 for the three wide stages (~96% of the BigVGAN FLOPs), fp16 activation x fp16 hi+lo
// weight for the narrow tail (the tail is sensitive to weight rounding, not to activation rounding);
// conv_post stays bf16x3 (bigvgan_forward)
int voc_prec(int policy, int si) {
  if (policy == ALCM_POLICY_BF16) return PREC_BF16;
  if (policy == ALCM_POLICY_SPLIT) return PREC_SPLIT;
  // stage 3 (C = 96, the costliest tail stage) tolerates fp16 weights: +1e-5 waveform rel-L2 emulated,
  // vs +2.5e-4 (stage 4) and +4.3e-4 (stage 5) (scripts/precision_emulate.py 96 tail)
  return si < 4 ? PREC_F16 : PREC_F16W2;
}

// the stage's upsampler runs on operand planes of its input (mixed policy: stages 0-3, +1.9e-4 waveform rel-L2
// emulated, scripts/precision_emulate.py 96 tail): a plane conv with a strided epilogue (the wide-layer kernel for
// N % 192 == 0, opconv_kernel for N <= 96) — the same eligibility opconv's strided paths check (the wide-layer kernel
// needs Cp % 64 == 0 and a tap window of at most 64 rows)
bool ups_planes_of(const VocStageShape& S, int prec) {
  const bool wide_ok = S.cout % 192 == 0 && S.cin % 64 == 0 && S.taps - 1 <= 64;
  return (prec == PREC_F16 || prec == PREC_BF16) && S.cin % 32 == 0 && (wide_ok || (S.cout <= 96 && S.cout % 4 == 0)) &&
         S.cpad == S.cin;
}

// the narrow stages' AMPBlock convs on the tail kernels (alcm_tconv.hip): every conv of the stage or none (its planes
// keep stale operand-padding channels, which only those kernels ignore)
bool stage_tconv(const VocStageShape& S, int prec, const Knobs& k) {
  if (S.nrb == 0 || !S.dense_weights) return false;
  for (int j = 0; j < S.nrb; ++j)
    for (int l = 0; l < S.ndil; ++l)
      if (!tconv_supported(k, prec, S.cout, S.cout, S.rb_k[j], S.dil[l])) return false;
  return true;
}

// whether alcm_opconv_sum closes the stage's three chains in its one-launch form with a plane output: the terms as
// the executor builds them (alcm_models.cpp plane_args), on placeholder pointers.  conv_sum_plan only tests pointers
// for null-ness and 16-byte alignment, and the real ones pass both: every workspace buffer lies a multiple of 256
// bytes behind the workspace base (Bump::take), every packed weight and bias is an allocation of its own, and a
// packed weight's kpad (k * Cp) and lo-plane offset (N * kpad) are multiples of 32.  (A workspace base that is not
// 16-byte aligned fails every conv of the forward with ALCM_E_INVALID, whatever is planned here.)
bool sum_writes_planes(const VocStageShape& S, int prec, int B, int To, int ncu, const Knobs& k) {
  void* const some = (void*)(uintptr_t)256;
  const int Cp = round_up(S.cout, 32);
  alcm_opconv_args t[3];
  std::memset(t, 0, sizeof(t));
  for (int j = 0; j < 3; ++j) {
    alcm_opconv_args& g = t[j];
    g.a = some; g.a_lo_off = (int64_t)B * To * Cp;
    g.B = B; g.T = To; g.C = S.cout; g.Cp = Cp;
    g.ksize = S.rb_k[j]; g.dil = 1; g.pad = (S.rb_k[j] - 1) / 2;
    g.w = some; g.kpad = round_up(S.rb_k[j] * Cp, 32); g.w_lo_off = (int64_t)S.cout * g.kpad; g.N = S.cout;
    g.bias = (const float*)some; g.res = (const float*)some;
    g.out_scale = 1.f / 3.f; g.prec = prec;
  }
  t[0].out_plane = some;
  ConvPlan pl[3];
  int launches = 0;
  return conv_sum_plan(t, 3, ncu, k, pl, &launches) == 0 && pl[0].kernel == CK_WCONV3_SUM;
}

}  // namespace

bool ups2_supported(int cin, int cout, int cpad, int rate, int taps) {
  if (rate != 2 || taps != 2) return false;
  return (cin == 96 && cpad == 96 && cout == 48) || (cin == 48 && cpad == 48 && cout == 24);
}

int voc_plan(const VocStageShape* st, int n, int policy, bool streams, int B, int M, int ncu, const Knobs& k,
             VocStagePlan* out) {
  if (!st || !out || n < 0 || B <= 0 || M <= 0) return ALCM_E_INVALID;
  // the base precision of the fp32-operand convs (conv_pre, the phase-conv upsamplers)
  const int split = policy == ALCM_POLICY_BF16 ? PREC_BF16 : PREC_SPLIT;
  int To = M;
  for (int si = 0; si < n; ++si) {
    const VocStageShape& S = st[si];
    if (S.nrb < 0 || S.nrb > ALCM_VOC_MAX_RB || S.ndil < 0 || S.ndil > ALCM_VOC_MAX_DIL) return ALCM_E_INVALID;
    To *= S.rate;
    VocStagePlan p;
    std::memset(&p, 0, sizeof(p));
    p.prec = voc_prec(policy, si);
    const int Cp = round_up(S.cout, 32);
    // ConvTranspose1d as S.rate phase convs (models.py:160-165, 187-188): on operand planes of the input where
    // ups_planes_of; else the split-precision stride-2 stages with the kernel's widths (stages 4-5) take both phases
    // in one pass over x; else the fp32-operand conv at the base precision
    if (ups_planes_of(S, p.prec)) p.ups = VU_PLANES;
    else if (split == PREC_SPLIT && S.rate == 2 && ups2_supported(S.cin, S.cout, S.cpad, S.rate, S.taps) && S.phases_share)
      p.ups = VU_UPS2;
    else p.ups = VU_PHASES;
    p.planes_from_prev = si > 0 && out[si - 1].writes_next;
    // fused: every stage whose width opconv's Activation1d epilogue supports at this precision; on the dense weights
    // where the tail kernels take every conv of the stage
    const bool fuse = opconv_act_supported(p.prec, S.cout, Cp);
    p.amp = !fuse ? VA_WIDE : stage_tconv(S, p.prec, k) ? VA_FUSED_DENSE : VA_FUSED;
    p.concurrent = streams && S.nrb <= 3;
    // the wide stages' conv1 -> Activation1d hand-off as an fp16 plane (ALCM_CONV1_H16=0: fp32, the A/B reference).
    // Only from B * To >= 1024 rows, where the fp32 route takes the same wide kernel (below it the fp32 output would
    // go to opconv_kernel, whose K order differs): the A/B stays bit-exact at every size
    // (which kernel an Activation1d launch of the stage gets is act_plan's choice, asked here without pointers: the
    // workspace buffers it will see are 256-byte aligned.  The fp16-input form exists on the MFMA-FIR kernel only)
    const auto act_kernel = [&](int nset, bool x16) { return act_kernel_for(k, nset, S.cout, Cp, p.prec, x16); };
    p.h16 = !fuse && k.conv1_h16 && act_kernel(1, true) == AK_MFMA && (int64_t)B * To >= 1024;
    // the three chains' first Activation1d in one pass over the upsampler output (their own planes, the same taps):
    // the narrow fused stages on the VALU kernel, the wide MFMA-FIR stages on its three-set form (ALCM_ACT_X3_MFMA)
    p.act3 = S.nrb == 3 && (fuse ? act_kernel(1, false) == AK_COOP : act_kernel(3, false) == AK_MFMA3) && S.act0_equal;
    // each chain on its own buffers when the chains run concurrently, and when act3 wrote three sets of planes (so the
    // serialised profile pass runs the same kernels as the concurrent one)
    p.own_bufs = p.concurrent || p.act3;
    // the wide stages' mean over the three chains in one alcm_opconv_sum call of their last conv2 + residual: the
    // output written once, not read and rewritten per chain (ALCM_WCONV_SUM=0: three accumulating launches, the
    // chains' last convs in order)
    p.sum3 = !fuse && S.nrb == 3 && p.own_bufs && k.wconv_sum;
    // the next stage's upsampler reads only the operand planes of this output: the one-launch sum form writes them
    // (the rounding to_planes applies to the fp32 value, bit for bit) instead of the fp32 output
    p.writes_next = p.sum3 && k.wconv_sum == 1 && si + 1 < n && voc_prec(policy, si + 1) == p.prec &&
                    ups_planes_of(st[si + 1], p.prec) && st[si + 1].cin == S.cout &&
                    sum_writes_planes(S, p.prec, B, To, ncu, k);
    out[si] = p;
  }
  return 0;
}

}  // namespace alcm
