"""Every operand, prologue and epilogue form of alcm_gemm (audiolcm_amd/csrc/alcm_gemm.hip) on each of its 51
instantiations against the float64 restatement of tests/_gemm_ref.py, which tests/test_gemm_forms_host.py pins against
torch and whose case table it shows to reach exactly those instantiations.

Per case and precision: the kernel that ran is the one the table names (the plan, and the one profile row); relative L2
against the unrounded float64 reference is under the bounds of test_gpu_ops.py (split 2e-5, bf16 1.5e-2, fp16 2e-3);
without a prologue, against the reference on operands rounded to bf16 / fp16 it is under the split bound as well (both
sides then hold the same operands and only the fp32 accumulation is left); with a prologue (computed in fp32 before the
rounding, so a few operands flip by one unit) the per-precision bound holds over the whole output and over the rows
that touch the padding alone; every element of the output buffer that the call does not store (guards, pitch and
phase gaps) keeps its bits, and the inputs are unchanged.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R
from conftest import rel_l2
from test_vocplan import switches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


def run_case(K, c, prec, errs, **patch):
    """One device call of a case; the checks every case shares.  Returns the output buffer (float32)."""
    from audiolcm_amd import _hip
    d, t = R.case_data(c["name"])
    if patch:
        d = dict(d, **patch)
    want = c["kernel"].format(p=prec) if not patch else None
    with switches(c["sw"]):
        out, plan, rows = R.run_device(K, _hip, d, t, prec)
    if want:
        assert plan["name"] == want, (c["name"], plan["name"])
    assert [(r["name"], r["launches"]) for r in rows] == [(plan["name"], 1)], rows
    true = R.reference(c["name"])
    w = true.written
    prior = t["out"]
    assert np.array_equal(out.view(np.int32)[~w], prior.view(np.int32)[~w]), f"{c['name']}: guard / gap overwritten"
    assert np.isfinite(out[w]).all()
    e_true = rel_l2(out[w], true.out[w])
    msg = f"{c['name']} prec {prec} {plan['name']}: vs float64 {e_true:.2e}"
    errs["true"] = max(errs.get("true", 0.0), e_true)
    bad = []
    if e_true >= R.TOL[prec]:
        bad.append(("float64", e_true))
    if R.has_prologue(d):
        e_edge = rel_l2(out[true.edge], true.out[true.edge])
        errs["edge"] = max(errs.get("edge", 0.0), e_edge)
        msg += f", edge rows {e_edge:.2e}"
        if e_edge >= R.TOL[prec]:
            bad.append(("edge rows", e_edge))
    elif R.ROUND[prec]:
        rnd = R.reference(c["name"], R.ROUND[prec])
        e_rnd = rel_l2(out[w], rnd.out[w])
        errs["rounded"] = max(errs.get("rounded", 0.0), e_rnd)
        msg += f", vs rounded operands {e_rnd:.2e}"
        if e_rnd >= R.SPLIT_TOL:
            bad.append(("rounded operands", e_rnd))
    print(msg)
    assert not bad, (c["name"], prec, bad)
    return out


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_gemm_forms(K, family, prec):
    cases = [c for c in R.CASES if c["family"] == family]
    errs, outs = {}, {}
    for c in cases:
        outs[c["name"]] = run_case(K, c, prec, errs)
    print(f"family {family} prec {prec}: kernels {sorted({c['kernel'].format(p=prec)[6:] for c in cases})}; largest " +
          ", ".join(f"{k} {v:.2e}" for k, v in sorted(errs.items())))

    for c in cases:
        w = R.reference(c["name"]).written
        if c.get("window_pair"):     # the same call on the tap-by-tap loader: test_window_conv_matches_tap_loader's bound
            y2 = run_case(K, c, prec, {}, disable_window=1)
            e = rel_l2(outs[c["name"]][w], y2[w])
            print(f"{c['name']} prec {prec}: window conv vs tap loader {e:.2e}")
            assert e < (1e-6 if prec == 1 else 1e-5)
        if c.get("skinny_pair"):     # the skinny kernel vs the MFMA tiles: test_gemm_skinny_rows's bound
            e = rel_l2(outs[c["name"]][w], outs[c["name"] + "_noskinny"][w])
            print(f"{c['name']} prec {prec}: skinny vs MFMA tiles {e:.2e}")
            assert e < 2 * (1e-5 if prec == 1 else 1e-2)

    if family == 7:   # every phase left the other phases' samples alone (run_case); together: F.conv_transpose1d
        for k, s in sorted({c["convT"][:2] for c in cases}):
            ph = [c for c in cases if c["convT"][:2] == (k, s)]
            d, t = R.case_data(ph[0]["name"])
            full = np.full(t["out"].size, np.nan)
            for c in ph:
                w = R.reference(c["name"]).written
                assert np.isnan(full[w]).all()
                full[w] = outs[c["name"]][w]
            B, N, To = d["M"] // d["out_rows_per_batch"], d["N"], d["out_rows_per_batch"] * s
            idx = (d["out_base"] + np.arange(B)[:, None, None] * d["o_sb"] + np.arange(N)[None, :, None] * d["o_sc"] +
                   np.arange(To)[None, None, :] * d["o_st"])
            assert np.isfinite(full).sum() == idx.size
            x = torch.tensor(t["a"]).double().reshape(B, d["a"]["C_in"], d["a"]["T_in"])
            ref = F.conv_transpose1d(x, torch.tensor(t["wT"]).double().reshape(d["wT_shape"]),
                                     torch.tensor(t["bias"]).double(), stride=s, padding=(k - s) // 2)
            e = rel_l2(full[idx], ref.numpy())
            print(f"conv_transpose1d k{k} s{s} prec {prec}: all phases vs F.conv_transpose1d {e:.2e}")
            assert e < R.TOL[prec]
