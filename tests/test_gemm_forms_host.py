"""The float64 restatement of alcm_gemm (tests/_gemm_ref.py) and its case table, checked without a device.

(a) The evaluator against torch in float64: F.conv1d with dilation and padding, nearest x2 + conv, F.conv_transpose1d
assembled from its phases, GroupNorm / LayerNorm + SiLU + conv through the prologue, and the two attention products on a
packed qkv buffer by einsum.  (b) The case table of tests/test_gpu_gemm_forms.py reaches, by the planner
(alcm_debug_gemm_plan), exactly the instantiations tests/data/gemm_plans.json names, each case the one it expects.
(c) On each case's data, every meaningful mutation of the evaluator (_gemm_ref.MUTANTS) moves the output by more than
the tolerance the GPU test applies to that case, so a kernel wrong in that way would fail there.
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R
from conftest import rel_l2
from audiolcm_amd import kernels as K
from test_gemmplan import TABLE
from test_vocplan import switches


def dense(d, r):
    """The stored elements of a result as [z][m][column]."""
    return r.out[R.out_index(d)]


def res_dense(d, t):
    return t["res"].astype(np.float64)[R.res_index(d)]


def as_bct(d, y, B):
    """[1][B*T][N] -> (B, N, T) as torch."""
    return torch.tensor(y[0].reshape(B, -1, d["N"]).transpose(0, 2, 1).copy())


def x_bct(d, t, B):
    a = d["a"]
    idx = (np.arange(B)[:, None, None] * a["sb"] + np.arange(a["C_in"])[None, :, None] * a["sc"] +
           np.arange(a["T_in"])[None, None, :] * a["st"])
    return torch.tensor(t["a"].astype(np.float64)[idx])


def agree(y, ref):
    e = rel_l2(np.asarray(y), np.asarray(ref))
    assert e < 1e-12, e


@pytest.mark.parametrize("nct", [False, True])
@pytest.mark.parametrize("k,dil,pad", [(5, 2, 4), (3, 1, 0), (7, 3, 11), (1, 1, 0)])
def test_evaluator_is_conv1d(nct, k, dil, pad):
    B, T_in, C, N = 2, 23, 12, 9
    T = T_in + 2 * pad - dil * (k - 1)
    d, t = R.conv_case(B, T, C, N, k, dil=dil, pad=pad, nct=nct, a_pitch=0 if nct else 3, out_nct=nct, seed=1)
    d["a"]["T_in"] = T_in            # (conv_case lays out same-length convs: restate the input for T != T_in)
    d["a"].update(dict(sb=C * T_in, sc=T_in) if nct else dict(sb=T_in * (C + 3)))
    t["a"] = R._randn((B * d["a"]["sb"],), 2)
    ref = F.conv1d(x_bct(d, t, B), torch.tensor(t["w"]).double(), torch.tensor(t["bias"]).double(), padding=pad,
                   dilation=dil)
    agree(as_bct(d, dense(d, R.evaluate(d, t)), B), ref)


def test_evaluator_is_nearest_x2_then_conv1d():
    B, T, C, N = 2, 26, 16, 10
    d, t = R.conv_case(B, T, C, N, 3, up=2, seed=3)
    xu = F.interpolate(x_bct(d, t, B), scale_factor=2.0, mode="nearest")
    ref = F.conv1d(xu, torch.tensor(t["w"]).double(), torch.tensor(t["bias"]).double(), padding=1)
    agree(as_bct(d, dense(d, R.evaluate(d, t)), B), ref)


@pytest.mark.parametrize("k,s", [(8, 4), (4, 2), (6, 2)])
def test_evaluator_phases_are_conv_transpose1d(k, s):
    B, T, Cin, N = 2, 13, 12, 6
    full, seen = None, None
    for r in range(s):
        d, t = R.transpose_phase_case(B, T, Cin, N, k, s, r, 5)
        res = R.evaluate(d, t)
        full = res.out.copy() if full is None else np.where(res.written, res.out, full)
        assert seen is None or not (seen & res.written).any()
        seen = res.written if seen is None else seen | res.written
    idx = (d["out_base"] + np.arange(B)[:, None, None] * d["o_sb"] + np.arange(N)[None, :, None] * d["o_sc"] +
           np.arange(T * s)[None, None, :] * d["o_st"])
    assert seen.sum() == idx.size and seen[idx].all()
    wT = torch.tensor(t["wT"]).double().reshape(d["wT_shape"])
    ref = F.conv_transpose1d(x_bct(d, t, B), wT, torch.tensor(t["bias"]).double(), stride=s, padding=(k - s) // 2)
    agree(full[idx], ref)


def test_evaluator_is_group_norm_silu_conv1d():
    B, T, C, N, groups = 2, 19, 16, 7, 4
    d, t = R.conv_case(B, T, C, N, 3, pro="affine", shift=1.0, seed=7)
    x = x_bct(d, t, B)
    gam, bet = torch.tensor(R._randn((C,), 8, 0.3, 1.0)).double(), torch.tensor(R._randn((C,), 9, 0.3)).double()
    xg = x.reshape(B, groups, -1)
    mean, rstd = xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-6).rsqrt()
    scale = gam[None, :] * rstd.repeat_interleave(C // groups, 1)
    shift = bet[None, :] - mean.repeat_interleave(C // groups, 1) * scale
    t = dict(t, pro_scale=scale.reshape(-1).numpy(), pro_shift=shift.reshape(-1).numpy())
    ref = F.conv1d(F.silu(F.group_norm(x, groups, gam, bet, 1e-6)), torch.tensor(t["w"]).double(),
                   torch.tensor(t["bias"]).double(), padding=1)
    agree(as_bct(d, dense(d, R.evaluate(d, t)), B), ref)


def test_evaluator_is_layer_norm_silu_conv1d():
    B, T, C, N = 2, 19, 12, 7
    d, t = R.conv_case(B, T, C, N, 9, pro="ln", x_offset=5.0, seed=10)
    d["a"]["pro_act"] = 1
    x = x_bct(d, t, B)
    xt = x.permute(0, 2, 1)
    t = dict(t, pro_mean=xt.mean(-1).reshape(-1).numpy(),
             pro_rstd=(xt.var(-1, unbiased=False) + 1e-5).rsqrt().reshape(-1).numpy())
    gam, bet = torch.tensor(t["pro_scale"]).double(), torch.tensor(t["pro_shift"]).double()
    h = F.silu(F.layer_norm(xt, (C,), gam, bet, 1e-5)).permute(0, 2, 1)
    ref = F.conv1d(h, torch.tensor(t["w"]).double(), torch.tensor(t["bias"]).double(), padding=4)
    agree(as_bct(d, dense(d, R.evaluate(d, t)), B), ref)


def test_evaluator_is_the_attention_einsums():
    B, L, nh, dh = 2, 11, 3, 8
    d, t = R.qk_case(B, L, nh, dh, 11)
    qkv = torch.tensor(t["a"]).double().reshape(B, L, 3, nh, dh)
    s = torch.einsum("bihd,bjhd->bhij", qkv[:, :, 0], qkv[:, :, 1]) * dh ** -0.5
    agree(dense(d, R.evaluate(d, t)), s.reshape(B * nh, L, L).numpy() + res_dense(d, t))
    d, t = R.pv_case(B, L, nh, dh, 12)
    Lp = d["a"]["Cpad"]
    p = torch.tensor(t["a"]).double().reshape(B, nh, L, Lp)[..., :L]
    v = torch.tensor(t["qkv"]).double().reshape(B, L, 3, nh, dh)[:, :, 2]
    o = torch.einsum("bhij,bjhd->bhid", p, v).reshape(B * nh, L, dh).numpy()
    agree(dense(d, R.evaluate(d, t)), o + t["out"].astype(np.float64)[R.out_index(d)])


def test_evaluator_epilogue_order_and_rounding():
    """out = ((act(acc*acc_scale + bias) + res) * out_scale) + prior, and operands rounded before the product."""
    d, t = R.conv_case(1, 9, 8, 6, 1, act=4, acc_scale=0.7, out_scale=0.5, accumulate=True, res="nct", seed=13)
    x = t["a"].astype(np.float64).reshape(9, 8)
    w = t["w"].astype(np.float64)[:, :, 0]
    prior = t["out"].astype(np.float64)[R.out_index(d)]
    for fmt, dt in ((None, None), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        xr, wr = (x, w) if dt is None else (torch.tensor(a).float().to(dt).double().numpy() for a in (x, w))
        ref = (np.tanh(xr @ wr.T * 0.7 + t["bias"].astype(np.float64)) + res_dense(d, t)[0]) * 0.5 + prior[0]
        agree(dense(d, R.evaluate(d, t, round_operands=fmt))[0], ref)
    # GEGLU: (wi_1, wi_0) interleaved, v_even * gelu(v_odd) -> column n / 2, act ignored
    d, t = R.conv_case(1, 9, 8, 6, 1, act=1, geglu=1, seed=14)
    x = t["a"].astype(np.float64).reshape(9, 8)
    v = torch.tensor(x @ t["w"].astype(np.float64)[:, :, 0].T + t["bias"].astype(np.float64))
    x2 = R.conv_case(1, 9, 8, 6, 1, act=1, geglu=2, seed=14)
    agree(dense(d, R.evaluate(d, t))[0], (v[:, 0::2] * F.gelu(v[:, 1::2])).numpy())
    agree(dense(x2[0], R.evaluate(*x2))[0], (v[:, 0::2] * F.gelu(v[:, 1::2], approximate="tanh")).numpy())


# ------------------------------------------------------------------ the case table reaches every instantiation
def planned_name(c, prec):
    d, t = R.case_data(c["name"])
    with switches(c["sw"]):
        return K.gemm_plan(R.gemm_args(d, R.fake_addresses(t), prec))["name"]


def test_cases_reach_every_recorded_instantiation():
    with open(TABLE) as f:
        recorded = set(json.load(f)["names"])
    assert len(recorded) == 51
    got, bad = set(), []
    for c in R.CASES:
        for prec in R.PRECS:
            name = planned_name(c, prec)
            got.add(name)
            if name != c["kernel"].format(p=prec):
                bad.append((c["name"], prec, name))
    assert not bad, bad
    assert got == recorded, (sorted(recorded - got), sorted(got - recorded))
    assert len({c["name"] for c in R.CASES}) == len(R.CASES)


def test_case_shapes_cross_the_tiles():
    """What the issue asks of the shapes, restated on the table: ragged N against the tile the case names, K padding,
    C_in < Cpad on the scalar loader, a pair-ending tile under GEGLU, guards and gaps round every output."""
    for c in R.CASES:
        d, t = R.case_data(c["name"])
        kern = c["kernel"]
        oi = R.out_index(d)
        assert oi.min() >= R.GUARD and t["out"].size - 1 - oi.max() >= R.GUARD
        assert np.unique(oi).size < oi.max() - oi.min() + 1 or d["M"] == 1, c["name"]     # gaps inside
        if d.get("accumulate"):
            assert np.abs(t["out"]).max() < 10
        else:
            assert (t["out"] == R.SENTINEL).all()
        if "gemm_kernel" in kern or "conv_kernel" in kern:
            bn = int(kern.split("<")[1].split(",")[1])
            assert d["N"] % bn or d.get("tile_n") or d["N"] in (64, 192, 128), c["name"]
        if d.get("geglu"):
            assert d["N"] % 2 == 0 and (d["N"] // 2) % 16 or d["N"] == 128   # (128: a pair ends each 64-wide tile)
        if "false, 0" in kern and "gemm_kernel" in kern and c["family"] != 10:
            assert d["a"]["C_in"] < d["a"]["Cpad"] or d["a"]["sc"] != 1
    d, _ = R.case_data("ln_k9_C20")
    assert d["a"]["C_in"] == 20 and d["a"]["Cpad"] == 24 and d["Kpad"] > 9 * 24
    for name in ("nct_k5d2_N24", "cl_k3_N20_act1", "affine_up2_C40", "geglu1_lin_N264", "skinny_M1_C36_N20_act0"):
        d, _ = R.case_data(name)
        assert d["Kpad"] > d["a"]["ksize"] * d["a"]["Cpad"], name


# ------------------------------------------------------------------ each case's data exposes each mistake
@pytest.mark.parametrize("family", R.FAMILIES)
def test_mutants_exceed_the_bound(family):
    """A reference wrong in one way differs from the true one by more than the bound of the GPU comparison that is
    meant to catch it: over the rows that touch the padding for the padding-row mutant, over the whole output otherwise."""
    low, seen = [], set()
    for c in (c for c in R.CASES if c["family"] == family):
        d, t = R.case_data(c["name"])
        true = R.reference(c["name"])
        tol = R.mutant_tolerance(d)
        for m in R.mutants_for(d, t):
            mut = R.evaluate(d, t, mutant=m)
            where = true.edge if m == "pro_pad_rows" else true.written
            e = rel_l2(mut.out[where], true.out[where])
            seen.add(m)
            low.append((e / tol, c["name"], m))
    low.sort()
    print(f"family {family}: mutants {sorted(seen)}; weakest (x the bound): {low[:3]}")
    assert low and low[0][0] > 1.0, [x for x in low if x[0] <= 1.0]


def test_every_mutant_is_applied_somewhere():
    seen = set()
    for c in R.CASES:
        seen.update(R.mutants_for(*R.case_data(c["name"])))
    assert seen == set(R.MUTANTS), set(R.MUTANTS) - seen
