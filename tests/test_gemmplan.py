"""The fp32-operand GEMM planner (audiolcm_amd/csrc/alcm_gemmplan.cpp): which kernel instantiation, grid and profile
row an alcm_gemm call gets, and which calls it rejects.

The CPU tests ask the library's diagnostics entry (alcm_debug_gemm_plan: nothing is launched, pointers are only tested
for null-ness and alignment) and compare with tests/data/gemm_plans.json.  The table was recorded from the build before
the planner existed: the host section of its alcm_gemm.hip (gemm(), fill_act and the launchers, unchanged) compiled for
the host with the kernel launches and prof_stop replaced by a record of the grid, the kernel arguments tpb / T_out, the
profile name and the cost, as was done for dense_plans.json.  A case is stored as one of the models' helper forms with
its parameters and a patch of fields (load_table), each recorded under ALCM_PROF_SHAPES off and on.  The cases are (a) for every gemm_kernel / conv_kernel /
gemm_skinny_kernel row of tests/data/model_launches.json a call in the argument form of the models' conv / lin / mha
helpers that the old dispatch gave exactly that row, (b) every family, tile, precision and switch, each condition of
the window conv and of the skinny kernel failing alone, and (c) every rejection message, with pairs of defects that pin
the order of the checks.  The last ten cases (the rows of model_launches.json's two cut-down configurations, dit_dh144
and text_dh96) were added later from the planner of commit 09c2a2d, checked against the rows the GPU recorded there.
The GPU tests check that a real call of each family records exactly the profile row the planner names and computes the
float64 restatement of the product.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import REPO, rel_l2

from audiolcm_amd import _hip
from audiolcm_amd import kernels as K
from test_vocplan import switches

TABLE = os.path.join(REPO, "tests", "data", "gemm_plans.json")
LAUNCHES = os.path.join(REPO, "tests", "data", "model_launches.json")
KNOB_ENV = {"gemm_skinny": "ALCM_GEMM_SKINNY", "prof_shapes": "ALCM_PROF_SHAPES"}
OPERAND_POINTERS = ("ptr", "pro_scale", "pro_shift", "pro_mean", "pro_rstd")
POINTERS = ("bias", "res", "out")
E_INVALID = -1
GEMM_ROW = r"alcm::(gemm_kernel|conv_kernel|gemm_skinny_kernel)<"


def row_args(d):
    """A table row's arguments as GemmArgs (a field the row leaves out is zero / NULL): a pointer field holds its
    recorded class (address & 15) on a made-up address of its own."""
    g = _hip.GemmArgs()
    n = 0
    for f, _ in _hip.GemmArgs._fields_:
        if f in ("a", "b"):
            o, od = getattr(g, f), d.get(f, {})
            for of, _ in _hip.Operand._fields_:
                if of in OPERAND_POINTERS:
                    n += 1
                    setattr(o, of, (n << 32) + od[of] if of in od else None)
                else:
                    setattr(o, of, od.get(of, 0))
        elif f in POINTERS:
            n += 1
            setattr(g, f, (n << 32) + d[f] if f in d else None)
        else:
            setattr(g, f, d.get(f, 0))
    return g


def _rup(x, m):
    return (x + m - 1) // m * m


# The argument forms of the models' launch helpers (alcm_models.cpp conv / lin / mha), as row dicts for row_args: a
# pointer field holds its address & 15, a field left out is zero / NULL.
def conv_form(B, T, C, N, k, prec, dil=1, up=1, cpad=None, pro=None, nct=False, res=False, **kw):
    """conv(): B clips of T output rows of a same-length conv, channels-last (or NCT) fp32 input, packed weight."""
    cpad = cpad or _rup(C, 8)
    T_in = T // up if up == 2 else T
    a = dict(kind=0, ptr=0, T_in=T_in, C_in=C, Cpad=cpad, ksize=k, dil=dil, pad=(k - 1) * dil // 2, up=up,
             rows_per_batch=T)
    a.update(dict(sb=C * T_in, st=1, sc=T_in) if nct else dict(sb=T_in * C, st=C, sc=1))
    if pro in ("affine", "affine_silu"):
        a.update(pro_scale=0, pro_shift=0, pro_sb=C)
    if pro == "ln":
        a.update(pro_mean=0, pro_rstd=0)
    if pro in ("silu", "affine_silu"):
        a.update(pro_act=1)
    kpad = _rup(k * cpad, 32)
    d = dict(M=B * T, N=N, Kpad=kpad, batch=1, zdiv=1, a=a, b=dict(kind=2, ptr=0, rows=N, w_lo_off=N * kpad),
             bias=0, acc_scale=1.0, out_scale=1.0, out=0, o_sb=T * N, o_st=N, o_sc=1, out_rows_per_batch=T, out_step=1,
             prec=prec)
    if res:
        d.update(res=0, r_sb=T * N, r_st=N, r_sc=1)
    d.update(kw)
    return d


def lin_form(R, C, N, prec, **kw):
    """lin(): R rows as one clip, k = 1."""
    d = conv_form(1, R, C, N, 1, prec, **kw)
    d["a"]["sb"] = d["o_sb"] = 0
    return d


def qk_form(B, L, nh, dh, prec):
    """mha()'s scores: q k^T per (clip, head) on the fused qkv buffer, B operand ACT."""
    I, Lp = nh * dh, _rup(L, 8)
    a = dict(kind=0, ptr=0, sb=0, st=3 * I, sc=1, T_in=L, C_in=dh, Cpad=dh, ksize=1, dil=1, up=1, rows_per_batch=L,
             zs1=L * 3 * I, zs2=dh)
    return dict(M=L, N=L, Kpad=_rup(dh, 32), batch=B * nh, zdiv=nh, a=a, b=dict(a), acc_scale=0.125, out_scale=1.0,
                out=0, o_st=Lp, o_sc=1, o_zs1=nh * L * Lp, o_zs2=L * Lp, out_rows_per_batch=L, out_step=1, prec=prec)


def pv_form(B, L, nh, dh, prec):
    """mha()'s output: P v, B operand ACT_T."""
    I, Lp = nh * dh, _rup(L, 8)
    a = dict(kind=0, ptr=0, sb=0, st=Lp, sc=1, T_in=L, C_in=Lp, Cpad=Lp, ksize=1, dil=1, up=1, rows_per_batch=L,
             zs1=nh * L * Lp, zs2=L * Lp)
    b = dict(kind=1, ptr=0, st=3 * I, sc=1, T_in=L, rows=dh, zs1=L * 3 * I, zs2=dh)
    return dict(M=L, N=dh, Kpad=_rup(Lp, 32), batch=B * nh, zdiv=nh, a=a, b=b, acc_scale=1.0, out_scale=1.0, out=0,
                o_st=I, o_sc=1, o_zs1=L * I, o_zs2=dh, out_rows_per_batch=L, out_step=1, prec=prec)


FORMS = {"conv": conv_form, "lin": lin_form, "qk": qk_form, "pv": pv_form}


def case_args(form, pos, kw, patch):
    """The row dict of a table case: a form with its parameters, then the patch ("a.T_in": 0 sets an operand field,
    null removes a pointer)."""
    d = FORMS[form](*pos, **kw)
    for key, v in patch.items():
        tgt, f = (d[key[0]], key[2:]) if key[:2] in ("a.", "b.") else (d, key)
        if v is None:
            tgt.pop(f)
        else:
            tgt[f] = v
    return d


def load_table():
    """The table as one row per (call, switches): args, knobs, rc, error, name, grid, flops, bytes (tpb, T_out for the
    window conv).  A case of the file is [form, parameters, keywords, patch, results], results one entry per recorded
    ALCM_GEMM_SKINNY value: [skinny, -1, index of the message] | [skinny, 0, -1] (no launch) | [skinny, 0, index of
    the name, its ALCM_PROF_SHAPES suffix, grid x, y, z, flops, bytes (, tpb, T_out)]."""
    with open(TABLE) as f:
        t = json.load(f)
    rows = []
    for form, pos, kw, patch, results in t["cases"]:
        args = case_args(form, pos, kw, patch)
        for sk, rc, idx, *rest in results:
            for shapes in (0, 1):
                r = dict(args=args, knobs=dict(gemm_skinny=sk, prof_shapes=shapes), rc=rc, error="", name="", grid=None)
                if rc:
                    r["error"] = t["errors"][idx]
                elif idx >= 0:
                    r.update(name=t["names"][idx] + (rest[0] if shapes else ""), grid=rest[1:4], flops=float(rest[4]),
                             bytes=float(rest[5]))
                    if len(rest) > 6:
                        r["tpb"], r["T_out"] = rest[6:]
                rows.append(r)
    return rows


def test_table_covers_every_family():
    table = load_table()
    ok = [r for r in table if r["rc"] == 0 and r["name"]]

    def has(part, **cond):
        return any(part in r["name"] and all(r["knobs"].get(k, r["args"].get(k)) == v for k, v in cond.items())
                   for r in ok)
    for prec in (0, 1, 2):
        for pro in ("true", "false"):
            assert has(f"conv_kernel<128, 64, 4, 1, {prec}, {pro}>"), (prec, pro)
            assert has(f"conv_kernel<128, 128, 2, 2, {prec}, {pro}>"), (prec, pro)
        assert has(f"gemm_skinny_kernel<{prec}>")
        for tile in ("64, 32, 4, 1", "256, 32, 4, 1", "256, 64, 4, 1", "128, 128, 2, 2"):
            for avec in ("true", "false"):
                assert has(f"gemm_kernel<{tile}, {avec}, 0, {prec}>"), (tile, avec, prec)
        for tile in ("256, 64, 4, 1", "128, 128, 2, 2"):
            for bkind in (1, 2):  # BK_ACT, BK_ACTT
                assert has(f"gemm_kernel<{tile}, true, {bkind}, {prec}>"), (tile, bkind, prec)
    assert has("conv_kernel<128, 64,", tile_n=64) and has("conv_kernel<128, 128,", tile_n=128)
    forced = [r for r in ok if r["args"].get("tile_n")]
    assert any(r["args"]["tile_n"] == 64 and r["args"]["N"] > 64 and r["args"]["N"] % 64 for r in forced)
    assert any(r["args"]["tile_n"] == 128 and r["args"]["N"] <= 64 for r in forced)
    assert has("gemm_kernel<", disable_window=1) and not has("conv_kernel<", disable_window=1)
    # ALCM_GEMM_SKINNY=0 on a skinny-eligible call and on a narrow-N call: the same arguments under both values
    by_args = {}
    for r in ok:
        by_args.setdefault(json.dumps(r["args"], sort_keys=True), {})[r["knobs"]["gemm_skinny"]] = r["name"]
    pairs = [v for v in by_args.values() if len(v) == 2]
    assert any("gemm_skinny_kernel" in v[1] and "gemm_kernel<" in v[0] for v in pairs)
    assert any("gemm_kernel<64, 32" in v[1] and "gemm_kernel<256, 32" in v[0] for v in pairs)
    assert any(r["rc"] == 0 and not r["name"] and r["grid"] is None for r in table), "M or N <= 0: no launch"
    assert {r["knobs"]["prof_shapes"] for r in ok} == {0, 1}
    # one row per rejection message of the planner's source
    with open(os.path.join(REPO, "audiolcm_amd", "csrc", "alcm_gemmplan.cpp")) as f:
        src = f.read()
    msgs = set(re.findall(r'(?:return|fail\(p,|[?:])\s*"([^"]+)"', src)) - {"true", "false"}
    assert len(msgs) == 19, msgs
    assert msgs == {r["error"] for r in table if r["rc"]}
    assert all(r["rc"] in (0, E_INVALID) for r in table)


def test_planner_reproduces_recorded_choices():
    """Every recorded call gets the return code, message, profile row, grid and cost it got before the planner."""
    table = load_table()
    assert len(table) > 500  # (each call under ALCM_PROF_SHAPES off and on)
    by_knobs = {}
    for r in table:
        by_knobs.setdefault(json.dumps(r["knobs"], sort_keys=True), []).append(r)
    bad = []
    for kj, rows in by_knobs.items():
        kv = json.loads(kj)  # (ALCM_PROF_SHAPES is on when set to anything: empty for off)
        with switches({KNOB_ENV["gemm_skinny"]: kv["gemm_skinny"], KNOB_ENV["prof_shapes"]: kv["prof_shapes"] or ""}):
            for r in rows:
                g = row_args(r["args"])
                if r["rc"]:
                    with pytest.raises(_hip.HipError) as e:
                        K.gemm_plan(g)
                    if f"({r['rc']}): {r['error']}" not in str(e.value):
                        bad.append((r, str(e.value)))
                    continue
                p = K.gemm_plan(g)
                if r["grid"] is None:
                    want = dict(name="", family="none", grid=[0, 0, 0], flops=0.0, bytes=0.0)
                else:
                    fam = {"conv_kernel": "window_conv", "gemm_skinny_kernel": "skinny", "gemm_kernel": "gemm"}
                    want = dict(name=r["name"], family=fam[re.match(GEMM_ROW, r["name"]).group(1)], grid=r["grid"],
                                flops=r["flops"], bytes=r["bytes"])
                    if "tpb" in r:  # the window conv's kernel arguments: row tiles per clip, rows per clip
                        if p["grid"][0] != r["tpb"] * (r["args"]["M"] // r["T_out"]) or \
                                r["tpb"] != (r["T_out"] + p["bm"] - 1) // p["bm"]:
                            bad.append((r, p))
                    if want["family"] != "skinny" and f"<{p['bm']}, {p['bn']}, {p['wm']}, {p['wn']}," not in r["name"]:
                        bad.append((r, p))
                if {k: p[k] for k in want} != want:
                    bad.append((r, p))
    assert not bad, f"{len(bad)} rows differ, first: {bad[0]}"


def test_table_names_every_recorded_model_launch():
    """Every gemm_kernel / conv_kernel / gemm_skinny_kernel row the model forwards recorded on the GPU before the
    planner existed (tests/data/model_launches.json, ALCM_PROF_SHAPES=1) is the row of some call of the table."""
    names = set()

    def walk(o):
        if isinstance(o, str):
            if re.match(GEMM_ROW, o):
                names.add(o)
        elif isinstance(o, dict):
            for k, v in o.items():
                walk(k), walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)
    with open(LAUNCHES) as f:
        walk(json.load(f))
    assert len(names) >= 100
    planned = {r["name"] for r in load_table() if r["knobs"]["prof_shapes"] == 1 and r["knobs"]["gemm_skinny"] == 1}
    assert names <= planned, sorted(names - planned)


# ------------------------------------------------------------------ GPU: a real call records the planned row
def _r(shape, seed, scale=1.0):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _conv(prologue):
    """k = 3 window conv at B = 1, T = 40, C = 32 (with a LayerNorm prologue: row statistics and affine)."""
    def run(N):
        import torch
        import torch.nn.functional as F
        x, w, b = _r((1, 40, 32), 500, 2.0) + 0.5, _r((N, 32, 3), 501, 0.1), _r((N,), 502, 0.1)
        gam, bet = 1 + _r((32,), 503, 0.1), _r((32,), 504, 0.1)
        xd = x.cuda()
        pro = None
        h = x.double()
        if prologue:
            mean, rstd = K.row_stats(xd, 1e-5)
            pro = dict(scale=gam.cuda(), shift=bet.cuda(), sb=0, mean=mean, rstd=rstd)
            h = F.layer_norm(h, (32,), gam.double(), bet.double(), 1e-5)
        ref = F.conv1d(h.permute(0, 2, 1), w.double(), b.double(), padding=1).permute(0, 2, 1)
        return lambda: K.conv1d(xd, w.cuda(), b.cuda(), padding=1, channels_last=True, prologue=pro), ref
    return run


def _lin(M, Kc, N, prologue=False):
    def run():
        import torch.nn.functional as F
        x, w, b = _r((1, M, Kc), 510, 0.5), _r((N, Kc, 1), 511, 1.0 / np.sqrt(Kc)), _r((N,), 512, 0.05)
        xd = x.cuda()
        pro, h = None, x.double()
        if prologue:
            mean, rstd = K.row_stats(xd, 1e-5)
            pro = dict(mean=mean, rstd=rstd)
            h = F.layer_norm(h, (Kc,), None, None, 1e-5)
        ref = F.linear(h, w[..., 0].double(), b.double())
        return lambda: K.conv1d(xd, w.cuda(), b.cuda(), channels_last=True, prologue=pro), ref
    return run


def _qk():
    import torch
    q, k = _r((2, 40, 8), 520), _r((2, 40, 8), 521)
    return lambda: K.bmm_nt(q.cuda(), k.cuda(), 8 ** -0.5), torch.einsum("zid,zjd->zij", q.double(), k.double()) * 8 ** -0.5


def _pv():
    import torch
    p, v = _r((2, 40, 40), 522).softmax(-1), _r((2, 40, 8), 523)
    return lambda: K.bmm_nn(p.cuda(), v.cuda()), torch.einsum("zij,zjd->zid", p.double(), v.double())


# family: (switches, the call and its float64 restatement, the instantiation it must reach)
GPU_CASES = {
    "window_narrow": ({}, lambda: _conv(False)(64), "conv_kernel<128, 64, 4, 1, 1, false>"),
    "window_wide_norm": ({}, lambda: _conv(True)(128), "conv_kernel<128, 128, 2, 2, 1, true>"),
    "window_wide": ({}, lambda: _conv(False)(128), "conv_kernel<128, 128, 2, 2, 1, false>"),
    "skinny": ({}, _lin(2, 64, 32), "gemm_skinny_kernel<1>"),
    "narrow_n_skinny1": ({"ALCM_GEMM_SKINNY": 1}, _lin(300, 32, 20), "gemm_skinny_kernel<1>"),
    "narrow_n_skinny0": ({"ALCM_GEMM_SKINNY": 0}, _lin(300, 32, 20), "gemm_kernel<256, 32, 4, 1, true, 0, 1>"),
    "narrow_n_norm_skinny1": ({"ALCM_GEMM_SKINNY": 1}, _lin(300, 32, 20, True), "gemm_kernel<64, 32, 4, 1, true, 0, 1>"),
    "narrow_n_norm_skinny0": ({"ALCM_GEMM_SKINNY": 0}, _lin(300, 32, 20, True), "gemm_kernel<256, 32, 4, 1, true, 0, 1>"),
    "mha_qk": ({}, _qk, "gemm_kernel<256, 64, 4, 1, true, 1, 1>"),
    "mha_pv": ({}, _pv, "gemm_kernel<256, 64, 4, 1, true, 2, 1>"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(GPU_CASES))
def test_profile_row_is_the_planned_one(family, monkeypatch):
    """One real alcm_gemm call per family at the smallest shape that reaches it, at PREC_SPLIT: the one recorded profile
    row, with its cost, is the plan's, and the output is the float64 F.conv1d / matmul restatement within the split
    bound of test_gemm_skinny_rows / test_gemm_narrow_n_small_tiles (1e-5).  M = 300, K = 32, N = 20 is eligible for
    the skinny kernel, so under ALCM_GEMM_SKINNY=1 it is that kernel's row; the same shape behind a norm prologue
    (never skinny) reaches the 64-row and 256-row narrow-N tiles."""
    import torch
    _hip.require_device(0)
    sw, make, inst = GPU_CASES[family]
    call, ref = make()
    planned = []
    real_gemm = K.gemm

    def planning_gemm(args):
        planned.append(K.gemm_plan(args))
        real_gemm(args)
    with switches(sw):
        torch.cuda.synchronize()
        monkeypatch.setattr(K, "gemm", planning_gemm)
        _hip.profile_begin()
        try:
            y = call()
            torch.cuda.synchronize()
        finally:
            rows = _hip.profile_end()
    assert len(planned) == 1 and planned[0]["name"] == "alcm::" + inst, planned
    p = planned[0]
    assert [(r["name"], r["launches"], r["flops"], r["bytes"]) for r in rows] == [(p["name"], 1, p["flops"], p["bytes"])]
    e = rel_l2(y.cpu().double().numpy(), ref.numpy())
    print(f"{family}: {p['name']} grid {p['grid']} vs float64 {e:.2e}")
    assert y.shape == ref.shape and e < 1e-5
