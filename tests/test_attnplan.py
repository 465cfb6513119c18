"""The fused-attention planner (audiolcm_amd/csrc/alcm_attnplan.cpp): which kernel (resident on operand rows, resident
on fp32 rows, tiled), template arguments, grid, block, scale and profile row an alcm_flash_attention(_ex) call gets, and
which calls it rejects.

The CPU tests ask the library's diagnostics entry (alcm_debug_attn_plan: nothing is launched, pointers are only tested
for null-ness and alignment) and compare with tests/data/attn_plans.json.  The table was recorded from commit ef9d8ab,
the build before the planner existed: flash_attention() of its alcm_attn.hip, unchanged, compiled for the host with the
kernels replaced by stubs that record their template and scalar arguments, hipLaunchKernelGGL by a record of grid and
block and prof_stop by a record of the row and the cost — the method of tests/test_gemmplan.py.  The function never read
ALCM_PROF_SHAPES; it was recorded with it off and on, the records were equal, and every row is asked under both here.
The cases are (a) every flash_attn* row of tests/data/model_launches.json in the argument forms of the models
(dit_attention, the DiT plane form and its fp32 form beyond 512 keys, the BERT and T5 towers), (b) L at 1, 64, 65, 512
and 513, dh at 4, 72 and 76, bias on and off, scale 0 and explicit, plane and fp32 input, both precisions, and (c)
every rejection of tests/test_gpu_attention.py::test_error_returns and of the source, alone and in pairs that pin the
order of the checks (the message is compared for fp32 input, where the old code had one wording per defect; the plane
branch reported one message for every defect, so there the code is compared).
The GPU tests check that a real call records exactly the profile row the planner names and stays within the bound of
tests/test_gpu_attention.py.
"""
import json
import os
import re

import pytest

from conftest import REPO

from audiolcm_amd import _hip
from audiolcm_amd import kernels as K
from test_gpu_attention import worst  # noqa: F401  (the module fixture that collects the worst |d| / bound)
from test_vocplan import switches

TABLE = os.path.join(REPO, "tests", "data", "attn_plans.json")
LAUNCHES = os.path.join(REPO, "tests", "data", "model_launches.json")
E_INVALID = -1
POINTERS = ("qkv", "qkv_plane", "out", "out_plane", "bias")


def attn_form(B, L, heads, dh, prec, inp="fp32", out="fp32", bld=0, scale=0.0, **patch):
    """The arguments of a call as a row dict: inp / out "fp32", "plane", "both" or "none", a bias of pitch bld (0:
    none); a pointer field holds its address & 15 (patch: another class), a missing one is NULL.  A patch key may
    carry a trailing underscore (B_ = 0: B after the form is built)."""
    d = dict(B=B, L=L, H=heads * dh, heads=heads, prec=prec, bld=bld, scale=scale)
    if inp in ("fp32", "both"):
        d["qkv"] = 0
    if inp in ("plane", "both"):
        d["qkv_plane"] = 0
    if out in ("fp32", "both"):
        d["out"] = 0
    if out in ("plane", "both"):
        d["out_plane"] = 0
    if bld:
        d["bias"] = 0
    d.update({k.rstrip("_"): v for k, v in patch.items()})
    return d


# the argument forms of the models (alcm_models.cpp): dit_attention (fp32 in and out: a helper of the recorded build
# that no forward reached, since removed), the DiT blocks' plane form (L <= 512) and fp32 form, the BERT tower and the
# T5 tower (position bias of pitch max_len, unscaled scores)
MODEL_FORMS = {
    "dit_attention": lambda B, L, prec: attn_form(B, L, 8, 72, prec),
    "dit_plane": lambda B, L, prec: attn_form(B, L, 8, 72, prec, "plane", "plane"),
    "dit_f32": lambda B, L, prec: attn_form(B, L, 8, 72, prec, "fp32", "plane"),
    "bert": lambda B, L, prec: attn_form(B, L, 12, 64, prec, "plane", "plane"),
    "t5": lambda B, L, prec: attn_form(B, L, 16, 64, prec, "plane", "plane", bld=77, scale=1.0),
}


def row_args(d):
    a = _hip.AttnArgs()
    for n, f in enumerate(POINTERS):
        setattr(a, f, ((n + 1) << 32) + d[f] if f in d else None)
    for f in ("B", "L", "H", "heads", "prec", "bld", "scale"):
        setattr(a, f, d[f])
    return a


def instantiation(p):
    tf = lambda b: "true" if b else "false"
    if p["form"] == "tiled":
        return f"flash_attn_kernel<{p['prec']}>"
    return f"flash_attn_res_kernel<{p['prec']}, {tf(p['bias'])}, {tf(p['form'] == 'resident_plane')}>"


def load_table():
    """One row per recorded call: args, rc, error | name, inst, grid, block, lp, dh, scale, flops, bytes.  A case of the
    file is [[B, L, heads, dh, prec], keywords of attn_form, result], result [-1, index of the message] or [0, index of
    the name, index of the instantiation, grid, block, Lp (0: the tiled kernel takes none), dh, scale, flops, bytes]."""
    with open(TABLE) as f:
        t = json.load(f)
    rows = []
    for pos, kw, res in t["cases"]:
        r = dict(args=attn_form(*pos, **kw), rc=res[0])
        if res[0]:
            r["error"] = t["errors"][res[1]]
        else:
            r.update(name=t["names"][res[1]], inst=t["insts"][res[2]])
            r.update(zip(("grid", "block", "lp", "dh", "scale", "flops", "bytes"), res[3:]))
        rows.append(r)
    return rows


def test_table_covers_every_branch():
    table = load_table()
    ok = [r for r in table if r["rc"] == 0]
    insts = {r["inst"] for r in ok}
    for prec in (0, 2):
        assert f"flash_attn_kernel<{prec}>" in insts
        for bias in ("true", "false"):
            for plane in ("true", "false"):
                assert f"flash_attn_res_kernel<{prec}, {bias}, {plane}>" in insts
    for plane in (False, True):
        sel = [r for r in table if ("qkv_plane" in r["args"]) == plane and ("qkv" in r["args"]) != plane]
        assert {1, 64, 65, 512, 513} <= {r["args"]["L"] for r in sel}
        assert {4, 72, 76} <= {r["args"]["H"] // r["args"]["heads"] for r in sel if r["args"]["heads"]}
        assert any(r["rc"] == 0 and r["args"]["scale"] > 0 for r in sel) and any(r["rc"] == 0 and r["args"]["bld"] for r in sel)
    assert any(r["rc"] and "qkv_plane" in r["args"] and r["args"]["L"] == 513 for r in table)
    assert {r["rc"] for r in table} == {0, E_INVALID}
    with open(os.path.join(REPO, "audiolcm_amd", "csrc", "alcm_attnplan.cpp")) as f:
        msgs = set(re.findall(r'"(flash_attention: [^"]+)"', f.read()))
    assert len(msgs) == 9, msgs
    old = {r["error"] for r in table if r["rc"] and "qkv_plane" not in r["args"]}
    assert msgs - old == {"flash_attention: qkv_plane must be 8-byte aligned",
                          "flash_attention: plane input only for L <= 512"}, (msgs, old)


def test_planner_reproduces_recorded_choices():
    """Every recorded call gets the return code, kernel instantiation, grid, block, kernel scalars, profile row and
    cost it got before the planner, under ALCM_PROF_SHAPES off and on."""
    table = load_table()
    assert len(table) > 150
    bad = []
    for shapes in ("", 1):
        with switches({"ALCM_PROF_SHAPES": shapes}):
            for r in table:
                a = row_args(r["args"])
                if r["rc"]:
                    with pytest.raises(_hip.HipError) as e:
                        K.attn_plan(a)
                    msg = f"({r['rc']}): " + (r["error"] if "qkv_plane" not in r["args"] else "")
                    if msg not in str(e.value):
                        bad.append((r, str(e.value)))
                    continue
                p = K.attn_plan(a)
                got = dict(p, inst=instantiation(p))
                if p["form"] == "tiled":
                    got["lp"] = 0
                want = {k: r[k] for k in ("name", "inst", "grid", "block", "lp", "dh", "scale", "flops", "bytes")}
                if {k: got[k] for k in want} != want:
                    bad.append((r, p))
    assert not bad, f"{len(bad)} rows differ, first: {bad[0]}"


def test_a_grid_beyond_2_31_is_refused_on_planes_too():
    """B * heads >= 2^31 on plane input: ALCM_E_INVALID (the old plane branch launched a truncated grid; the fp32
    branch always refused).  No tensor of that size exists."""
    for inp in ("plane", "fp32"):
        with pytest.raises(_hip.HipError, match=r"\(-1\)"):
            K.attn_plan(row_args(attn_form(1 << 29, 1, 4, 4, 2, inp, "plane")))


def test_table_names_every_recorded_model_launch():
    """Every flash_attn* row the model forwards recorded on the GPU before the planner existed (model_launches.json)
    is what the planner names for that forward's calls, and each of those calls is a case of the table."""
    with open(LAUNCHES) as f:
        launches = json.load(f)["rows"]
    in_table = {json.dumps(r["args"], sort_keys=True) for r in load_table() if r["rc"] == 0}
    seen = 0
    for cid, rows in launches.items():
        want = {n for n in rows if n.startswith("alcm::flash_attn")}
        m = re.fullmatch(r"(dit|text)-B(\d+)-[TL](\d+)-(bf16|mixed)(-\w+)*", cid)
        if not m:
            assert not want, cid
            continue
        B, n, prec = int(m.group(2)), int(m.group(3)), 0 if m.group(4) == "bf16" else 2
        if m.group(1) == "dit":
            L = n + 155  # the 154 context tokens and the time token
            calls = [MODEL_FORMS["dit_plane" if L <= 512 else "dit_f32"](B, L, prec)]
        else:
            calls = [MODEL_FORMS["bert"](B, n, prec), MODEL_FORMS["t5"](B, n, prec)]
        assert {K.attn_plan(row_args(c))["name"] for c in calls} == want, cid
        assert all(json.dumps(c, sort_keys=True) in in_table for c in calls), cid
        seen += len(want)
    assert seen >= 15


# ------------------------------------------------------------------ GPU: a real call records the planned row
@pytest.mark.gpu
@pytest.mark.parametrize("L,in_plane,bld,inst", [(77, True, 77, "flash_attn_res_kernel<2, true, true>"),
                                                 (449, False, 0, "flash_attn_res_kernel<2, false, false>"),
                                                 (513, False, 0, "flash_attn_kernel<2>")])
def test_profile_row_is_the_planned_one(worst, L, in_plane, bld, inst):  # noqa: F811
    """One real call per form at B = 2, heads = 2, dh = 36: the one recorded profile row, with its cost, is the plan's,
    and every element is within the derived bound of tests/test_gpu_attention.py of its fp64 reference."""
    import torch
    import test_gpu_attention as A
    _hip.require_device(0)
    B, heads, dh, prec = 2, 2, 36, 2
    p = K.attn_plan(row_args(attn_form(B, L, heads, dh, prec, "plane" if in_plane else "fp32", "fp32", bld)))
    assert instantiation(p) == inst, p
    qkv = A.pack(*A.make_qkv(B, L, heads, dh))
    kw = dict(bias=A.make_bias(heads, bld).cuda() if bld else None)
    src = dict(qkv_plane=A.to_plane(qkv, prec).cuda()) if in_plane else {}
    torch.cuda.synchronize()
    _hip.profile_begin()
    try:
        y = K.flash_attention(None if in_plane else qkv.cuda(), heads, prec, **src, **kw)
        torch.cuda.synchronize()
    finally:
        rows = _hip.profile_end()
    assert [(r["name"], r["launches"], r["flops"], r["bytes"]) for r in rows] == [(p["name"], 1, p["flops"], p["bytes"])]
    R, Aabs, vmax = A.reference(B, L, heads, dh, "plain", prec, 0.0, bld, 0.0)
    ratio = float(((y.cpu().double() - R).abs() / A.bound(R, Aabs, vmax, prec, False, L)).max())
    print(f"{inst} L{L}: grid {p['grid']} x {p['block']}, worst |d|/bound {ratio:.3f}")
    key = ("resident" if L <= 512 else "tiled", "fp16", "fp32")
    worst[key] = max(worst.get(key, (0.0, "")), (ratio, f"B{B} L{L} heads{heads} dh{dh} plain"))
    assert y.shape == R.shape and bool(torch.isfinite(y).all()) and ratio <= 1.0
