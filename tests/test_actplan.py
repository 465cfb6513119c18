"""The Activation1d-on-planes planner (audiolcm_amd/csrc/alcm_actplan.cpp): which kernel instantiation, grid, kernel
scalars and profile row a call of alcm_activation1d_op / alcm_activation1d_op_f16in / the three-set form gets, and which
calls it rejects.

The CPU tests ask the library's diagnostics entry (alcm_debug_act_plan: nothing is launched, pointers are only tested
for null-ness and alignment) and compare with tests/data/act_plans.json.  The table was recorded from commit ef9d8ab,
the build before the planner existed: the host sections of its alcm_opconv.hip (activation1d_x3, activation1d_op_h16,
activation1d_op) and alcm_act.hip (act_coop, act_mfma3, act_mfma), unchanged, compiled for the host with the kernels
replaced by stubs that record their template arguments and scalar arguments, hipLaunchKernelGGL by a record of grid and
block and prof_stop by a record of the row and the cost — the method of tests/test_gemmplan.py.  Those sections never
read ALCM_PROF_SHAPES; they were recorded with it off and on, the records were equal, and every row is asked under
both here.  A case is stored as one of the three entries' argument forms with its parameters and a patch of fields
(load_table).  The cases are (a) every Activation1d call of the BigVGAN forward for each case of
tests/data/voc_launches.json, in the forms the models' act_planes, act_first3 and the fp16 hand-off give it, (b) each
kernel, precision, tile width, switch and pointer alignment class alone, and (c) every rejection, each defect alone and
in pairs that pin the order of the checks (the message is compared where the old entry had one wording per defect: the
one-set fp32 form; the other two forms reported one message for every defect, so there the code is compared).
The GPU tests check that a real call records exactly the profile row the planner names and computes the float64
oracle Activation1d.
"""
import json
import os
import re

import pytest

from conftest import REPO, rel_l2

from audiolcm_amd import _hip, recipe
from audiolcm_amd import kernels as K
from test_vocplan import switches

TABLE = os.path.join(REPO, "tests", "data", "act_plans.json")
VOC_PLANS = os.path.join(REPO, "tests", "data", "voc_plans.json")
VOC_LAUNCHES = os.path.join(REPO, "tests", "data", "voc_launches.json")
KNOB_ENV = {"act_mfma": "ALCM_ACT_MFMA", "act_defer": "ALCM_ACT_DEFER", "act_x3_mfma": "ALCM_ACT_X3_MFMA"}
E_INVALID = -1
POINTERS = ("x", "up_filter", "down_filter")
SET_POINTERS = ("y", "alpha_exp", "inv_beta")


def _rup(x, m):
    return (x + m - 1) // m * m


def act_form(form, B, T, C, prec, **patch):
    """The arguments of one of the models' forms as a row dict: "op" (act_planes / alcm_activation1d_op), "h16" (the
    fp16 hand-off, alcm_activation1d_op_f16in) or "x3" (act_first3).  A pointer field holds its address & 15, None or a
    missing field is NULL; y / alpha_exp / inv_beta are lists, one per parameter set (patch: y1 = 4).  A patch key may
    carry a trailing underscore (B_ = 0: B after the form is built)."""
    nset = 3 if form == "x3" else 1
    d = dict(x=0, x_is_f16=int(form == "h16"), nset=nset, B=B, T=T, C=C, Cp=_rup(C, 32), prec=prec, up_filter=0,
             down_filter=0, y=[0] * nset, alpha_exp=[0] * nset, inv_beta=[0] * nset)
    for key, v in patch.items():
        m = re.fullmatch(r"(y|alpha_exp|inv_beta)(\d)", key)
        if m:
            d[m.group(1)][int(m.group(2))] = v
        else:
            d[key.rstrip("_")] = v
    return d


def row_args(d):
    """A row dict as ActArgs: every pointer on a made-up address of its own with the recorded class."""
    a = _hip.ActArgs()
    n = 0
    for f in POINTERS:
        n += 1
        setattr(a, f, None if d.get(f) is None else (n << 32) + d[f])
    for f in SET_POINTERS:
        for i, v in enumerate(d[f]):
            n += 1
            getattr(a, f)[i] = None if v is None else (n << 32) + v
    for f in ("x_is_f16", "nset", "B", "T", "C", "Cp", "prec"):
        setattr(a, f, d[f])
    return a


def instantiation(p):
    """The kernel template-id a plan names, as the recorder's stub kernels spelled it."""
    tf = lambda b: "true" if b else "false"
    if p["kernel"] == "coop":
        return f"act_coop_kernel<{p['prec']}, {p['np']}, {p['nset']}>"
    if p["kernel"] == "mfma3":
        return "act_mfma3_kernel<64>"
    return f"act_mfma_kernel<64, {tf(p['defer'])}, {tf(p['in16'])}>"


def load_table():
    """One row per recorded (call, switches): args, form, knobs, rc, error | name, inst, grid, block, tiles_t, tiles_c,
    strips_t, y_lo, flops, bytes.  A case of the file is [form, [B, T, C, prec], patch, switches, result], result
    [-1, index of the message] or [0, index of the name, index of the instantiation, grid, block, tiles_t, tiles_c,
    strips_t, y_lo, flops, bytes] (a scalar the kernel does not take is 0)."""
    with open(TABLE) as f:
        t = json.load(f)
    rows = []
    for form, pos, patch, knobs, res in t["cases"]:
        r = dict(form=form, args=act_form(form, *pos, **patch), knobs=knobs, rc=res[0])
        if res[0]:
            r["error"] = t["errors"][res[1]]
        else:
            r.update(name=t["names"][res[1]], inst=t["insts"][res[2]])
            r.update(zip(("grid", "block", "tiles_t", "tiles_c", "strips_t", "y_lo"), res[3:9]))
            r.update(flops=float(res[9]), bytes=float(res[10]))
        rows.append(r)
    return rows


def stage_act_calls(plans, B, M, policy, cfg=None):
    """The Activation1d calls of alcm_bigvgan_forward executing `plans` (alcm_models.cpp chain_fused / chain_wide /
    act_first3 and the output head), as (form, B, T, C, prec) in launch order per chain."""
    cfg = cfg or recipe.BigVGANConfig()
    calls, T = [], M
    nrb, ndil = len(cfg.resblock_kernel_sizes), len(cfg.resblock_dilation_sizes[0])
    for si, (p, rate) in enumerate(zip(plans, cfg.upsample_rates)):
        T *= rate
        C = cfg.stage_channels(si)
        one = ("op", B, T, C, p["prec"])
        if p["act3"]:
            calls.append(("x3", B, T, C, p["prec"]))
        for _ in range(nrb):
            for l in range(ndil):
                if not (l == 0 and p["act3"]) and (p["amp"] == "wide" or l == 0):
                    calls.append(one)
                if p["amp"] == "wide":
                    calls.append(("h16", B, T, C, p["prec"]) if p["h16"] else one)
    if _hip.POLICIES[policy] == _hip.POLICY_BF16 or cfg.stage_channels(len(plans) - 1) != 24:
        calls.append(("op", B, T, cfg.stage_channels(len(plans) - 1), _hip.PREC_BF16 if policy == "bf16" else 1))
    return calls


def voc_case(cid):
    """policy, streams, B, M and switches of a voc_launches.json case id."""
    m = re.fullmatch(r"(\w+)-streams(\d)-B(\d+)-M(\d+)(?:-(ALCM_\w+)=(\d+))?", cid)
    return m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), ({m.group(5): m.group(6)} if m.group(5) else {})


def knob_env(knobs, shapes=0):
    env = {KNOB_ENV[k]: knobs.get(k, 1) for k in KNOB_ENV}
    env["ALCM_PROF_SHAPES"] = shapes or ""  # (on when set to anything: empty for off)
    return env


def test_table_covers_every_branch():
    table = load_table()
    ok = [r for r in table if r["rc"] == 0]
    insts = {r["inst"] for r in ok}
    for prec in (0, 1, 2):
        for nset in (1, 3):
            assert f"act_coop_kernel<{prec}, 16, {nset}>" in insts or prec == 1, (prec, nset)
            assert f"act_coop_kernel<{prec}, 32, {nset}>" in insts, (prec, nset)
    assert any(r["inst"].startswith("act_coop_kernel<1, 16,") and r["args"]["Cp"] % 64 for r in ok)
    assert any(r["inst"].startswith("act_coop_kernel<2, 16,") and r["args"]["prec"] == 3 for r in ok), "F16W2 as F16"
    for d in ("true", "false"):
        for i in ("true", "false"):
            assert f"act_mfma_kernel<64, {d}, {i}>" in insts
    assert "act_mfma3_kernel<64>" in insts
    for k in KNOB_ENV:
        assert any(r["knobs"].get(k) == 0 for r in ok), k
    # each operand off the MFMA kernels' 16-byte line, alone: the fp32 forms fall back, the fp16 form is refused
    mfma_shape = [r for r in table if r["args"]["C"] == 192 and r["args"]["prec"] == 2 and not r["knobs"]]
    for cls in (4, 8):
        for form, sets in (("op", 1), ("h16", 1), ("x3", 3)):
            rows = [r for r in mfma_shape if r["form"] == form]
            assert any(r["args"]["x"] == cls and r["args"]["y"] == [0] * sets for r in rows), (form, "x", cls)
            for i in range(sets):
                assert any(r["args"]["x"] == 0 and [j for j, v in enumerate(r["args"]["y"]) if v == cls] == [i]
                           for r in rows), (form, "y", i, cls)
    assert {r["rc"] for r in table} == {0, E_INVALID}
    # one row per rejection message of the planner's source; the one-set fp32 form's old wording is the planner's
    with open(os.path.join(REPO, "audiolcm_amd", "csrc", "alcm_actplan.cpp")) as f:
        msgs = set(re.findall(r'"(activation1d_op[^"]*: [^"]+)"', f.read()))
    assert len(msgs) == 7, msgs
    old = {r["error"] for r in table if r["rc"] and r["form"] == "op"} - {"act_mfma: too large"}
    assert msgs - old == {m for m in msgs if m.startswith("activation1d_op_f16in")}, (msgs, old)
    assert any(r["rc"] and r["form"] == "h16" and r["error"].startswith("activation1d_op_f16in: needs") for r in table)


def test_planner_reproduces_recorded_choices():
    """Every recorded call gets the return code, kernel instantiation, grid, kernel scalars, profile row and cost it
    got before the planner, under ALCM_PROF_SHAPES off and on."""
    table = load_table()
    assert len(table) > 250
    by_knobs = {}
    for r in table:
        by_knobs.setdefault(json.dumps(r["knobs"], sort_keys=True), []).append(r)
    bad = []
    for kj, rows in by_knobs.items():
        for shapes in (0, 1):
            with switches(knob_env(json.loads(kj), shapes)):
                for r in rows:
                    a = row_args(r["args"])
                    if r["rc"]:
                        with pytest.raises(_hip.HipError) as e:
                            K.act_plan(a)
                        # (the MFMA launcher below the old entry had its own wording for the one defect it found)
                        old = "activation1d_op: problem too large" if r["error"] == "act_mfma: too large" else r["error"]
                        msg = f"({r['rc']}): " + (old if r["form"] == "op" else "")
                        if msg not in str(e.value):
                            bad.append((r, str(e.value)))
                        continue
                    p = K.act_plan(a)
                    got = dict(p, inst=instantiation(p), block=256)
                    want = {k: r[k] for k in ("name", "inst", "grid", "block", "tiles_t", "tiles_c", "strips_t", "y_lo",
                                              "flops", "bytes")}
                    if {k: got[k] for k in want} != want:
                        bad.append((r, p))
    assert not bad, f"{len(bad)} rows differ, first: {bad[0]}"


def test_stage_planner_and_launch_planner_agree():
    """For every case of voc_plans.json: a stage with act3 gets the three-set kernel its form implies (the MFMA one on
    a wide stage, the VALU one on a fused stage), a stage without it would not get the MFMA three-set kernel, and the
    fp16 hand-off is planned exactly where the fp16-input launch is accepted (on the MFMA kernel)."""
    with open(VOC_PLANS) as f:
        cases = json.load(f)["cases"]
    cfg = recipe.BigVGANConfig()
    for cid, c in cases.items():
        with switches(c["knobs"]):
            T = c["M"]
            for si, p in enumerate(c["stages"]):
                T *= cfg.upsample_rates[si]
                C = cfg.stage_channels(si)
                x3 = K.act_plan(row_args(act_form("x3", c["B"], T, C, p["prec"])))["kernel"]
                if p["act3"]:
                    assert x3 == ("mfma3" if p["amp"] == "wide" else "coop"), (cid, si)
                elif p["amp"] == "wide":
                    assert x3 != "mfma3", (cid, si)
                h16 = row_args(act_form("h16", c["B"], T, C, p["prec"]))
                if p["h16"]:
                    assert K.act_plan(h16)["kernel"] == "mfma", (cid, si)
                elif p["amp"] == "wide" and c["knobs"].get("ALCM_CONV1_H16", 1) not in (0, "0") and c["B"] * T >= 1024:
                    with pytest.raises(_hip.HipError):
                        K.act_plan(h16)


def test_table_names_every_recorded_voc_launch():
    """The act_* rows alcm_bigvgan_forward recorded on the GPU before the planner existed (voc_launches.json), with
    their launch counts, are what the planner names for the calls of that forward — and each of those calls is a case
    of the table."""
    with open(VOC_LAUNCHES) as f:
        launches = json.load(f)
    in_table = {(r["form"], r["args"]["B"], r["args"]["T"], r["args"]["C"], r["args"]["prec"],
                 json.dumps(r["knobs"], sort_keys=True)) for r in load_table() if r["rc"] == 0}
    cfg = recipe.BigVGANConfig()
    env_knob = {v: k for k, v in KNOB_ENV.items()}
    assert len(launches) >= 20
    for cid, rows in launches.items():
        policy, streams, B, M, sw = voc_case(cid)
        want = {n: c for n, c in rows.items() if n.startswith("alcm::act_")}
        got = {}
        with switches(sw):
            for call in stage_act_calls(K.voc_plan(cfg, policy, streams, B, M, 256), B, M, policy):
                name = K.act_plan(row_args(act_form(*call)))["name"]
                got[name] = got.get(name, 0) + 1
                knobs = {env_knob[e]: int(v) for e, v in sw.items() if e in env_knob}
                assert call + (json.dumps(knobs, sort_keys=True),) in in_table, (cid, call)
        assert got == want, (cid, got, want)


def test_one_size_bound_for_every_form():
    """B * T * Cp >= 2^40 is ALCM_E_INVALID on the fp16-input form too.  The old fp16-input entry had only the MFMA
    launcher's bounds (workgroups and T * C below 2^31), so it took 2^40 .. 2^46 elements: planes of 2 TB and more,
    which no device holds — no call that could run changes."""
    for form in ("op", "h16", "x3"):
        with pytest.raises(_hip.HipError, match=r"\(-1\): activation1d_op: problem too large"):
            K.act_plan(row_args(act_form(form, 1 << 20, 1 << 13, 192, 2)))


def test_forms_without_an_old_entry_are_refused():
    """Two parameter sets, or three sets of an fp16 plane: no kernel, ALCM_E_INVALID."""
    for patch in (dict(nset=2, y=[0, 0], alpha_exp=[0, 0], inv_beta=[0, 0]), dict(x_is_f16=1)):
        with pytest.raises(_hip.HipError, match=r"\(-1\)"):
            K.act_plan(row_args(act_form("x3", 2, 70, 192, 2, **patch)))


# ------------------------------------------------------------------ GPU: a real call records the planned row
def _r(shape, seed, scale=1.0):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _decode(pl, C, prec):
    import torch
    if prec == 1:
        return pl[0, ..., :C].view(torch.bfloat16).float() + pl[1, ..., :C].view(torch.bfloat16).float()
    return pl[0, ..., :C].view(torch.float16).float()


@pytest.fixture(scope="module")
def oracle_act():
    """x (2, C, T), three SnakeBeta parameter sets, the recipe's taps and the float64-oracle Activation1d of each set as
    (2, T, C), computed once per (C, T)."""
    import functools
    from oracle import alcm_oracle as O
    f = recipe.kaiser_sinc_filter1d(0.25, 0.3, 12)

    @functools.lru_cache(maxsize=None)
    def make(C, T):
        x = _r((2, C, T), 77, 1.2)
        sets = [(_r((C,), 78 + 2 * i, 0.3), _r((C,), 79 + 2 * i, 0.3)) for i in range(3)]
        refs = [O.activation1d(x, a, b, f, f).permute(0, 2, 1).contiguous() for a, b in sets]
        return x, sets, f, refs
    return make


def _profiled(call):
    import torch
    torch.cuda.synchronize()
    _hip.profile_begin()
    try:
        y = call()
        torch.cuda.synchronize()
    finally:
        rows = _hip.profile_end()
    return y, [(r["name"], r["launches"], r["flops"], r["bytes"]) for r in rows]


# C, T, prec, fp16 input, the instantiation: one whole 128-row tile and a ragged one (coop NP 16), 64-row tiles (NP 32),
# a ragged wave tile and a second strip of 8 wave tiles (mfma)
ONE_SET = [(24, 130, 2, False, "act_coop_kernel<2, 16, 1>"), (24, 130, 1, False, "act_coop_kernel<1, 16, 1>"),
           (64, 70, 1, False, "act_coop_kernel<1, 32, 1>"), (192, 70, 2, False, "act_mfma_kernel<64, true, false>"),
           (192, 518, 2, False, "act_mfma_kernel<64, true, false>"), (192, 70, 2, True, "act_mfma_kernel<64, true, true>")]
# the tolerances of test_gpu_ops.py test_activation1d_op (fp16 planes, split planes) and test_activation1d_mfma
TOL = {2: 1e-3, 1: 2e-5}


def _planned(form, T, C, prec, inst):
    p = K.act_plan(row_args(act_form(form, 2, T, C, prec)))
    assert instantiation(p) == inst, p
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("C,T,prec,x16,inst", ONE_SET)
def test_one_set_profile_row_and_values(oracle_act, C, T, prec, x16, inst):
    """One real call per kernel branch: the one recorded profile row, with its cost, is the plan's, and the planes hold
    the float64 oracle Activation1d within the operand format's bound.  The fp16-input call runs on fp16-representable
    input and equals the fp32-input call on it bit for bit."""
    import torch
    _hip.require_device(0)
    x, sets, f, refs = oracle_act(C, T)
    (a, b), ref = sets[0], refs[0]
    xd = x.permute(0, 2, 1).contiguous().cuda()
    if x16:
        from oracle import alcm_oracle as O
        x16d = xd.half().view(torch.int16).unsqueeze(0).contiguous()
        xd = xd.half().float()
        ref = O.activation1d(xd.cpu().permute(0, 2, 1), a, b, f, f).permute(0, 2, 1)
        pl, rows = _profiled(lambda: K.activation1d_op_f16in(x16d, a.cuda(), b.cuda(), f, f, prec))
        assert torch.equal(pl, K.activation1d_op(xd, a.cuda(), b.cuda(), f, f, prec))
    else:
        pl, rows = _profiled(lambda: K.activation1d_op(xd, a.cuda(), b.cuda(), f, f, prec))
    p = _planned("h16" if x16 else "op", T, C, prec, inst)
    assert rows == [(p["name"], 1, p["flops"], p["bytes"])]
    pl = pl.cpu()
    assert pl.shape[-1] == _rup(C, 32) and bool(torch.all(pl[..., C:] == 0))
    e = rel_l2(_decode(pl, C, prec).numpy(), ref.numpy())
    print(f"{inst} C{C} T{T}: grid {p['grid']} vs float64 oracle {e:.2e}")
    assert e < TOL[prec]
    if p["kernel"] == "mfma":  # test_activation1d_mfma's second bound: within 2.5x the VALU kernel's error
        with switches({"ALCM_ACT_MFMA": 0}):
            valu = K.activation1d_op(xd, a.cuda(), b.cuda(), f, f, prec).cpu()
        e_valu = rel_l2(_decode(valu, C, prec).numpy(), ref.numpy())
        print(f"    VALU kernel {e_valu:.2e}")
        assert e < 2.5 * e_valu


@pytest.mark.gpu
@pytest.mark.parametrize("C,T,prec,inst", [(24, 130, 2, "act_coop_kernel<2, 16, 3>"), (192, 70, 2, "act_mfma3_kernel<64>")])
def test_three_sets_profile_row_and_values(oracle_act, C, T, prec, inst):
    """The three-set call: one row, the plan's; each set's planes equal its single call bit for bit and hold the
    oracle's values."""
    import torch
    _hip.require_device(0)
    x, sets, f, refs = oracle_act(C, T)
    xd = x.permute(0, 2, 1).contiguous().cuda()
    al, be = [a.cuda() for a, _ in sets], [b.cuda() for _, b in sets]
    ys, rows = _profiled(lambda: K.activation1d_op_x3(xd, al, be, f, f, prec))
    p = _planned("x3", T, C, prec, inst)
    assert rows == [(p["name"], 1, p["flops"], p["bytes"])]
    for i in range(3):
        assert torch.equal(ys[i], K.activation1d_op(xd, al[i], be[i], f, f, prec)), i
        e = rel_l2(_decode(ys[i].cpu(), C, prec).numpy(), refs[i].numpy())
        print(f"{inst} set {i}: vs float64 oracle {e:.2e}")
        assert e < TOL[prec]
