"""The operand-plane conv planner (audiolcm_amd/csrc/alcm_convplan.cpp): which kernel, tile, K parts and profile name
an alcm_opconv / alcm_opconv_sum / alcm_opconv_dense call gets, and which calls it rejects.

The CPU tests ask the library's diagnostics entry (alcm_debug_conv_plan: nothing is launched, pointers are only
tested for null-ness and alignment) and compare with tests/data/conv_plans.json, a table of (arguments, switches,
profile names) recorded from the build before the planner existed while it ran the benchmark and the GPU op tests.
tests/data/dense_plans.json is the same for alcm_opconv_dense (the BigVGAN tail convs): recorded from the build before
dense_conv_plan existed, its dispatch function compiled for the host with the two launch sites replaced by a record of
the instantiation and the launch geometry, over every ALCM_TCONV value, (C, precision), tap count, epilogue form and
a set of (B, T) from one partial tile to the benchmark's stage 3-5 shapes.
The GPU tests check that a real call of each kernel family records exactly the profile row the planner names.
"""
import contextlib
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import REPO

from audiolcm_amd import _hip
from audiolcm_amd import kernels as K

TABLE = os.path.join(REPO, "tests", "data", "conv_plans.json")
DENSE_TABLE = os.path.join(REPO, "tests", "data", "dense_plans.json")
KNOB_ENV = {"wconv": ("ALCM_WCONV", 8), "wconv3": ("ALCM_WCONV3", -1), "wconv3_grid": ("ALCM_WCONV3_GRID", 0),
            "nconv": ("ALCM_NCONV", -1), "opconv_tile": ("ALCM_OPCONV_TILE", 0), "lin1": ("ALCM_LIN1", -1),
            "ups_t160": ("ALCM_UPS_T160", 1), "wconv_sum": ("ALCM_WCONV_SUM", 1), "ksplit": ("ALCM_KSPLIT", 1),
            "prof_shapes": ("ALCM_PROF_SHAPES", 0), "tconv": ("ALCM_TCONV", 1)}
POINTERS = ("a", "w", "bias", "res", "out", "act_plane", "act_alpha_exp", "act_inv_beta", "act_up_filter",
            "act_down_filter", "geglu_plane", "out_plane", "ksplit_ws")
E_INVALID = -1


@contextlib.contextmanager
def knobs(**kv):
    """The ALCM_* switches of a table row (or of a test) for the duration of the block."""
    old = {}
    try:
        for k, v in kv.items():
            env, dflt = KNOB_ENV[k]
            old[env] = os.environ.get(env)
            if v == dflt:
                os.environ.pop(env, None)
            else:
                os.environ[env] = str(v)
        _hip.reload_knobs()
        yield
    finally:
        for env, v in old.items():
            if v is None:
                os.environ.pop(env, None)
            else:
                os.environ[env] = v
        _hip.reload_knobs()


def row_args(d, index=0, out0=None):
    """A table row's arguments as OpConvArgs (a field the row leaves out is zero / NULL): a pointer field holds its
    recorded class (address & 15) on a made-up address of its own; recorded aliasing (out == res, a sum term's out == args[0].out) is kept."""
    a = _hip.OpConvArgs()
    for f, _ in _hip.OpConvArgs._fields_:
        if f in POINTERS:
            setattr(a, f, ((index * 16 + POINTERS.index(f) + 1) << 32) + d[f] if f in d else None)
        elif f == "out_scale":
            a.out_scale = 1.0
        else:
            setattr(a, f, d.get(f, 0))
    if d.get("out_is_res"):
        a.out = a.res
    if index > 0 and d.get("out_is_out0"):
        a.out = out0
    return a


def plan_rc(args, n, form, ncu):
    out = (_hip.ConvPlanInfo * 3)()
    nl = C.c_int(0)
    form = int(form)
    rc = _hip.lib().alcm_debug_conv_plan(args if form == 1 else C.byref(args), n, form, ncu, out, C.byref(nl))
    return rc, _hip.lib().alcm_last_error().decode() if rc else ""


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_every_kernel_family():
    names = [n for r in load_table() for n in r.get("names", [])]
    sums = [r for r in load_table() if "terms" in r and r["rc"] == 0 and len(r["names"]) == 1]

    def has(*parts):
        return any(all(p in n for p in parts) for n in names)
    assert has("lin_plane_kernel<64, 2,") and has("lin_plane_kernel<32, 4,")
    assert has("wconv3_kernel<", ", 1, false>") and has("wconv3_kernel<", ", 1, true> + ksplit_reduce")
    assert any("out" in r["terms"][0] for r in sums) and any("out_plane" in r["terms"][0] for r in sums)
    for bm in ("128, 192>", "160, 192>", "256, 96>"):
        assert has("wconv2_kernel<", "false, " + bm), bm
    assert has("wconv2_kernel<", ", true, ") and has("wconv2_kernel<", "+ ksplit_reduce")
    rows = [r for r in load_table() if "args" in r and r["rc"] == 0]
    w2 = [r for r in rows if "wconv2_kernel" in r["names"][0]]
    assert any(r["args"].get("out_stride", 0) > 0 for r in w2) and any(r["args"]["N"] % 96 for r in w2)
    assert has("nconv_kernel<", "true>") and has("nconv_kernel<", "false>")
    for tile in ("128, 192, 2, 2", "128, 128, 2, 2", "128, 96, 2, 2", "256, 48, 4, 1", "256, 32, 4, 1", "256, 16, 4, 1"):
        assert has("opconv_kernel<" + tile), tile
    for tile in ("256, 96, 4, 1, 2, 1,", "256, 96, 4, 1, 2, 2,", "512, 48, 4, 1, 2, 1,", "512, 48, 4, 1, 2, 2,",
                 "512, 32, 4, 1, 2, 1,", "512, 32, 4, 1, 2, 2,"):  # ALCM_OPCONV_TILE = 1 / 2
        assert has("opconv_kernel<" + tile), tile
    oc = [r for r in rows if "opconv_kernel<128, 96" in r["names"][0]]
    assert any(r["args"]["N"] % 128 == 0 for r in oc), "the under-filled 96-column case"
    assert any(r["args"]["prec"] == 1 for r in rows if "opconv_kernel" in r["names"][0]), "SPLIT"


def test_planner_reproduces_recorded_choices():
    """Every recorded call gets the kernel instantiation (profile name) and K parts it got before the planner."""
    table = load_table()
    assert len(table) > 100
    by_knobs = {}
    for r in table:
        by_knobs.setdefault(json.dumps(r["knobs"], sort_keys=True), []).append(r)
    bad = []
    for kj, rows in by_knobs.items():
        with knobs(**json.loads(kj)):
            for r in rows:
                if "terms" in r:
                    n = len(r["terms"])
                    arr = (_hip.OpConvArgs * n)()
                    for i, t in enumerate(r["terms"]):
                        arr[i] = row_args(t, i, arr[0].out if i else None)
                    call = lambda: K.conv_plan(list(arr), r["ncu"])
                else:
                    a = row_args(r["args"])
                    call = lambda: K.conv_plan(a, r["ncu"])
                if r["rc"]:
                    with pytest.raises(_hip.HipError) as e:
                        call()
                    if f"({r['rc']}): {r['error']}" not in str(e.value):
                        bad.append((r, str(e.value)))
                    continue
                got = call()
                if [p["name"] for p in got] != r["names"] or ("ksplit" in r and got[0]["ksplit"] != r["ksplit"]):
                    bad.append((r, got))
    assert not bad, f"{len(bad)} rows differ, first: {bad[0]}"


def sum_terms():
    """Three terms eligible for the one-launch sum form under ALCM_WCONV3=1 (B=2, T=512, C=Cp=N=192, k=3/5/7, F16)."""
    arr = (_hip.OpConvArgs * 3)()
    for i, k in enumerate((3, 5, 7)):
        a = arr[i]
        a.a, a.w, a.bias, a.res = (0x100 + i) << 24, (0x200 + i) << 24, (0x300 + i) << 24, (0x400 + i) << 24
        a.a_lo_off, a.w_lo_off = 2 * 512 * 192, 192 * k * 192
        a.B, a.T, a.C, a.Cp, a.N = 2, 512, 192, 192, 192
        a.ksize, a.dil, a.pad, a.kpad = k, 1, (k - 1) // 2, k * 192
        a.prec = _hip.PREC_F16
    arr[0].out, arr[0].out_scale = 0x500 << 24, 1.0 / 3
    return arr


DEFECTS = {
    "null a": (lambda a: setattr(a, "a", None), "opconv: bad arguments"),
    "null w": (lambda a: setattr(a, "w", None), "opconv: bad arguments"),
    "plane & 15": (lambda a: setattr(a, "a", a.a + 8), "opconv: operands must be 16-byte aligned"),
    "weight & 15": (lambda a: setattr(a, "w", a.w + 4), "opconv: operands must be 16-byte aligned"),
    "a_lo_off % 8": (lambda a: setattr(a, "a_lo_off", a.a_lo_off + 4), "opconv: operands must be 16-byte aligned"),
    "kpad < ksize*Cp": (lambda a: setattr(a, "kpad", a.ksize * a.Cp - 32), "opconv: kpad mismatch"),
    "kpad % 32": (lambda a: setattr(a, "kpad", a.ksize * a.Cp + 16), "opconv: kpad mismatch"),
    "C = 0": (lambda a: setattr(a, "C", 0), "opconv: C must be in (0, Cp]"),
    "C > Cp": (lambda a: setattr(a, "C", a.Cp + 1), "opconv: C must be in (0, Cp]"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_sum_plan_rejects_what_opconv_rejects(defect):
    """The one-launch sum form validates every term as alcm_opconv does (it used to run only its shape checks)."""
    spoil, msg = DEFECTS[defect]
    with knobs(wconv3=1):
        plans = K.conv_plan(list(sum_terms()), 256)
        assert [p["kernel"] for p in plans] == ["wconv3_sum"] and plans[0]["name"] == "alcm::wconv3_kernel<2, 3, false>"
        for i in range(3):
            arr = sum_terms()
            spoil(arr[i])
            assert plan_rc(arr, 3, True, 256) == (E_INVALID, msg), (defect, i)
        one = sum_terms()[1]
        one.out = 0x500 << 24
        assert K.conv_plan(one, 256)[0]["kernel"] == "wconv3"
        spoil(one)
        assert plan_rc(one, 1, False, 256) == (E_INVALID, msg)


def test_ksplit_parts():
    """The one K-parts search reproduces both users' results: the DiT FFN down-projection on wconv3 (B=32, T=467,
    Cp=2304, N=576: 192 tiles of 256 x 192 on 256 CUs) and the text towers' linears on wconv2 (2464 rows, 128 x 192
    tiles on 512 two-workgroup slots; test_wconv2_ksplit_text_linears)."""
    parts = _hip.lib().alcm_debug_ksplit_parts
    e = 32 * 467 * 576.0
    assert parts(32 * 2 * 3, 256, 2304 // 64, e, 8 * e) == 4
    assert parts(32 * 2 * 3, 256, 2304 // 64, e, 3 * e) == 1  # the workspace holds no 4 slices: 2 / 3 parts gain nothing
    for Cc, N, want in ((1024, 1024, 4), (3072, 768, 6), (768, 768, 3)):
        tiles = ((2464 + 127) // 128) * ((N + 191) // 192)
        assert parts(tiles, 512, Cc // 64, 2464.0 * N, 8 * 2464.0 * N) == want, (Cc, N)
        a = _hip.OpConvArgs()
        a.a, a.w, a.bias, a.res, a.out, a.ksplit_ws = (i << 32 for i in range(1, 7))
        a.B, a.T, a.C, a.Cp, a.N, a.ksize, a.dil, a.kpad, a.prec = 1, 2464, Cc, Cc, N, 1, 1, Cc, _hip.PREC_F16
        a.out_scale, a.ksplit_ws_floats = 1.0, 8 * 2464 * N
        p, = K.conv_plan(a, 256)
        assert p["name"] == "alcm::wconv2_kernel<2, false, 128, 192> + ksplit_reduce" and p["ksplit"] == want
        assert p["grid"] == tiles * want


# ------------------------------------------------------------------ the tail convs (alcm_opconv_dense)
PLAN_KEYS = ("name", "inst", "block", "ncg", "tiles_per_batch", "tiles", "wslots", "flops", "bytes", "grid")


def dense_call(B, T, Cc, prec, k, dil, epi):
    """A dense_plans.json case as the row dict row_args takes: the models' arguments of an AMPBlock conv1 (epi 0:
    Activation1d planes only), conv2 (1: + residual and fp32 state) or a resblock's last conv2 (2: residual into the
    accumulated output, no activation)."""
    kpad = (k * Cc + 31) // 32 * 32
    d = dict(a=0, w=0, bias=0, B=B, T=T, C=Cc, Cp=(Cc + 31) // 32 * 32, N=Cc, ksize=k, dil=dil, pad=(k - 1) * dil // 2,
             kpad=kpad, w_lo_off=Cc * kpad, prec=prec)
    if epi < 2:
        d.update(act_plane=0, act_alpha_exp=0, act_inv_beta=0, act_up_filter=0, act_down_filter=0,
                 act_plane_lo_off=B * T * d["Cp"])
    if epi > 0:
        d.update(res=0, out=0)
    if epi == 2:
        d.update(accumulate=1)
    return d


def load_dense_table():
    with open(DENSE_TABLE) as f:
        return json.load(f)


def dense_expected(t, case, tk, ncu, shapes=False):
    """The recorded plan of a table case under ALCM_TCONV = tk on ncu compute units, keyed as PLAN_KEYS."""
    B, T, Cc, prec, k, dil, epi, flops, nbytes, per_tk = case
    name, inst, block, ncg, tpb, ntiles, wslots, *grids = per_tk[t["tks"].index(tk)]
    return dict(name=t["names"][name] + (f" T{T} k{k}" if shapes else ""), inst=t["insts"][inst], block=block, ncg=ncg,
                tiles_per_batch=tpb, tiles=ntiles, wslots=wslots, flops=float(flops), bytes=float(nbytes),
                grid=grids[t["ncus"].index(ncu)])


def built_tail_instantiations():
    """The template-ids the launcher can emit: its list of built tile configurations (alcm_tconv.hip, tc_pick) times
    the three epilogue forms, spelled as ConvPlan::inst spells them."""
    with open(os.path.join(REPO, "audiolcm_amd", "csrc", "alcm_tconv.hip")) as f:
        src = f.read()
    cfgs = re.findall(r"^\s*tc_match<(CK_TCONV2?), ([0-9, ]+)>,$", src, re.M)
    out = set()
    for fam, nums in cfgs:
        Cc, NS, NPB, BM, R, KMAX, OCC, STG = (int(x) for x in nums.split(","))
        for epi in ("true, false, false, false", "true, true, true, false", "false, true, false, true"):
            if fam == "CK_TCONV2":
                out.add(f"tconv2_kernel<{Cc}, {NS}, {NPB}, {BM}, {R}, {epi}, {OCC}, {STG}>")
            else:
                out.add(f"tconv_kernel<{Cc}, {NS}, {NPB}, {BM}, {R}, {KMAX}, {OCC}, {epi}>")
    assert len(out) == 3 * len(cfgs)
    return out


def test_dense_table_reaches_every_instantiation():
    """The recorded calls reach every instantiation the launcher is built with, and name no other."""
    t = load_dense_table()
    built = built_tail_instantiations()
    assert len(built) == 51
    used = {t["insts"][r[1]] for c in t["cases"] for r in c[9]}
    assert used == built == set(t["insts"])
    grids = [(c[0] * r[4] * r[3], r[7]) for c in t["cases"] for r in c[9]]  # (tiles, grid at the first ncu)
    assert any(g == n for n, g in grids) and any(g < n for n, g in grids), "one workgroup per tile, and tile walkers"


def test_dense_planner_reproduces_recorded_choices():
    """Every recorded alcm_opconv_dense call gets the instantiation, launch geometry, kernel arguments (ncg,
    tiles_per_batch, ntiles, wslots), cost and profile name the dispatch had before the planner, under every ALCM_TCONV
    value and CU count, and every recorded rejection keeps its code and message."""
    t = load_dense_table()
    assert len(t["cases"]) >= 375 and len(t["rejects"]) >= 80
    bad, checked = [], 0
    for tk in t["tks"]:
        for shapes in (False, True):
            with knobs(tconv=tk, prof_shapes=int(shapes)):
                for c in t["cases"]:
                    a = row_args(dense_call(*c[:7]))
                    for ncu in t["ncus"]:
                        p, = K.conv_plan(a, ncu, dense=True)
                        want = dense_expected(t, c, tk, ncu, shapes)
                        checked += 1
                        if {k: p[k] for k in PLAN_KEYS} != want or p["kernel"] != want["inst"].split("_")[0]:
                            bad.append((tk, ncu, c[:7], want, p))
    with knobs(tconv=0):
        for c in t["cases"]:
            checked += 1
            if plan_rc(row_args(dense_call(*c[:7])), 1, 2, 256) != (E_INVALID, t["off_error"]):
                bad.append((0, c[:7]))
    for r in t["rejects"]:
        with knobs(**r["knobs"]):
            checked += 1
            got = plan_rc(row_args(r["args"]), 1, 2, r["ncu"])
            if got != (r["rc"], r["error"]):
                bad.append((r["what"], r["knobs"], got, r["error"]))
    assert not bad, f"{len(bad)} of {checked} differ, first: {bad[0]}"
    assert checked == len(t["cases"]) * (len(t["tks"]) * 2 * len(t["ncus"]) + 1) + len(t["rejects"])


def _out_is_res(d):
    d["out_is_res"] = 1


DENSE_DEFECTS = {  # what the dispatch used to let through: (spoil the row dict, form it applies to, message)
    "act, out == res": (_out_is_res, 1, "tconv: fused activation: out aliases res"),
    "act_plane & 3": (lambda d: d.update(act_plane=2), 0, "tconv: act_plane alignment"),
    "out_plane set": (lambda d: d.update(out_plane=0), 2, "tconv: no plane output"),
    "B = 0": (lambda d: d.update(B=0), 1, "opconv_dense: bad arguments"),
    "T < 0": (lambda d: d.update(T=-5), 0, "opconv_dense: bad arguments"),
}


@pytest.mark.parametrize("defect", sorted(DENSE_DEFECTS))
def test_dense_plan_rejects_what_the_dispatch_let_through(defect):
    """alcm_opconv_dense, from the C entry and from the models alike (one front door), refuses before any launch: a
    fused-activation call whose out is its res (tiles recompute halo rows: alcm_opconv refuses it too), a misaligned
    act_plane, an out_plane (there is no such epilogue; it used to be ignored), and B <= 0 / T <= 0 (the internal path
    did not check).  The same arguments without the defect plan."""
    spoil, epi, msg = DENSE_DEFECTS[defect]
    for Cc, prec, k in ((96, 2, 3), (48, 3, 7), (24, 3, 11)):
        d = dense_call(2, 300, Cc, prec, k, 1, epi)
        p, = K.conv_plan(row_args(d), 256, dense=True)
        assert p["kernel"] in ("tconv", "tconv2") and p["grid"] > 0 and p["block"] > 0
        spoil(d)
        assert plan_rc(row_args(d), 1, 2, 256) == (E_INVALID, msg), (defect, Cc)
    # (only the fused activation is refused: without it the call plans as it always did)
    if defect == "act, out == res":
        d = dense_call(2, 300, 48, 3, 7, 1, 2)
        _out_is_res(d)
        assert K.conv_plan(row_args(d), 256, dense=True)[0]["inst"].endswith("false, true, false, true>")


# ------------------------------------------------------------------ GPU: a real call records the planned row
def _conv_args(B, T, Cc, N, k, dil, prec, seed, out_plane=False, ws=False):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, Cc), generator=g) * 0.5
    w = torch.randn((N, Cc, k), generator=g) / np.sqrt(Cc * k)
    planes = K.operand_planes(x.cuda(), prec)
    Cp = planes.shape[3]
    packed = K.pack_conv_weight(torch.nn.functional.pad(w, (0, 0, 0, Cp - Cc)).contiguous().cuda())
    bias = (torch.randn((N,), generator=g) * 0.05).cuda()
    out = torch.empty((1, B, T, N), dtype=torch.int16, device="cuda") if out_plane else torch.empty((B, T, N), device="cuda")
    a = _hip.OpConvArgs()
    a.a, a.a_lo_off, a.B, a.T, a.C, a.Cp = _hip.ptr(planes), B * T * Cp, B, T, Cc, Cp
    a.ksize, a.dil, a.pad = k, dil, (k - 1) * dil // 2
    a.w, a.w_lo_off, a.kpad, a.N = _hip.ptr(packed.data), packed.lo_off, packed.kpad, N
    a.bias, a.out_scale, a.prec = _hip.ptr(bias), 1.0, int(prec)
    keep = [planes, packed, bias, out]
    if out_plane:
        a.out_plane = _hip.ptr(out)
    else:
        a.out = _hip.ptr(out)
    if ws:
        wsb = torch.empty(8 * B * T * N, device="cuda")
        a.ksplit_ws, a.ksplit_ws_floats = _hip.ptr(wsb), wsb.numel()
        keep.append(wsb)
    return a, keep


FAMILIES = {  # kernel family: (switches, [(B, T, C, N, k, dil, prec)], out_plane, workspace)
    "lin_plane": ({}, [(2, 300, 192, 192, 1, 1, 2)], True, False),
    "wconv3": ({"wconv3": 1}, [(2, 600, 192, 192, 3, 1, 2)], False, False),
    "wconv3_ksplit": ({}, [(2, 500, 768, 192, 3, 1, 2)], False, True),
    "wconv3_sum": ({"wconv3": 1}, [(2, 512, 192, 192, k, 1, 2) for k in (3, 5, 7)], False, False),
    "wconv2": ({}, [(2, 600, 192, 192, 3, 1, 0)], False, False),
    "nconv": ({}, [(2, 300, 24, 24, 3, 1, 2)], False, False),
    "opconv_kernel": ({}, [(2, 300, 48, 48, 7, 3, 1)], False, False),
}
TAIL_FAMILIES = {  # the tail convs through alcm_opconv_dense: (C, k, prec, epilogue form as dense_call) at B = 2, T = 300
    "tconv2_c96_persistent": (96, 3, 2, 0),
    "tconv_c48_resident": (48, 7, 3, 1),
    "tconv2_c24_per_tile": (24, 11, 3, 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_profile_row_is_the_planned_one(family):
    import torch
    _hip.require_device(0)
    sw, shapes, out_plane, ws = FAMILIES[family]
    built = [_conv_args(*s, seed=300 + i, out_plane=out_plane, ws=ws) for i, s in enumerate(shapes)]
    arr = (_hip.OpConvArgs * len(built))(*[b[0] for b in built])
    for i in range(1, len(built)):
        arr[i].out = None
    with knobs(**sw):
        if len(built) == 1:
            plans = K.conv_plan(arr[0])
        else:
            plans = K.conv_plan(list(arr))
        assert len(plans) == 1 and plans[0]["ncu"] == torch.cuda.get_device_properties(0).multi_processor_count
        assert family.startswith(plans[0]["kernel"]) and (plans[0]["ksplit"] > 1) == family.endswith("ksplit"), plans
        _hip.profile_begin()
        if len(built) == 1:
            _hip.check(_hip.lib().alcm_opconv(C.byref(arr[0]), _hip.stream_handle()), "opconv")
        else:
            _hip.check(_hip.lib().alcm_opconv_sum(arr, len(built), _hip.stream_handle()), "opconv_sum")
        torch.cuda.synchronize()
        rows = _hip.profile_end()
    assert [(r["name"], r["launches"]) for r in rows] == [(plans[0]["name"], 1)], (rows, plans)


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(TAIL_FAMILIES))
def test_tail_profile_row_is_the_planned_one(family):
    """One alcm_opconv_dense launch per tail family, on K.opconv(..., dense=True)'s packing: the recorded profile row is
    the plan's, and the plan is the recorded table's for this device's CU count (the kernels' numerics are
    test_gpu_ops.py's; what could go wrong here is the launcher taking another instantiation or grid than planned)."""
    import torch
    from audiolcm_amd.recipe import kaiser_sinc_filter1d
    _hip.require_device(0)
    Cc, k, prec, epi = TAIL_FAMILIES[family]
    B, T = 2, 300
    g = torch.Generator().manual_seed(400 + Cc)
    planes = K.operand_planes((torch.randn((B, T, Cc), generator=g) * 0.5).cuda(), prec)
    packed = K.pack_conv_weight((torch.randn((Cc, Cc, k), generator=g) / np.sqrt(Cc * k)).cuda())  # cpad = C: dense K
    bias = (torch.randn((Cc,), generator=g) * 0.05).cuda()
    res, out = torch.randn((B, T, Cc), generator=g).cuda(), torch.zeros((B, T, Cc), device="cuda")
    ae, ib = K.snake_params((torch.randn((Cc,), generator=g) * 0.3).cuda(), (torch.randn((Cc,), generator=g) * 0.3).cuda())
    ae, ib = ae.contiguous(), ib.contiguous()
    f = kaiser_sinc_filter1d(0.25, 0.3, 12).reshape(-1).float().cpu().contiguous()
    y = torch.zeros((1, B, T, (Cc + 31) // 32 * 32), dtype=torch.int16, device="cuda")
    a = _hip.OpConvArgs()
    a.a, a.B, a.T, a.C, a.Cp = _hip.ptr(planes), B, T, Cc, planes.shape[3]
    a.ksize, a.dil, a.pad = k, 1, (k - 1) // 2
    a.w, a.w_lo_off, a.kpad, a.N = _hip.ptr(packed.data), packed.lo_off, packed.kpad, Cc
    a.bias, a.out_scale, a.prec = _hip.ptr(bias), 1.0, prec
    if epi < 2:
        a.act_plane, a.act_alpha_exp, a.act_inv_beta = _hip.ptr(y), _hip.ptr(ae), _hip.ptr(ib)
        a.act_up_filter = a.act_down_filter = f.data_ptr()
    if epi > 0:
        a.res, a.out = _hip.ptr(res), _hip.ptr(out)
    if epi == 2:
        a.accumulate = 1
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    t = load_dense_table()
    assert ncu in t["ncus"], f"the table holds no grids for {ncu} compute units"
    case, = [c for c in t["cases"] if c[:7] == [B, T, Cc, prec, k, 1, epi]]
    plan, = K.conv_plan(a, dense=True)
    assert plan["ncu"] == ncu and family.startswith(plan["kernel"] + "_")
    assert {key: plan[key] for key in PLAN_KEYS} == dense_expected(t, case, 1, ncu)
    _hip.profile_begin()
    _hip.check(_hip.lib().alcm_opconv_dense(C.byref(a), _hip.stream_handle()), "opconv_dense")
    torch.cuda.synchronize()
    rows = _hip.profile_end()
    assert [(r["name"], r["launches"], r["flops"], r["bytes"]) for r in rows] == \
        [(plan["name"], 1, plan["flops"], plan["bytes"])], (rows, plan)
