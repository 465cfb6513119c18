"""The operand-plane conv planner (audiolcm_amd/csrc/alcm_convplan.cpp): which kernel, tile, K parts and profile name
an alcm_opconv / alcm_opconv_sum call gets, and which calls it rejects.

The CPU tests ask the library's diagnostics entry (alcm_debug_conv_plan: nothing is launched, pointers are only
tested for null-ness and alignment) and compare with tests/data/conv_plans.json, a table of (arguments, switches,
profile names) recorded from the build before the planner existed while it ran the benchmark and the GPU op tests.
The GPU tests check that a real call of each kernel family records exactly the profile row the planner names.
"""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import REPO

from audiolcm_amd import _hip
from audiolcm_amd import kernels as K

TABLE = os.path.join(REPO, "tests", "data", "conv_plans.json")
KNOB_ENV = {"wconv": ("ALCM_WCONV", 8), "wconv3": ("ALCM_WCONV3", -1), "wconv3_grid": ("ALCM_WCONV3_GRID", 0),
            "nconv": ("ALCM_NCONV", -1), "opconv_tile": ("ALCM_OPCONV_TILE", 0), "lin1": ("ALCM_LIN1", -1),
            "ups_t160": ("ALCM_UPS_T160", 1), "wconv_sum": ("ALCM_WCONV_SUM", 1), "ksplit": ("ALCM_KSPLIT", 1),
            "prof_shapes": ("ALCM_PROF_SHAPES", 0)}
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


def plan_rc(args, n, as_sum, ncu):
    out = (_hip.ConvPlanInfo * 3)()
    nl = C.c_int(0)
    rc = _hip.lib().alcm_debug_conv_plan(args if as_sum else C.byref(args), n, int(as_sum), ncu, out, C.byref(nl))
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
