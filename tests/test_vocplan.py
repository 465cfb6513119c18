"""The BigVGAN stage planner (audiolcm_amd/csrc/alcm_vocplan.cpp): which upsampler form, AMPBlock form and chain
schedule every stage of the vocoder gets for a shape, a precision policy, a switch set and a batch.

tests/data/voc_plans.json holds, per case, the decisions the forward made before the planner existed (the booleans it
derived inside its stage loop, printed per stage while it ran on the recipe's weights on 256 compute units), as the
plan's fields.  The library's diagnostics entry (alcm_debug_voc_plan: host only, nothing is launched) must give them
back.  tests/test_gpu_vocplan.py checks that executing the plan launches what that forward launched.
"""
import contextlib
import json
import os

import pytest

from conftest import REPO

from audiolcm_amd import _hip, recipe
from audiolcm_amd import kernels as K

TABLE = os.path.join(REPO, "tests", "data", "voc_plans.json")


def load_table():
    with open(TABLE) as f:
        return json.load(f)


@contextlib.contextmanager
def switches(env):
    """The ALCM_* switches of a table case for the duration of the block."""
    old = {e: os.environ.get(e) for e in env}
    try:
        for e, v in env.items():
            os.environ[e] = str(v)
        _hip.reload_knobs()
        yield
    finally:
        for e, v in old.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v
        _hip.reload_knobs()


def plan_of(case, ncu):
    with switches(case["knobs"]):
        return K.voc_plan(recipe.BigVGANConfig(), case["policy"], case["streams"], case["B"], case["M"], ncu)


@pytest.fixture(scope="module")
def planned():
    t = load_table()
    return {cid: (c, plan_of(c, t["ncu"])) for cid, c in t["cases"].items()}


def test_table_covers_every_plan_form():
    cases = load_table()["cases"]
    assert len(cases) >= 25
    stages = [s for c in cases.values() for s in c["stages"]]
    assert {s["ups"] for s in stages} == set(_hip.VOC_UPS)
    assert {s["amp"] for s in stages} == set(_hip.VOC_AMP)
    for field in ("act3", "sum3", "writes_next", "concurrent", "own_bufs", "planes_from_prev"):
        assert {s[field] for s in stages} == {0, 1}, field
    assert any({s["h16"] for s in c["stages"] if s["amp"] == "wide"} == {0, 1} for c in cases.values()), \
        "h16 on and off within one forward"
    assert {s["prec"] for s in stages} == {_hip.PREC_BF16, _hip.PREC_SPLIT, _hip.PREC_F16, _hip.PREC_F16W2}


def test_planner_reproduces_recorded_decisions(planned):
    bad = [(cid, si, want, got) for cid, (c, plans) in planned.items()
           for si, (want, got) in enumerate(zip(c["stages"], plans)) if want != got]
    assert all(len(plans) == len(c["stages"]) == 6 for c, plans in planned.values())
    assert not bad, f"{len(bad)} stages differ, first: {bad[0]}"


def test_plan_invariants(planned):
    """What held only by construction inside the stage loop."""
    cfg = recipe.BigVGANConfig()
    shapes = K.voc_stage_shapes(cfg)
    for cid, (c, plans) in planned.items():
        To = c["M"]
        with switches(c["knobs"]):
            for si, (h, p) in enumerate(zip(shapes, plans)):
                To *= h.rate
                if p["amp"] == "fused_dense":  # every conv of the stage is one the tail kernels take
                    for k in cfg.resblock_kernel_sizes:
                        for d in cfg.resblock_dilation_sizes[0]:
                            a = _hip.OpConvArgs()
                            a.a, a.w, a.bias, a.res, a.out = (i << 32 for i in range(1, 6))
                            a.B, a.T, a.C, a.Cp, a.N = c["B"], To, h.cout, (h.cout + 31) // 32 * 32, h.cout
                            a.ksize, a.dil, a.pad, a.kpad = k, d, (k - 1) * d // 2, (k * h.cout + 31) // 32 * 32
                            a.out_scale, a.accumulate, a.prec = 1.0, 1, p["prec"]
                            assert K.conv_plan(a, 256, dense=True)[0]["kernel"] in ("tconv", "tconv2"), (cid, si, k, d)
                assert p["planes_from_prev"] == (plans[si - 1]["writes_next"] if si else 0), (cid, si)
                if p["planes_from_prev"]:
                    assert p["ups"] == "planes", (cid, si)
                if p["sum3"]:
                    assert len(cfg.resblock_kernel_sizes) == 3 and p["amp"] == "wide" and p["own_bufs"], (cid, si)
                if p["writes_next"]:
                    assert p["sum3"] and si + 1 < len(plans), (cid, si)
                if p["h16"]:
                    assert p["amp"] == "wide" and p["prec"] == _hip.PREC_F16 and c["B"] * To >= 1024, (cid, si)
                assert p["own_bufs"] == (p["concurrent"] or p["act3"]), (cid, si)


def test_plan_depends_on_the_device_only_through_the_sum_form():
    """On fewer compute units a smaller batch fills the chip: the one-launch sum form, and with it the plane hand-off
    to the next stage, starts earlier; nothing else moves."""
    # B = 2, M = 624: stages 0-2 have 80 / 156 / 156 full 256 x 192 tiles
    c = dict(policy="mixed", streams=1, B=2, M=624, knobs={})
    few, many = plan_of(c, 64), plan_of(c, 256)
    assert [p["writes_next"] for p in few] == [1, 1, 1, 0, 0, 0] and not any(p["writes_next"] for p in many)
    strip = lambda ps: [{k: v for k, v in p.items() if k not in ("writes_next", "planes_from_prev")} for p in ps]
    assert strip(few) == strip(many)


def test_bad_arguments_are_refused():
    shapes = K.voc_stage_shapes(recipe.BigVGANConfig())
    for B, M in ((0, 20), (1, 0)):
        with pytest.raises(_hip.HipError):
            _hip.debug_voc_plan(shapes, _hip.POLICY_MIXED, True, B, M, 256)
    shapes[2].nrb = _hip.VOC_MAX_RB + 1
    with pytest.raises(_hip.HipError):
        _hip.debug_voc_plan(shapes, _hip.POLICY_MIXED, True, 1, 20, 256)
