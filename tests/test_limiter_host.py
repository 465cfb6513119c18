"""The limiter's host side without a GPU: ``limiter.plan``, the refusals of ``check_level`` / ``plan_edit`` / the command
line (each names its flag), the ALCM_E_INVALID cases of ``alcm_limiter`` (all returned before any HIP call, so they need
no device), and the float64 restatement of ``tests/_limiter_ref.py`` that the GPU tests compare against, checked on its
own: s <= r everywhere, the ramp arrives at the peak, and the scan form of the release equals the loop."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

import _limiter_ref as ref
from conftest import REPO

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
E_INVALID = -1


def test_plan_geometry():
    from audiolcm_amd import limiter
    assert (limiter.CHUNK, limiter.LANES, limiter.SPAN) == (8, 256, 2048) and limiter.MAX_LOOKAHEAD == 1024
    p = limiter.plan(16000, 32000)
    assert (p.rate, p.n, p.lookahead) == (16000, 32000, 80)
    assert p.release_coef == math.exp(-1.0 / (0.1 * 16000))
    p = limiter.plan(48000, 5, 2.5, 50.0)
    assert p.lookahead == 120 and p.release_coef == math.exp(-1.0 / (0.05 * 48000))
    assert limiter.plan(44100, 0, 0.0).lookahead == 0
    assert limiter.plan(192000, 0, 5.0).lookahead == 960
    assert limiter.plan(16000, 0, 64.0).lookahead == 1024


def test_plan_refusals():
    from audiolcm_amd import limiter
    with pytest.raises(ValueError, match="--limiter-lookahead-ms.*1024"):
        limiter.plan(16000, 0, 64.1)
    with pytest.raises(ValueError, match="--limiter-lookahead-ms.*1024"):
        limiter.plan(48000, 0, 22.0)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--limiter-lookahead-ms"):
            limiter.plan(16000, 0, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--limiter-release-ms"):
            limiter.plan(16000, 0, 5.0, bad)
    with pytest.raises(ValueError, match="--limiter-release-ms.*never releases"):
        limiter.plan(192000, 0, 5.0, 1e18)
    with pytest.raises(ValueError):
        limiter.plan(0, 0)


def test_check_level_takes_the_limiter():
    from audiolcm_amd import audio_in
    lv = audio_in.check_level(-14.0, None, False, True)
    assert (lv.loudness, lv.peak_dbfs, lv.limiter, lv.lookahead_ms, lv.release_ms) == (-14.0, -1.0, True, 5.0, 100.0)
    lv = audio_in.check_level(None, -3.0, True, True, 2.0, 30.0)
    assert (lv.peak_dbfs, lv.true_peak, lv.limiter, lv.lookahead_ms, lv.release_ms) == (-3.0, True, True, 2.0, 30.0)
    assert audio_in.check_level(-14.0).limiter is False
    assert audio_in.check_level(-14.0) == audio_in.Level(-14.0, -1.0, False)        # the level of before, unchanged
    with pytest.raises(ValueError, match="--limiter.*--loudness.*--peak"):
        audio_in.check_level(limiter=True)
    with pytest.raises(ValueError, match="--limiter-lookahead-ms"):
        audio_in.check_level(-14.0, limiter=True, limiter_lookahead_ms=-1.0)
    with pytest.raises(ValueError, match="--limiter-release-ms"):
        audio_in.check_level(-14.0, limiter=True, limiter_release_ms=0.0)
    assert audio_in.check_level(-14.0, limiter_release_ms=0.0).limiter is False     # the times belong to the limiter


def _wav(path, n, rate):
    pcm = (np.random.default_rng(0).uniform(-0.5, 0.5, n) * 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", len(pcm)) + pcm)
    return str(path)


def test_plan_edit_refusals(tmp_path):
    from audiolcm_amd import audio_in
    a16 = _wav(tmp_path / "a16.wav", 24000, 16000)
    plan = audio_in.plan_edit(a16, loudness=-14.0, limiter=True, limiter_lookahead_ms=3.0)
    assert plan.level == audio_in.Level(-14.0, -1.0, False, True, 3.0, 100.0)
    with pytest.raises(ValueError, match="--limiter.*--loudness"):
        audio_in.plan_edit(a16, limiter=True)
    with pytest.raises(ValueError, match="--keep-original.*--limiter"):
        audio_in.plan_edit(a16, [(0.5, 1.0)], keep_original=True, limiter=True)
    with pytest.raises(ValueError, match="--extend.*--limiter"):
        audio_in.plan_edit(a16, extend_s=1.0, limiter=True)
    for vary in (False, True):
        with pytest.raises(ValueError, match="--limiter.*--loop-from.*period"):
            audio_in.plan_edit(a16, loop_from=True, loop_vary=vary, loudness=-14.0 if vary else None, limiter=True)
    with pytest.raises(ValueError, match="--limiter-release-ms"):
        audio_in.plan_edit(a16, loudness=-14.0, limiter=True, limiter_release_ms=-5.0)


def test_cli_flags_and_refusals(tmp_path, monkeypatch):
    from audiolcm_amd import cli, infer_api

    def stop(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(cli, "build_models", stop)
    monkeypatch.setattr(infer_api, "_build", stop)
    opt = cli.parse_args([])
    assert (opt.limiter, opt.limiter_lookahead_ms, opt.limiter_release_ms) == (False, 5.0, 100.0)
    opt = cli.parse_args(["--loudness", "-14", "--limiter", "--limiter-lookahead-ms", "2", "--limiter-release-ms", "40"])
    assert (opt.limiter, opt.limiter_lookahead_ms, opt.limiter_release_ms) == (True, 2.0, 40.0)
    a16 = _wav(tmp_path / "a16.wav", 24000, 16000)
    base = ["--synthetic-seed", "0", "-b", CONFIG]
    for argv, msg in (
            (["--limiter"], "--limiter.*--loudness.*--peak"),
            (["--limiter", "--loudness", "-14", "--limiter-lookahead-ms", "-1"], "--limiter-lookahead-ms"),
            (["--limiter", "--loudness", "-14", "--limiter-release-ms", "0"], "--limiter-release-ms"),
            (["--limiter", "--loudness", "-14", "--limiter-lookahead-ms", "30", "--out-sample-rate", "48000"],
             "--limiter-lookahead-ms.*1024"),
            (["--limiter", "--loudness", "-14", "--loop"], "--limiter.*--loop.*period"),
            (["--limiter", "--loop-from", a16], "--limiter.*--loop-from.*period"),
            (["--limiter", "--loudness", "-14", "--loop-from", a16, "--loop-vary"], "--limiter.*--loop-from.*period"),
            (["--limiter", "--init-audio", a16, "--extend", "1.0"], "--extend.*--limiter"),
            (["--limiter", "--init-audio", a16, "--inpaint", "--mask-spans", "0.5-1.0", "--keep-original"],
             "--keep-original.*--limiter")):
        with pytest.raises(ValueError, match=msg):
            cli.build(cli.parse_args(argv + base))
    for fn, args in ((infer_api.AudioLCMInfer, ("rain",)), (infer_api.AudioLCMBatchInfer, (["rain"],)),
                     (infer_api.AudioLCMLongInfer, ("rain", 12.0))):
        with pytest.raises(ValueError, match="--limiter.*--loudness"):
            fn(*args, synthetic_seed=0, config_path=CONFIG, limiter=True)
        with pytest.raises(ValueError, match="--limiter-lookahead-ms.*1024"):
            fn(*args, synthetic_seed=0, config_path=CONFIG, loudness=-14.0, limiter=True, limiter_lookahead_ms=70.0)
    with pytest.raises(ValueError, match="--limiter.*--loop.*period"):
        infer_api.AudioLCMLongInfer("rain", 12.0, synthetic_seed=0, config_path=CONFIG, loudness=-14.0, loop=True,
                                    limiter=True)
    with pytest.raises(ValueError, match="--limiter.*--loop-from.*period"):
        infer_api.AudioLCMEditInfer("rain", a16, synthetic_seed=0, config_path=CONFIG, loop_from=True, limiter=True)


def test_alcm_limiter_refuses_before_any_hip_call():
    """Every refusal is decided from the arguments alone; the pointers are never dereferenced."""
    from audiolcm_amd import _hip
    L = _hip.lib()
    wsb = L.alcm_limiter_workspace_bytes
    assert wsb(2, 5000, 80) == 8 * 2 * (5000 + 3 * 3) and wsb(1, 2048, 0) == 8 * (2048 + 3)
    assert wsb(0, 100, 80) == 0 and wsb(1, 0, 80) == 0 and wsb(1, 100, -1) == 0 and wsb(1, 100, 1025) == 0
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    f = lambda a: a                                                                 # noqa: E731  (raw addresses)
    good = dict(x=f(p), env=None, os=1, gain=f(p), y=f(p), B=1, N=100, ldx=100, ld_env=0, ldy=100, ceiling=0.9,
                lookahead=80, release_coef=0.999, ws=p, ws_bytes=wsb(1, 100, 80), stream=None)
    order = list(good)

    def rc(**kw):
        a = dict(good, **kw)
        return L.alcm_limiter(*(a[k] for k in order))
    cases = [dict(x=None), dict(gain=None), dict(y=None), dict(env=f(p), os=2, ld_env=400), dict(env=f(p), os=0),
             dict(B=-1), dict(N=-1), dict(ldx=99), dict(ldy=99), dict(env=f(p), os=4, ld_env=399),
             dict(env=f(p), os=1, ld_env=99), dict(ceiling=0.0), dict(ceiling=-1.0), dict(ceiling=float("inf")),
             dict(ceiling=float("nan")), dict(lookahead=-1), dict(lookahead=1025), dict(release_coef=1.0),
             dict(release_coef=-0.1), dict(release_coef=float("nan")), dict(ws=None), dict(ws=p + 4),
             dict(ws_bytes=wsb(1, 100, 80) - 1)]
    for kw in cases:
        assert rc(**kw) == E_INVALID, kw
        assert b"limiter" in L.alcm_last_error(), kw
    assert rc(B=0) == 0 and rc(N=0, ws=None, ws_bytes=0) == 0                       # nothing to do: no launch


# ---------------------------------------------------------------------------- the restatement itself
def _case(La, a=math.exp(-1.0 / 1600.0), n=1500, seed=3):
    x, _ = ref.edge_signal(n, 700, 80, seed)
    out, d = ref.limiter(x, np.float32(2.5), ref.ceiling_of(-1.0), La, a)
    return x, out, d


@pytest.mark.parametrize("La", [0, 1, 80, 300])
def test_restatement_attack_stays_under_the_required_gain(La):
    c = ref.ceiling_of(-1.0)
    x, out, d = _case(La)
    over = d["e"] > c
    assert over.sum() > 10 and d["r"].min() < 0.4
    assert (d["s"] <= d["r"] * (1 + 1e-15)).all()                                   # the mean's own rounding
    assert (d["y"] <= d["s"]).all() and (d["y"] > 0).all()
    assert np.abs(out).max() <= c
    assert np.abs(d["u"].astype(np.float64) * d["y"]).max() <= float(c) * (1 + 1e-15)
    first = int(np.argmax(over))
    if first > La:
        assert (d["s"][:first - La] == 1.0).all() and (out[:first - La] == d["u"][:first - La]).all()
    p = 350                                                                         # the isolated spike
    assert over[p] and abs(d["s"][p] - d["r"][p]) <= 1e-15                           # the ramp arrives at the peak
    if 1 < La <= 80:                                                                # no other peak within the ramp
        assert d["s"][p - La // 2] > d["s"][p] and d["s"][p - La] > d["s"][p - La // 2]


@pytest.mark.parametrize("n,La", [(4133, 80), (4133, 0), (4133, 1), (4133, 3), (4133, 511), (4133, 512), (4133, 1024),
                                  (1, 80), (50, 80), (2048, 80)])
def test_tile_arithmetic_of_the_kernel_gives_the_restatements_attack(n, La):
    """``ref.tile_attack`` restates the kernel's first launch index for index (halo, doubling maximum, tile-local prefix
    sum, the difference (P[n + La] - P[n - 1]) / (La + 1)); ``ref.curve`` is the definition.  Bar: a running sum of k
    values of at most 1 is off by at most (k - 1) u k, u = 2^-53, k = span + La <= 3072, and s takes the difference of
    two of them over La + 1: 2 * 3071 * 3072 * 2^-53 / (La + 1) = 2.1e-9 / (La + 1), plus one ulp of the quotient.
    Measured: 1.0e-13 at the worst over these shapes, three orders under the 6e-8 of an fp32 ulp."""
    from audiolcm_amd import limiter
    c = ref.ceiling_of(-1.0)
    x, _ = ref.edge_signal(n, limiter.SPAN, 80)
    _, e = ref.envelope(x, np.float32(2.5))
    r, s = ref.curve(e, c, La)
    got = ref.tile_attack(e, c, La, limiter.SPAN)
    err = float(np.abs(got - s).max())
    print(f"N {n}, La {La}: the tile arithmetic is within {err:.2e} of the definition's s")
    assert err <= 2 * 3071 * 3072 * 2.0 ** -53 / (La + 1) + 2.0 ** -52


def test_tile_arithmetic_leaves_a_tile_of_ones_exact():
    """The prefix sum starts at the tile, so before the first ramp every s is exactly 1, whatever came in earlier tiles'
    sums: the clip is untouched, bit for bit, until La before its first peak."""
    from audiolcm_amd import limiter
    n, La, c = 3 * limiter.SPAN + 37, 80, ref.ceiling_of(-1.0)
    e = np.full(n, 0.5, np.float32)
    first = 2 * limiter.SPAN + 5
    e[first] = 2.25
    e[100] = 1.7                                        # an earlier tile's sums are not whole numbers
    s = ref.tile_attack(e, c, La, limiter.SPAN)
    assert (s[limiter.SPAN:first - La] == 1.0).all() and s[first - La] < 1.0
    assert abs(s[first] - float(c) / 2.25) <= 1e-14     # the ramp arrives; the difference of two sums rounds


@pytest.mark.parametrize("a", [0.0, math.exp(-1.0 / 1600.0), math.exp(-1.0 / 160000.0)])
def test_restatement_scan_equals_loop(a):
    _, _, d = _case(80, a)
    y = ref.release_scan(d["s"], a)
    assert np.abs(y - d["y"]).max() <= 1e-12
    assert (y <= d["s"]).all()                                                      # the last map's C is s[n] itself
    if a == 0.0:
        assert (d["y"] == d["s"]).all()


def test_restatement_pipeline_reaches_the_target_a_static_gain_misses():
    rate, c = 16000, ref.ceiling_of(-1.0)
    x = ref.burst_signal(rate)
    st = ref.static64(x, rate, -14.0, c)
    lim = ref.pipeline64(x, rate, -14.0, c, 80, math.exp(-1.0 / 1600.0), 3)
    print(f"static {st['lufs_out']:.3f} LUFS, limiter {lim['lufs_out']:.3f} LUFS")
    assert lim["binds"] and np.abs(lim["wav"]).max() <= c and np.abs(st["wav"]).max() <= c
    assert abs(st["lufs_out"] + 14.0) - abs(lim["lufs_out"] + 14.0) >= 3.0
    assert min(st["margin"], lim["margin"]) >= 0.5
