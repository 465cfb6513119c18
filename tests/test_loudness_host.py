"""The loudness meter's host plan (audiolcm_amd/loudness.py), ``audio_in.check_level`` and the command-line options,
without a GPU.

The definition (ITU-R BS.1770-4, EBU R 128) is restated here in float64: K-weighting as a plain recursion loop over the
two biquads, mean squares over 400 ms blocks every 100 ms, the absolute gate at -70 LUFS and the relative gate 10 LU
under the mean of what the absolute gate kept."""
import math
import os
import struct

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
SHELF_A = (-1.69065929318241, 0.73248077421585)
HIGHPASS_A = (-1.99004745483398, 0.99007225036621)


def _biquad(x, b0, b1, b2, a1, a2):
    y = np.empty_like(x)
    x1 = x2 = y1 = y2 = 0.0
    for n in range(x.size):
        v = b0 * x[n] + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, x[n], y1, v
        y[n] = v
    return y


def _ref_lufs(x, hop):
    """Integrated loudness of the float64 clip x at 48 kHz with the standard's own table."""
    y = _biquad(_biquad(x, *SHELF_B, *SHELF_A), 1.0, -2.0, 1.0, *HIGHPASS_A)
    nb = (x.size - 4 * hop) // hop + 1
    z = np.array([np.mean(y[j * hop:j * hop + 4 * hop] ** 2) for j in range(nb)])
    l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    rel = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    keep &= l > rel
    return -0.691 + 10.0 * np.log10(z[keep].mean())


def test_k_weighting_meets_the_standards_table():
    from audiolcm_amd import loudness
    shelf, highpass = loudness.k_weighting(48000)
    np.testing.assert_allclose(shelf, SHELF_B + SHELF_A, rtol=0, atol=1e-12)
    np.testing.assert_allclose(highpass, (1.0, -2.0, 1.0) + HIGHPASS_A, rtol=0, atol=1e-12)


@pytest.mark.parametrize("rate,hop", [(16000, 1600), (44100, 4410), (8000, 800), (11025, 1103)])
def test_plan_geometry(rate, hop):
    from audiolcm_amd import loudness
    for n in (4 * hop, 4 * hop + hop - 1, 4 * hop + hop, 7 * rate + 13):
        pl = loudness.plan(rate, n)
        assert (pl.hop, pl.block, pl.nb, pl.nh) == (hop, 4 * hop, (n - 4 * hop) // hop + 1, n // hop)
        assert pl.nb == pl.nh - 3
    with pytest.raises(ValueError, match="400 ms"):
        loudness.plan(rate, 4 * hop - 1)


def test_tables_are_the_powers_of_the_transition_matrix():
    """coef: the ten biquad coefficients, then M^(CHUNK 2^j) and M^SPAN; M is checked against the recursion loop: the
    state-space form s' = M s + u x gives the loop's output for an impulse."""
    from audiolcm_amd import loudness
    for rate in (8000, 48000):
        shelf, highpass = loudness.k_weighting(rate)
        coef = loudness.tables(rate)
        assert coef.dtype == np.float64 and coef.size == loudness.COEF_DOUBLES == 154
        np.testing.assert_array_equal(coef[:10], shelf + highpass)
        M = loudness.transition(rate)
        for j in range(loudness.SCAN_STEPS + 1):
            want = np.linalg.matrix_power(M, loudness.CHUNK << j)
            np.testing.assert_allclose(coef[10 + 16 * j:26 + 16 * j].reshape(4, 4), want, rtol=1e-9, atol=1e-300)
        assert loudness.CHUNK << loudness.SCAN_STEPS == loudness.SPAN == 8192
        # impulse response through the state-space form against the loop
        b0, b1, b2, a1, a2 = shelf
        s = np.array([b1 - a1 * b0, b2 - a2 * b0, 0.0, 0.0])            # the state after x = 1 from zero state
        s[2:] = np.array([-2.0, 1.0]) * b0 - np.array(highpass[3:]) * b0  # y1 = y = b0
        x = np.zeros(64)
        x[0] = 1.0
        y = _biquad(_biquad(x, *shelf), *highpass)
        for n in range(1, 64):
            assert abs((s[0] + s[2]) - y[n]) <= 1e-12 * max(1.0, abs(y[n]))    # y = y1 + t1, y1 = s1 for x = 0
            s = M @ s


def test_997_hz_full_scale_sine_measures_minus_3_01_lufs():
    """The standard's calibration point: a 0 dBFS 997 Hz sine reads -3.01 LKFS (the float64 restatement: -3.0103)."""
    t = np.arange(2 * 48000, dtype=np.float64) / 48000.0
    assert abs(_ref_lufs(np.sin(2.0 * np.pi * 997.0 * t), 4800) - (-3.01)) <= 0.01


def test_check_level():
    from audiolcm_amd import audio_in
    assert audio_in.check_level(None, None, False) is None
    lv = audio_in.check_level(-23, None, False)
    assert (lv.loudness, lv.peak_dbfs, lv.true_peak) == (-23.0, -1.0, False)      # a target implies -1 dBFS
    lv = audio_in.check_level(None, -3, True)
    assert (lv.loudness, lv.peak_dbfs, lv.true_peak) == (None, -3.0, True)
    lv = audio_in.check_level(-14.0, 0.0, False)
    assert (lv.loudness, lv.peak_dbfs) == (-14.0, 0.0)
    for bad in (dict(loudness=0.5), dict(loudness=-70.5), dict(loudness=float("nan")), dict(peak_dbfs=0.1),
                dict(peak_dbfs=float("-inf")), dict(peak_dbfs=float("nan")), dict(true_peak=True)):
        with pytest.raises(ValueError):
            audio_in.check_level(**bad)


def _wav(path, n, rate):
    pcm = (np.random.default_rng(0).uniform(-0.5, 0.5, n) * 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", len(pcm)) + pcm)
    return str(path)


def test_keep_original_refuses_a_level(tmp_path):
    from audiolcm_amd import audio_in, cli
    a16 = _wav(tmp_path / "a16.wav", 24000, 16000)
    for kw in (dict(loudness=-23.0), dict(peak_dbfs=-1.0)):
        with pytest.raises(ValueError, match="bit for bit"):
            audio_in.plan_edit(a16, [(0.5, 1.0)], keep_original=True, **kw)
        plan = audio_in.plan_edit(a16, [(0.5, 1.0)], **kw)                      # an inpainting of the clip takes them
        assert plan.level == audio_in.check_level(**kw)
    assert audio_in.plan_edit(a16, [(0.5, 1.0)], keep_original=True).level is None
    with pytest.raises(ValueError, match="bit for bit"):
        cli.build(cli.parse_args(["--init-audio", a16, "--inpaint", "--mask-spans", "0.5-1.0", "--keep-original",
                                  "--loudness", "-23", "--synthetic-seed", "0", "-b", CONFIG]))


def test_level_is_checked_before_any_model(monkeypatch):
    from audiolcm_amd import cli, infer_api

    def stop(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(cli, "build_models", stop)
    monkeypatch.setattr(infer_api, "_build", stop)
    for fn, args in ((infer_api.AudioLCMInfer, ("rain",)), (infer_api.AudioLCMBatchInfer, (["rain"],)),
                     (infer_api.AudioLCMLongInfer, ("rain", 12.0))):
        with pytest.raises(ValueError, match="LUFS"):
            fn(*args, synthetic_seed=0, config_path=CONFIG, loudness=3.0)
        with pytest.raises(ValueError, match="true_peak"):
            fn(*args, synthetic_seed=0, config_path=CONFIG, true_peak=True)
    with pytest.raises(ValueError, match="dBFS"):
        cli.build(cli.parse_args(["--peak", "2", "--synthetic-seed", "0", "-b", CONFIG]))


def test_cli_parses_the_level_options():
    from audiolcm_amd.cli import parse_args
    opt = parse_args([])
    assert opt.loudness is None and opt.peak is None and opt.true_peak is False
    assert (opt.sample_rate, opt.ddim_steps, opt.scale, opt.H, opt.W) == (22050, 100, 5.0, 20, 312)
    opt = parse_args(["--loudness", "-23", "--peak", "-1.5", "--true-peak"])
    assert (opt.loudness, opt.peak, opt.true_peak) == (-23.0, -1.5, True)
    assert (opt.sample_rate, opt.ddim_steps, opt.scale, opt.H, opt.W) == (22050, 100, 5.0, 20, 312)
    assert math.isclose(parse_args(["--loudness=-14"]).loudness, -14.0)
