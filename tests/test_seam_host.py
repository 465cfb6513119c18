"""The fade laws' host side without a GPU: the plan fields and every refusal of ``fade_law`` / ``match_gain`` (each names
its flags, before any model is built), the ALCM_E_INVALID cases of ``alcm_seam_stats`` and ``alcm_wave_paste_law`` (all
returned before any HIP call, so they need no device), and the float64 restatement of ``tests/_seam_ref.py`` that the
GPU tests compare against, checked on its own: the geometry on a hand-made case, rho = 1 gives the linear law back, and
independent noise loses a quarter of its power through the linear fade and none through the matched one."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import _seam_ref as ref
from conftest import REPO

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
E_INVALID = -1


def _wav(path, n, rate):
    pcm = (np.random.default_rng(0).uniform(-0.5, 0.5, n) * 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", len(pcm)) + pcm)
    return str(path)


def test_plan_fields_and_refusals(tmp_path):
    from audiolcm_amd import audio_in
    a16 = _wav(tmp_path / "a16.wav", 48000, 16000)
    plan = audio_in.plan_edit(a16, [(0.5, 1.0)], keep_original=True)
    assert (plan.fade_law, plan.match_gain) == ("linear", False)
    for kw in (dict(mask_spans=[(0.5, 1.0)], keep_original=True), dict(extend_s=1.0), dict(loop_from=True)):
        for law in audio_in.FADE_LAWS:
            plan = audio_in.plan_edit(a16, fade_law=law, match_gain=law != "matched", **kw)
            assert (plan.fade_law, plan.match_gain) == (law, law != "matched"), kw
    assert audio_in.plan_loop(a16, fade_law="matched").fade_law == "matched"
    with pytest.raises(ValueError, match="--fade-law.*linear, equal-power, matched.*'cubic'"):
        audio_in.plan_edit(a16, [(0.5, 1.0)], keep_original=True, fade_law="cubic")
    with pytest.raises(ValueError, match="--fade-law.*'cubic'"):
        audio_in.plan_loop(a16, fade_law="cubic")
    for kw in (dict(), dict(mask_spans=[(0.5, 1.0)]), dict(joint=True)):          # variation, inpainting: no paste
        for opt in (dict(fade_law="matched"), dict(fade_law="equal-power"), dict(match_gain=True)):
            with pytest.raises(ValueError, match="--fade-law, --match-gain.*--keep-original, --extend, --loop-from"):
                audio_in.plan_edit(a16, **kw, **opt)
    for opt in (dict(fade_law="matched"), dict(match_gain=True)):
        with pytest.raises(ValueError, match="--fade-law, --match-gain.*--loop-vary.*pastes nothing"):
            audio_in.plan_edit(a16, loop_from=True, loop_vary=True, **opt)
        with pytest.raises(ValueError, match="--fade-law, --match-gain.*--loop-vary"):
            audio_in.plan_loop(a16, vary=True, **opt)


def test_cli_flags_and_refusals(tmp_path, monkeypatch):
    from audiolcm_amd import cli, infer_api

    def stop(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(cli, "build_models", stop)
    monkeypatch.setattr(infer_api, "_build", stop)
    opt = cli.parse_args([])
    assert (opt.fade_law, opt.match_gain) == ("linear", False)
    opt = cli.parse_args(["--fade-law", "equal-power", "--match-gain"])
    assert (opt.fade_law, opt.match_gain) == ("equal-power", True)
    with pytest.raises(SystemExit):
        cli.parse_args(["--fade-law", "cubic"])
    a16 = _wav(tmp_path / "a16.wav", 48000, 16000)
    base = ["--synthetic-seed", "0", "-b", CONFIG]
    used_with = "--fade-law.*--match-gain.*--keep-original, --extend or --loop-from"
    for argv, msg in (
            (["--fade-law", "matched"], used_with),
            (["--match-gain"], used_with),
            (["--match-gain", "--duration", "12"], used_with),
            (["--fade-law", "equal-power", "--loop"], used_with),
            (["--fade-law", "matched", "--init-audio", a16], used_with),
            (["--match-gain", "--init-audio", a16, "--inpaint", "--mask-spans", "0.5-1.0"], used_with),
            (["--fade-law", "matched", "--loop-from", a16, "--loop-vary"], "--fade-law.*--match-gain.*--loop-vary"),
            (["--match-gain", "--loop-from", a16, "--loop-vary"], "--fade-law.*--match-gain.*--loop-vary")):
        with pytest.raises(ValueError, match=msg):
            cli.build(cli.parse_args(argv + base))
    # accepted requests get as far as the models
    for argv in (["--init-audio", a16, "--inpaint", "--mask-spans", "0.5-1.0", "--keep-original", "--fade-law", "matched",
                  "--match-gain"],
                 ["--init-audio", a16, "--extend", "1.0", "--fade-law", "equal-power"],
                 ["--loop-from", a16, "--match-gain"]):
        with pytest.raises(AssertionError, match="a model was built"):
            cli.build(cli.parse_args(argv + base))
    with pytest.raises(ValueError, match="--fade-law, --match-gain.*--keep-original"):
        infer_api.AudioLCMEditInfer("rain", a16, synthetic_seed=0, config_path=CONFIG, fade_law="matched")
    with pytest.raises(ValueError, match="--fade-law, --match-gain.*--loop-vary"):
        infer_api.AudioLCMEditInfer("rain", a16, synthetic_seed=0, config_path=CONFIG, loop_from=True, loop_vary=True,
                                    match_gain=True)
    with pytest.raises(ValueError, match="--fade-law.*'cubic'"):
        infer_api.AudioLCMEditInfer("rain", a16, synthetic_seed=0, config_path=CONFIG, mask_spans=[(0.5, 1.0)],
                                    keep_original=True, fade_law="cubic")
    with pytest.raises(AssertionError, match="a model was built"):
        infer_api.AudioLCMEditInfer("rain", a16, synthetic_seed=0, config_path=CONFIG, mask_spans=[(0.5, 1.0)],
                                    keep_original=True, fade_law="matched", match_gain=True)


def test_the_c_entries_refuse_before_any_hip_call():
    """Every refusal is decided from the arguments alone, in the paste's words; the pointers are never dereferenced."""
    from audiolcm_amd import _hip
    L = _hip.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    stats = dict(orig=p, gen=p, mask=p, B=1, N=96, gen_start=8, Ng=40, T=12, frame_samples=8, R=12, ring=0, rho=p, gam=p,
                 sums=p, stream=None)
    paste = dict(orig=p, gen=p, mask=p, ramp=p, rho=p, gam=p, out=p, B=1, N=96, gen_start=8, Ng=40, T=12,
                 frame_samples=8, R=12, ring=0, stream=None)
    shared = [(dict(orig=None), "null orig, out or mask"), (dict(mask=None), "null orig, out or mask"),
              (dict(B=-1), "negative B, N, Ng, gen_start, T or R"), (dict(N=-1), "negative"), (dict(Ng=-1), "negative"),
              (dict(gen_start=-1), "negative"), (dict(T=-1), "negative"), (dict(R=-1), "negative"),
              (dict(frame_samples=0), "frame_samples outside 1 .. 2^20"),
              (dict(frame_samples=(1 << 20) + 1, N=0, Ng=0, gen_start=0), "frame_samples outside 1 .. 2^20"),
              (dict(T=11), "the mask's T * frame_samples is shorter than N"),
              (dict(gen_start=60), "gen reaches past the clip"), (dict(R=129), "R exceeds 16 frames"),
              (dict(gen=None), "null gen or ramp"),
              (dict(ring=1, T=13), "N must be the mask's T * frame_samples, one period"),
              (dict(ring=1, Ng=97), "gen is longer than the ring"), (dict(ring=1, gen_start=96), "gen starts past the ring")]
    for name, good, fn, extra in (
            ("seam_stats", stats, L.alcm_seam_stats,
             [(dict(rho=None), "null rho, gam or sums"), (dict(gam=None), "null rho, gam or sums"),
              (dict(sums=None), "null rho, gam or sums"), (dict(sums=p + 4), "sums is not 8-byte aligned")]),
            ("wave_paste_law", paste, L.alcm_wave_paste_law,
             [(dict(out=None), "null orig, out or mask"), (dict(ramp=None), "null gen or ramp")])):
        order = list(good)
        for kw, words in shared + extra:
            a = dict(good, **kw)
            assert fn(*(a[k] for k in order)) == E_INVALID, (name, kw)
            msg = L.alcm_last_error().decode()
            assert msg.startswith(name + ": ") and words in msg, (name, kw, msg)
        a = dict(good, B=0)                                                      # nothing to do: no launch
        assert fn(*(a[k] for k in order)) == 0
    a = dict(stats, T=0, N=0, Ng=0, gen_start=0)
    assert L.alcm_seam_stats(*(a[k] for k in stats)) == 0
    a = dict(paste, N=0, Ng=0, gen_start=0, rho=None, gam=None)                  # both tables are optional
    assert L.alcm_wave_paste_law(*(a[k] for k in paste)) == 0
    # the ring takes gen up to the start of the period and across the wrap, where the line refuses
    a = dict(stats, ring=1, gen_start=90, B=0)
    assert L.alcm_seam_stats(*(a[k] for k in stats)) == 0


# ---------------------------------------------------------------------------- the restatement itself
def test_geometry_on_a_hand_made_case():
    """4 samples per frame, frames 1 and 3 regenerated: the one-frame gap between them splits 2 + 2, the 12 kept samples
    round the wrap of the ring 6 + 6; 3 samples per frame and a one-frame gap: the tie in its middle goes right."""
    m = np.array([0, 1, 0, 1, 0, 0], np.float32)
    d, edge, frame = ref.geometry(m, 4, 24, ring=False)
    assert d.tolist() == [4, 3, 2, 1, 0, 0, 0, 0, 1, 2, 2, 1, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert edge.tolist() == [1] * 4 + [-1] * 4 + [2, 2, 3, 3] + [-1] * 4 + [4] * 8
    assert frame.tolist() == [1] * 4 + [1] * 4 + [1, 1, 3, 3] + [3] * 4 + [3] * 8
    d, edge, frame = ref.geometry(m, 4, 24, ring=True)                              # round the wrap: 4 + 8 kept samples
    assert d[16:].tolist() + d[:4].tolist() == [1, 2, 3, 4, 5, 6, 6, 5, 4, 3, 2, 1]
    assert edge[16:].tolist() + edge[:4].tolist() == [4] * 6 + [1] * 6
    m = np.array([1, 0, 1], np.float32)                                             # 3 samples per frame: a tie at n = 4
    d, edge, frame = ref.geometry(m, 3, 9, ring=False)
    assert d.tolist() == [0, 0, 0, 1, 2, 1, 0, 0, 0] and edge[3:6].tolist() == [1, 2, 2] and frame[3:6].tolist() == [0, 2, 2]
    assert ref.runs(np.array([1, 1, 0, 1], np.float32), False) == [([0, 1], [0, 2]), ([3], [3, 4])]
    assert ref.runs(np.array([1, 1, 0, 1], np.float32), True) == [([3, 0, 1], [3, 2])]
    assert ref.runs(np.ones(3, np.float32), True) == [([0, 1, 2], [])]
    assert ref.runs(np.zeros(3, np.float32), True) == []


def _noise(seed_o, seed_g, T=40, fs=512):
    B = 2
    orig = np.random.default_rng(seed_o).standard_normal((B, T * fs)).astype(np.float32)
    gen = np.random.default_rng(seed_g).standard_normal((B, T * fs)).astype(np.float32)
    mask = np.zeros((B, T), np.float32)
    mask[0, 16:24] = 1.0
    mask[1, 14:22] = 1.0
    return orig, gen, mask, fs


NOISE_SEEDS = (11, 12)
NOISE_R = 4096


def test_restatement_rho_one_is_the_linear_law():
    orig, gen, mask, fs = _noise(*NOISE_SEEDS)
    lin, g = ref.blend_linear(orig, gen, mask, fs, 0, NOISE_R)
    out, g2, _ = ref.blend(orig, gen, mask, fs, 0, NOISE_R, rho=np.ones((2, mask.shape[1] + 1)))
    assert np.array_equal(g, g2) and ((g > 0) & (g < 1)).sum() == 2 * 2 * (NOISE_R - 1)
    assert np.abs(out - lin).max() <= 1e-12 * np.abs(lin).max()
    # and rho = 0 with gen == orig is not: the equal-power law lifts correlated signals by up to 3 dB
    out, _, _ = ref.blend(orig, orig, mask, fs, 0, NOISE_R)
    mid = np.abs(g - 0.5) < 1e-3
    assert mid.any() and np.allclose(out[mid] / orig[mid].astype(np.float64), np.sqrt(2.0), rtol=1e-3)


def test_restatement_keeps_the_power_of_independent_noise():
    orig, gen, mask, fs = _noise(*NOISE_SEEDS)
    rho, gam, sums = ref.stats(orig, gen, mask, fs, 0, NOISE_R)
    assert (rho[mask_edges(mask)] < 0.05).all() and np.abs(gam[mask > 0] - 1.0).max() < 0.03
    lin, g = ref.blend_linear(orig, gen, mask, fs, 0, NOISE_R)
    outside = (g == 0) | (g == 1)
    p_lin = ref.zone_power(lin, g, outside)
    out, _, _ = ref.blend(orig, gen, mask, fs, 0, NOISE_R, rho=rho)
    p_matched = ref.zone_power(out, g, outside)
    out, _, _ = ref.blend(orig, gen, mask, fs, 0, NOISE_R, rho=rho, gam=gam)
    p_gain = ref.zone_power(out, g, outside)
    # expected 0.75 and 1; the issue's bars are 0.85 and [0.9, 1.1]: these seeds hold them with room
    assert 0.72 < p_lin < 0.78, p_lin
    assert 0.96 < p_matched < 1.04 and 0.96 < p_gain < 1.04, (p_matched, p_gain)


def mask_edges(mask):
    """Boolean (B, T + 1): the junctions of a line mask."""
    reg = np.pad(mask > 0, ((0, 0), (1, 1)))
    return reg[:, 1:] != reg[:, :-1]


def test_restatement_gain_and_degenerate_cases():
    rng = np.random.default_rng(5)
    fs, T, R = 8, 12, 7
    orig = rng.uniform(-1, 1, (2, T * fs)).astype(np.float32)
    mask = np.zeros((2, T), np.float32)
    mask[0, 4:6] = 1.0
    mask[1, :] = 1.0
    rho, gam, sums = ref.stats(orig, (0.25 * orig).astype(np.float32), mask, fs, 0, R)
    assert np.allclose(rho[0, [4, 6]], 1.0) and (gam[0, 4:6] == 2.0).all() and (gam[0, :4] == 1.0).all()   # clamped
    assert (rho[1] == 1.0).all() and (gam[1] == 1.0).all() and not sums[1].any()                     # no zone at all
    rho, gam, _ = ref.stats(orig, (-orig).astype(np.float32), mask, fs, 0, R)
    assert (rho[0, [4, 6]] == 0.0).all() and np.allclose(gam[0, 4:6], 1.0)
    rho, gam, _ = ref.stats(orig, np.zeros_like(orig), mask, fs, 0, R)                                # a silent gen
    assert (rho == 1.0).all() and (gam == 1.0).all()
    rho, gam, sums = ref.stats(orig, (0.8 * orig).astype(np.float32)[:, 30:60], mask, fs, 30, R)      # gen cuts the left zone
    assert np.isclose(gam[0, 4], 1.25, rtol=1e-6)
    assert np.isclose(sums[0, 4, 0], float(orig[0, 30]) ** 2 + float(orig[0, 31]) ** 2, rtol=1e-14)
