"""Host side of loops made from a recording: ``windows.ring_edit_regions`` / ``ring_paste_regions`` (the circular runs of
regenerated frames, widened and merged round the ring), ``windows.seam_mask``, the request plan ``audio_in.plan_loop``
and the refusals of ``--loop-from`` and ``AudioLCMEditInfer(loop_from=True)``, all before any model is built."""
import os

import numpy as np
import pytest

from conftest import REPO


def _union(L, *frames):
    u = np.zeros(L, dtype=bool)
    u[[f % L for f in frames]] = True
    return u


def test_a_run_across_the_wrap_is_one_region():
    from audiolcm_amd.windows import long_windows, loop_windows, ring_edit_regions, seam_mask
    plan = ring_edit_regions(seam_mask(60, 4), 40, 20)
    spans, W = long_windows(48, 40, 20)
    assert plan == [("line", 36, 48, [s for s, _ in spans], W)]
    assert plan == [("line", 36, 48, [0, 8], 40)]
    # the same seam on a ring of 44 frames: 48 frames of region cover the ring, which is then denoised as a ring
    assert ring_edit_regions(seam_mask(44, 4), 40, 20) == [("ring", *loop_windows(44, 40, 20))]
    assert ring_edit_regions(seam_mask(48, 4), 40, 20) == [("ring", *loop_windows(48, 40, 20))]   # total == L
    assert ring_edit_regions(seam_mask(49, 4), 40, 20)[0][:3] == ("line", 25, 48)                 # one frame is left
    assert ring_edit_regions(np.ones(30, dtype=bool), 40) == [("ring", *loop_windows(30, 40))]
    assert ring_edit_regions(np.zeros(60, dtype=bool), 40, 20) == []
    # the default overlap is min(window, L) // 2
    assert ring_edit_regions(seam_mask(60, 4), 40) == plan
    assert ring_edit_regions(seam_mask(30, 2), 40) == [("ring", *loop_windows(30, 40, 15))]
    with pytest.raises(ValueError, match="overlap"):
        ring_edit_regions(seam_mask(60, 4), 40, 40)


def test_separate_spans_and_merging():
    from audiolcm_amd.windows import ring_edit_regions
    L = 200
    two = ring_edit_regions(_union(L, 50, 51, 120), 40, 10)
    assert [(k, a, R) for k, a, R, _, _ in two] == [("line", 40, 22), ("line", 110, 21)]
    assert two[0][3:] == ([0], 22) and two[1][3:] == ([0], 21)      # one window each: a region below the window
    # regions that touch after widening are merged: 50 + 10 == 80 - 10 - 10 ... 60 == 60
    touch = ring_edit_regions(_union(L, 49, 70), 40, 10)
    assert [(a, R) for _, a, R, _, _ in touch] == [(39, 42)]
    apart = ring_edit_regions(_union(L, 48, 70), 40, 10)
    assert [(a, R) for _, a, R, _, _ in apart] == [(38, 21), (60, 21)]
    # also across the wrap: frames 195 and 5 widen to [185, 206) and [-5, 16), which overlap round the ring
    wrap = ring_edit_regions(_union(L, 195, 5), 40, 10)
    assert [(a, R) for _, a, R, _, _ in wrap] == [(185, 31)]
    wrap = ring_edit_regions(_union(L, 189, 10), 40, 10)             # 189 + 1 + 10 == 200 == 10 - 10 + 200: they touch
    assert [(a, R) for _, a, R, _, _ in wrap] == [(179, 42)]
    wrap = ring_edit_regions(_union(L, 188, 10), 40, 10)             # one kept frame between them
    assert [(a, R) for _, a, R, _, _ in wrap] == [(0, 21), (178, 21)]
    # a region longer than one window is covered by long_windows' plan
    from audiolcm_amd.windows import long_windows
    long = ring_edit_regions(_union(L, *range(180, 260)), 40, 10)
    spans, W = long_windows(100, 40, 10)
    assert long == [("line", 170, 100, [s for s, _ in spans], W)] and len(spans) > 2
    with pytest.raises(ValueError, match="at most 32"):
        ring_edit_regions(_union(2000, *range(100, 900)), 40, 20)


@pytest.mark.parametrize("k", [1, 7, 59, 60, 131])
def test_rolling_the_union_rolls_the_regions(k):
    from audiolcm_amd.windows import ring_edit_regions, ring_paste_regions, seam_mask
    for L, union in ((60, seam_mask(60, 4)), (200, _union(200, 50, 51, 52)), (97, _union(97, 0)),
                     (200, _union(200, *range(180, 260)))):
        (kind, a, R, starts, W), = ring_edit_regions(union, 40, 20)
        assert ring_edit_regions(np.roll(union, k), 40, 20) == [(kind, (a + k) % L, R, starts, W)]
        (a, n), = ring_paste_regions(union, 16)
        assert ring_paste_regions(np.roll(union, k), 16) == [((a + k) % L, n)]
    two = _union(200, 50, 120)
    assert ([(r[1] - k) % 200 for r in ring_edit_regions(np.roll(two, k), 40, 10)].count(40) == 1)


def test_ring_paste_regions():
    from audiolcm_amd.windows import ring_paste_regions, seam_mask
    assert ring_paste_regions(seam_mask(120, 4), 32) == [(84, 72)]                    # one region across the wrap
    assert ring_paste_regions(seam_mask(72, 4), 32) == [("ring",)]                    # 72 frames cover the ring
    assert ring_paste_regions(seam_mask(73, 4), 32) == [(37, 72)]
    assert ring_paste_regions(seam_mask(60, 4), 32) == [("ring",)]
    assert ring_paste_regions(np.zeros(60, dtype=bool), 32) == []
    assert ring_paste_regions(np.ones(60, dtype=bool), 0) == [("ring",)]
    assert ring_paste_regions(_union(300, 50, 51, 200), 32) == [(18, 66), (168, 65)]  # ascending a
    assert ring_paste_regions(_union(300, 50, 115), 32) == [(18, 130)]                # 83 == 83: they touch
    assert ring_paste_regions(_union(300, 50, 116), 32) == [(18, 65), (84, 65)]
    assert ring_paste_regions(_union(300, 290, 40), 32) == [(258, 115)]               # merged across the wrap
    assert ring_paste_regions(_union(300, 290, 40), 0) == [(40, 1), (290, 1)]         # no halo: the runs themselves
    assert ring_paste_regions(_union(10, 9, 0), 0) == [(9, 2)]


def test_ring_paste_cut():
    """The cut of a whole-ring paste lies in the middle of the longest run of kept frames, with the fade's reach of
    kept frames either side; without such a run it is the wrap."""
    from audiolcm_amd.windows import ring_paste_cut, seam_mask
    assert ring_paste_cut(seam_mask(44, 4), 1) == 22                  # kept 4 .. 39: 4 + 36 // 2
    assert ring_paste_cut(seam_mask(100, 32), 1) == 50                # the defaults of loop_from on a 3.2 s recording
    assert ring_paste_cut(seam_mask(64, 32), 1) == 0                  # nothing is kept: the wrap
    assert ring_paste_cut(np.ones(60, dtype=bool), 1) == 0 and ring_paste_cut(np.zeros(60, dtype=bool), 1) == 0
    m = seam_mask(32, 8)
    m[14:19] = True                                                   # kept runs 8 .. 13 and 19 .. 23: the longer one
    assert ring_paste_cut(m, 1) == 11 and not m[10] and not m[11]
    assert ring_paste_cut(m, 3) == 11 and ring_paste_cut(m, 4) == 0   # 3 kept frames either side of the cut, not 4
    assert ring_paste_cut(_union(10, 3), 0) == 8                      # a run across the wrap: kept 4 .. 12, 4 + 9 // 2
    assert ring_paste_cut(_union(10, *range(9)), 0) == 0              # one kept frame has no two sides
    for union, f in ((seam_mask(44, 4), 1), (m, 3), (_union(97, 5, 50), 16)):
        a, L = ring_paste_cut(union, f), len(union)
        assert not any(union[(a + j) % L] for j in range(-max(f, 1), max(f, 1)))
        for k in (1, 7, L - 1):
            assert ring_paste_cut(np.roll(union, k), f) == (a + k) % L


def test_seam_mask_bounds():
    from audiolcm_amd.windows import seam_mask
    m = seam_mask(10, 3)
    assert m.dtype == bool and m.tolist() == [True] * 3 + [False] * 4 + [True] * 3
    assert seam_mask(2, 1).all() and seam_mask(10, 5).all() and seam_mask(11, 5).sum() == 10
    for L, s in ((10, 0), (10, 6), (1, 1), (11, 6), (10, -1)):
        with pytest.raises(ValueError, match="seam"):
            seam_mask(L, s)


def test_ring_spans_mask():
    from audiolcm_amd.audio_in import ring_spans_mask
    L = 100                                         # 3.2 s: a frame is 32 ms
    assert ring_spans_mask([(0.32, 0.64)], L).nonzero()[0].tolist() == list(range(10, 20))
    assert ring_spans_mask([(3.04, 0.16)], L).nonzero()[0].tolist() == [0, 1, 2, 3, 4, 95, 96, 97, 98, 99]
    assert ring_spans_mask([(0.33, 0.63)], L).nonzero()[0].tolist() == list(range(11, 19))    # whole frames inside


def _write(path, n, rate=16000, seed=0):
    from audiolcm_amd.wavio import write_pcm16
    x = np.random.default_rng(seed).uniform(-0.5, 0.5, n).astype(np.float32)
    write_pcm16(str(path), x, rate, scale=32768.0)
    return str(path)


def test_plan_loop(tmp_path):
    from audiolcm_amd.audio_in import plan_edit, plan_loop
    from audiolcm_amd.wavio import read_wav
    rec = _write(tmp_path / "rec.wav", 100 * 512 + 37)
    plan = plan_loop(rec)
    assert (plan.mode, plan.samples.size, plan.dropped, plan.seam_frames) == ("loop_from", 100 * 512, 37, 32)
    assert np.array_equal(plan.samples, read_wav(rec)[0][:100 * 512])
    assert (plan.rate, plan.out_rate, plan.frame_samples, plan.fade, plan.pcm_scale) == (16000, 16000, 512, 512, 32768.0)
    assert plan.mask is None and plan.level is None
    assert plan_loop(rec, seam_s=0.5).seam_frames == 16 and plan_loop(rec, seam_s=0.51).seam_frames == 16
    assert plan_loop(rec, seam_s=0.513).seam_frames == 17                      # rounded up to whole frames
    assert plan_loop(rec, seam_s=1.6).seam_frames == 50                        # 2 m == L
    spans = plan_loop(rec, mask_spans=[(1.6, 1.92), (3.04, 0.16)], fade_ms=8.0)
    assert spans.mask.nonzero()[0].tolist() == [0, 1, 2, 3, 4] + list(range(50, 60)) + [95, 96, 97, 98, 99]
    assert spans.fade == 128
    same = plan_edit(rec, loop_from=True)
    assert (same.mode, same.seam_frames, same.dropped) == ("loop_from", 32, 37)
    vary = plan_loop(rec, vary=True, out_sample_rate=44100, loudness=-16.0, loop_fade_ms=8.0)
    assert (vary.mode, vary.samples.size, vary.dropped, vary.out_rate) == ("loop_vary", 100 * 512, 37, 44100)
    assert vary.level.loudness == -16.0 and vary.loop_fade == 353 and vary.resample_out and vary.pcm_scale == 32767.0
    rec3 = _write(tmp_path / "rec3.wav", 103 * 512)
    assert plan_loop(rec3, vary=True, out_sample_rate=44100).dropped == 3 * 512  # a multiple of 5 frames at 44.1 kHz
    assert plan_loop(rec3, vary=True, out_sample_rate=48000).dropped == 0
    assert plan_loop(rec3, vary=True).samples.size == 103 * 512
    # refusals
    for kw in (dict(loudness=-16.0), dict(peak_dbfs=-1.0), dict(out_sample_rate=48000)):
        with pytest.raises(ValueError, match="--loop-vary"):
            plan_loop(rec, **kw)
    with pytest.raises(ValueError, match="--loop-seam"):
        plan_loop(rec, seam_s=1.61)                                            # 2 * 51 > 100
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="--loop-seam"):
            plan_loop(rec, seam_s=bad)
    with pytest.raises(ValueError, match="--loop-from"):
        plan_loop(_write(tmp_path / "short.wav", 1023), seam_s=0.01)
    assert plan_loop(_write(tmp_path / "two.wav", 1024), seam_s=0.01).seam_frames == 1
    with pytest.raises(ValueError, match="--loop-from"):
        plan_loop(_write(tmp_path / "four.wav", 4 * 512), vary=True, out_sample_rate=44100)   # no 5 frames
    with pytest.raises(ValueError, match="--mask-spans"):
        plan_loop(rec, vary=True, mask_spans=[(1.0, 2.0)])
    with pytest.raises(ValueError, match="--loop-fade-ms"):
        plan_loop(rec, vary=True, loop_fade_ms=-1.0)
    with pytest.raises(ValueError, match="sample rate"):
        plan_loop(_write(tmp_path / "r48.wav", 48000, rate=48000))             # another rate needs resample
    for kw in (dict(keep_original=True, mask_spans=[(1.0, 2.0)]), dict(extend_s=1.0)):
        with pytest.raises(ValueError, match="--loop-from"):
            plan_edit(rec, loop_from=True, **kw)
    with pytest.raises(ValueError, match="--loop-from"):
        plan_edit(rec, loop_vary=True)


def test_cli_loop_from_refusals(monkeypatch, tmp_path, capsys):
    from audiolcm_amd import cli

    def no_model(*a, **k):
        raise AssertionError("a refused request must not reach the model")
    monkeypatch.setattr(cli, "build_models", no_model)
    rec = _write(tmp_path / "rec.wav", 100 * 512 + 37)
    short = _write(tmp_path / "short.wav", 1000)
    base = ["--synthetic-seed", "0", "-b", os.path.join(REPO, "configs", "audiolcm.yaml")]
    opt = cli.parse_args([])
    assert (opt.loop_from, opt.loop_seam, opt.loop_vary, opt.strength) == (None, 1.0, False, 0.5)
    assert cli.parse_args(["--loop-from", rec]).strength == 1.0                # pure noise in the seam by default
    assert cli.parse_args(["--loop-from", rec, "--loop-vary"]).strength == 0.5
    assert cli.parse_args(["--loop-from", rec, "--strength", "0.3", "--loop-seam", "0.5"]).strength == 0.3
    for flag, extra in (("--loop", ["--loop"]), ("--init-audio", ["--init-audio", rec]), ("--inpaint", ["--inpaint"]),
                        ("--keep-original", ["--keep-original"]), ("--duration", ["--duration", "3"]),
                        ("--extend", ["--extend", "2"]), ("--loudness", ["--loudness", "-16"]),
                        ("--peak", ["--peak", "-2"]), ("--true-peak", ["--true-peak"]),
                        ("--out-sample-rate", ["--out-sample-rate", "48000"])):
        with pytest.raises(ValueError, match="--loop-from") as e:
            cli.build(cli.parse_args(base + ["--loop-from", rec] + extra))
        assert flag in str(e.value)
    for flag, extra in (("--loop", ["--loop"]), ("--init-audio", ["--init-audio", rec]), ("--inpaint", ["--inpaint"]),
                        ("--keep-original", ["--keep-original"]), ("--duration", ["--duration", "3"]),
                        ("--extend", ["--extend", "2"])):
        with pytest.raises(ValueError, match="--loop-from") as e:              # with --loop-vary just the same
            cli.build(cli.parse_args(base + ["--loop-from", rec, "--loop-vary"] + extra))
        assert flag in str(e.value)
    with pytest.raises(ValueError, match="--loop-from"):
        cli.build(cli.parse_args(base + ["--loop-vary"]))
    with pytest.raises(ValueError, match="--loop-from"):                       # shorter than two frames
        cli.build(cli.parse_args(base + ["--loop-from", short]))
    with pytest.raises(ValueError, match="--loop-seam"):                       # 2 * seam > L
        cli.build(cli.parse_args(base + ["--loop-from", rec, "--loop-seam", "1.7"]))
    with pytest.raises(ValueError, match="--mask-spans"):
        cli.build(cli.parse_args(base + ["--loop-from", rec, "--loop-vary", "--mask-spans", "1-2"]))
    with pytest.raises(ValueError, match="--long-joint is used with --duration or with --init-audio"):
        cli.build(cli.parse_args(base + ["--loop-from", rec, "--long-joint"]))  # its own refusal, as before
    # --loop's own refusals keep their words
    with pytest.raises(ValueError, match="--loop generates from text: it does not combine with --init-audio"):
        cli.build(cli.parse_args(base + ["--loop", "--init-audio", rec]))
    capsys.readouterr()
    for ok in (["--loop-from", rec], ["--loop-from", rec, "--loop-seam", "0.25", "--fade-ms", "8"],
               ["--loop-from", rec, "--mask-spans", "1-1.5,3.1-0.1"], ["--loop-from", rec, "--strength", "0.8"],
               ["--loop-from", rec, "--resample"], ["--loop-from", rec, "--loop-vary"],
               ["--loop-from", rec, "--loop-vary", "--out-sample-rate", "44100", "--loudness", "-16", "--peak", "-2",
                "--true-peak", "--loop-fade-ms", "8"]):
        with pytest.raises(AssertionError, match="must not reach"):           # these pass the checks
            cli.build(cli.parse_args(base + ok))
    assert "37 samples" in capsys.readouterr().out                             # the trimmed samples are reported


def test_edit_infer_loop_from_refusals(monkeypatch, tmp_path):
    from audiolcm_amd import infer_api

    def no_model(*a, **k):
        raise AssertionError("a refused request must not reach the model")
    monkeypatch.setattr(infer_api, "_build", no_model)
    rec = _write(tmp_path / "rec.wav", 100 * 512)
    short = _write(tmp_path / "short.wav", 1000)
    for kw in (dict(keep_original=True, mask_spans=[(1.0, 2.0)]), dict(extend_s=1.0), dict(loudness=-16.0),
               dict(peak_dbfs=-1.0), dict(out_sample_rate=48000), dict(loop_seam_s=1.7), dict(loop_seam_s=0.0)):
        with pytest.raises(ValueError, match="loop_from|loop_seam_s"):
            infer_api.AudioLCMEditInfer("a dog", rec, synthetic_seed=0, loop_from=True, **kw)
    with pytest.raises(ValueError, match="loop_from"):
        infer_api.AudioLCMEditInfer("a dog", short, synthetic_seed=0, loop_from=True)
    with pytest.raises(ValueError, match="loop_from"):
        infer_api.AudioLCMEditInfer("a dog", rec, synthetic_seed=0, loop_vary=True)
    for kw in (dict(), dict(loop_seam_s=0.5, fade_ms=8.0), dict(mask_spans=[(1.0, 1.5)]), dict(loop_vary=True),
               dict(loop_vary=True, out_sample_rate=44100, loudness=-16.0, loop_fade_ms=8.0)):
        with pytest.raises(AssertionError, match="must not reach"):
            infer_api.AudioLCMEditInfer("a dog", rec, synthetic_seed=0, loop_from=True, **kw)
