"""The host plan of seamless loops: ``AudioLCMPipeline.loop_windows`` (the windows of a ring), ``pipeline.ring_weights``
(the normalised window weights alcm_lcm_step_ring averages with), ``audio_in.loop_frames`` (the period) and the
``--loop`` flag's refusals.  No GPU."""
import os

import numpy as np
import pytest

from conftest import REPO

# (L, window, overlap) -> starts: the vector layout whose last window wraps, the element layout, a ring of one window's
# length (two windows, two cut points), the 30 s clip, a ring of 1.5 windows, and one whose starts are rounded to 4
PLANS = [((24, 16, 8), [0, 8, 16]), ((23, 15, 7), [0, 7, 15]), ((312, 312, None), [0, 156]),
         ((936, 312, None), [0, 156, 312, 468, 624, 780]), ((60, 40, 20), [0, 20, 40]), ((72, 40, 20), [0, 16, 36, 52])]


def _planner():
    from audiolcm_amd.pipeline import AudioLCMPipeline
    pipe = AudioLCMPipeline.__new__(AudioLCMPipeline)
    pipe.latent_shape = (20, 312)
    return pipe


def _gaps(starts, L):
    return [b - a for a, b in zip(starts, list(starts[1:]) + [L])]


@pytest.mark.parametrize("args,want", PLANS)
def test_loop_windows(args, want):
    starts, W, overlap = _planner().loop_windows(*args)
    assert starts == want
    assert W == min(args[1], args[0]) and overlap == (W // 2 if args[2] is None else args[2])
    assert max(_gaps(starts, args[0])) <= W - overlap     # cyclic neighbours share at least `overlap` frames


def test_loop_windows_properties():
    plan = _planner().loop_windows
    for L in (4, 5, 6, 7, 8):                               # rounding to 4 would collide here: the starts stay distinct
        starts, W, overlap = plan(L)
        assert len(starts) >= 2 and len(set(starts)) == len(starts) and starts[0] == 0 and starts == sorted(starts)
        assert max(_gaps(starts, L)) <= W - overlap and starts[-1] < L
    assert plan(4)[0] == [0, 2]
    for window, overlap in ((312, None), (40, 20), (16, 8), (15, 7)):
        for L in list(range(2, 401)) + [624, 845, 936, 1872]:
            W = min(window, L)
            ov = W // 2 if overlap is None else overlap
            if not 0 < ov < W or max(2, -(-L // (W - ov))) > 32:
                with pytest.raises(ValueError):
                    plan(L, window, overlap)
                continue
            starts, w, o = plan(L, window, overlap)
            assert (w, o) == (W, ov)
            gaps = _gaps(starts, L)
            assert len(starts) >= 2 and starts[0] == 0 and min(gaps) > 0 and max(gaps) <= W - ov and starts[-1] < L
            K = max(2, -(-L // (W - ov)))
            raw = [k * L // K for k in range(K)]
            rounded = [s - s % 4 for s in raw]
            rg = _gaps(rounded, L)
            if L % 4 == 0 and W % 4 == 0 and min(rg) > 0 and max(rg) <= W - ov:
                assert starts == rounded                    # the 16-byte path, where rounding keeps the plan's rules
            else:
                assert starts == raw, (L, window, overlap, starts)
    with pytest.raises(ValueError):
        plan(24, 16, 16)                                    # overlap must be below the window
    with pytest.raises(ValueError):
        plan(24, 16, 0)
    with pytest.raises(ValueError, match="32"):
        plan(1872, 40, 20)                                  # 94 windows


def _restated(starts, W, L, overlap):
    """The definition element by element in float64: (wn before rounding, windows per frame)."""
    w = [min(1.0, (min(j, W - 1 - j) + 1) / (overlap + 1)) for j in range(W)]
    wn = np.zeros((len(starts), W), dtype=np.float64)
    cover = np.zeros(L, dtype=np.int64)
    for t in range(L):
        ks = [(k, (t - s) % L) for k, s in enumerate(starts) if (t - s) % L < W]
        tot = sum(w[o] for _, o in ks)
        cover[t] = len(ks)
        for k, o in ks:
            wn[k, o] = w[o] / tot
    return wn, cover


@pytest.mark.parametrize("args", [a for a, _ in PLANS] + [(70, 40, 20), (40, 40, 20), (16, 16, 8), (4, None, None)])
def test_ring_weights(args):
    from audiolcm_amd.pipeline import ring_weights
    L = args[0]
    starts, W, overlap = _planner().loop_windows(*args)
    wn = ring_weights(starts, W, L, overlap)
    assert wn.shape == (len(starts), W) and wn.dtype == np.float32
    want, cover = _restated(starts, W, L, overlap)
    assert np.array_equal(wn, want.astype(np.float32))
    assert (wn > 0).all() and cover.min() >= 1
    if L == W:
        assert (cover == len(starts)).all()                 # every window covers the whole ring
    total = np.zeros(L, dtype=np.float64)
    for k, s in enumerate(starts):
        np.add.at(total, (s + np.arange(W)) % L, wn[k].astype(np.float64))
    assert np.abs(total - 1.0).max() <= 2e-7
    for k, s in enumerate(starts):
        single = cover[(s + np.arange(W)) % L] == 1
        assert (wn[k][single] == np.float32(1.0)).all()
    assert ring_weights(tuple(starts), W, L, overlap) is wn   # built once per argument tuple
    with pytest.raises(ValueError):
        wn[0, 0] = 0.0                                        # and the cached table cannot be changed


def test_ring_weights_rotate_with_the_plan():
    """On an evenly spaced plan every window has the same table: no frame of the ring is special."""
    from audiolcm_amd.pipeline import ring_weights
    wn = ring_weights([0, 20, 40], 40, 60, 20)
    assert np.array_equal(wn[0], wn[1]) and np.array_equal(wn[1], wn[2])
    up = np.arange(1, 21) / 21.0
    np.testing.assert_allclose(wn[0][:20], up / (up + up[::-1]), rtol=1e-6)


@pytest.mark.parametrize("starts,W,L,overlap", [
    ([0], 40, 40, 20),                  # one window cannot close a ring
    ([], 40, 40, 20),
    (list(range(33)), 40, 72, 20),      # more than 32 windows
    ([0, 20], 0, 60, 0),                # no window length
    ([0, 20], 61, 60, 20),              # a window longer than the ring
    ([0, 20], 40, 60, -1),              # negative overlap
    ([4, 20], 40, 60, 20),              # does not start at 0
    ([0, 20, 20], 40, 60, 20),          # not strictly ascending
    ([0, 30, 20], 40, 60, 20),          # descending
    ([0, 20, 60], 40, 60, 20),          # a start on L
    ([0, 41], 40, 81, 20),              # frame 40 under no window
    ([0, 20], 40, 61, 20),              # frame 60 under no window: the gap across the wrap
])
def test_ring_weights_refuses(starts, W, L, overlap):
    from audiolcm_amd.pipeline import ring_weights
    with pytest.raises(ValueError):
        ring_weights(starts, W, L, overlap)


def test_ring_weights_takes_32_windows():
    from audiolcm_amd.pipeline import ring_weights
    starts = list(range(0, 32 * 4, 4))
    assert ring_weights(starts, 8, 128, 4).shape == (32, 8)


def test_loop_frames():
    from audiolcm_amd.audio_in import loop_frames, loop_multiple
    assert [loop_multiple(r) for r in (16000, 32000, 48000, 96000, 44100, 22050, 8000)] == [1, 1, 1, 1, 5, 5, 1]
    assert loop_frames(1.0, 16000) == 32 and loop_frames(1.0, 48000) == 32 and loop_frames(1.0) == 32
    assert loop_frames(1.0, 44100) == 35                       # 32 rounded up to a multiple of 5
    assert loop_frames(3.0) == 94 and loop_frames(3.0, 44100) == 95
    assert loop_frames(10.0) == 313 and loop_frames(29.952) == 936
    assert loop_frames(0.01) == 2                              # a ring has two windows
    for rate in (16000, 48000, 44100, 22050, 32000):
        L = loop_frames(2.5, rate)
        assert L >= 2.5 * 16000 / 512 and (L * 512 * rate) % 16000 == 0   # a whole number of output samples
    with pytest.raises(ValueError):
        loop_frames(0.0)


def test_cli_loop_refusals(monkeypatch):
    from audiolcm_amd import cli

    def no_model(*a, **k):
        raise AssertionError("a refused request must not reach the model")
    monkeypatch.setattr(cli, "build_models", no_model)
    base = ["--synthetic-seed", "0", "-b", os.path.join(REPO, "configs", "audiolcm.yaml")]
    opt = cli.parse_args([])
    assert opt.loop is False and opt.loop_fade_ms == 32.0
    opt = cli.parse_args(["--loop", "--loop-fade-ms", "8", "--duration", "3"])
    assert opt.loop is True and opt.loop_fade_ms == 8.0 and cli.loop_period(opt) == 94
    assert cli.loop_period(cli.parse_args(["--loop", "--W", "40"])) == 40
    for extra in (["--init-audio", "missing.wav"], ["--inpaint"], ["--keep-original"],
                  ["--inpaint", "--init-audio", "missing.wav", "--mask-spans", "1-2", "--keep-original"]):
        with pytest.raises(ValueError, match="--loop"):
            cli.build(cli.parse_args(base + ["--loop", "--duration", "3"] + extra))
    with pytest.raises(ValueError, match="--loop"):            # 312 frames are no whole number of samples at 44.1 kHz
        cli.build(cli.parse_args(base + ["--loop", "--out-sample-rate", "44100"]))
    with pytest.raises(ValueError, match="--loop-fade-ms"):
        cli.build(cli.parse_args(base + ["--loop", "--loop-fade-ms", "-1"]))
    for ok in (["--loop"], ["--loop", "--duration", "3"], ["--loop", "--duration", "3", "--long-joint"],
               ["--loop", "--long-joint"], ["--loop", "--duration", "1", "--out-sample-rate", "44100"],
               ["--loop", "--duration", "3", "--loudness", "-16", "--peak", "-2", "--true-peak"]):
        with pytest.raises(AssertionError, match="must not reach"):   # these pass the checks
            cli.build(cli.parse_args(base + ok))
