"""The host plan of joint long-form denoising: ``pipeline.joint_weights`` (the normalised window weights that
alcm_lcm_step_joint averages overlapping windows with) and the ``--long-joint`` flag.  No GPU."""
import os

import numpy as np
import pytest

from conftest import REPO

# (L, W, overlap): two windows, three windows on frames 30 .. 39, the vector-path layout, the 30 s clip, one window
CASES = [(60, 40, 20), (70, 40, 20), (72, 40, 20), (936, 312, 156), (40, 40, 20)]


def _starts(L, W, overlap):
    from audiolcm_amd.pipeline import AudioLCMPipeline
    pipe = AudioLCMPipeline.__new__(AudioLCMPipeline)
    pipe.latent_shape = (20, 312)
    spans, w = pipe.long_windows(L, W, overlap)
    assert w == W
    return [s for s, _ in spans]


def _restated(starts, W, L, overlap):
    """The definition once more, element by element in float64: (wn as float64 before rounding, windows per frame)."""
    w = [min(1.0, (min(j, W - 1 - j) + 1) / (overlap + 1)) for j in range(W)]
    wn = np.zeros((len(starts), W), dtype=np.float64)
    cover = np.zeros(L, dtype=np.int64)
    for t in range(L):
        ks = [k for k, s in enumerate(starts) if s <= t < s + W]
        tot = sum(w[t - starts[k]] for k in ks)
        cover[t] = len(ks)
        for k in ks:
            wn[k, t - starts[k]] = w[t - starts[k]] / tot
    return wn, cover


@pytest.mark.parametrize("L,W,overlap", CASES)
def test_joint_weights(L, W, overlap):
    from audiolcm_amd.pipeline import joint_weights
    starts = _starts(L, W, overlap)
    wn = joint_weights(starts, W, L, overlap)
    assert wn.shape == (len(starts), W) and wn.dtype == np.float32
    want, cover = _restated(starts, W, L, overlap)
    assert np.array_equal(wn, want.astype(np.float32))
    assert (wn > 0).all() and cover.min() >= 1
    total = np.zeros(L, dtype=np.float64)
    for k, s in enumerate(starts):
        total[s:s + W] += wn[k].astype(np.float64)
    assert np.abs(total - 1.0).max() <= 2.0 ** -22
    for k, s in enumerate(starts):
        single = cover[s:s + W] == 1
        assert (wn[k][single] == np.float32(1.0)).all()
    assert joint_weights(tuple(starts), W, L, overlap) is wn   # built once per argument tuple
    with pytest.raises(ValueError):
        wn[0, 0] = 0.0                                          # and the cached table cannot be changed


def test_joint_weights_layouts():
    from audiolcm_amd.pipeline import joint_weights
    assert _starts(70, 40, 20) == [0, 20, 30] and _starts(72, 40, 20) == [0, 20, 32]
    assert _starts(936, 312, 156) == [0, 156, 312, 468, 624] and _starts(40, 40, 20) == [0]
    _, cover = _restated([0, 20, 30], 40, 70, 20)
    assert (cover[30:40] == 3).all() and cover.max() == 3 and (cover[:20] == 1).all() and (cover[60:] == 1).all()
    one = joint_weights([0], 40, 40, 20)
    assert one.shape == (1, 40) and (one == np.float32(1.0)).all()
    # the ramp: over `overlap` frames at each end, the two windows' weights cross over linearly
    wn = joint_weights([0, 20], 40, 60, 20)
    up = np.arange(1, 21) / 21.0
    np.testing.assert_allclose(wn[1][:20], up / (up + up[::-1]), rtol=1e-6)
    np.testing.assert_allclose(wn[0][20:], up[::-1] / (up + up[::-1]), rtol=1e-6)


@pytest.mark.parametrize("starts,W,L,overlap", [
    ([0, 20, 20], 40, 60, 20),          # not strictly ascending
    ([0, 30, 20], 40, 60, 20),          # descending
    ([4, 20], 40, 60, 20),              # does not start at 0
    ([0, 41], 40, 81, 20),              # frame 40 under no window
    ([0, 20], 40, 61, 20),              # does not end at L
    ([0, 20], 40, 59, 20),
    ([], 40, 40, 20),                   # no window
    (list(range(33)), 40, 72, 20),      # more than 32 windows
    ([0, 20], 40, 60, -1),              # negative overlap
])
def test_joint_weights_refuses(starts, W, L, overlap):
    from audiolcm_amd.pipeline import joint_weights
    with pytest.raises(ValueError):
        joint_weights(starts, W, L, overlap)


def test_joint_weights_takes_32_windows():
    from audiolcm_amd.pipeline import joint_weights
    starts = list(range(0, 32 * 4, 4))
    wn = joint_weights(starts, 8, starts[-1] + 8, 4)
    assert wn.shape == (32, 8)


def test_cli_long_joint_flag(monkeypatch):
    from audiolcm_amd import cli

    def no_model(*a, **k):
        raise AssertionError("a refused request must not reach the model")
    monkeypatch.setattr(cli, "build_models", no_model)
    base = ["--synthetic-seed", "0", "-b", os.path.join(REPO, "configs", "audiolcm.yaml")]
    assert cli.parse_args([]).long_joint is False
    opt = cli.parse_args(["--duration", "3", "--long-joint"])
    assert opt.long_joint is True and opt.duration == 3.0
    with pytest.raises(ValueError, match="--long-joint"):
        cli.build(cli.parse_args(base + ["--long-joint"]))
    with pytest.raises(AssertionError, match="must not reach"):   # with --duration it passes the checks
        cli.build(cli.parse_args(base + ["--duration", "3", "--long-joint"]))
