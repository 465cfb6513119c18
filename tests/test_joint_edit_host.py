"""The host side of joint editing and extension: ``pipeline.joint_edit_regions`` (the regions and window plans of
``edit_long(joint=True)``), ``audio_in.extend_counts`` (junction and output length), and what ``plan_edit`` and the
command line accept and refuse for ``--extend`` and ``--long-joint --init-audio``.  No GPU."""
import math
import os

import numpy as np
import pytest

from conftest import REPO


def _restated(union, window, overlap):
    """The definition once more, frame by frame: mark every frame within `overlap` of a regenerated one, cut the marks
    into maximal runs (runs that touch are one), and cover each with windows at the stride window - overlap, the last
    one shifted back to end at the region's end."""
    L = len(union)
    near = [any(union[max(t - overlap, 0):t + overlap + 1]) for t in range(L)]
    plan, t = [], 0
    while t < L:
        if not near[t]:
            t += 1
            continue
        b = t
        while b < L and near[b]:
            b += 1
        R, W = b - t, min(window, b - t)
        starts = [0]
        while starts[-1] + W < R:
            starts.append(min(starts[-1] + W - overlap, R - W))
        plan.append((t, b, starts, W))
        t = b
    return plan


def _union(L, *runs):
    u = [False] * L
    for lo, hi in runs:
        u[lo:hi] = [True] * (hi - lo)
    return u


@pytest.mark.parametrize("L,runs,want", [
    (100, [(0, 10)], [(0, 30, [0], 30)]),                            # a run at the clip's start: one short window
    (100, [(90, 100)], [(70, 100, [0], 30)]),                        # and at its end
    (100, [(30, 80)], [(10, 100, [0, 20, 40, 50], 40)]),             # a long run: the last window shifted back
    (200, [(30, 40), (70, 80)], [(10, 100, [0, 20, 40, 50], 40)]),   # two runs whose contexts touch merge
    (200, [(30, 40), (81, 90)], [(10, 60, [0, 10], 40), (61, 110, [0, 9], 40)]),   # one frame apart: two regions
    (100, [], []),                                                   # nothing to do
    (30, [(0, 30)], [(0, 30, [0], 30)]),                             # a clip shorter than a window
])
def test_joint_edit_regions(L, runs, want):
    from audiolcm_amd.pipeline import joint_edit_regions, joint_weights, paste_regions
    union = _union(L, *runs)
    got = joint_edit_regions(union, 40, 20)
    assert got == want == _restated(union, 40, 20)
    assert [(a, b) for a, b, _, _ in got] == paste_regions(union, 20)
    for a, b, starts, W in got:
        joint_weights(starts, W, b - a, 20)     # every plan is one the step kernel takes


def test_joint_edit_regions_refuses_more_than_32_windows():
    from audiolcm_amd.pipeline import JOINT_MAX_WINDOWS, joint_edit_regions
    assert JOINT_MAX_WINDOWS == 32
    ok = joint_edit_regions(_union(700, (20, 640)), 40, 20)           # [0, 660): 40 + 31 * 20 frames, 32 windows
    assert len(ok) == 1 and len(ok[0][2]) == 32
    with pytest.raises(ValueError, match="32"):
        joint_edit_regions(_union(700, (20, 641)), 40, 20)            # one frame more: 33
    with pytest.raises(ValueError, match="overlap"):
        joint_edit_regions(_union(100, (20, 30)), 40, 40)
    assert joint_edit_regions(_union(100, (40, 50)), 40) == joint_edit_regions(_union(100, (40, 50)), 40, 20)


@pytest.mark.parametrize("n,extend_s", [(24000, 2.0), (512, 0.001), (24064, 1.0), (1023, 0.5), (480000, 20.0),
                                        (24000, 0.03)])
def test_extend_counts(n, extend_s):
    """The junction is the last whole frame of the recording; the file holds the recording and the extension; the
    frames cover the file."""
    from audiolcm_amd.audio_in import extend_counts
    J, frames, n_out = extend_counts(n, extend_s)
    extra = int(round(extend_s * 16000))
    assert J == n // 512 and J * 512 <= n < (J + 1) * 512
    assert n_out == n + extra
    assert J + frames == math.ceil(n_out / 512) and frames >= 1
    assert (J + frames) * 512 >= n_out > (J + frames - 1) * 512


def test_extend_counts_values_and_refusals():
    from audiolcm_amd.audio_in import extend_counts
    assert extend_counts(24000, 2.0) == (46, 64, 56000)      # 46.875 frames: the partial frame is generated again
    assert extend_counts(24064, 1.0) == (47, 32, 40064)      # whole frames: the junction is the recording's end
    assert extend_counts(512, 1 / 16000) == (1, 1, 513)
    with pytest.raises(ValueError, match="one"):
        extend_counts(511, 2.0)
    for bad in (0.0, -1.0, 1e-6, float("nan")):
        with pytest.raises(ValueError, match="extend_s"):
            extend_counts(24000, bad)


def _wav(path, n, rate=16000):
    from audiolcm_amd.wavio import write_pcm16
    pcm = np.random.default_rng(5).integers(-32768, 32768, n).astype("<i2")
    write_pcm16(path, pcm.astype(np.float32) / np.float32(32768.0), rate, scale=32768.0)
    return pcm


def test_plan_edit_extend(tmp_path):
    from audiolcm_amd.audio_in import plan_edit
    src = str(tmp_path / "in.wav")
    pcm = _wav(src, 24000)
    plan = plan_edit(src, extend_s=2.0)
    assert (plan.mode, plan.extend_frames, plan.n_out, plan.n_samples) == ("extend", 64, 56000, 24000)
    assert (plan.rate, plan.out_rate, plan.frame_samples, plan.fade) == (16000, 16000, 512, 512)
    assert plan.pcm_scale == 32768.0 and plan.level is None and not plan.native and not plan.resample_out
    # the recording's whole frames, as they were read: no zero padding that could be kept as audio
    assert plan.samples.shape == (46 * 512,)
    assert np.array_equal(plan.samples, pcm[:46 * 512].astype(np.float32) / np.float32(32768.0))
    assert plan_edit(src, extend_s=2.0, fade_ms=8.0).fade == 128
    for kw, word in ((dict(mask_spans=[(0.2, 0.4)]), "mask_spans"),
                     (dict(mask_spans=[(0.2, 0.4)], keep_original=True), "keep_original"),
                     (dict(loudness=-16.0), "loudness"), (dict(peak_dbfs=-1.0), "peak_dbfs"),
                     (dict(out_sample_rate=48000), "out_sample_rate"), (dict(extend_s=0.0), "extend_s")):
        with pytest.raises(ValueError, match=word):
            plan_edit(src, **{"extend_s": 2.0, **kw})
    with pytest.raises(ValueError, match="true_peak"):
        plan_edit(src, extend_s=2.0, true_peak=True)
    short = str(tmp_path / "short.wav")
    _wav(short, 500)
    with pytest.raises(ValueError, match="one latent frame"):
        plan_edit(short, extend_s=2.0)
    other = str(tmp_path / "8k.wav")
    _wav(other, 24000, 8000)
    with pytest.raises(ValueError, match="sample rate"):
        plan_edit(other, extend_s=2.0)                       # another rate needs resample=True


def test_plan_edit_joint(tmp_path):
    from audiolcm_amd.audio_in import plan_edit
    src = str(tmp_path / "in.wav")
    _wav(src, 30 * 16000)
    for kw, mode in ((dict(), "variation"), (dict(mask_spans=[(2.0, 14.0)]), "inpaint"),
                     (dict(mask_spans=[(2.0, 14.0)], keep_original=True), "keep_original")):
        plain, joint = plan_edit(src, **kw), plan_edit(src, joint=True, **kw)
        assert plain.mode == joint.mode == mode and plain.joint is False and joint.joint is True
        assert (joint.extend_frames, joint.n_out) == (0, 0)
        assert joint.samples.shape == (938 * 512,) and np.array_equal(plain.samples, joint.samples)   # 937.5 frames
        assert (plain.pcm_scale, plain.fade, plain.out_rate) == (joint.pcm_scale, joint.fade, joint.out_rate)


def test_cli_extend_and_long_joint_flags(monkeypatch, tmp_path):
    from audiolcm_amd import cli

    def no_model(*a, **k):
        raise AssertionError("a refused request must not reach the model")
    monkeypatch.setattr(cli, "build_models", no_model)
    src, short = str(tmp_path / "in.wav"), str(tmp_path / "short.wav")
    _wav(src, 24000)
    _wav(short, 500)
    base = ["--synthetic-seed", "0", "-b", os.path.join(REPO, "configs", "audiolcm.yaml")]
    assert cli.parse_args([]).extend is None and cli.parse_args(["--extend", "2.5"]).extend == 2.5

    def refused(flags, word):
        with pytest.raises(ValueError, match=word):
            cli.build(cli.parse_args(base + flags))

    refused(["--extend", "2"], "--init-audio")
    ext = ["--init-audio", src, "--extend", "2"]
    refused(ext + ["--inpaint", "--mask-spans", "0.2-0.4"], "--inpaint")
    refused(ext + ["--mask-spans", "0.2-0.4"], "--mask-spans")
    refused(ext + ["--keep-original"], "--keep-original")
    refused(ext + ["--loop"], "--extend does not combine with --loop")
    refused(ext + ["--duration", "3"], "--extend does not combine with --duration")
    refused(ext + ["--loudness", "-16"], "--loudness")
    refused(ext + ["--peak", "-1"], "--peak")
    refused(ext + ["--true-peak"], "--true-peak")
    refused(ext + ["--out-sample-rate", "48000"], "--out-sample-rate")
    refused(["--init-audio", short, "--extend", "2"], "one latent frame")
    refused(["--init-audio", src, "--extend", "0"], "extend_s")
    refused(["--long-joint"], "--long-joint")
    # what is accepted passes every check and reaches the model
    for flags in (ext, ext + ["--fade-ms", "8"], ext + ["--long-joint"], ["--init-audio", src, "--long-joint"],
                  ["--init-audio", src, "--long-joint", "--inpaint", "--mask-spans", "0.2-0.8"],
                  ["--init-audio", src, "--long-joint", "--inpaint", "--mask-spans", "0.2-0.8", "--keep-original"],
                  ["--init-audio", src]):
        with pytest.raises(AssertionError, match="must not reach"):
            cli.build(cli.parse_args(base + flags))
