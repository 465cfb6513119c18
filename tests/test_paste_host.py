"""Host side of keep-original inpainting at any clip length: the window plan and the decode regions of
``AudioLCMPipeline.edit_long``, the fade table of ``kernels.wave_paste``, the exact PCM16 round trip and the new
flags.  No GPU."""
import numpy as np
import pytest
import torch


def _union(L, *spans):
    u = [False] * L
    for lo, hi in spans:            # inclusive frame ranges, as the tables below are written
        u[lo:hi + 1] = [True] * (hi + 1 - lo)
    return u


@pytest.mark.parametrize("spans,starts", [([(50, 54)], [30]), ([(30, 89)], [10, 30, 50]), ([(95, 99)], [60]),
                                          ([(0, 4)], [0]), ([], [])])
def test_edit_window_plan(spans, starts):
    from audiolcm_amd.pipeline import edit_windows
    assert edit_windows(_union(100, *spans), 40, 20) == (starts, 40)
    assert edit_windows(_union(100, *spans), 40) == (starts, 40)   # the default overlap is half a window


def test_edit_window_plan_short_clip_and_errors():
    from audiolcm_amd.pipeline import edit_windows
    assert edit_windows(_union(30, (3, 7)), 40) == ([0], 30)       # one window, at 0, of the clip's own length
    assert edit_windows(_union(30, (0, 29)), 40) == ([0], 30)
    for bad in (0, 40, 41):
        with pytest.raises(ValueError):
            edit_windows(_union(100, (50, 54)), 40, bad)
    # every regenerated frame lies in a window that starts at or before it, whatever the layout
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        u = (torch.rand(100, generator=g) < 0.05).tolist()
        starts, W = edit_windows(u, 40, 20)
        done = [False] * 100
        for s in starts:
            assert 0 <= s <= 60
            done[s:s + W] = [True] * W
        assert all(d or not r for d, r in zip(done, u))


@pytest.mark.parametrize("spans,regions", [([(50, 54)], [(42, 63)]), ([(10, 12), (25, 27)], [(2, 36)]),
                                           ([(0, 3)], [(0, 12)]), ([(97, 99)], [(89, 100)]), ([], []),
                                           ([(10, 12), (40, 41)], [(2, 21), (32, 50)])])
def test_paste_regions(spans, regions):
    from audiolcm_amd.pipeline import paste_regions
    assert paste_regions(_union(100, *spans), 8) == regions


def test_paste_regions_touching_merge():
    from audiolcm_amd.pipeline import paste_regions
    assert paste_regions(_union(100, (10, 11), (28, 29)), 8) == [(2, 38)]     # [2, 20) and [20, 38) touch
    assert paste_regions(_union(100, (10, 11), (29, 30)), 8) == [(2, 20), (21, 39)]
    assert paste_regions(_union(100, (10, 11)), 0) == [(10, 12)]


@pytest.mark.parametrize("R", [1, 2, 64, 512, 700, 8192])
def test_paste_ramp(R):
    from audiolcm_amd.kernels import paste_ramp_host
    r = paste_ramp_host(R)
    assert r.dtype == torch.float32 and r.shape == (R,) and r[0] == 1.0
    assert bool((r[1:] < r[:-1]).all()) and bool((r > 0).all())
    if R % 2 == 0:
        assert r[R // 2] == 0.5
    d = np.arange(R, dtype=np.float64)
    assert np.array_equal(r.numpy(), (0.5 * (1.0 + np.cos(np.pi * d / R))).astype(np.float32))


def test_paste_ramp_empty():
    from audiolcm_amd.kernels import paste_ramp_host
    assert paste_ramp_host(0).shape == (0,)


def test_write_pcm16_scale_round_trips_every_value(tmp_path):
    from audiolcm_amd.wavio import pcm16, read_pcm16, read_wav, write_pcm16
    every = np.arange(-32768, 32768, dtype=np.int32).astype("<i2")
    p = str(tmp_path / "all.wav")
    write_pcm16(p, every.astype(np.float32) / np.float32(32768.0), 16000, scale=32768.0)
    x, sr = read_wav(p)
    assert sr == 16000 and np.array_equal(read_pcm16(p)[0], every)
    q = str(tmp_path / "again.wav")
    write_pcm16(q, x, 16000, scale=32768.0)
    assert open(q, "rb").read() == open(p, "rb").read()
    # the default scale is today's: 32767, under which the same samples do not all come back
    d = str(tmp_path / "default.wav")
    write_pcm16(d, x, 16000)
    back = read_pcm16(d)[0]
    assert np.array_equal(back, np.clip(np.rint(x * np.float32(32767.0)), -32768, 32767).astype("<i2"))
    assert np.array_equal(back, pcm16(x)) and int((back != every).sum()) == 32751
    assert int(np.abs(back.astype(np.int32) - every).max()) == 1


def test_spans_to_mask_inward():
    from audiolcm_amd.infer_api import fade_samples_of, keep_original_mask, spans_to_mask
    # 0.5 - 1.0 s = samples 8000 .. 16000: frames 15 .. 31 outward (today's default), 16 .. 30 inward
    out, inn = spans_to_mask([(0.5, 1.0)], 47), spans_to_mask([(0.5, 1.0)], 47, inward=True)
    assert np.flatnonzero(out).tolist() == list(range(15, 32)) and np.flatnonzero(inn).tolist() == list(range(16, 31))
    assert spans_to_mask([(0.064, 0.128)], 10, inward=True).tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]  # frame-aligned
    assert np.array_equal(keep_original_mask([(0.5, 1.0)], 47), inn)
    with pytest.raises(ValueError, match="whole latent frame"):
        keep_original_mask([(0.5, 0.52)], 47)
    assert fade_samples_of(32.0) == 512 and fade_samples_of(0.0) == 0


def test_keep_original_flags():
    from audiolcm_amd.cli import build, parse_args
    from audiolcm_amd.infer_api import AudioLCMEditInfer
    o = parse_args([])
    assert (o.keep_original, o.fade_ms) == (False, 32.0)
    o = parse_args(["--keep-original", "--fade-ms", "16"])
    assert (o.keep_original, o.fade_ms) == (True, 16.0)
    with pytest.raises(ValueError, match="--keep-original"):
        build(parse_args(["--keep-original", "--init-audio", "a.wav"]))
    with pytest.raises(NotImplementedError):                       # --inpaint alone still raises as it did
        build(parse_args(["--inpaint", "--keep-original"]))
    with pytest.raises(ValueError, match="mask_spans"):
        AudioLCMEditInfer("a dog barks", "missing.wav", keep_original=True)
