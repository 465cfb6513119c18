"""Host side of audio-conditioned generation (variation, inpainting, long-form): the strength schedule, the edit
noise draws, the span -> latent-frame mask, the RIFF reader, the long-form window layout and the CLI flags.  No GPU."""
import struct

import numpy as np
import pytest
import torch


def test_sample_plan_strength():
    """scheduling_lcm.py:171 with strength 0.5: the origin list 20 i - 1 for i <= 25, reversed, at the indices
    floor(linspace(0, 25, S, endpoint=False))."""
    from audiolcm_amd import schedule
    assert [p["t"] for p in schedule.sample_plan(2, 50, strength=0.5)] == [499, 259]
    assert [p["t"] for p in schedule.sample_plan(4, 50, strength=0.5)] == [499, 379, 259, 139]
    origin = (np.arange(1, 26) * 20 - 1)[::-1]
    for S in (1, 2, 3, 4, 5):
        idx = np.floor(np.linspace(0, 25, S, endpoint=False)).astype(int)
        plan = schedule.sample_plan(S, 50, strength=0.5)
        assert [p["t"] for p in plan] == [int(v) for v in origin[idx]]
        assert [p["add_noise"] for p in plan] == [True] * (S - 1) + [False]
        assert plan[-1]["prev_t"] == plan[-1]["t"]


def test_sample_plan_default_strength_is_todays_plan():
    from audiolcm_amd import schedule
    for S in (1, 2, 4):
        assert schedule.sample_plan(S, 50, strength=1.0) == schedule.sample_plan(S, 50)
    assert [p["t"] for p in schedule.sample_plan(2, 50)] == [999, 499]


def test_sample_plan_strength_too_small_raises():
    from audiolcm_amd import schedule
    with pytest.raises(ValueError, match="original_steps x strength"):
        schedule.sample_plan(2, 50, strength=0.02)


def test_edit_noise_extends_prompt_noise():
    from audiolcm_amd import recipe
    seeds = [3, 11, 4]
    for S in (1, 2, 4):
        xT, nz = recipe.prompt_noise(seeds, S, 20, 24)
        n0, noise, e0 = recipe.edit_noise(seeds, S, 20, 24)
        assert torch.equal(n0, xT) and torch.equal(noise, nz) and noise.shape == (S - 1, 3, 20, 24)
        assert e0.shape == (3, 20, 24) and e0.dtype == torch.float32
        assert torch.equal(e0, recipe.edit_noise(seeds, S, 20, 24)[2])
        assert not torch.equal(e0, n0)
        # per prompt: a clip's draws do not depend on its neighbours
        assert torch.equal(recipe.edit_noise([11], S, 20, 24)[2][0], e0[1])


def test_window_seed_is_a_function_of_seed_and_window():
    from audiolcm_amd import recipe
    assert recipe.window_seed(7, 0) == 7
    seen = {recipe.window_seed(s, k) for s in range(64) for k in range(8)}
    assert len(seen) == 64 * 8 and all(0 <= v < 2 ** 63 for v in seen)


def test_spans_to_mask_edges():
    from audiolcm_amd.infer_api import parse_spans, spans_to_mask
    # one latent frame = 512 samples = 32 ms at 16 kHz
    assert spans_to_mask([], 10).tolist() == [0.0] * 10 and spans_to_mask([], 10).dtype == np.float32
    assert spans_to_mask([(0.064, 0.128)], 10).tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]      # frame-aligned [2, 4)
    assert spans_to_mask([(0.064, 0.129)], 10).tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0]      # ends mid-frame: outward
    assert spans_to_mask([(0.070, 0.128)], 10).tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]      # starts mid-frame: outward
    assert spans_to_mask([(0.256, 5.0)], 10).tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1]        # past the clip: clipped
    assert spans_to_mask([(4.0, 5.0)], 10).tolist() == [0.0] * 10
    assert spans_to_mask([(-1.0, 0.01)], 10).tolist() == [1] + [0] * 9
    assert spans_to_mask([(0.0, 0.032), (0.288, 0.32)], 10).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert spans_to_mask([(0.2, 0.1)], 10).tolist() == [0.0] * 10                              # empty span
    assert parse_spans("2.0-4.5,7-8") == [(2.0, 4.5), (7.0, 8.0)]
    with pytest.raises(ValueError):
        parse_spans("2.0")


def _wav_bytes(pcm: np.ndarray, sr=16000, channels=1, bits=16, extra=b""):
    data = pcm.tobytes()
    fmt = struct.pack("<IHHIIHH", 16, 1, channels, sr, sr * channels * bits // 8, channels * bits // 8, bits)
    body = b"WAVE" + b"fmt " + fmt + extra + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_read_wav_round_trips_write_pcm16(tmp_path):
    from audiolcm_amd.wavio import pcm16, read_pcm16, read_wav, write_pcm16
    x = np.sin(np.arange(3000, dtype=np.float32) * 0.05) * 0.9
    p = str(tmp_path / "a.wav")
    write_pcm16(p, x, 16000)
    y, sr = read_wav(p)
    assert sr == 16000 and y.dtype == np.float32 and y.shape == x.shape and np.abs(y).max() <= 1.0
    assert np.array_equal(np.rint(y * 32768.0).astype(np.int16), pcm16(x))
    assert np.array_equal(read_pcm16(p)[0], pcm16(x))
    assert np.abs(y - x).max() <= 1.0 / 32767 + 0.5 / 32768  # one quantisation step plus the 32767 / 32768 scale
    # a LIST chunk of odd length (word-aligned with a pad byte) before `data`: the 44-byte reader would misread it
    q = str(tmp_path / "b.wav")
    extra = b"LIST" + struct.pack("<I", 7) + b"INFOabc" + b"\x00"
    with open(q, "wb") as f:
        f.write(_wav_bytes(pcm16(x), extra=extra))
    z, sr = read_wav(q)
    assert sr == 16000 and np.array_equal(z, y)


def test_read_wav_refuses_other_formats(tmp_path):
    from audiolcm_amd.wavio import read_wav
    pcm = np.zeros(64, dtype="<i2")
    for name, kw in (("stereo", dict(channels=2)), ("u8", dict(bits=8))):
        p = str(tmp_path / f"{name}.wav")
        with open(p, "wb") as f:
            f.write(_wav_bytes(pcm, **kw))
        with pytest.raises(ValueError):
            read_wav(p)
    p = str(tmp_path / "junk.wav")
    with open(p, "wb") as f:
        f.write(b"not a wave file at all")
    with pytest.raises(ValueError):
        read_wav(p)


def test_load_init_audio_pads_crops_and_checks_rate(tmp_path):
    from audiolcm_amd.infer_api import load_init_audio
    from audiolcm_amd.wavio import write_pcm16
    p = str(tmp_path / "a.wav")
    write_pcm16(p, np.full(1000, 0.5, np.float32), 16000)
    x = load_init_audio(p, 845)
    assert x.shape == (1024,) and np.all(x[1000:] == 0) and np.all(x[:1000] > 0.49)
    assert load_init_audio(p, 1).shape == (512,)
    write_pcm16(p, np.zeros(1024, np.float32), 22050)
    with pytest.raises(ValueError, match="sample rate"):
        load_init_audio(p, 845)


def test_long_windows_layout():
    from audiolcm_amd.pipeline import AudioLCMPipeline
    pipe = AudioLCMPipeline.__new__(AudioLCMPipeline)
    pipe.latent_shape = (20, 312)
    assert pipe.long_windows(936) == ([(0, 0), (156, 156), (312, 156), (468, 156), (624, 156)], 312)
    assert pipe.long_windows(60, 40, 20) == ([(0, 0), (20, 20)], 40)
    assert pipe.long_windows(70, 40, 20) == ([(0, 0), (20, 20), (30, 30)], 40)   # last window shifted to end at 70
    assert pipe.long_windows(24) == ([(0, 0)], 24)
    for L in range(313, 1000, 37):
        spans, W = pipe.long_windows(L)
        end = W
        for start, known in spans[1:]:
            assert known >= 156 and start + known == end and start + W <= L
            end = start + W
        assert end == L
    with pytest.raises(ValueError):
        pipe.long_windows(100, 40, 40)


def test_cli_edit_flags():
    from audiolcm_amd.cli import build, parse_args
    o = parse_args([])
    assert (o.init_audio, o.strength, o.mask_spans, o.duration, o.inpaint) == (None, 0.5, None, None, False)
    o = parse_args(["--init-audio", "a.wav", "--strength", "0.3", "--inpaint", "--mask-spans", "2.0-4.5,7-8",
                    "--duration", "30"])
    assert (o.init_audio, o.strength, o.mask_spans, o.duration, o.inpaint) == ("a.wav", 0.3, "2.0-4.5,7-8", 30.0, True)
    with pytest.raises(NotImplementedError):
        build(parse_args(["--inpaint"]))
    with pytest.raises(NotImplementedError):
        build(parse_args(["--inpaint", "--init-audio", "a.wav"]))
    with pytest.raises(NotImplementedError):
        build(parse_args(["--plms"]))
    with pytest.raises(ValueError):
        build(parse_args(["--mask-spans", "1-2"]))
