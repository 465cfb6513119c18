"""Recordings in at any rate and audio out at any rate, end to end on the HIP path with the synthetic weights:
``AudioLCMEditInfer(resample=True)`` on a 48 kHz stereo PCM24 file, ``out_sample_rate`` on the long-form entry point,
the keep-original edit at the recording's own rate (``AudioLCMPipeline.edit_long(rate=...)``) and the two command-line
flags.  The Python entry points share one model build (``infer_api._build`` is what every one of them calls first)."""
import os
import struct

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
F48 = 1536                      # one latent frame at 48 kHz


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, infer_api
    _hip.require_device(0)
    return infer_api._build(CONFIG, None, None, 0, True, encoder=True)


@pytest.fixture()
def api(built, monkeypatch):
    from audiolcm_amd import infer_api
    monkeypatch.setattr(infer_api, "_build", lambda *a, **k: built)
    return infer_api


def _write_wav(path, x, rate, bits):
    """x (N, channels) float -> PCM16 or PCM24 file; returns the integer samples."""
    ch = x.shape[1]
    full = 1 << (bits - 1)
    q = np.clip(np.rint(x * full), -full, full - 1).astype("<i4")
    data = q.astype("<i2").tobytes() if bits == 16 else q.reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    block = ch * bits // 8
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * block, block, bits))
        f.write(b"data" + struct.pack("<I", len(data)) + data)
    return q


def _noise(n, ch, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, (n, ch))


def test_edit_infer_reads_a_48k_stereo_pcm24_file(api, tmp_path):
    from audiolcm_amd.wavio import read_wav
    src = str(tmp_path / "in48.wav")
    _write_wav(src, 0.5 * _noise(72000, 2), 48000, 24)       # 1.5 s
    path = api.AudioLCMEditInfer("a dog barks", src, strength=0.5, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / "edit"), resample=True)
    x, sr = read_wav(path)
    assert sr == 16000 and x.shape == (47 * 512,) and np.isfinite(x).all() and np.abs(x).max() > 0
    with pytest.raises(ValueError, match="only mono PCM16"):      # as before: read_wav's own refusal
        api.AudioLCMEditInfer("a dog barks", src, strength=0.5, synthetic_seed=0, seed=3, config_path=CONFIG,
                              outpath=str(tmp_path / "edit2"))


def test_loader_resamples_what_the_kernel_resamples(built, tmp_path):
    """``load_init_audio(resample=True)`` is ``read_audio`` -> one ``kernels.resample`` -> pad and crop."""
    from audiolcm_amd import kernels
    from audiolcm_amd.infer_api import load_init_audio, load_init_audio_whole
    from audiolcm_amd.wavio import read_audio
    src = str(tmp_path / "in441.wav")
    _write_wav(src, 0.5 * _noise(10000, 2), 44100, 16)
    x, sr = read_audio(src)
    want = kernels.resample(torch.from_numpy(x).cuda()[None], 44100, 16000, channels=2)[0].cpu().numpy()
    assert want.shape == (3629,)
    got, n = load_init_audio_whole(src, resample=True)
    assert n == 3629 and got.shape == (8 * 512,) and np.array_equal(got[:n], want) and not got[n:].any()
    assert np.array_equal(load_init_audio(src, 3, resample=True), want[:3 * 512])


def test_long_infer_out_sample_rate(api, built, tmp_path):
    from audiolcm_amd.wavio import read_pcm16
    path = api.AudioLCMLongInfer("a dog barks", duration_s=2, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / "a"), out_sample_rate=48000)
    pcm, sr = read_pcm16(path)
    assert sr == 48000 and pcm.shape == (96000,) and np.abs(pcm).max() > 0
    # out_sample_rate=None: the file is what the code path before this keyword writes, the pipeline's waveform through
    # write_pcm16 at 16 kHz, byte for byte
    from audiolcm_amd.infer_api import struct_caption
    from audiolcm_amd.pipeline import AudioLCMPipeline
    from audiolcm_amd.wavio import write_pcm16
    path = api.AudioLCMLongInfer("a dog barks", duration_s=2, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / "b"), out_sample_rate=None)
    model, sampler, vocoder, orig_steps = built
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                            latent_shape=(model.mel_dim, model.mel_length))
    with torch.no_grad():
        c = model.get_learned_conditioning({"ori_caption": ["a dog barks"],
                                            "struct_caption": [struct_caption("a dog barks")]})
        wav = pipe.generate_long(c, [3], 63)["wav"].cpu().numpy()
    ref = str(tmp_path / "ref.wav")
    write_pcm16(ref, wav[0], 16000)
    with open(path, "rb") as f, open(ref, "rb") as g:
        got, want = f.read(), g.read()
    assert len(got) == 44 + 2 * 63 * 512 and got == want


# ---------------------------------------------------------------------------- keep-original at 48 kHz
LO, HI = 32 * F48, 46 * F48     # the whole 32 ms frames inside 1.0 - 1.5 s
FADE = F48                      # 32 ms at 48 kHz


def _check_kept_48k(path, pcm):
    from audiolcm_amd.wavio import read_pcm16
    got, sr = read_pcm16(path)
    assert sr == 48000 and got.shape == (144000,)
    assert np.array_equal(got[:LO - FADE], pcm[:LO - FADE]) and np.array_equal(got[HI + FADE:], pcm[HI + FADE:])
    assert not np.array_equal(got[LO:HI], pcm[LO:HI])


def test_keep_original_at_the_recordings_own_rate(api, tmp_path):
    src, src441 = str(tmp_path / "in48.wav"), str(tmp_path / "in441.wav")
    x = _noise(144000, 1)                                    # 3 s, full-range PCM16
    pcm = _write_wav(src, x, 48000, 16)[:, 0].astype("<i2")
    _write_wav(src441, x[:132300], 44100, 16)
    kw = dict(strength=0.5, mask_spans=[(1.0, 1.5)], synthetic_seed=0, seed=3, config_path=CONFIG,
              keep_original=True, fade_ms=32, resample=True)
    path = api.AudioLCMEditInfer("a dog barks", src, outpath=str(tmp_path / "edit"), **kw)
    _check_kept_48k(path, pcm)
    with pytest.raises(ValueError, match="48000"):
        api.AudioLCMEditInfer("a dog barks", src441, outpath=str(tmp_path / "edit2"), **kw)


def test_edit_long_native_needs_a_halo_past_the_filter(built):
    from audiolcm_amd import recipe
    from audiolcm_amd.pipeline import AudioLCMPipeline
    model, sampler, vocoder, orig_steps = built
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                            latent_shape=(model.mel_dim, model.mel_length))
    ctx = recipe.synthetic_context(1).cuda()
    wav = torch.zeros((1, 20 * F48))
    mask = torch.zeros((1, 20))
    mask[0, 8:10] = 1.0
    # fade 1536 at 48 kHz = 512 at 16 kHz, |first| = 34: 547 samples are needed, one frame of halo has 512
    with pytest.raises(ValueError, match="halo_frames"):
        pipe.edit_long(ctx, [1], wav=wav, mask=mask, keep_original=True, rate=48000, fade_samples=F48, halo_frames=1)
    with pytest.raises(ValueError, match="125 Hz"):
        pipe.edit_long(ctx, [1], wav=wav, mask=mask, keep_original=True, rate=44100)
    with pytest.raises(ValueError, match="multiple of 1536"):
        pipe.edit_long(ctx, [1], wav=wav[:, :-1], mask=mask, keep_original=True, rate=48000)


# ---------------------------------------------------------------------------- the command line
def _cli(tmp_path, *flags):
    from audiolcm_amd.cli import main
    txt, out = str(tmp_path / "p.txt"), str(tmp_path / "out")
    with open(txt, "w") as f:
        f.write("a dog barks\n")
    recs = main(["--synthetic-seed", "0", "--prompt_txt", txt, "--outdir", out, "--ddim_steps", "2", "-b", CONFIG,
                 *flags])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")]
    return recs[0]["audio_path"]


def test_cli_keep_original_resample(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    src = str(tmp_path / "in48.wav")
    pcm = _write_wav(src, _noise(144000, 1), 48000, 16)[:, 0].astype("<i2")
    _check_kept_48k(_cli(tmp_path, "--init-audio", src, "--inpaint", "--mask-spans", "1.0-1.5", "--keep-original",
                         "--resample"), pcm)


def test_cli_out_sample_rate(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.wavio import read_pcm16
    pcm, sr = read_pcm16(_cli(tmp_path, "--W", "40", "--out-sample-rate", "44100"))
    assert sr == 44100 and pcm.shape == (-(-40 * 512 * 441 // 160),) and np.abs(pcm).max() > 0
