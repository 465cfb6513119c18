"""The front end by composition: each mode's file from ``AudioLCMEditInfer`` is, byte for byte, a pipeline primitive's
waveform through ``write_pcm16``; the command line writes the bytes the Python entry point writes; and ``run_edit`` on a
batch is ``edit`` on the posterior of the one recording expanded to the batch.  Synthetic weights, 2 steps, split
precision, 1.5 s inputs (47 latent frames; 94 at 3 s); one model build for the module, which both front ends are given
in place of their own."""
import os
import struct

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
PROMPT = "a dog barks"
SPANS = [(0.5, 1.0)]


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, infer_api
    _hip.require_device(0)
    return infer_api._build(CONFIG, None, None, 0, True, encoder=True)


@pytest.fixture()
def api(built, monkeypatch):
    """Both front ends on the one shared model."""
    from audiolcm_amd import cli, infer_api
    monkeypatch.setattr(infer_api, "_build", lambda *a, **k: built)
    monkeypatch.setattr(cli, "build_models", lambda *a, **k: (built[0], built[2]))
    return infer_api


@pytest.fixture(scope="module")
def pipe(built):
    from audiolcm_amd.pipeline import AudioLCMPipeline
    model, sampler, vocoder, orig_steps = built
    return AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                            latent_shape=(model.mel_dim, model.mel_length))


def _cond(built, n=1):
    from audiolcm_amd.infer_api import struct_caption
    with torch.no_grad():
        return built[0].get_learned_conditioning({"ori_caption": [PROMPT] * n,
                                                  "struct_caption": [struct_caption(PROMPT)] * n})


def _write_wav(path, n, rate, seed=3):
    """n samples of full-range mono PCM16 noise at ``rate``."""
    q = np.random.default_rng(seed).integers(-32768, 32768, n).astype("<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * n) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16))
        f.write(b"data" + struct.pack("<I", 2 * n) + q.tobytes())
    return str(path)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _ref_bytes(tmp_path, wav, rate, **kw):
    from audiolcm_amd.wavio import write_pcm16
    ref = str(tmp_path / "ref.wav")
    write_pcm16(ref, wav.cpu().numpy(), rate, **kw)
    return _bytes(ref)


def _infer(api, src, tmp_path, **kw):
    return _bytes(api.AudioLCMEditInfer(PROMPT, src, synthetic_seed=0, seed=3, config_path=CONFIG,
                                        outpath=str(tmp_path / "py"), **kw))


@pytest.mark.parametrize("spans", [None, SPANS], ids=["variation", "inpaint"])
def test_edit_infer_is_pipeline_edit(api, built, pipe, tmp_path, spans):
    from audiolcm_amd.infer_api import load_init_audio, spans_to_mask
    src = _write_wav(tmp_path / "in.wav", 24000, 16000)
    got = _infer(api, src, tmp_path, mask_spans=spans)
    loaded = load_init_audio(src, 845)
    assert loaded.shape == (47 * 512,)
    mask = None if spans is None else torch.from_numpy(spans_to_mask(spans, 47))[None]
    wav = pipe.edit(_cond(built), [3], wav=torch.from_numpy(loaded)[None], mask=mask)["wav"][0]
    assert len(got) == 44 + 2 * 47 * 512 and got == _ref_bytes(tmp_path, wav, 16000)


def test_keep_original_is_edit_long_at_16k(api, built, pipe, tmp_path):
    from audiolcm_amd.infer_api import keep_original_mask, load_init_audio_whole
    src = _write_wav(tmp_path / "in.wav", 24000, 16000)
    got = _infer(api, src, tmp_path, mask_spans=SPANS, keep_original=True, fade_ms=32)
    loaded, n = load_init_audio_whole(src)
    assert n == 24000
    out = pipe.edit_long(_cond(built), [3], wav=loaded[None], mask=keep_original_mask(SPANS, 47)[None],
                         keep_original=True, fade_samples=512)
    assert len(got) == 44 + 2 * 24000 and got == _ref_bytes(tmp_path, out["wav"][0, :24000], 16000, scale=32768.0)


def test_keep_original_is_edit_long_at_48k(api, built, pipe, tmp_path):
    from audiolcm_amd.infer_api import keep_original_mask
    from audiolcm_amd.wavio import read_audio
    src = _write_wav(tmp_path / "in48.wav", 144000, 48000)           # 3 s: 93.75 -> 94 frames of 1536
    got = _infer(api, src, tmp_path, mask_spans=[(1.0, 1.5)], keep_original=True, fade_ms=32, resample=True)
    x, sr = read_audio(src)
    loaded = np.pad(x[:, 0], (0, 94 * 1536 - 144000))
    out = pipe.edit_long(_cond(built), [3], wav=loaded[None], mask=keep_original_mask([(1.0, 1.5)], 94)[None],
                         keep_original=True, rate=48000, fade_samples=1536)
    assert sr == 48000 and len(got) == 44 + 2 * 144000
    assert got == _ref_bytes(tmp_path, out["wav"][0, :144000], 48000, scale=32768.0)


CLI_CASES = {
    "inpaint": (16000, [], {}, 47 * 512),
    "keep_original": (16000, ["--keep-original"], dict(keep_original=True), 24000),
    "keep_original_resample": (48000, ["--keep-original", "--resample"], dict(keep_original=True, resample=True),
                               72000),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_cli_writes_what_the_python_entry_point_writes(api, tmp_path, case):
    from audiolcm_amd.cli import main
    rate, flags, kw, n_out = CLI_CASES[case]
    src = _write_wav(tmp_path / "in.wav", 3 * rate // 2, rate)       # 1.5 s
    txt, out = str(tmp_path / "p.txt"), str(tmp_path / "cli")
    with open(txt, "w") as f:
        f.write(PROMPT + "\n")
    recs = main(["--synthetic-seed", "0", "--prompt_txt", txt, "--outdir", out, "-b", CONFIG, "--init-audio", src,
                 "--inpaint", "--mask-spans", "0.5-1.0", *flags,
                 "--precision", "split", "--seed", "3", "--ddim_steps", "2", "--sample_rate", "16000"])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")]
    want = _infer(api, src, tmp_path, mask_spans=SPANS, **kw)
    assert len(want) == 44 + 2 * n_out and _bytes(recs[0]["audio_path"]) == want


def test_run_edit_on_a_batch_is_edit_on_the_expanded_posterior(built, pipe, tmp_path):
    """The recording is encoded once and its posterior expanded to the batch; each row then has its own seed."""
    from audiolcm_amd.audio_in import plan_edit, spans_to_mask
    from audiolcm_amd.mel import MelNet
    from audiolcm_amd.models import DiagonalGaussianDistribution
    plan = plan_edit(_write_wav(tmp_path / "in.wav", 24000, 16000), SPANS)
    c = _cond(built, 2)
    wav, rate, mel = pipe.run_edit(plan, c, [3, 4])
    with torch.no_grad():
        post = built[0].encode_first_stage(MelNet()(plan.samples))
    init = DiagonalGaussianDistribution(post.parameters.expand(2, -1, -1).contiguous())
    ref = pipe.edit(c, [3, 4], latent=init, mask=torch.from_numpy(spans_to_mask(SPANS, 47)).expand(2, 47))
    assert rate == 16000 and wav.shape == (2, 47 * 512)
    assert torch.equal(wav, ref["wav"]) and torch.equal(mel, ref["mel"])
    assert not torch.equal(wav[0], wav[1])
