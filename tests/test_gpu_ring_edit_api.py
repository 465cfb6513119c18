"""Loops made from a recording through the public surface: AudioLCMEditInfer(loop_from=True) and the CLI's --loop-from,
with --loop-vary, on a small PCM16 file; and --init-audio alone, which keeps its route and its default strength."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

FS = 512
CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
L, TAIL = 60, 37            # the recording: 60 whole latent frames and 37 samples that are trimmed
PROMPT = "a dog barks"


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, infer_api
    _hip.require_device(0)
    return infer_api._build(CONFIG, None, None, 0, True, encoder=True)


@pytest.fixture()
def api(built, monkeypatch):
    """Both front ends on one model build."""
    from audiolcm_amd import cli, infer_api
    monkeypatch.setattr(infer_api, "_build", lambda *a, **k: built)
    monkeypatch.setattr(cli, "build_models", lambda *a, **k: (built[0], built[2]))
    return infer_api


@pytest.fixture()
def recording(tmp_path):
    """Full-range PCM16 noise at 16 kHz: (path, the PCM)."""
    from audiolcm_amd.wavio import read_pcm16, write_pcm16
    path = str(tmp_path / "in.wav")
    pcm = np.random.default_rng(3).integers(-32768, 32768, L * FS + TAIL).astype("<i2")
    write_pcm16(path, pcm.astype(np.float32) / np.float32(32768.0), 16000, scale=32768.0)
    assert np.array_equal(read_pcm16(path)[0], pcm)
    return path, pcm


def _cli(tmp_path, name, *flags):
    from audiolcm_amd.cli import main
    txt, out = str(tmp_path / "p.txt"), str(tmp_path / name)
    with open(txt, "w") as f:
        f.write(PROMPT + "\n")
    recs = main(["--synthetic-seed", "0", "--prompt_txt", txt, "--outdir", out, "--ddim_steps", "2", "--W", "40",
                 "--sample_rate", "16000", "-b", CONFIG, *flags])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")]
    return recs[0]["audio_path"]


def _check_loop_file(path, pcm, m, fade, span=None):
    """One period of L frames at 16 kHz: the recording's PCM wherever a sample is at least ``fade`` samples, round the
    ring, from the m frames either side of the wrap (and from the frames ``span`` = (a, b), regenerated too); new audio
    in the seam."""
    from audiolcm_amd.wavio import read_pcm16
    got, sr = read_pcm16(path)
    assert sr == 16000 and got.shape == (L * FS,)
    lo, hi = m * FS + fade - 1, (L - m) * FS - fade + 1
    assert hi > lo
    for a, b in ([(lo, hi)] if span is None else [(lo, span[0] * FS - fade + 1), (span[1] * FS + fade - 1, hi)]):
        assert b > a and np.array_equal(got[a:b], pcm[a:b])
    assert not np.array_equal(got[:m * FS], pcm[:m * FS]) and not np.array_equal(got[(L - m) * FS:], pcm[(L - m) * FS:L * FS])
    assert not np.array_equal(got[m * FS:lo], pcm[m * FS:lo])                  # the fade does something
    return got


def test_edit_infer_loop_from(api, recording, tmp_path):
    src, pcm = recording
    path = api.AudioLCMEditInfer(PROMPT, src, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / "seam"), loop_from=True, loop_seam_s=0.25)
    assert path == os.path.join(str(tmp_path / "seam"), "a-dog-barks_0.wav")
    got = _check_loop_file(path, pcm, 8, 512)                                   # ceil(0.25 * 16000 / 512) = 8 frames
    # further spans, one of them across the wrap, and a shorter fade
    path = api.AudioLCMEditInfer(PROMPT, src, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / "spans"), loop_from=True, loop_seam_s=0.1, fade_ms=8.0,
                                 mask_spans=[(0.95, 1.03), (1.75, 0.33)])
    # the span across the wrap holds the frames 55 .. 59 and 0 .. 9; 0.95 .. 1.03 s: frames 30 and 31
    more = _check_loop_file(path, pcm, 10, 128, span=(30, 32))
    assert not np.array_equal(more[30 * FS:32 * FS], pcm[30 * FS:32 * FS])
    assert np.array_equal(got[30 * FS:32 * FS], pcm[30 * FS:32 * FS])


def test_cli_loop_from(api, recording, tmp_path, capsys):
    src, pcm = recording
    path = _cli(tmp_path, "seam", "--loop-from", src, "--loop-seam", "0.25")
    assert f"{TAIL} samples" in capsys.readouterr().out                         # the trimmed samples are reported
    got = _check_loop_file(path, pcm, 8, 512)
    again = _check_loop_file(_cli(tmp_path, "again", "--loop-from", src, "--loop-seam", "0.25", "--resample"), pcm, 8, 512)
    assert np.array_equal(got, again)                   # a 16 kHz mono file is read as it is with --resample too
    other = _check_loop_file(_cli(tmp_path, "fade", "--loop-from", src, "--loop-seam", "0.25", "--fade-ms", "8",
                                  "--strength", "0.6"), pcm, 8, 128)
    assert not np.array_equal(got[:8 * FS], other[:8 * FS])


def test_cli_loop_vary(api, recording, tmp_path):
    from audiolcm_amd.wavio import read_pcm16
    src, pcm = recording
    got, sr = read_pcm16(_cli(tmp_path, "vary", "--loop-from", src, "--loop-vary"))
    assert sr == 16000 and got.shape == (L * FS,) and np.abs(got.astype(np.int64)).max() > 0
    assert not np.array_equal(got[20 * FS:40 * FS], pcm[20 * FS:40 * FS])       # the whole ring is made again
    up, sr = read_pcm16(_cli(tmp_path, "vary48", "--loop-from", src, "--loop-vary", "--out-sample-rate", "48000",
                             "--peak", "-6"))
    assert sr == 48000 and up.shape == (L * FS * 3,)                            # one period under the header's rate
    assert np.abs(up.astype(np.int64)).max() <= round(32767 * 10 ** (-6 / 20)) + 1
    lab, sr = read_pcm16(_cli(tmp_path, "label", "--loop-from", src, "--loop-vary", "--sample_rate", "22050"))
    assert sr == 22050 and np.array_equal(lab, got)     # --sample_rate only labels the 16 kHz samples, as for --loop


def test_cli_init_audio_alone_is_the_variation_at_strength_half(api, built, recording, tmp_path):
    """Without the new options --init-audio is routed as it was and at the default strength it had, now that the
    flag's default is resolved after parsing: the file is ``run_edit`` on ``plan_edit``'s variation at 0.5 from this
    tree.  (That those bytes are the ones written before is what the existing "unchanged" tests pin.)"""
    from audiolcm_amd.audio_in import plan_edit
    from audiolcm_amd.infer_api import struct_caption
    from audiolcm_amd.pipeline import AudioLCMPipeline
    from audiolcm_amd.wavio import write_pcm16
    src, _ = recording
    path = _cli(tmp_path, "plain", "--init-audio", src)
    model, _, vocoder, orig_steps = built
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, guidance_scale=5.0, latent_shape=(20, 40),
                            original_inference_steps=orig_steps)
    with torch.no_grad():
        c = model.get_learned_conditioning({"ori_caption": [PROMPT], "struct_caption": [struct_caption(PROMPT)]})
        wav, rate, _ = pipe.run_edit(plan_edit(src), c, [0], 0.5)
    want = str(tmp_path / "want.wav")
    write_pcm16(want, wav[0].cpu().numpy(), 16000, scale=32767.0)
    with open(path, "rb") as f, open(want, "rb") as g:
        data = f.read()
        assert len(data) == 44 + 2 * (L + 1) * FS and data == g.read()
