"""``loudness=`` / ``peak_dbfs=`` on the public entry points, end to end on the HIP path with the synthetic weights and
a 40-frame latent (1.28 s): the files that are written are decoded and measured by a float64 restatement of ITU-R
BS.1770-4 written here (a plain recursion loop); without the options the files are, byte for byte, what ``GenSamples``
wrote before the options existed.  The entry points share one model build.

Bar: the target +- 0.1 LU on the decoded PCM16, which covers its quantisation; a clip whose peak met the ceiling may
only lie under the target."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
PROMPTS = ["a dog barks", "rain falls on a tin roof", "a car passes by"]
FRAMES = 40
LU_TOL = 0.1


def _biquad(x, b0, b1, b2, a1, a2):
    xp = np.concatenate([np.zeros(2), x])
    f = (b0 * xp[2:] + b1 * xp[1:-1] + b2 * xp[:-2]).tolist()
    y1 = y2 = 0.0
    out = []
    for v in f:
        v = v - a1 * y1 - a2 * y2
        y2 = y1
        y1 = v
        out.append(v)
    return np.array(out)


def _lufs(x, rate):
    """Integrated loudness of the float64 clip x at ``rate``."""
    K = math.tan(math.pi * 1681.974450955533 / rate)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    y = _biquad(x, (Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
                2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / rate)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    y = _biquad(y, 1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    hop = (rate + 5) // 10
    nb = (x.size - 4 * hop) // hop + 1
    z = np.array([np.mean(y[j * hop:j * hop + 4 * hop] ** 2) for j in range(nb)])
    l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    keep &= l > -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    return -0.691 + 10.0 * np.log10(z[keep].mean())


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, infer_api
    _hip.require_device(0)
    return infer_api._build(CONFIG, None, None, 0, True)


@pytest.fixture()
def api(built, monkeypatch):
    from audiolcm_amd import infer_api
    monkeypatch.setattr(infer_api, "_build", lambda *a, **k: built)
    monkeypatch.setattr(built[0], "mel_length", FRAMES)
    return infer_api


def _check_level(path, rate, n, target, peak_dbfs):
    from audiolcm_amd.wavio import read_pcm16
    pcm, sr = read_pcm16(path)
    assert sr == rate and pcm.shape == (n,)
    top = int(np.abs(pcm.astype(np.int32)).max())
    limit = int(np.float32(10.0 ** (peak_dbfs / 20.0)) * np.float32(32767.0)) + 1   # the ceiling in PCM16 steps
    assert 0 < top <= limit < 32767                                                  # so nothing sits at full scale
    got = _lufs(pcm.astype(np.float64) / 32767.0, rate)
    bound = top >= limit - 1
    print(f"{os.path.basename(path)}: {got:.3f} LUFS for {target}, peak {top} of {limit}{' (bound)' if bound else ''}")
    assert got <= target + LU_TOL and (bound or got >= target - LU_TOL), (got, target, top, limit)
    return got


def test_batch_infer_writes_the_target_loudness(api, tmp_path):
    out = str(tmp_path / "lv")
    path = api.AudioLCMBatchInfer(PROMPTS, config_path=CONFIG, synthetic_seed=0, batch_size=2, outpath=out, seed=7,
                                  loudness=-23.0)
    assert path == os.path.join(out, "a-car-passes-by_0.wav")
    for p in PROMPTS:
        _check_level(os.path.join(out, p.replace(" ", "-") + "_0.wav"), 16000, FRAMES * 512, -23.0, -1.0)


def test_batch_infer_without_the_options_writes_what_it_wrote(api, built, tmp_path):
    """The options left off: the files of ``GenSamples`` driven as before, byte for byte; and a level changes them."""
    from audiolcm_amd.infer_api import GenSamples, struct_caption, wav_name_for
    a, b, c = (str(tmp_path / d) for d in "abc")
    api.AudioLCMBatchInfer(PROMPTS[:2], config_path=CONFIG, synthetic_seed=0, outpath=a, seed=7)
    api.AudioLCMBatchInfer(PROMPTS[:2], config_path=CONFIG, synthetic_seed=0, outpath=c, seed=7, loudness=-30.0)
    model, sampler, vocoder, orig_steps = built
    os.makedirs(b)
    gen = GenSamples(sampler, model, b, vocoder, save_mel=False, save_wav=True, original_inference_steps=orig_steps)
    assert gen.level is None
    with torch.no_grad():
        gen.gen_batch([dict(ori_caption=p, struct_caption=struct_caption(p)) for p in PROMPTS[:2]],
                      [wav_name_for(p) for p in PROMPTS[:2]], seeds=[7, 8])
    for p in PROMPTS[:2]:
        name = wav_name_for(p) + "_0.wav"
        with open(os.path.join(a, name), "rb") as f, open(os.path.join(b, name), "rb") as g:
            got, want = f.read(), g.read()
        assert len(got) == 44 + 2 * FRAMES * 512 and got == want
        with open(os.path.join(c, name), "rb") as f:
            assert f.read() != want


def test_long_infer_measures_at_the_output_rate_after_the_crop(api, tmp_path):
    path = api.AudioLCMLongInfer("a dog barks", duration_s=2, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / "long"), out_sample_rate=48000, loudness=-20.0, peak_dbfs=-2.0)
    _check_level(path, 48000, 96000, -20.0, -2.0)
