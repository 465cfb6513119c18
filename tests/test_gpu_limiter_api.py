"""The limiter in the level stage, end to end on the HIP path: ``kernels.normalize_loudness(limiter=...)`` against the
float64 pipeline of ``tests/_limiter_ref.py`` (the float64 meter of ``test_gpu_loudness.py`` restated, the limiter's
restatement and the same number of passes), and ``limiter=`` / ``--limiter`` on the public entry points with the
synthetic weights and a 40-frame latent, as ``test_gpu_loudness_api.py`` runs them.

The clip is the material a static gain under a ceiling leaves too quiet: a quiet tone and noise with a short loud burst
every 250 ms (2 s, target -14 LUFS, ceiling -1 dBFS).  Before the GPU is touched the float64 pipeline alone must end at
least 3 LU nearer the target than the static gain does, with every block 0.5 LU or more from both gates.

Bars: ``lufs_out`` within 0.01 LU of the float64 pipeline's (the meter's own bar); with ``true_peak`` the 4x peak of
the output within 4 * 2^-24 of the float64 pipeline's, relative; the files' peaks at most the ceiling in PCM16 steps."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import _limiter_ref as ref
from conftest import REPO

pytestmark = pytest.mark.gpu

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
PROMPTS = ["a dog barks", "rain falls on a tin roof"]
FRAMES = 40
LU_TOL = 0.01
TARGET, PEAK_DBFS, PASSES = -14.0, -1.0, 3
C = ref.ceiling_of(PEAK_DBFS)


def _times(rate):
    from audiolcm_amd import limiter
    return limiter.plan(rate, int(round(2.0 * rate)))


def _quiet(rate):
    n = int(round(2.0 * rate))
    t = np.arange(n) / rate
    return (0.1 * np.sin(2 * np.pi * 330.0 * t) + 0.02 * np.random.default_rng(2).standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _expected(rate):
    """Once per rate: the burst clip, the quiet clip, and the float64 results for both (read-only)."""
    pl = _times(rate)
    x, q = ref.burst_signal(rate), _quiet(rate)
    st = ref.static64(x, rate, TARGET, C)
    lim = ref.pipeline64(x, rate, TARGET, C, pl.lookahead, pl.release_coef, PASSES)
    ql = ref.pipeline64(q, rate, TARGET, C, pl.lookahead, pl.release_coef, PASSES)
    for v in (x, q, lim["wav"], ql["wav"]):
        v.setflags(write=False)
    return x, q, st, lim, ql


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip
    _hip.require_device(0)
    return torch.device("cuda")


@pytest.mark.parametrize("rate", [16000, 48000])
def test_normalize_with_a_limiter_reaches_the_target(rate):
    x, q, st, lim, ql = _expected(rate)
    print(f"{rate} Hz float64: static {st['lufs_out']:.3f} LUFS, limiter {lim['lufs_out']:.3f} LUFS")
    assert lim["binds"] and not ql["binds"]
    assert abs(st["lufs_out"] - TARGET) - abs(lim["lufs_out"] - TARGET) >= 3.0
    assert min(st["margin"], lim["margin"], ql["margin"]) >= 0.5
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    xs = torch.from_numpy(np.stack([x, q])).cuda()
    res = kernels.normalize_loudness(xs, rate, TARGET, PEAK_DBFS, limiter=_times(rate), passes=PASSES, report=True)
    plain = kernels.normalize_loudness(xs, rate, TARGET, PEAK_DBFS)
    assert "lufs_out" not in plain
    got = res["lufs_out"].cpu().numpy()
    print(f"{rate} Hz gpu: {got[0]:.4f} LUFS for {lim['lufs_out']:.4f}; quiet {got[1]:.4f} for {ql['lufs_out']:.4f}")
    assert abs(got[0] - lim["lufs_out"]) <= LU_TOL and abs(got[1] - ql["lufs_out"]) <= LU_TOL
    assert abs(got[1] - TARGET) <= LU_TOL
    wav = res["wav"].cpu().numpy()
    assert np.abs(wav).max() <= C
    # the clip that never reaches the ceiling: the bytes of the level stage without a limiter
    assert torch.equal(res["wav"][1].view(torch.int32), plain["wav"][1].view(torch.int32))
    assert torch.equal(res["gain"][1:], plain["gain"][1:]) and torch.equal(res["lufs"], plain["lufs"])
    assert not torch.equal(res["wav"][0], plain["wav"][0])


def test_true_peak_limits_the_oversampled_estimate(dev):
    """The limiter sees ``resample(wav, rate, 4 * rate)``; the 4x peak of what it returns equals the float64 pipeline's
    (fed the same oversampled copy).  Its overshoot over the ceiling is printed, not asserted: the limited clip is not
    band-limited the way the copy was."""
    from audiolcm_amd import kernels
    rate = 16000
    pl = _times(rate)
    x = _expected(rate)[0]
    xs = torch.from_numpy(x[None].copy()).to(dev)
    env = kernels.resample(xs, rate, 4 * rate).cpu().numpy()[0]
    assert env.size == 4 * x.size
    want = ref.pipeline64(x, rate, TARGET, C, pl.lookahead, pl.release_coef, PASSES, env, 4)
    assert want["binds"] and want["margin"] >= 0.5
    res = kernels.normalize_loudness(xs, rate, TARGET, PEAK_DBFS, true_peak=True, limiter=pl, passes=PASSES,
                                     report=True)
    assert abs(float(res["lufs_out"][0]) - want["lufs_out"]) <= LU_TOL
    assert float(res["wav"].abs().max()) <= C
    peak_got = float(kernels.resample(res["wav"], rate, 4 * rate).abs().max())
    peak_want = float(kernels.resample(torch.from_numpy(want["wav"][None].copy()).to(dev), rate, 4 * rate).abs().max())
    print(f"4x peak {peak_got:.7f} for {peak_want:.7f}; over the ceiling by {20 * math.log10(peak_got / float(C)):+.3f} dB")
    assert abs(peak_got - peak_want) <= 4 * 2.0 ** -24 * peak_want


# ---------------------------------------------------------------------------- the entry points
@pytest.fixture(scope="module")
def built(dev):
    from audiolcm_amd import infer_api
    return infer_api._build(CONFIG, None, None, 0, True)


@pytest.fixture()
def api(built, monkeypatch):
    from audiolcm_amd import cli, infer_api
    monkeypatch.setattr(infer_api, "_build", lambda *a, **k: built)
    monkeypatch.setattr(cli, "build_models", lambda *a, **k: (built[0], built[2]))
    monkeypatch.setattr(built[0], "mel_length", FRAMES)
    return infer_api


def _no_limiter(monkeypatch):
    from audiolcm_amd import kernels

    def stop(*a, **k):
        raise AssertionError("the limiter ran without being asked for")
    monkeypatch.setattr(kernels, "limit", stop)


def _peak_ok(path, rate, n):
    from audiolcm_amd.wavio import read_pcm16
    pcm, sr = read_pcm16(path)
    assert sr == rate and pcm.shape == (n,)
    top = int(np.abs(pcm.astype(np.int32)).max())
    limit = int(C * np.float32(32767.0)) + 1
    assert 0 < top <= limit, (top, limit)
    return pcm


def test_batch_infer_with_a_limiter(api, built, tmp_path, monkeypatch):
    """``limiter=True``: the files' peaks are at most the ceiling.  Without it: the files of ``GenSamples`` driven as
    before the option existed, byte for byte, and the limiter is never called."""
    from audiolcm_amd.infer_api import GenSamples, struct_caption, wav_name_for
    a, b, c = (str(tmp_path / d) for d in "abc")
    api.AudioLCMBatchInfer(PROMPTS, config_path=CONFIG, synthetic_seed=0, outpath=a, seed=7, loudness=TARGET, limiter=True)
    for p in PROMPTS:
        _peak_ok(os.path.join(a, wav_name_for(p) + "_0.wav"), 16000, FRAMES * 512)
    _no_limiter(monkeypatch)
    api.AudioLCMBatchInfer(PROMPTS, config_path=CONFIG, synthetic_seed=0, outpath=b, seed=7, loudness=TARGET)
    model, sampler, vocoder, orig_steps = built
    os.makedirs(c)
    gen = GenSamples(sampler, model, c, vocoder, False, True, orig_steps, 2, 5.0, None, TARGET, None, False)
    with torch.no_grad():
        gen.gen_batch([dict(ori_caption=p, struct_caption=struct_caption(p)) for p in PROMPTS],
                      [wav_name_for(p) for p in PROMPTS], seeds=[7, 8])
    for p in PROMPTS:
        name = wav_name_for(p) + "_0.wav"
        with open(os.path.join(b, name), "rb") as f, open(os.path.join(c, name), "rb") as g:
            assert f.read() == g.read()


def test_cli_with_a_limiter(api, tmp_path, monkeypatch):
    """``--limiter`` with its two times: the file's peak is at most the ceiling.  Without the flag the command line has
    no route that avoids the new option plumbing to compare against (``cli.GenSamples`` reads the flags from ``opt``),
    so this half rests on the guard: ``kernels.limit`` is never called, which leaves ``normalize_loudness`` on the
    branch that is the code of before, and two such runs write the same bytes.  The byte comparison against the entry
    driven as before the option existed is ``test_batch_infer_with_a_limiter``'s."""
    from audiolcm_amd.cli import main
    txt = str(tmp_path / "p.txt")
    with open(txt, "w") as f:
        f.write("a dog barks\n")

    def run(out, *flags):
        recs = main(["--synthetic-seed", "0", "--prompt_txt", txt, "--outdir", str(tmp_path / out), "--ddim_steps", "2",
                     "-b", CONFIG, "--W", str(FRAMES), "--loudness", "-14", *flags])
        return recs[0]["audio_path"]
    lim = _peak_ok(run("lim", "--limiter", "--limiter-lookahead-ms", "4", "--limiter-release-ms", "80"), 22050,
                   FRAMES * 512)
    _no_limiter(monkeypatch)
    plain = _peak_ok(run("plain"), 22050, FRAMES * 512)
    again = _peak_ok(run("again"), 22050, FRAMES * 512)
    assert (plain == again).all() and lim.shape == plain.shape
