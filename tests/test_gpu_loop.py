"""Seamless loops end to end on the HIP path: LCMSampler.sample_joint(ring=True), AudioLCMPipeline.generate_loop,
AudioLCMLongInfer(loop=True) and the CLI's --loop.

The reference generates one open window, so parity is against a composition of the fp32 oracle's own functions written
here (``_oracle_ring``): per LCM step the oracle's DiT on every window's frames (modular slices of the ring), its step,
the weighted mean with ``ring_weights``' table and one re-noise of the ring.  Relative L2 <= 1e-4, the split-policy
latent bar that tests/test_gpu_joint.py uses for the open plan.  What makes the result a loop is checked on the result
itself: rotating the noise rotates the latent (the open plan fails that), and the decode of the circularly padded latent
continues past the clip's end with the clip's own start."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_l2

pytestmark = pytest.mark.gpu

T, OVERLAP, S = 40, 20, 2
CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")
PLANS = {60: [0, 20, 40], 70: [0, 17, 35, 52], 40: [0, 20]}   # 70: the element path; 40: both windows cover the ring


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip
    from audiolcm_amd.pipeline import AudioLCMPipeline
    _hip.require_device(0)
    return AudioLCMPipeline.from_recipe(0, split=True)


@pytest.fixture(scope="module")
def case():
    """Shared inputs (B = 2): the context and the DiT weights of the oracle."""
    from audiolcm_amd import recipe
    return dict(ctx=recipe.synthetic_context(2), Wd=recipe.dit_state(0), seeds=[5, 6])


def _oracle_ring(Wd, ctx, x_T, noise, starts, W, overlap):
    """sample_joint(ring=True) as a loop over the oracle's dit_forward / lcm_step_scalars / lcm_step on each window's
    frames (s + j) mod L."""
    from audiolcm_amd.pipeline import ring_weights
    from oracle import alcm_oracle as O
    B, _, L = x_T.shape
    wn = torch.from_numpy(ring_weights(starts, W, L, overlap).copy())
    ts = O.lcm_timesteps(S, 50)
    ac = O.alphas_cumprod()
    w_emb = O.guidance_embedding(torch.tensor(5.0 - 1).repeat(B), 256)
    img = den = x_T
    with torch.no_grad():
        for i, t in enumerate(ts):
            tt = torch.full((B,), t, dtype=torch.long)
            sc = O.lcm_step_scalars(t, ts[i + 1] if i + 1 < len(ts) else t, ac)
            den = torch.zeros_like(img)
            for k, s in enumerate(starts):
                f = (s + torch.arange(W)) % L
                xs = img[:, :, f]
                _, dk = O.lcm_step(O.dit_forward(Wd, xs, tt, ctx, w_emb), xs, sc, None)
                den[:, :, f] += wn[k] * dk
            img = sc["sqrt_a_prev"] * den + sc["sqrt_b_prev"] * noise[i] if i + 1 < len(ts) else den
    return den


@pytest.fixture(scope="module")
def refs(case):
    """The oracle composition per ring length, computed once."""
    from audiolcm_amd import recipe
    cache = {}

    def get(L):
        if L not in cache:
            x_T, noise = recipe.prompt_noise(case["seeds"], S, 20, L)
            cache[L] = _oracle_ring(case["Wd"], case["ctx"], x_T, noise, PLANS[L], T, OVERLAP)
        return cache[L]
    return get


@pytest.fixture(scope="module")
def loop24(pipe, case):
    """One loop of 24 frames with a halo of 16, shared by the decode and the seam tests."""
    return pipe.generate_loop(case["ctx"].cuda(), case["seeds"], 24, halo_frames=16)


@pytest.mark.parametrize("L", list(PLANS), ids=["three-windows", "element-path", "one-window-long"])
def test_ring_matches_oracle(pipe, case, refs, L):
    assert pipe.loop_windows(L, T, OVERLAP) == (PLANS[L], T, OVERLAP)
    out = pipe.generate_loop(case["ctx"].cuda(), case["seeds"], L, window=T, overlap=OVERLAP)
    err = rel_l2(out["latent"].cpu().numpy(), refs(L).numpy())
    print(f"loop L={L}: latent against the oracle composition {err:.2e}")
    assert err <= 1e-4
    assert out["latent"].shape == (2, 20, L) and out["wav"].shape == (2, L * 512) and out["rate"] == 16000
    assert out["mel"].shape[0] == 2 and out["mel"].shape[-1] == 2 * L
    assert torch.isfinite(out["latent"]).all() and torch.isfinite(out["wav"]).all()


def test_rotating_the_noise_rotates_the_loop(pipe, case, refs):
    """No frame of the ring is special: with x_T and the noise rolled by 20 frames (the windows' spacing) every window
    sees the input of its neighbour, so the latent is the first one rolled by 20 up to fp32 summation order.  Each run
    is within 1e-4 of the oracle composition, for which the rotation is exact up to that order: 2e-4.  The open plan of
    ``generate_long(joint=True)`` (``long_windows``) on the same inputs has two ends and is nowhere near."""
    from audiolcm_amd import recipe
    ctx = case["ctx"].cuda()
    x_T, noise = recipe.prompt_noise(case["seeds"], S, 20, 60)
    kw = dict(S=S, conditioning=ctx, length=60, window=T, overlap=OVERLAP, seeds=case["seeds"])
    roll = lambda t: torch.roll(t, 20, dims=-1)   # noqa: E731
    a, _ = pipe.sampler.sample_joint(starts=PLANS[60], x_T=x_T, noise=noise, ring=True, **kw)
    b, _ = pipe.sampler.sample_joint(starts=PLANS[60], x_T=roll(x_T), noise=roll(noise), ring=True, **kw)
    e_ref = rel_l2(a.cpu().numpy(), refs(60).numpy())
    err = rel_l2(b.cpu().numpy(), roll(a).cpu().numpy())
    print(f"loop L=60: rolled run against the rolled latent {err:.2e} (the run against the oracle {e_ref:.2e})")
    assert e_ref <= 1e-4 and err <= 2e-4
    spans, W = pipe.long_windows(60, T, OVERLAP)
    starts = [s for s, _ in spans]
    oa, _ = pipe.sampler.sample_joint(starts=starts, x_T=x_T, noise=noise, **kw)
    ob, _ = pipe.sampler.sample_joint(starts=starts, x_T=roll(x_T), noise=roll(noise), **kw)
    open_err = rel_l2(ob.cpu().numpy(), roll(oa).cpu().numpy())
    print(f"open plan {starts} on the same inputs: {open_err:.2e}")
    assert open_err > 1e-2
    want = pipe.generate_long(ctx, case["seeds"], 60, window=T, overlap=OVERLAP, joint=True)["latent"]
    assert torch.equal(oa, want)                  # and that open run is generate_long(joint=True)'s latent


def test_circular_decode_continues_with_the_clips_start(pipe, loop24):
    """The 512 samples after the clip's end in the extended waveform and the clip's first 512 are two renderings of the
    same audio: 1e-3, the waveform parity bar (the fp32 oracle alone gives 4.3e-6 at this halo).  With a halo taken from
    the wrong ends they are unrelated (the oracle gives 0.96)."""
    L, h = 24, 16
    ext, z = loop24["ext"], loop24["latent"]
    assert ext.shape == (2, (L + 2 * h) * 512)
    a, b = h * 512, (h + L) * 512
    err = rel_l2(ext[:, b:b + 512].cpu().numpy(), ext[:, a:a + 512].cpu().numpy())
    wrong = pipe.decode(torch.cat([z[:, :, :h], z, z[:, :, L - h:]], 2).contiguous())["wav"]
    bad = rel_l2(wrong[:, b:b + 512].cpu().numpy(), wrong[:, a:a + 512].cpu().numpy())
    plain = pipe.decode(z)["wav"]
    cut = rel_l2(plain[:, :512].cpu().numpy(), ext[:, b:b + 512].cpu().numpy())
    print(f"loop L=24 h=16: continuation against the start {err:.2e}; wrong halo {bad:.2e}; plain decode's start "
          f"against the continuation {cut:.2e}")
    assert err <= 1e-3
    assert bad > 1e-1


def test_seam_close(pipe, case, loop24):
    from audiolcm_amd import kernels
    L, h, R = 24, 16, 512
    wav, ext = loop24["wav"], loop24["ext"]
    a, N = h * 512, L * 512
    assert wav.shape == (2, N)
    assert torch.equal(wav[:, R:], ext[:, a + R:a + N])          # the clip, bit for bit
    assert torch.equal(wav[:, 0], ext[:, a + N])                 # the sample that follows wav[:, N - 1] in the decode
    assert torch.equal(wav, kernels.wave_loop(ext, a, N, R))
    mel = loop24["mel"]
    assert mel.shape[-1] == 2 * L
    # for the record: the step across the wrap next to the largest step the waveform takes inside the period
    w = wav.cpu().numpy().astype(np.float64)
    wrap, steps = np.abs(w[:, 0] - w[:, -1]), np.abs(np.diff(w, axis=1)).max(1)
    print(f"loop L=24: |wav[0] - wav[N-1]| {wrap.tolist()}, largest step inside {steps.tolist()}")
    for bad in (dict(halo_frames=0), dict(halo_frames=25), dict(fade_samples=16 * 512 + 1, halo_frames=16),
                dict(fade_samples=-1)):
        with pytest.raises(ValueError):
            pipe.generate_loop(case["ctx"].cuda(), case["seeds"], L, **bad)
    with pytest.raises(ValueError, match="multiple of 5"):
        pipe.generate_loop(case["ctx"].cuda(), case["seeds"], L, out_sample_rate=44100)


def test_loop_shard_invariance(pipe):
    """Clip 1 of a B = 3 run against its own B = 1 run, at test_joint_shard_invariance's bar of 1e-6."""
    from audiolcm_amd import recipe
    ctx = recipe.synthetic_context(3).cuda()
    full = pipe.generate_loop(ctx, [0, 1, 2], 70, window=T, overlap=OVERLAP)
    part = pipe.generate_loop(ctx[1:2], [1], 70, window=T, overlap=OVERLAP)
    e_lat = rel_l2(part["latent"].cpu().numpy(), full["latent"][1:2].cpu().numpy())
    e_wav = rel_l2(part["wav"].cpu().numpy(), full["wav"][1:2].cpu().numpy())
    print(f"loop shard invariance, clip 1 of B = 3 against B = 1: latent {e_lat:.2e} wav {e_wav:.2e}")
    assert e_lat < 1e-6
    assert e_wav < 1e-6


def test_loop_is_another_sampler_than_the_open_plan(pipe, case):
    ctx = case["ctx"].cuda()
    loop = pipe.generate_loop(ctx, case["seeds"], 60, window=T, overlap=OVERLAP)["latent"]
    joint = pipe.generate_long(ctx, case["seeds"], 60, window=T, overlap=OVERLAP, joint=True)
    again = pipe.generate_long(ctx, case["seeds"], 60, window=T, overlap=OVERLAP, joint=True)
    assert torch.equal(joint["latent"], again["latent"]) and torch.equal(joint["wav"], again["wav"])
    assert rel_l2(loop.cpu().numpy(), joint["latent"].cpu().numpy()) > 1e-2


def test_loop_30s_mixed(pipe, case):
    """A 30 s loop (936 frames, six windows of 312, decoded as 1000 frames) at B = 1, mixed policy."""
    from audiolcm_amd import _hip
    ctx = case["ctx"][:1].cuda()
    pipe.set_split("mixed")
    try:
        _hip.profile_begin()
        out = pipe.generate_loop(ctx, [0], 936)
        rows = _hip.profile_end()
    finally:
        pipe.set_split(True)
    assert out["latent"].shape == (1, 20, 936) and out["wav"].shape == (1, 936 * 512)
    assert torch.isfinite(out["latent"]).all() and torch.isfinite(out["wav"]).all()
    ring = [r for r in rows if "lcm_step_ring" in r["name"]]
    assert [r["name"] for r in ring] == ["alcm::lcm_step_ring_kernel<4>"] and ring[0]["launches"] == S
    gather = [r for r in rows if "ring_gather" in r["name"]]
    assert [r["name"] for r in gather] == ["alcm::ring_gather_kernel<4>"] and gather[0]["launches"] == 1
    crop = [r for r in rows if "wave_loop" in r["name"]]
    assert [r["name"] for r in crop] == ["alcm::wave_loop_kernel<4>"] and crop[0]["launches"] == 1
    assert not [r for r in rows if "lcm_step_joint" in r["name"] or "joint_gather" in r["name"]]
    assert not [r for r in rows if "lcm_step_edit" in r["name"]]


# ------------------------------------------------------------------------------------------- the public surface
@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, infer_api
    _hip.require_device(0)
    return infer_api._build(CONFIG, None, None, 0, True)


@pytest.fixture()
def api(built, monkeypatch):
    """Both front ends on one model build."""
    from audiolcm_amd import cli, infer_api
    monkeypatch.setattr(infer_api, "_build", lambda *a, **k: built)
    monkeypatch.setattr(cli, "build_models", lambda *a, **k: (built[0], built[2]))
    return infer_api


def _cond(model, prompt):
    from audiolcm_amd.infer_api import struct_caption
    return model.get_learned_conditioning({"ori_caption": [prompt], "struct_caption": [struct_caption(prompt)]})


@pytest.mark.parametrize("rate", [48000, 44100])
def test_loop_at_an_output_rate(api, tmp_path, rate):
    """A 1 s request: 32 frames at 48 kHz and 35 at 44.1 kHz, where a frame is 1411.2 samples; the file holds exactly
    the period, under the rate, at the target loudness (tests/test_gpu_loudness_api.py's bar and its float64 meter)."""
    from test_gpu_loudness_api import _check_level
    from audiolcm_amd.audio_in import loop_frames
    L = loop_frames(1.0, rate)
    assert L == {48000: 32, 44100: 35}[rate]
    path = api.AudioLCMLongInfer("rain falls on a tin roof", duration_s=1.0, config_path=CONFIG, synthetic_seed=0,
                                 outpath=str(tmp_path / "loop"), seed=3, out_sample_rate=rate, loop=True,
                                 loudness=-20.0, peak_dbfs=-2.0)
    assert (L * 512 * rate) % 16000 == 0
    _check_level(path, rate, L * 512 * rate // 16000, -20.0, -2.0)


def test_api_and_cli_loop(api, built, tmp_path):
    from audiolcm_amd.cli import main
    from audiolcm_amd.pipeline import AudioLCMPipeline
    from audiolcm_amd.wavio import read_wav, write_pcm16
    model, _, vocoder, orig_steps = built
    prompt = "a dog barks"
    kw = dict(duration_s=3.0, config_path=CONFIG, synthetic_seed=0, seed=3)
    path = api.AudioLCMLongInfer(prompt, outpath=str(tmp_path / "a"), loop=True, **kw)
    assert path == os.path.join(str(tmp_path / "a"), "a-dog-barks_0.wav")
    w, sr = read_wav(path)
    assert sr == 16000 and w.shape == (94 * 512,) and np.abs(w).max() > 0     # ceil(3 * 16000 / 512) = 94 frames
    # without the flag: the bytes of generate_long, as before
    plain = api.AudioLCMLongInfer(prompt, outpath=str(tmp_path / "b"), **kw)
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                            latent_shape=(model.mel_dim, model.mel_length))
    with torch.no_grad():
        want = pipe.generate_long(_cond(model, prompt), [3], 94)["wav"][0].cpu().numpy()
    write_pcm16(str(tmp_path / "want_api.wav"), want, 16000)
    with open(plain, "rb") as f, open(str(tmp_path / "want_api.wav"), "rb") as g:
        got = f.read()
        assert got == g.read()
    with open(path, "rb") as f:
        assert f.read() != got                                               # and the flag changes them

    txt = str(tmp_path / "p.txt")
    with open(txt, "w") as f:
        f.write(prompt + "\n")
    args = ["--duration", "3", "--W", "40", "--synthetic-seed", "0", "--prompt_txt", txt, "--ddim_steps", "2",
            "--sample_rate", "16000", "-b", CONFIG]
    recs = main(args + ["--loop", "--outdir", str(tmp_path / "c")])
    assert [r["audio_path"] for r in recs] == [os.path.join(str(tmp_path / "c"), "a-dog-barks_0.wav")]
    x, sr = read_wav(recs[0]["audio_path"])
    assert sr == 16000 and x.shape == (94 * 512,) and np.abs(x).max() > 0
    again = main(args + ["--loop", "--long-joint", "--outdir", str(tmp_path / "d")])   # accepted and redundant
    with open(recs[0]["audio_path"], "rb") as f, open(again[0]["audio_path"], "rb") as g:
        looped = f.read()
        assert looped == g.read()
    recs = main(args + ["--outdir", str(tmp_path / "e")])
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, guidance_scale=5.0, latent_shape=(20, 40),
                            original_inference_steps=orig_steps)
    with torch.no_grad():
        want = pipe.generate_long(_cond(model, prompt), [0], 94)["wav"][0].cpu().numpy()
    write_pcm16(str(tmp_path / "want_cli.wav"), want, 16000)
    with open(recs[0]["audio_path"], "rb") as f, open(str(tmp_path / "want_cli.wav"), "rb") as g:
        got = f.read()
        assert got == g.read()
    assert got != looped
    # --sample_rate still only labels the 16 kHz samples
    recs = main(args[:-4] + ["--sample_rate", "22050", "-b", CONFIG, "--loop", "--outdir", str(tmp_path / "f")])
    with open(recs[0]["audio_path"], "rb") as f:
        labelled = f.read()
    assert len(labelled) == len(looped) and labelled[44:] == looped[44:]
    assert int.from_bytes(labelled[24:28], "little") == 22050
