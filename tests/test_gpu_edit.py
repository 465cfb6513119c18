"""Audio-conditioned generation end to end on the HIP path: variation, text-guided inpainting and long-form
continuation (LCMSampler.sample_edit, AudioLCMPipeline.edit / generate_long, the two Infer functions and the CLI).

The reference has no LCM edit path, so parity is against compositions of the fp32 oracle's own functions written here
(``_oracle_edit``): relative L2 <= 1e-4, the split-policy latent bar, over the regenerated frames; kept
frames, the mask-1 and mask-0 limits and the first long-form window are exact."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, golden, rel_l2

pytestmark = pytest.mark.gpu

T = 40
STRENGTH_TS = {(2, 0.5): [499, 259], (4, 0.5): [499, 379, 259, 139]}  # scheduling_lcm.py:171 at strength 0.5


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip
    from audiolcm_amd.pipeline import AudioLCMPipeline
    _hip.require_device(0)
    return AudioLCMPipeline.from_recipe(0, split=True, encoder=True)


@pytest.fixture(scope="module")
def case():
    """Shared inputs (B = 2, T = 40): context, a known latent, and the DiT weights of the oracle."""
    from audiolcm_amd import recipe
    ctx = recipe.synthetic_context(2)
    z0 = torch.randn((2, 20, T), generator=torch.Generator().manual_seed(77))
    mask = torch.zeros((2, T))
    mask[:, 10:26] = 1.0   # regenerate frames 10..25
    return dict(ctx=ctx, z0=z0, mask=mask, Wd=recipe.dit_state(0))


def _oracle_edit(Wd, ctx, z0, n0, noise, S, strength, mask=None, uc=None, cfg_scale=1.0):
    """sample_edit as a loop over the oracle's dit_forward / lcm_step_scalars / lcm_step: start from the noised latent
    (regenerated frames from pure noise at strength 1), and after every step blend the denoised estimate with z0."""
    from oracle import alcm_oracle as O
    B = z0.shape[0]
    ts = O.lcm_timesteps(S, 50) if strength == 1.0 else STRENGTH_TS[(S, strength)]
    ac = O.alphas_cumprod()
    w_emb = O.guidance_embedding(torch.tensor(5.0 - 1).repeat(B), 256)
    m = torch.ones((B, 1, z0.shape[2])) if mask is None else mask[:, None, :]
    sc0 = O.lcm_step_scalars(ts[0], ts[0], ac)
    keep = sc0["sqrt_a"] * z0 + sc0["sqrt_b"] * n0
    regen = keep if strength < 1.0 else n0
    img = m * regen + (1 - m) * keep
    den = img
    with torch.no_grad():
        for i, t in enumerate(ts):
            tt = torch.full((B,), t, dtype=torch.long)
            eps = O.dit_forward(Wd, img, tt, ctx, w_emb)
            if uc is not None:
                eps = O.cfg_combine(O.dit_forward(Wd, img, tt, uc, w_emb), eps, cfg_scale)
            sc = O.lcm_step_scalars(t, ts[i + 1] if i + 1 < len(ts) else t, ac)
            _, den = O.lcm_step(eps, img, sc, None)
            den = m * den + (1 - m) * z0
            img = sc["sqrt_a_prev"] * den + sc["sqrt_b_prev"] * noise[i] if i + 1 < len(ts) else den
    return den


@pytest.mark.parametrize("S", [2, 4])
def test_variation_matches_oracle(pipe, case, S):
    from audiolcm_amd import recipe
    seeds = [5, 6]
    z, last = pipe.sampler.sample_edit(S=S, conditioning=case["ctx"].cuda(), init=case["z0"].cuda(), strength=0.5,
                                       seeds=seeds)
    assert pipe.sampler.timesteps.tolist() == STRENGTH_TS[(S, 0.5)] and torch.equal(z, last)
    n0, noise, _ = recipe.edit_noise(seeds, S, 20, T)
    ref = _oracle_edit(case["Wd"], case["ctx"], case["z0"], n0, noise, S, 0.5)
    err = rel_l2(z.cpu().numpy(), ref.numpy())
    print(f"variation S={S}: {err:.2e}")
    assert err <= 1e-4
    assert rel_l2(z.cpu().numpy(), case["z0"].numpy()) > 1e-2   # it is a variation, not the input


@pytest.mark.parametrize("strength,cfg", [(1.0, False), (0.5, False), (1.0, True)])
def test_inpainting_matches_oracle(pipe, case, strength, cfg):
    from audiolcm_amd import recipe
    seeds, S = [8, 9], 2
    uc = torch.zeros_like(case["ctx"]) if cfg else None
    z, _ = pipe.sampler.sample_edit(S=S, conditioning=case["ctx"].cuda(), init=case["z0"].cuda(),
                                    mask=case["mask"], strength=strength, seeds=seeds,
                                    unconditional_conditioning=uc.cuda() if cfg else None,
                                    unconditional_guidance_scale=3.0 if cfg else 1.0)
    n0, noise, _ = recipe.edit_noise(seeds, S, 20, T)
    ref = _oracle_edit(case["Wd"], case["ctx"], case["z0"], n0, noise, S, strength, case["mask"], uc, 3.0)
    z = z.cpu()
    regen = case["mask"][0] == 1
    err = rel_l2(z[:, :, regen].numpy(), ref[:, :, regen].numpy())
    print(f"inpaint strength={strength} cfg={cfg}: {err:.2e}")
    assert err <= 1e-4
    assert torch.equal(z[:, :, ~regen], case["z0"][:, :, ~regen])
    assert rel_l2(z[:, :, regen].numpy(), case["z0"][:, :, regen].numpy()) > 1e-2


def test_mask_one_strength_one_is_plain_sampling(pipe, case):
    seeds = [5, 6]
    ctx = case["ctx"].cuda()
    want, want_last = pipe.sampler.sample(S=2, batch_size=2, shape=(20, T), conditioning=ctx, seeds=seeds, verbose=False)
    for mask in (torch.ones((2, T)), None):
        z, last = pipe.sampler.sample_edit(S=2, conditioning=ctx, init=case["z0"].cuda(), mask=mask, strength=1.0,
                                           seeds=seeds)
        assert torch.equal(z, want) and torch.equal(last, want_last)


def test_mask_zero_returns_the_input(pipe, case):
    z0 = case["z0"].cuda()
    z, _ = pipe.sampler.sample_edit(S=2, conditioning=case["ctx"].cuda(), init=z0, mask=torch.zeros((2, T)),
                                    strength=0.5, seeds=[1, 2])
    assert torch.equal(z, z0)


def test_mask_zero_from_waveform_is_the_reconstruction(pipe, case):
    from audiolcm_amd.mel import MelNet
    wav = torch.from_numpy(golden("mel_B2.npz")["wav"])
    out = pipe.edit(case["ctx"].cuda(), [1, 2], wav=wav, mask=0, sample_posterior=False)
    post = pipe.model.encode_first_stage(MelNet()(wav))
    zm = pipe.model.scale_factor * post.mode()
    assert out["latent"].shape == (2, 20, 48) and torch.equal(out["latent"], zm)
    assert torch.equal(out["wav"], pipe.vocoder(pipe.model.decode_first_stage(zm)).squeeze(1))


def test_edit_from_waveform(pipe, case):
    wav = torch.from_numpy(golden("mel_B2.npz")["wav"])
    ctx = case["ctx"].cuda()
    a = pipe.edit(ctx, [1, 2], wav=wav, strength=0.5)
    assert a["latent"].shape == (2, 20, 48) and a["mel"].shape == (2, 80, 96) and a["wav"].shape == (2, 96 * 256)
    assert all(torch.isfinite(a[k]).all() for k in ("latent", "mel", "wav"))
    b = pipe.edit(ctx, [1, 2], wav=wav, strength=0.5)
    assert torch.equal(a["latent"], b["latent"]) and torch.equal(a["wav"], b["wav"])
    c = pipe.edit(ctx, [3, 4], wav=wav, strength=0.5)
    assert not torch.equal(a["latent"], c["latent"])
    with pytest.raises(ValueError):
        pipe.edit(ctx, [1, 2])
    with pytest.raises(ValueError):
        pipe.edit(ctx, [1, 2], wav=wav, latent=a["latent"])


def test_edit_shard_invariance(pipe, case):
    from audiolcm_amd import recipe
    ctx = recipe.synthetic_context(3).cuda()
    z0 = torch.randn((3, 20, T), generator=torch.Generator().manual_seed(78)).cuda()
    mask = case["mask"][:1].repeat(3, 1)
    full = pipe.edit(ctx, [0, 1, 2], latent=z0, mask=mask, strength=0.5)
    part = pipe.edit(ctx[1:2], [1], latent=z0[1:2], mask=mask[1:2], strength=0.5)
    assert rel_l2(part["latent"].cpu().numpy(), full["latent"][1:2].cpu().numpy()) < 1e-6
    assert rel_l2(part["wav"].cpu().numpy(), full["wav"][1:2].cpu().numpy()) < 1e-6


def test_sample_edit_argument_errors(pipe, case):
    ctx, z0 = case["ctx"].cuda(), case["z0"].cuda()
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="strength"):
            pipe.sampler.sample_edit(S=2, conditioning=ctx, init=z0, strength=bad, seeds=[0, 1])
    with pytest.raises(ValueError, match="original_steps x strength"):
        pipe.sampler.sample_edit(S=2, conditioning=ctx, init=z0, strength=0.02, seeds=[0, 1])
    for shape in ((2, T + 1), (1, T), (2, 20, T)):
        with pytest.raises(ValueError, match="mask"):
            pipe.sampler.sample_edit(S=2, conditioning=ctx, init=z0, mask=torch.zeros(shape), seeds=[0, 1])
    with pytest.raises(ValueError, match="845"):
        pipe.sampler.sample_edit(S=2, conditioning=ctx[:1], init=torch.zeros((1, 20, 846), device="cuda"), seeds=[0])


def test_long_form_small(pipe, case):
    from audiolcm_amd import recipe
    seeds = [5, 6]
    ctx = case["ctx"].cuda()
    out = pipe.generate_long(ctx, seeds, latent_len=60, window=40, overlap=20)
    assert out["latent"].shape == (2, 20, 60) and out["wav"].shape == (2, 60 * 512) and torch.isfinite(out["wav"]).all()
    plain, _ = pipe.sampler.sample(S=2, batch_size=2, shape=(20, 40), conditioning=ctx, seeds=seeds, verbose=False)
    assert torch.equal(out["latent"][:, :, :40], plain)
    # window 1 by hand: the previous 20 frames known, 20 new ones, the documented seeds
    init = torch.cat([plain[:, :, 20:], torch.zeros((2, 20, 20), device="cuda")], 2)
    mask = torch.cat([torch.zeros((2, 20)), torch.ones((2, 20))], 1)
    wseeds = [recipe.window_seed(s, 1) for s in seeds]
    z1, _ = pipe.sampler.sample_edit(S=2, conditioning=ctx, init=init, mask=mask, strength=1.0, seeds=wseeds)
    assert torch.equal(out["latent"][:, :, 40:], z1[:, :, 20:])
    n0, noise, _ = recipe.edit_noise(wseeds, 2, 20, 40)
    ref = _oracle_edit(case["Wd"], case["ctx"], init.cpu(), n0, noise, 2, 1.0, mask)
    err = rel_l2(out["latent"][:, :, 40:].cpu().numpy(), ref[:, :, 20:].numpy())
    print(f"long-form window 1: {err:.2e}")
    assert err <= 1e-4
    # the stride does not divide: the last window is shifted to end at 70
    odd = pipe.generate_long(ctx, seeds, latent_len=70, window=40, overlap=20)
    assert odd["latent"].shape == (2, 20, 70) and odd["wav"].shape == (2, 70 * 512)
    assert torch.isfinite(odd["latent"]).all() and torch.isfinite(odd["wav"]).all()
    assert torch.equal(odd["latent"][:, :, :60], out["latent"])


def test_long_form_30s_mixed(pipe, case):
    """A 30 s clip (936 latent frames = 312 + 4 x 156) out of the 10 s model, mixed policy."""
    ctx = case["ctx"][:1].cuda()
    pipe.set_split("mixed")
    try:
        out = pipe.generate_long(ctx, [0], latent_len=936)
        plain = pipe.generate(ctx, seeds=[0])["latent"]
    finally:
        pipe.set_split(True)
    assert out["latent"].shape == (1, 20, 936) and out["wav"].shape == (1, 936 * 512)
    assert torch.isfinite(out["latent"]).all() and torch.isfinite(out["wav"]).all()
    assert torch.equal(out["latent"][:, :, :312], plain)


def _sine_wav(path, seconds):
    from audiolcm_amd.wavio import write_pcm16
    t = np.arange(int(16000 * seconds), dtype=np.float32) / 16000.0
    write_pcm16(path, 0.3 * np.sin(2 * np.pi * 440.0 * t), 16000)


@pytest.mark.parametrize("spans", [None, [(0.5, 1.0)]], ids=["variation", "inpaint"])
def test_edit_infer_api(tmp_path, spans):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.infer_api import AudioLCMEditInfer
    from audiolcm_amd.wavio import read_wav
    cfg = os.path.join(REPO, "configs", "audiolcm.yaml")
    src = str(tmp_path / "in.wav")
    _sine_wav(src, 1.5)   # 24000 samples: padded to 47 latent frames
    path = AudioLCMEditInfer("a dog barks", src, strength=0.5, mask_spans=spans, config_path=cfg, synthetic_seed=0,
                             outpath=str(tmp_path / "edit"), seed=3)
    assert path == os.path.join(str(tmp_path / "edit"), "a-dog-barks_0.wav")
    x, sr = read_wav(path)
    assert sr == 16000 and x.shape == (47 * 512,) and np.abs(x).max() > 0
    with open(src, "r+b") as f:   # the same file claiming 22.05 kHz: refused before any model is built
        f.seek(24)
        f.write((22050).to_bytes(4, "little"))
    with pytest.raises(ValueError, match="sample rate"):
        AudioLCMEditInfer("a dog barks", src, config_path=cfg, synthetic_seed=0, outpath=str(tmp_path / "bad"))


def test_long_infer_api(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.infer_api import AudioLCMLongInfer
    from audiolcm_amd.wavio import read_wav
    path = AudioLCMLongInfer("rain falls on a tin roof", duration_s=12.0,
                             config_path=os.path.join(REPO, "configs", "audiolcm.yaml"), synthetic_seed=0,
                             outpath=str(tmp_path / "long"), seed=3)
    assert path == os.path.join(str(tmp_path / "long"), "rain-falls-on-a-tin-roof_0.wav")
    w, sr = read_wav(path)
    assert sr == 16000 and w.shape == (12 * 16000,) and np.abs(w).max() > 0


def test_cli_inpaint(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.cli import main
    from audiolcm_amd.wavio import read_wav
    src, txt, out = str(tmp_path / "in.wav"), str(tmp_path / "p.txt"), str(tmp_path / "out")
    _sine_wav(src, 1.5)
    with open(txt, "w") as f:
        f.write("a dog barks\n")
    recs = main(["--init-audio", src, "--inpaint", "--mask-spans", "0.5-1.0", "--synthetic-seed", "0",
                 "--prompt_txt", txt, "--outdir", out, "--ddim_steps", "2", "--sample_rate", "16000",
                 "-b", os.path.join(REPO, "configs", "audiolcm.yaml")])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")]
    x, sr = read_wav(recs[0]["audio_path"])
    assert sr == 16000 and x.shape == (47 * 512,) and np.abs(x).max() > 0
