"""Inpainting at any clip length with the input kept outside the spans, end to end on the HIP path:
AudioLCMPipeline.edit_long (windowed edit, region decode, kernels.wave_paste), AudioLCMEditInfer(keep_original=True)
and the CLI's --keep-original.

The windows are compared bit for bit with LCMSampler.sample_edit calls made by hand on the documented windows and
seeds; the regenerated frames with the composition of the fp32 oracle's own functions (``_oracle_edit``, restated from
test_gpu_edit.py) at relative L2 <= 1e-4, the split-policy latent bar; kept latent frames and kept
samples are exact."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, golden, rel_l2

pytestmark = pytest.mark.gpu

L, W, OV = 100, 40, 20
FS = 512
STRENGTH_TS = {(2, 0.5): [499, 259]}  # scheduling_lcm.py:171 at strength 0.5
SEEDS = [5, 6]


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
    """Shared inputs (B = 2, L = 100): context, a known latent, the DiT weights of the oracle, and the mel_B2.npz
    waveform tiled to 100 latent frames."""
    from audiolcm_amd import recipe
    wav = np.tile(golden("mel_B2.npz")["wav"], (1, 3))[:, :L * FS]
    return dict(ctx=recipe.synthetic_context(2), Wd=recipe.dit_state(0), wav=torch.from_numpy(wav.copy()),
                z0=torch.randn((2, 20, L), generator=torch.Generator().manual_seed(79)))


def _span(lo, hi, rows=(0, 1)):
    m = torch.zeros((2, L))
    for b in rows:
        m[b, lo:hi + 1] = 1.0
    return m


def _oracle_edit(Wd, ctx, z0, n0, noise, S, strength, mask):
    """sample_edit as a loop over the oracle's dit_forward / lcm_step_scalars / lcm_step: start from the noised latent
    and after every step blend the denoised estimate with z0 (test_gpu_edit.py, strength < 1 with a mask)."""
    from oracle import alcm_oracle as O
    B = z0.shape[0]
    ts = STRENGTH_TS[(S, strength)]
    ac = O.alphas_cumprod()
    w_emb = O.guidance_embedding(torch.tensor(5.0 - 1).repeat(B), 256)
    m = mask[:, None, :]
    sc0 = O.lcm_step_scalars(ts[0], ts[0], ac)
    img = sc0["sqrt_a"] * z0 + sc0["sqrt_b"] * n0
    den = img
    with torch.no_grad():
        for i, t in enumerate(ts):
            eps = O.dit_forward(Wd, img, torch.full((B,), t, dtype=torch.long), ctx, w_emb)
            sc = O.lcm_step_scalars(t, ts[i + 1] if i + 1 < len(ts) else t, ac)
            _, den = O.lcm_step(eps, img, sc, None)
            den = m * den + (1 - m) * z0
            img = sc["sqrt_a_prev"] * den + sc["sqrt_b_prev"] * noise[i] if i + 1 < len(ts) else den
    return den


def _by_hand(pipe, ctx, z_in, mask, starts, seeds=SEEDS):
    """The documented loop: window k is one sample_edit call on [s, s + W) with the mask still to do."""
    from audiolcm_amd import recipe
    z, m = z_in.clone(), mask.clone()
    for k, s in enumerate(starts):
        zk, _ = pipe.sampler.sample_edit(S=2, conditioning=ctx, init=z[:, :, s:s + W].contiguous(), mask=m[:, s:s + W],
                                         strength=0.5, seeds=[recipe.window_seed(sd, k) for sd in seeds])
        z[:, :, s:s + W] = zk
        m[:, s:s + W] = 0.0
    return z


def test_one_window_is_edit(pipe, case):
    ctx, z40 = case["ctx"].cuda(), case["z0"][:, :, :W].cuda()
    for mask in (_span(10, 25)[:, :W], None):
        a = pipe.edit_long(ctx, SEEDS, latent=z40, mask=mask, window=W, overlap=OV)
        b = pipe.edit(ctx, SEEDS, latent=z40, mask=mask)
        assert all(torch.equal(a[k], b[k]) for k in ("latent", "mel", "wav"))
        assert not torch.equal(a["latent"], z40)


def test_span_inside_one_window(pipe, case):
    from audiolcm_amd import recipe
    ctx, z0, mask = case["ctx"].cuda(), case["z0"].cuda(), _span(50, 54)
    out = pipe.edit_long(ctx, SEEDS, latent=z0, mask=mask, window=W, overlap=OV)
    assert out["latent"].shape == (2, 20, L) and out["wav"].shape == (2, L * FS) and out["mel"].shape == (2, 80, 2 * L)
    assert torch.equal(out["latent"], _by_hand(pipe, ctx, z0, mask, [30]))
    keep = mask[0] == 0
    assert torch.equal(out["latent"][:, :, keep], z0[:, :, keep])
    n0, noise, _ = recipe.edit_noise(SEEDS, 2, 20, W)       # window 0 has the prompts' own seeds
    ref = _oracle_edit(case["Wd"], case["ctx"], case["z0"][:, :, 30:70], n0, noise, 2, 0.5, mask[:, 30:70])
    got = out["latent"][:, :, 50:55].cpu()
    err = rel_l2(got.numpy(), ref[:, :, 20:25].numpy())
    print(f"edit_long span 50..54: {err:.2e}")
    assert err <= 1e-4
    assert rel_l2(got.numpy(), case["z0"][:, :, 50:55].numpy()) > 1e-2    # regenerated, not the input


def test_span_longer_than_a_window(pipe, case):
    ctx, z0, mask = case["ctx"].cuda(), case["z0"].cuda(), _span(30, 89)
    out = pipe.edit_long(ctx, SEEDS, latent=z0, mask=mask, window=W, overlap=OV)
    assert torch.equal(out["latent"], _by_hand(pipe, ctx, z0, mask, [10, 30, 50]))
    keep = mask[0] == 0
    assert torch.equal(out["latent"][:, :, keep], z0[:, :, keep])
    assert torch.isfinite(out["wav"]).all()


def test_shard_invariance(pipe, case):
    ctx, z0, mask = case["ctx"].cuda(), case["z0"].cuda(), _span(30, 89)
    full = pipe.edit_long(ctx, SEEDS, latent=z0, mask=mask, window=W, overlap=OV)
    part = pipe.edit_long(ctx[1:2], SEEDS[1:2], latent=z0[1:2], mask=mask[1:2], window=W, overlap=OV)
    assert rel_l2(part["latent"].cpu().numpy(), full["latent"][1:2].cpu().numpy()) < 1e-6
    assert rel_l2(part["wav"].cpu().numpy(), full["wav"][1:2].cpu().numpy()) < 1e-6


def test_empty_mask_returns_the_input_without_a_dit_call(pipe, case, monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("an empty mask must not reach the sampler")
    monkeypatch.setattr(pipe.sampler, "sample_edit", no_call)
    z0 = case["z0"].cuda()
    out = pipe.edit_long(case["ctx"].cuda(), SEEDS, latent=z0, mask=torch.zeros((2, L)), window=W, overlap=OV)
    assert torch.equal(out["latent"], z0) and out["wav"].shape == (2, L * FS)
    kept = pipe.edit_long(case["ctx"].cuda(), SEEDS, wav=case["wav"], mask=torch.zeros((2, L)), window=W, overlap=OV,
                          keep_original=True, halo_frames=8)
    assert torch.equal(kept["wav"].cpu(), case["wav"]) and kept["regions"] == []


def test_edit_long_argument_errors(pipe, case):
    ctx, z0 = case["ctx"].cuda(), case["z0"].cuda()
    with pytest.raises(ValueError):
        pipe.edit_long(ctx, SEEDS)
    with pytest.raises(ValueError):
        pipe.edit_long(ctx, SEEDS, wav=case["wav"], latent=z0)
    with pytest.raises(ValueError, match="keep_original"):
        pipe.edit_long(ctx, SEEDS, latent=z0, mask=_span(50, 54), keep_original=True)
    with pytest.raises(ValueError, match="halo_frames"):
        pipe.edit_long(ctx, SEEDS, wav=case["wav"], mask=_span(50, 54), window=W, overlap=OV, keep_original=True,
                       halo_frames=0, fade_samples=512)
    with pytest.raises(ValueError, match="mask"):
        pipe.edit_long(ctx, SEEDS, latent=z0, mask=torch.zeros((2, L + 1)))


# ---------------------------------------------------------------------------- keep_original from a waveform
def _z_in(pipe, wav, seeds):
    """The scaled posterior sample of the whole clip, as edit_long documents it."""
    from audiolcm_amd import kernels, recipe
    from audiolcm_amd.mel import MelNet
    post = pipe.model.encode_first_stage(MelNet()(wav))
    e0 = recipe.edit_noise(seeds, 2, 20, L)[2].cuda()
    return kernels.latent_init(None, moments=post.parameters.float().contiguous(), e0=e0,
                               scale=float(pipe.model.scale_factor), want_x=False)[0]


@pytest.fixture(scope="module")
def kept(pipe, case):
    """One keep-original edit shared by the tests below: clip 0 regenerates frames 50..54, clip 1 nothing."""
    mask = _span(50, 54, rows=(0,))
    out = pipe.edit_long(case["ctx"].cuda(), SEEDS, wav=case["wav"], mask=mask, window=W, overlap=OV,
                         keep_original=True, halo_frames=8, fade_samples=512)
    return mask, out


def test_keep_original_keeps_the_input_outside_the_fade(pipe, case, kept):
    mask, out = kept
    wav, got = case["wav"], out["wav"].cpu()
    assert got.shape == wav.shape and out["regions"] == [(42, 63)] and set(out) == {"latent", "wav", "regions"}
    lo, hi, R = 50 * FS, 55 * FS, 512
    assert torch.equal(got[0, :lo - R + 1], wav[0, :lo - R + 1]) and torch.equal(got[0, hi + R - 1:], wav[0, hi + R - 1:])
    # inside the span: the region's own decode, bit for bit
    gen = pipe.decode(out["latent"][:, :, 42:63].contiguous())["wav"].cpu()
    assert torch.equal(got[0, lo:hi], gen[0, (50 - 42) * FS:(55 - 42) * FS])
    assert not torch.equal(got[0, lo:hi], wav[0, lo:hi])
    # the fades lie between the two, within the blend's 1e-6 of the definition
    from audiolcm_amd.kernels import paste_ramp_host
    ramp = paste_ramp_host(R).double()
    d = torch.arange(1, R)
    for sl, g in ((slice(hi, hi + R - 1), ramp[d]), (slice(lo - R + 1, lo), ramp[d].flip(0))):
        o, n = wav[0, sl].double(), gen[0, sl.start - 42 * FS:sl.stop - 42 * FS].double()
        assert (got[0, sl].double() - (o + g * (n - o))).abs().max() <= 1e-6


def test_clip_with_an_empty_mask_comes_back_exact(pipe, case, kept):
    mask, out = kept
    z_in = _z_in(pipe, case["wav"], SEEDS)
    assert torch.equal(out["wav"][1].cpu(), case["wav"][1])
    assert torch.equal(out["latent"][1], z_in[1])
    keep = mask[0] == 0
    assert torch.equal(out["latent"][0][:, keep], z_in[0][:, keep])
    assert not torch.equal(out["latent"][0][:, ~keep], z_in[0][:, ~keep])
    # and the window that was run is the documented one on the documented latent
    assert torch.equal(out["latent"], _by_hand(pipe, case["ctx"].cuda(), z_in, mask, [30]))


# ---------------------------------------------------------------------------- the Infer function and the CLI
SPAN = (8000, 16000)    # 0.5 - 1.0 s
FADE = 512              # 32 ms


def _noise_wav(path):
    """1.5 s of full-range PCM16 noise (values at and beyond +-16384, where a 32767 writer would be one step off)."""
    from audiolcm_amd.wavio import read_pcm16, write_pcm16
    pcm = np.random.default_rng(3).integers(-32768, 32768, 24000).astype("<i2")
    write_pcm16(path, pcm.astype(np.float32) / np.float32(32768.0), 16000, scale=32768.0)
    assert np.array_equal(read_pcm16(path)[0], pcm)
    return pcm


def _check_kept_file(path, pcm):
    from audiolcm_amd.wavio import read_pcm16
    got, sr = read_pcm16(path)
    assert sr == 16000 and got.shape == (24000,)
    lo, hi = SPAN[0] - FADE, SPAN[1] + FADE
    assert np.array_equal(got[:lo], pcm[:lo]) and np.array_equal(got[hi:], pcm[hi:])
    assert not np.array_equal(got[SPAN[0]:SPAN[1]], pcm[SPAN[0]:SPAN[1]])


def _infer(tmp_path, **kw):
    from audiolcm_amd.infer_api import AudioLCMEditInfer
    src = str(tmp_path / "in.wav")
    pcm = _noise_wav(src)
    path = AudioLCMEditInfer("a dog barks", src, strength=0.5, mask_spans=[(0.5, 1.0)], synthetic_seed=0, seed=3,
                             config_path=os.path.join(REPO, "configs", "audiolcm.yaml"),
                             outpath=str(tmp_path / "edit"), **kw)
    assert path == os.path.join(str(tmp_path / "edit"), "a-dog-barks_0.wav")
    return path, pcm


def test_edit_infer_keep_original(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check_kept_file(*_infer(tmp_path, keep_original=True))


def test_edit_infer_default_is_unchanged(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.wavio import read_wav
    x, sr = read_wav(_infer(tmp_path)[0])
    assert sr == 16000 and x.shape == (47 * 512,) and np.abs(x).max() > 0


def _cli(tmp_path, *flags):
    from audiolcm_amd.cli import main
    src, txt, out = str(tmp_path / "in.wav"), str(tmp_path / "p.txt"), str(tmp_path / "out")
    pcm = _noise_wav(src)
    with open(txt, "w") as f:
        f.write("a dog barks\n")
    recs = main(["--init-audio", src, "--inpaint", "--mask-spans", "0.5-1.0", "--synthetic-seed", "0", "--prompt_txt",
                 txt, "--outdir", out, "--ddim_steps", "2", "--sample_rate", "16000", "-b",
                 os.path.join(REPO, "configs", "audiolcm.yaml"), *flags])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")] and set(recs[0]) == {
        "caption", "audio_path"}
    return recs[0]["audio_path"], pcm


def test_cli_keep_original(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check_kept_file(*_cli(tmp_path, "--keep-original"))


def test_cli_default_is_unchanged(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.wavio import read_wav
    x, sr = read_wav(_cli(tmp_path)[0])
    assert sr == 16000 and x.shape == (47 * 512,) and np.abs(x).max() > 0
