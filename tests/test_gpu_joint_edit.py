"""Joint denoising from a recording end to end on the HIP path: LCMSampler.sample_joint(init=...),
AudioLCMPipeline.edit_long(joint=True) and extend, AudioLCMEditInfer(joint=..., extend_s=...) and the CLI's
--long-joint --init-audio and --extend.

The reference has neither an edit path nor a joint one, so parity is against a composition of the fp32 oracle's own
functions written here (``_oracle_joint_edit``): the start of ``sample_edit`` on the long latent, and per LCM step the
oracle's DiT on every window's slice, its step, the weighted mean with ``joint_weights``' table, the mask blend with z0
and one re-noise of the long latent.  Relative L2 <= 1e-4, the split-policy latent bar that the joint and
the chained tests use; one window is ``sample_edit`` bit for bit, and kept frames and kept samples are exact."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_l2

pytestmark = pytest.mark.gpu

T, OVERLAP, S = 40, 20, 2
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
    """Shared inputs (B = 2): the context, the DiT weights of the oracle and a known latent of 100 frames."""
    from audiolcm_amd import recipe
    return dict(ctx=recipe.synthetic_context(2), Wd=recipe.dit_state(0),
                z0=torch.randn((2, 20, 100), generator=torch.Generator().manual_seed(81)))


def _starts(L):
    from audiolcm_amd.pipeline import _long_windows
    spans, W = _long_windows(L, T, OVERLAP)
    return [s for s, _ in spans], W


def _oracle_joint_edit(Wd, ctx, z0, mask, seeds, strength, uc=None, cfg_scale=1.0):
    """sample_joint(init=z0, mask=mask) as a loop over the oracle's dit_forward / lcm_step_scalars / lcm_step on each
    window's slice, with the draws of recipe.edit_noise at the latent's whole length."""
    from audiolcm_amd import recipe
    from audiolcm_amd.pipeline import joint_weights
    from oracle import alcm_oracle as O
    B, _, L = z0.shape
    starts, W = _starts(L)
    wn = torch.from_numpy(joint_weights(starts, W, L, OVERLAP).copy())
    n0, noise, _ = recipe.edit_noise(seeds, S, 20, L)
    ts = O.lcm_timesteps(S, 50) if strength == 1.0 else STRENGTH_TS[(S, strength)]
    ac = O.alphas_cumprod()
    w_emb = O.guidance_embedding(torch.tensor(5.0 - 1).repeat(B), 256)
    m = torch.ones((B, 1, L)) if mask is None else mask[:, None, :]
    sc0 = O.lcm_step_scalars(ts[0], ts[0], ac)
    keep = sc0["sqrt_a"] * z0 + sc0["sqrt_b"] * n0
    regen = keep if strength < 1.0 else n0
    img = m * regen + (1 - m) * keep
    den = img
    with torch.no_grad():
        for i, t in enumerate(ts):
            tt = torch.full((B,), t, dtype=torch.long)
            sc = O.lcm_step_scalars(t, ts[i + 1] if i + 1 < len(ts) else t, ac)
            den = torch.zeros_like(img)
            for k, s in enumerate(starts):
                xs = img[:, :, s:s + W]
                eps = O.dit_forward(Wd, xs, tt, ctx, w_emb)
                if uc is not None:
                    eps = O.cfg_combine(O.dit_forward(Wd, xs, tt, uc, w_emb), eps, cfg_scale)
                _, dk = O.lcm_step(eps, xs, sc, None)
                den[:, :, s:s + W] += wn[k] * dk
            den = m * den + (1 - m) * z0
            img = sc["sqrt_a_prev"] * den + sc["sqrt_b_prev"] * noise[i] if i + 1 < len(ts) else den
    return den


def _mask(L):
    """Clip 0 regenerates a span that crosses the first two windows' overlap (frames 20 .. 39), clip 1 the clip's end."""
    m = torch.zeros((2, L))
    m[0, 15:45] = 1.0
    m[1, L - 22:] = 1.0
    return m


def _joint(pipe, ctx, z0, mask, strength=1.0, seeds=SEEDS, **kw):
    L = z0.shape[2]
    starts, W = _starts(L)
    return pipe.sampler.sample_joint(S=S, conditioning=ctx, length=L, starts=starts, window=W, overlap=OVERLAP,
                                     seeds=seeds, init=z0, mask=mask, strength=strength, **kw)


# ---------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("L", [60, 70], ids=["two-windows", "triple-overlap"])
def test_sample_joint_edit_matches_oracle(pipe, case, L, strength):
    z0, mask = case["z0"][:, :, :L].contiguous(), _mask(L)
    assert _starts(L) == ({60: [0, 20], 70: [0, 20, 30]}[L], T)
    z, last = _joint(pipe, case["ctx"].cuda(), z0.cuda(), mask, strength)
    ref = _oracle_joint_edit(case["Wd"], case["ctx"], z0, mask, SEEDS, strength)
    z = z.cpu()
    regen = mask[:, None, :].expand_as(z) == 1
    err, err_regen = rel_l2(z.numpy(), ref.numpy()), rel_l2(z[regen].numpy(), ref[regen].numpy())
    print(f"sample_joint(init) L={L} strength={strength}: latent {err:.2e}, regenerated frames {err_regen:.2e}")
    assert err <= 1e-4 and err_regen <= 1e-4
    assert torch.equal(z[~regen], z0[~regen]) and torch.equal(z, last.cpu())   # kept frames are the input's bits
    assert rel_l2(z[regen].numpy(), z0[regen].numpy()) > 1e-2                   # and the others are regenerated
    if strength < 1.0:
        assert pipe.sampler.timesteps.tolist() == STRENGTH_TS[(S, strength)]


def test_sample_joint_edit_with_guidance_matches_oracle(pipe, case):
    z0, mask = case["z0"][:, :, :60].contiguous(), _mask(60)
    ctx, uc = case["ctx"], torch.zeros_like(case["ctx"])
    z, _ = _joint(pipe, ctx.cuda(), z0.cuda(), mask, unconditional_conditioning=uc.cuda(),
                  unconditional_guidance_scale=3.0)
    ref = _oracle_joint_edit(case["Wd"], ctx, z0, mask, SEEDS, 1.0, uc=uc, cfg_scale=3.0)
    err = rel_l2(z.cpu().numpy(), ref.numpy())
    print(f"sample_joint(init) with guidance: {err:.2e}")
    assert err <= 1e-4
    plain, _ = _joint(pipe, ctx.cuda(), z0.cuda(), mask)
    assert rel_l2(z.cpu().numpy(), plain.cpu().numpy()) > 1e-2   # the guidance does something


def test_one_window_is_sample_edit(pipe, case):
    ctx = case["ctx"].cuda()
    for L in (T, 24):
        z0, mask = case["z0"][:, :, :L].contiguous().cuda(), _mask(60)[:, :L].contiguous()
        for m, strength in ((mask, 1.0), (mask, 0.5), (None, 0.5)):
            got = _joint(pipe, ctx, z0, m, strength)
            want = pipe.sampler.sample_edit(S=S, conditioning=ctx, init=z0, mask=m, strength=strength, seeds=SEEDS)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    uc = torch.zeros_like(ctx)
    kw = dict(unconditional_conditioning=uc, unconditional_guidance_scale=3.0)
    got = _joint(pipe, ctx, z0, mask, 1.0, **kw)
    want = pipe.sampler.sample_edit(S=S, conditioning=ctx, init=z0, mask=mask, strength=1.0, seeds=SEEDS, **kw)
    assert torch.equal(got[0], want[0])


def test_no_mask_at_strength_one_is_plain_joint_sampling(pipe, case):
    from audiolcm_amd import _hip
    ctx, z0 = case["ctx"].cuda(), case["z0"][:, :, :70].contiguous().cuda()
    starts, W = _starts(70)
    want = pipe.sampler.sample_joint(S=S, conditioning=ctx, length=70, starts=starts, window=W, overlap=OVERLAP,
                                     seeds=SEEDS)
    _hip.profile_begin()
    got = _joint(pipe, ctx, z0, None, 1.0)
    rows = [r["name"] for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert rows == ["alcm::lcm_step_joint_kernel<1>"]            # without a mask the step is the open entry
    _hip.profile_begin()
    _joint(pipe, ctx, z0, _mask(70), 1.0)
    rows = [(r["name"], r["launches"]) for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]
    assert rows == [("alcm::lcm_step_joint_edit_kernel<1>", S)]   # with one, every step is the edit entry


def test_sample_joint_edit_argument_errors(pipe, case):
    ctx, z0 = case["ctx"].cuda(), case["z0"][:, :, :60].contiguous().cuda()
    with pytest.raises(ValueError, match="ring"):
        pipe.sampler.sample_joint(S=S, conditioning=ctx, length=60, starts=[0, 20], window=T, overlap=OVERLAP,
                                  seeds=SEEDS, init=z0, ring=True)
    with pytest.raises(ValueError, match="mask"):
        _joint(pipe, ctx, z0, torch.zeros((2, 61)))
    with pytest.raises(ValueError, match="strength"):
        _joint(pipe, ctx, z0, None, 0.0)
    with pytest.raises(ValueError):
        pipe.sampler.sample_joint(S=S, conditioning=ctx, length=70, starts=[0, 20, 30], window=T, overlap=OVERLAP,
                                  seeds=SEEDS, init=z0)     # a latent of 60 frames for a plan of 70


# ---------------------------------------------------------------------------- edit_long(joint=True) from a latent
L = 100


def _span(lo, hi, rows=(0, 1)):
    m = torch.zeros((2, L))
    for b in rows:
        m[b, lo:hi] = 1.0
    return m


def _edit(pipe, ctx, z0, mask, **kw):
    return pipe.edit_long(ctx, kw.pop("seeds", SEEDS), latent=z0, mask=mask, window=T, overlap=OVERLAP, joint=True, **kw)


@pytest.fixture(scope="module")
def long_span(pipe, case):
    """One joint edit of frames 30 .. 79 (the region [10, 100), four windows) shared by the tests below."""
    mask = _span(30, 80)
    return mask, _edit(pipe, case["ctx"].cuda(), case["z0"].cuda(), mask)


def test_region_of_one_window_is_sample_edit(pipe, case):
    from audiolcm_amd import recipe
    from audiolcm_amd.pipeline import joint_edit_regions
    ctx, z0, mask = case["ctx"].cuda(), case["z0"].cuda(), _span(5, 15)
    assert joint_edit_regions((mask > 0).any(0).tolist(), T, OVERLAP) == [(0, 35, [0], 35)]
    out = _edit(pipe, ctx, z0, mask)
    zk, _ = pipe.sampler.sample_edit(S=S, conditioning=ctx, init=z0[:, :, :35].contiguous(), mask=mask[:, :35],
                                     strength=0.5, seeds=[recipe.window_seed(sd, 0) for sd in SEEDS])
    assert torch.equal(out["latent"][:, :, :35], zk) and torch.equal(out["latent"][:, :, 35:], z0[:, :, 35:])
    assert not torch.equal(out["latent"][:, :, 5:15], z0[:, :, 5:15])
    assert out["wav"].shape == (2, L * FS) and out["mel"].shape == (2, 80, 2 * L)


def test_region_of_several_windows_matches_oracle(pipe, case, long_span):
    from audiolcm_amd import recipe
    from audiolcm_amd.pipeline import joint_edit_regions
    mask, out = long_span
    assert joint_edit_regions((mask > 0).any(0).tolist(), T, OVERLAP) == [(10, 100, [0, 20, 40, 50], T)]
    ref = _oracle_joint_edit(case["Wd"], case["ctx"], case["z0"][:, :, 10:].contiguous(), mask[:, 10:],
                             [recipe.window_seed(sd, 0) for sd in SEEDS], 0.5)
    got = out["latent"].cpu()
    err = rel_l2(got[:, :, 30:80].numpy(), ref[:, :, 20:70].numpy())
    print(f"edit_long(joint=True) frames 30 .. 79: {err:.2e}")
    assert err <= 1e-4
    # frames outside the mask are the input, bit for bit
    assert torch.equal(got[:, :, :30], case["z0"][:, :, :30]) and torch.equal(got[:, :, 80:], case["z0"][:, :, 80:])
    assert torch.isfinite(out["wav"]).all() and out["wav"].shape == (2, L * FS)


def test_joint_edit_is_another_sampler_than_the_chain(pipe, case, long_span):
    mask, out = long_span
    ctx, z0 = case["ctx"].cuda(), case["z0"].cuda()
    chain = pipe.edit_long(ctx, SEEDS, latent=z0, mask=mask, window=T, overlap=OVERLAP)["latent"]
    again = pipe.edit_long(ctx, SEEDS, latent=z0, mask=mask, window=T, overlap=OVERLAP, joint=False)["latent"]
    assert torch.equal(chain, again)
    assert rel_l2(out["latent"][:, :, 30:80].cpu().numpy(), chain[:, :, 30:80].cpu().numpy()) > 1e-2


def test_joint_edit_dit_calls(pipe, case, long_span, monkeypatch):
    """S calls of K rows per region and clip; none for an empty mask."""
    calls = []
    dit = pipe.model.unet.diffusion_model
    fwd = dit.forward_cached
    monkeypatch.setattr(dit, "forward_cached", lambda x, *a, **k: (calls.append(x.shape[0]), fwd(x, *a, **k))[1])
    ctx, z0 = case["ctx"].cuda(), case["z0"].cuda()
    mask, full = long_span
    one = [_edit(pipe, ctx[b:b + 1], z0[b:b + 1], mask[b:b + 1], seeds=SEEDS[b:b + 1]) for b in range(2)]
    assert calls == [4] * S * 2
    # a clip does not depend on its batch: B = 2 is two B = 1 runs, bit for bit
    for b in range(2):
        assert torch.equal(one[b]["latent"], full["latent"][b:b + 1])
    del calls[:]
    two = _edit(pipe, ctx, z0, _span(5, 15) + _span(60, 70))       # two regions: one window, then two
    assert calls == [2] * S + [2] * S * 2 and not torch.equal(two["latent"], z0)
    del calls[:]
    out = _edit(pipe, ctx, z0, torch.zeros((2, L)))
    assert calls == [] and torch.equal(out["latent"], z0)


def test_joint_edit_keep_original_from_a_waveform(pipe, case):
    """Every sample further than the fade from the span is the input's, bit for bit, as with the chain."""
    wav = 0.1 * torch.randn((2, L * FS), generator=torch.Generator().manual_seed(83))
    mask = _span(50, 55, rows=(0,))
    out = pipe.edit_long(case["ctx"].cuda(), SEEDS, wav=wav, mask=mask, window=T, overlap=OVERLAP, keep_original=True,
                         halo_frames=8, fade_samples=512, joint=True)
    got = out["wav"].cpu()
    lo, hi, R = 50 * FS, 55 * FS, 512
    assert got.shape == wav.shape and out["regions"] == [(42, 63)]
    assert torch.equal(got[0, :lo - R + 1], wav[0, :lo - R + 1]) and torch.equal(got[0, hi + R - 1:], wav[0, hi + R - 1:])
    assert torch.equal(got[1], wav[1])
    gen = pipe.decode(out["latent"][:, :, 42:63].contiguous())["wav"].cpu()
    assert torch.equal(got[0, lo:hi], gen[0, (50 - 42) * FS:(55 - 42) * FS])
    assert not torch.equal(got[0, lo:hi], wav[0, lo:hi])


# ---------------------------------------------------------------------------- extend
L0, EXTRA = 24, 40


@pytest.fixture(scope="module")
def extended(pipe, case):
    wav = 0.1 * torch.randn((2, L0 * FS), generator=torch.Generator().manual_seed(85))
    return wav, pipe.extend(case["ctx"].cuda(), SEEDS, wav, EXTRA, window=T, overlap=OVERLAP)


def test_extend_keeps_the_recording(pipe, extended):
    from audiolcm_amd import kernels, recipe
    from audiolcm_amd.mel import MelNet
    wav, out = extended
    got, N, R = out["wav"].cpu(), L0 * FS, 512
    assert set(out) == {"latent", "wav", "region"} and out["region"] == (4, 64)
    assert got.shape == (2, 64 * FS) and out["latent"].shape == (2, 20, 64)
    assert torch.isfinite(got).all() and torch.isfinite(out["latent"]).all()
    assert torch.equal(got[:, :N - R + 1], wav[:, :N - R + 1])           # the recording, up to the fade
    assert not torch.equal(got[:, N - R + 1:N], wav[:, N - R + 1:N])     # the fade closes the junction
    gen = pipe.decode(out["latent"])["wav"].cpu()                        # halo 32 >= 24: the whole clip is decoded
    assert torch.equal(got[:, N:], gen[:, N:])                           # from the junction on: the decode's bits
    post = pipe.model.encode_first_stage(MelNet()(wav.cuda()))
    e0 = recipe.edit_noise(SEEDS, S, 20, L0)[2].cuda()
    z_rec = kernels.latent_init(None, moments=post.parameters.float().contiguous(), e0=e0,
                                scale=float(pipe.model.scale_factor), want_x=False)[0]
    assert torch.equal(out["latent"][:, :, :L0], z_rec)


def test_extend_matches_oracle(pipe, case, extended):
    from audiolcm_amd import recipe
    _, out = extended
    lat = out["latent"].cpu()
    assert _starts(60) == ([0, 20], T)
    z0 = torch.cat([lat[:, :, 4:L0], torch.zeros((2, 20, EXTRA))], 2)
    mask = torch.zeros((2, 60))
    mask[:, 20:] = 1.0
    ref = _oracle_joint_edit(case["Wd"], case["ctx"], z0, mask, [recipe.window_seed(sd, 0) for sd in SEEDS], 1.0)
    err = rel_l2(lat[:, :, L0:].numpy(), ref[:, :, 20:].numpy())
    print(f"extend, the {EXTRA} new frames: {err:.2e}")
    assert err <= 1e-4
    # a continuation of the recording, not the clip the same seeds make from text alone
    alone = pipe.generate_long(case["ctx"].cuda(), SEEDS, L0 + EXTRA, window=T, overlap=OVERLAP)["latent"].cpu()
    assert rel_l2(lat[:, :, L0:].numpy(), alone[:, :, L0:].numpy()) > 1e-2


def test_extend_argument_errors(pipe, case, extended):
    wav, ctx = extended[0], case["ctx"].cuda()
    with pytest.raises(ValueError, match="extra_frames"):
        pipe.extend(ctx, SEEDS, wav, 0, window=T, overlap=OVERLAP)
    with pytest.raises(ValueError, match="32"):
        pipe.extend(ctx, SEEDS, wav, 700, window=T, overlap=OVERLAP)     # 720 frames: 35 windows of 40
    with pytest.raises(ValueError, match="512"):
        pipe.extend(ctx, SEEDS, wav[:, :100], 8, window=T, overlap=OVERLAP)
    with pytest.raises(ValueError, match="32"):
        _edit(pipe, ctx, torch.zeros((2, 20, 720), device="cuda"), None)


# ---------------------------------------------------------------------------- full size, once
def test_joint_variation_30s_mixed(pipe, case, monkeypatch):
    """A variation of a 30 s latent (936 frames, five windows of 312) at B = 1, mixed policy: S DiT calls, S joint
    edit steps on the 16-byte path and no step of another kind."""
    from audiolcm_amd import _hip
    calls = []
    dit = pipe.model.unet.diffusion_model
    fwd = dit.forward_cached
    monkeypatch.setattr(dit, "forward_cached", lambda x, *a, **k: (calls.append(x.shape[0]), fwd(x, *a, **k))[1])
    z0 = torch.randn((1, 20, 936), generator=torch.Generator().manual_seed(87)).cuda()
    pipe.set_split("mixed")
    try:
        _hip.profile_begin()
        out = pipe.edit_long(case["ctx"][:1].cuda(), [0], latent=z0, strength=0.5, joint=True)
        rows = _hip.profile_end()
    finally:
        pipe.set_split(True)
    assert calls == [5] * S
    assert out["latent"].shape == (1, 20, 936) and out["wav"].shape == (1, 936 * FS)
    assert torch.isfinite(out["latent"]).all() and torch.isfinite(out["wav"]).all()
    assert rel_l2(out["latent"].cpu().numpy(), z0.cpu().numpy()) > 1e-2
    steps = [(r["name"], r["launches"]) for r in rows if "lcm_step" in r["name"]]
    assert steps == [("alcm::lcm_step_joint_edit_kernel<4>", S)]


# ---------------------------------------------------------------------------- the Infer function and the CLI
CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")


def _noise_wav(path, n):
    """n samples of full-range PCM16 noise at 16 kHz."""
    from audiolcm_amd.wavio import read_pcm16, write_pcm16
    pcm = np.random.default_rng(3).integers(-32768, 32768, n).astype("<i2")
    write_pcm16(path, pcm.astype(np.float32) / np.float32(32768.0), 16000, scale=32768.0)
    assert np.array_equal(read_pcm16(path)[0], pcm)
    return pcm


def _check_extended_file(path, pcm):
    """24000 samples (46 whole frames and a partial one) continued by 2 s: the junction is sample 46 * 512."""
    from audiolcm_amd.wavio import read_pcm16
    got, sr = read_pcm16(path)
    assert sr == 16000 and got.shape == (24000 + 32000,)
    keep = 46 * FS - 512
    assert np.array_equal(got[:keep], pcm[:keep])
    assert not np.array_equal(got[46 * FS:24000], pcm[46 * FS:])     # the partial frame is generated again
    assert np.abs(got[24000:].astype(np.int64)).max() > 0


def _cli(tmp_path, n, *flags):
    from audiolcm_amd.cli import main
    src, txt, out = str(tmp_path / "in.wav"), str(tmp_path / "p.txt"), str(tmp_path / "out")
    pcm = _noise_wav(src, n)
    with open(txt, "w") as f:
        f.write("a dog barks\n")
    recs = main(["--init-audio", src, "--synthetic-seed", "0", "--prompt_txt", txt, "--outdir", out, "--ddim_steps", "2",
                 "--sample_rate", "16000", "-b", CONFIG, *flags])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")]
    return recs[0]["audio_path"], pcm


def test_edit_infer_extend(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.infer_api import AudioLCMEditInfer
    src = str(tmp_path / "in.wav")
    pcm = _noise_wav(src, 24000)
    path = AudioLCMEditInfer("a dog barks", src, synthetic_seed=0, seed=3, config_path=CONFIG,
                             outpath=str(tmp_path / "ext"), extend_s=2.0)
    assert path == os.path.join(str(tmp_path / "ext"), "a-dog-barks_0.wav")
    _check_extended_file(path, pcm)


def test_cli_extend(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check_extended_file(*_cli(tmp_path, 24000, "--extend", "2.0"))


def test_cli_long_joint_with_init_audio_is_not_cropped(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.wavio import read_wav
    x, sr = read_wav(_cli(tmp_path, 30 * 16000, "--long-joint")[0])
    # 30 s are 937.5 frames: all 938 are written, not the 845 the DiT takes at once
    assert sr == 16000 and x.shape == (938 * FS,) and np.abs(x[845 * FS:]).max() > 0 and np.isfinite(x).all()


def test_init_audio_alone_is_unchanged(tmp_path, monkeypatch):
    """Without the new arguments a request runs the path it ran: ``joint=False`` writes the default's bytes, and so
    does ``joint=True`` for a recording of one window, which ``edit_long`` hands to ``edit``.  The three requests share
    one set of models."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import infer_api
    from audiolcm_amd.infer_api import AudioLCMEditInfer
    build, built = infer_api._build, {}

    def build_once(*a, **k):
        if repr((a, k)) not in built:
            built[repr((a, k))] = build(*a, **k)
        return built[repr((a, k))]
    monkeypatch.setattr(infer_api, "_build", build_once)
    src = str(tmp_path / "in.wav")
    _noise_wav(src, 24000)
    data = []
    for name, kw in (("default", {}), ("chain", dict(joint=False)), ("joint", dict(joint=True))):
        path = AudioLCMEditInfer("a dog barks", src, strength=0.5, synthetic_seed=0, seed=3, config_path=CONFIG,
                                 outpath=str(tmp_path / name), **kw)
        with open(path, "rb") as f:
            data.append(f.read())
    assert len(data[0]) == 44 + 2 * 47 * FS and data[0] == data[1] == data[2]
