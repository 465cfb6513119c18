"""Joint long-form denoising end to end on the HIP path: LCMSampler.sample_joint, AudioLCMPipeline.generate_long(joint=
True), AudioLCMLongInfer(joint=True) and the CLI's --long-joint.

The reference generates one window, so parity is against a composition of the fp32 oracle's own functions written here
(``_oracle_joint``): per LCM step the oracle's DiT on every window's slice, its step, the weighted mean with
``joint_weights``' table and one re-noise of the long latent.  Relative L2 <= 1e-4, the split-policy latent bar
 that the chained long-form test uses; one window is ``sample`` bit for bit."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_l2

pytestmark = pytest.mark.gpu

T, OVERLAP, S = 40, 20, 2


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


def _oracle_joint(Wd, ctx, seeds, L, uc=None, cfg_scale=1.0):
    """sample_joint as a loop over the oracle's dit_forward / lcm_step_scalars / lcm_step on each window's slice."""
    from audiolcm_amd import recipe
    from audiolcm_amd.pipeline import AudioLCMPipeline, joint_weights
    from oracle import alcm_oracle as O
    planner = AudioLCMPipeline.__new__(AudioLCMPipeline)
    planner.latent_shape = (20, 312)
    spans, W = planner.long_windows(L, T, OVERLAP)
    starts = [s for s, _ in spans]
    wn = torch.from_numpy(joint_weights(starts, W, L, OVERLAP).copy())
    img, noise = recipe.prompt_noise(seeds, S, 20, L)
    B = img.shape[0]
    ts = O.lcm_timesteps(S, 50)
    ac = O.alphas_cumprod()
    w_emb = O.guidance_embedding(torch.tensor(5.0 - 1).repeat(B), 256)
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
            img = sc["sqrt_a_prev"] * den + sc["sqrt_b_prev"] * noise[i] if i + 1 < len(ts) else den
    return den, starts, W


@pytest.fixture(scope="module")
def refs(case):
    """The oracle composition per clip length, computed once."""
    cache = {}

    def get(L):
        if L not in cache:
            cache[L] = _oracle_joint(case["Wd"], case["ctx"], case["seeds"], L)
        return cache[L]
    return get


@pytest.mark.parametrize("L", [60, 70], ids=["two-windows", "triple-overlap"])
def test_joint_matches_oracle(pipe, case, refs, L):
    out = pipe.generate_long(case["ctx"].cuda(), case["seeds"], L, window=T, overlap=OVERLAP, joint=True)
    ref, starts, W = refs(L)
    assert (starts, W) == ({60: [0, 20], 70: [0, 20, 30]}[L], T)
    err = rel_l2(out["latent"].cpu().numpy(), ref.numpy())
    print(f"joint long-form L={L}: {err:.2e}")
    assert err <= 1e-4
    assert out["latent"].shape == (2, 20, L) and out["wav"].shape == (2, L * 512)
    assert torch.isfinite(out["latent"]).all() and torch.isfinite(out["wav"]).all()


def test_joint_dit_calls(pipe, case, refs, monkeypatch):
    """By default a DiT call takes the windows of one clip (3 rows here), whatever the batch; ``clips_per_call`` packs
    several clips into a call.  Either way every row gets its own context, timestep and guidance rows and lands in its
    own eps rows: both meet the oracle bar."""
    calls = []
    dit = pipe.model.unet.diffusion_model
    fwd = dit.forward_cached
    monkeypatch.setattr(dit, "forward_cached", lambda x, *a, **k: (calls.append(x.shape[0]), fwd(x, *a, **k))[1])
    ref = refs(70)[0].numpy()
    kw = dict(S=S, conditioning=case["ctx"].cuda(), length=70, starts=[0, 20, 30], window=T, overlap=OVERLAP,
              seeds=case["seeds"])
    for per_call, want in ((1, [3, 3] * S), (2, [6] * S)):
        del calls[:]
        z, _ = pipe.sampler.sample_joint(clips_per_call=per_call, **kw)
        assert calls == want
        err = rel_l2(z.cpu().numpy(), ref)
        print(f"joint long-form L=70, {per_call} clip(s) per DiT call: {err:.2e}")
        assert err <= 1e-4
    monkeypatch.setattr(type(pipe.sampler), "JOINT_DIT_ROWS", 4)   # the row limit caps the clips of a call
    del calls[:]
    pipe.sampler.sample_joint(clips_per_call=2, **kw)
    assert calls == [3, 3] * S


def test_joint_with_guidance_matches_oracle(pipe, case):
    ctx, uc = case["ctx"], torch.zeros_like(case["ctx"])
    z, last = pipe.sampler.sample_joint(S=S, conditioning=ctx.cuda(), length=60, starts=[0, 20], window=T,
                                        overlap=OVERLAP, seeds=case["seeds"], unconditional_conditioning=uc.cuda(),
                                        unconditional_guidance_scale=3.0)
    ref, _, _ = _oracle_joint(case["Wd"], ctx, case["seeds"], 60, uc=uc, cfg_scale=3.0)
    err = rel_l2(z.cpu().numpy(), ref.numpy())
    print(f"joint long-form with guidance: {err:.2e}")
    assert err <= 1e-4 and torch.equal(z, last)
    plain, _ = pipe.sampler.sample_joint(S=S, conditioning=ctx.cuda(), length=60, starts=[0, 20], window=T,
                                         overlap=OVERLAP, seeds=case["seeds"])
    assert rel_l2(z.cpu().numpy(), plain.cpu().numpy()) > 1e-2   # the guidance does something


def test_one_window_is_plain_sampling(pipe, case):
    ctx = case["ctx"].cuda()
    out = pipe.generate_long(ctx, case["seeds"], T, window=T, overlap=OVERLAP, joint=True)
    want, _ = pipe.sampler.sample(S=S, batch_size=2, shape=(20, T), conditioning=ctx, seeds=case["seeds"],
                                  verbose=False)
    assert torch.equal(out["latent"], want)
    short = pipe.generate_long(ctx, case["seeds"], 24, window=T, overlap=OVERLAP, joint=True)   # shorter than a window
    want, _ = pipe.sampler.sample(S=S, batch_size=2, shape=(20, 24), conditioning=ctx, seeds=case["seeds"],
                                  verbose=False)
    assert torch.equal(short["latent"], want)


def test_joint_is_another_sampler_than_the_chain(pipe, case):
    ctx = case["ctx"].cuda()
    joint = pipe.generate_long(ctx, case["seeds"], 60, window=T, overlap=OVERLAP, joint=True)["latent"]
    chained = pipe.generate_long(ctx, case["seeds"], 60, window=T, overlap=OVERLAP)["latent"]
    again = pipe.generate_long(ctx, case["seeds"], 60, window=T, overlap=OVERLAP, joint=False)["latent"]
    assert torch.equal(chained, again)
    assert rel_l2(joint.cpu().numpy(), chained.cpu().numpy()) > 1e-2


def test_joint_shard_invariance(pipe):
    """Clip 1 of a B = 3 run against its own B = 1 run, at test_edit_shard_invariance's bar of 1e-6.  The DiT picks
    its kernels by the rows of a call (one row differs by 4.7e-6 between a call of 5 rows and one of 6 at 40 frames), so
    ``sample_joint`` calls it on one clip's windows at a time: 3 rows in both runs here."""
    from audiolcm_amd import recipe
    ctx = recipe.synthetic_context(3).cuda()
    full = pipe.generate_long(ctx, [0, 1, 2], 70, window=T, overlap=OVERLAP, joint=True)
    part = pipe.generate_long(ctx[1:2], [1], 70, window=T, overlap=OVERLAP, joint=True)
    e_lat = rel_l2(part["latent"].cpu().numpy(), full["latent"][1:2].cpu().numpy())
    e_wav = rel_l2(part["wav"].cpu().numpy(), full["wav"][1:2].cpu().numpy())
    print(f"joint shard invariance, clip 1 of B = 3 against B = 1: latent {e_lat:.2e} wav {e_wav:.2e}")
    assert e_lat < 1e-6
    assert e_wav < 1e-6


def test_sample_joint_argument_errors(pipe, case):
    ctx = case["ctx"].cuda()
    with pytest.raises(ValueError, match="845"):
        pipe.sampler.sample_joint(S=S, conditioning=ctx, length=1000, starts=[0, 154], window=846, overlap=20,
                                  seeds=case["seeds"])
    with pytest.raises(ValueError):
        pipe.sampler.sample_joint(S=S, conditioning=ctx, length=61, starts=[0, 20], window=T, overlap=OVERLAP,
                                  seeds=case["seeds"])
    with pytest.raises(ValueError, match="x_T"):
        pipe.sampler.sample_joint(S=S, conditioning=ctx, length=60, starts=[0, 20], window=T, overlap=OVERLAP,
                                  x_T=torch.zeros((2, 20, 40)))


def test_joint_30s_mixed(pipe, case):
    """A 30 s clip (936 frames, five windows of 312) at B = 1, mixed policy: S joint steps and no edit step."""
    from audiolcm_amd import _hip
    ctx = case["ctx"][:1].cuda()
    pipe.set_split("mixed")
    try:
        _hip.profile_begin()
        out = pipe.generate_long(ctx, [0], latent_len=936, joint=True)
        rows = _hip.profile_end()
    finally:
        pipe.set_split(True)
    assert out["latent"].shape == (1, 20, 936) and out["wav"].shape == (1, 936 * 512)
    assert torch.isfinite(out["latent"]).all() and torch.isfinite(out["wav"]).all()
    joint = [r for r in rows if "lcm_step_joint" in r["name"]]
    assert [r["name"] for r in joint] == ["alcm::lcm_step_joint_kernel<4>"] and joint[0]["launches"] == S
    assert not [r for r in rows if "lcm_step_edit" in r["name"]]
    gather = [r for r in rows if "joint_gather" in r["name"]]
    assert len(gather) == 1 and gather[0]["launches"] == 1


def test_long_infer_api_joint(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.infer_api import AudioLCMLongInfer
    from audiolcm_amd.wavio import read_wav
    path = AudioLCMLongInfer("rain falls on a tin roof", duration_s=12.0,
                             config_path=os.path.join(REPO, "configs", "audiolcm.yaml"), synthetic_seed=0,
                             outpath=str(tmp_path / "long"), seed=3, joint=True)
    assert path == os.path.join(str(tmp_path / "long"), "rain-falls-on-a-tin-roof_0.wav")
    w, sr = read_wav(path)
    assert sr == 16000 and w.shape == (12 * 16000,) and np.abs(w).max() > 0


def test_cli_long_joint(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.cli import main
    from audiolcm_amd.wavio import read_wav
    txt, out = str(tmp_path / "p.txt"), str(tmp_path / "out")
    with open(txt, "w") as f:
        f.write("a dog barks\n")
    recs = main(["--duration", "3", "--long-joint", "--W", "40", "--synthetic-seed", "0", "--prompt_txt", txt,
                 "--outdir", out, "--ddim_steps", "2", "--sample_rate", "16000",
                 "-b", os.path.join(REPO, "configs", "audiolcm.yaml")])
    assert [r["audio_path"] for r in recs] == [os.path.join(out, "a-dog-barks_0.wav")]
    x, sr = read_wav(recs[0]["audio_path"])
    assert sr == 16000 and x.shape == (94 * 512,) and np.abs(x).max() > 0   # ceil(3 * 16000 / 512) = 94 frames
