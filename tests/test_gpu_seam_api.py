"""``fade_law`` and ``match_gain`` through the pipeline on the synthetic weights: ``edit_long(keep_original=True)``,
``extend`` and ``loop_from`` (a region of the ring, and the ring cut open) against the composition they document: the
pipeline's own ``decode`` of each region, then the float64 restatement of tests/_seam_ref.py (its own tables) on the
recording and that decode.  The bar is the blend's, 32 * 2^-24 * max(|orig|, gam |gen|) per sample (tests/
test_gpu_seam_ops.py); the tables' own 2^-23 moves a sample by less than a tenth of it.  Samples of g = 0 are the
input's bits, regenerated frames the decode's where gam is 1, the sample count is the input's, and "linear" is the call
without the argument, byte for byte."""
import os

import numpy as np
import pytest
import torch

import _seam_ref as ref
from conftest import REPO, golden

pytestmark = pytest.mark.gpu

FS = 512
W, OV = 40, 20
SEEDS = [5, 6]
BAR = 32 * 2.0 ** -24
FORMS = [("matched", False), ("matched", True)]


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip
    from audiolcm_amd.pipeline import AudioLCMPipeline
    _hip.require_device(0)
    return AudioLCMPipeline.from_recipe(0, split=True, encoder=True)


@pytest.fixture(scope="module")
def ctx():
    from audiolcm_amd import recipe
    return recipe.synthetic_context(2)


def check_composition(got, orig, gen, mask, gen_start, R, ring, match_gain):
    """``got`` (B, N) fp32 against the restatement of the matched law on orig (B, N) and the decode gen (B, Ng)."""
    rho, gam, sums = ref.stats(orig, gen, mask, FS, gen_start, R, ring)
    assert (sums[..., 0] > 0).any() and (rho < 1).any()                   # something was measured
    want, g, scale = ref.blend(orig, gen, mask, FS, gen_start, R, ring, rho, gam if match_gain else None)
    assert got.shape == orig.shape
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= BAR * scale).all(), float((err / np.maximum(scale, 1e-30)).max() / 2.0 ** -24)
    keep, take = g == 0.0, g == 1.0
    assert keep.any() and take.any() and ((g > 0) & (g < 1)).any()
    assert np.array_equal(got[keep].view(np.uint32), orig[keep].view(np.uint32))
    if not match_gain:
        inside, gi = ref.in_gen(orig.shape[1], gen_start, gen.shape[1], ring)
        full = np.zeros_like(orig)
        full[:, inside] = gen[:, gi[inside]]
        assert np.array_equal(got[take].view(np.uint32), full[take].view(np.uint32))
    else:
        assert (gam[mask > 0] != 1.0).any()
    # and the law is not the linear one: the fade differs from orig + g (gen - orig) by more than the bar somewhere
    lin, _ = ref.blend_linear(orig, gen, mask, FS, gen_start, R, ring)
    assert (np.abs(got - lin) > 4 * BAR * scale).any()


# ---------------------------------------------------------------------------- edit_long(keep_original=True)
L = 100


@pytest.fixture(scope="module")
def recording():
    return torch.from_numpy(np.tile(golden("mel_B2.npz")["wav"], (1, 3))[:, :L * FS].copy())


def _edit(pipe, ctx, wav, **kw):
    mask = torch.zeros((2, L))
    mask[0, 50:55] = 1.0
    mask[1, 52:54] = 1.0
    out = pipe.edit_long(ctx.cuda(), SEEDS, wav=wav, mask=mask, window=W, overlap=OV, keep_original=True, halo_frames=8,
                         fade_samples=512, **kw)
    assert out["regions"] == [(42, 63)]
    return mask.numpy(), out


@pytest.mark.parametrize("law,gain", FORMS)
def test_edit_long_is_the_composition(pipe, ctx, recording, law, gain):
    mask, out = _edit(pipe, ctx, recording, fade_law=law, match_gain=gain)
    gen = pipe.decode(out["latent"][:, :, 42:63].contiguous())["wav"].cpu().numpy()
    check_composition(out["wav"].cpu().numpy(), recording.numpy(), gen, mask, 42 * FS, 512, False, gain)


def test_edit_long_linear_is_the_default(pipe, ctx, recording):
    _, a = _edit(pipe, ctx, recording)
    _, b = _edit(pipe, ctx, recording, fade_law="linear", match_gain=False)
    assert torch.equal(a["wav"], b["wav"]) and torch.equal(a["latent"], b["latent"])
    with pytest.raises(ValueError, match="fade_law"):
        _edit(pipe, ctx, recording, fade_law="cubic")
    with pytest.raises(ValueError, match="fade_law and match_gain.*keep_original"):
        pipe.edit_long(ctx.cuda(), SEEDS, wav=recording, window=W, overlap=OV, match_gain=True)


# ---------------------------------------------------------------------------- extend
L0, EXTRA = 24, 40


@pytest.fixture(scope="module")
def short():
    return 0.1 * torch.randn((2, L0 * FS), generator=torch.Generator().manual_seed(85))


@pytest.mark.parametrize("law,gain", FORMS)
def test_extend_is_the_composition(pipe, ctx, short, law, gain):
    out = pipe.extend(ctx.cuda(), SEEDS, short, EXTRA, window=W, overlap=OV, fade_law=law, match_gain=gain)
    got = out["wav"].cpu().numpy()
    assert got.shape == (2, (L0 + EXTRA) * FS)
    gen = pipe.decode(out["latent"].contiguous())["wav"].cpu().numpy()          # the halo of 32 frames reaches frame 0
    orig = np.concatenate([short.numpy(), np.zeros((2, EXTRA * FS), np.float32)], 1)
    mask = np.zeros((2, L0 + EXTRA), np.float32)
    mask[:, L0:] = 1.0
    check_composition(got, orig, gen, mask, 0, FS, False, gain)


def test_extend_linear_is_the_default(pipe, ctx, short):
    a = pipe.extend(ctx.cuda(), SEEDS, short, EXTRA, window=W, overlap=OV)
    b = pipe.extend(ctx.cuda(), SEEDS, short, EXTRA, window=W, overlap=OV, fade_law="linear")
    assert torch.equal(a["wav"], b["wav"])


# ---------------------------------------------------------------------------- loop_from
def _loop_recording(n):
    return torch.rand((2, n * FS), generator=torch.Generator().manual_seed(93)) - 0.5


@pytest.mark.parametrize("law,gain", FORMS)
@pytest.mark.parametrize("n,halo,route", [(60, 8, "region"), (44, 32, "ring")])
def test_loop_from_is_the_composition(pipe, ctx, n, halo, route, law, gain):
    from audiolcm_amd.windows import ring_paste_cut, seam_mask
    m = 4
    wav = _loop_recording(n)
    out = pipe.loop_from(ctx.cuda(), SEEDS, wav, seam_frames=m, window=W, overlap=OV, halo_frames=halo, fade_law=law,
                         match_gain=gain)
    z = out["latent"]
    if route == "region":
        assert out["regions"] == [(n - m - halo, 2 * (m + halo))]
        a = n - m - halo
        idx = (a + torch.arange(2 * (m + halo), device="cuda")) % n
        gen = pipe.decode(z[:, :, idx].contiguous())["wav"]
    else:       # the ring cut open at frame a and decoded once round with the circular halo
        assert out["regions"] == [("ring",)]
        a = ring_paste_cut(seam_mask(n, m).astype(bool).tolist(), 1)
        idx = (torch.arange(n + 2 * halo, device="cuda") + a - halo) % n
        gen = pipe.decode(z[:, :, idx].contiguous())["wav"][:, halo * FS:(halo + n) * FS]
    mask = np.broadcast_to(seam_mask(n, m).astype(np.float32), (2, n)).copy()
    check_composition(out["wav"].cpu().numpy(), wav.numpy(), gen.cpu().numpy(), mask, a * FS, FS, True, gain)


def test_loop_from_linear_is_the_default(pipe, ctx):
    wav = _loop_recording(60)
    kw = dict(seam_frames=4, window=W, overlap=OV, halo_frames=8)
    a = pipe.loop_from(ctx.cuda(), SEEDS, wav, **kw)
    b = pipe.loop_from(ctx.cuda(), SEEDS, wav, fade_law="linear", match_gain=False, **kw)
    assert torch.equal(a["wav"], b["wav"])
    with pytest.raises(ValueError, match="fade_law and match_gain.*keep_original"):
        pipe.edit_loop(ctx.cuda(), SEEDS, wav=wav, window=W, overlap=OV, fade_law="matched")


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_a_kept_file_under_the_matched_law(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd.cli import main
    from audiolcm_amd.wavio import read_pcm16, write_pcm16
    src, txt, outdir = str(tmp_path / "in.wav"), str(tmp_path / "p.txt"), str(tmp_path / "out")
    pcm = np.random.default_rng(3).integers(-32768, 32768, 24000).astype("<i2")
    write_pcm16(src, pcm.astype(np.float32) / np.float32(32768.0), 16000, scale=32768.0)
    with open(txt, "w") as f:
        f.write("a dog barks\n")
    recs = main(["--init-audio", src, "--inpaint", "--mask-spans", "0.5-1.0", "--synthetic-seed", "0", "--prompt_txt", txt,
                 "--outdir", outdir, "--ddim_steps", "2", "--sample_rate", "16000", "-b",
                 os.path.join(REPO, "configs", "audiolcm.yaml"), "--keep-original", "--fade-law", "matched",
                 "--match-gain"])
    got, sr = read_pcm16(recs[0]["audio_path"])
    assert sr == 16000 and got.shape == (24000,)
    lo, hi = 8000 - 512, 16000 + 512
    assert np.array_equal(got[:lo], pcm[:lo]) and np.array_equal(got[hi:], pcm[hi:])
    assert not np.array_equal(got[8000:16000], pcm[8000:16000])
