"""Loops made from a recording end to end on the HIP path: LCMSampler.sample_ring_edit, AudioLCMPipeline.edit_loop,
loop_from and _encode_ring.

The reference has neither an edit path nor a ring, so parity is against a composition of the fp32 oracle's own
functions written here (``_oracle_ring_edit``): the loop of tests/test_gpu_loop.py's ``_oracle_ring`` (per LCM step the
oracle's DiT on every window's frames, modular slices of the ring, its step and the weighted mean with ``ring_weights``'
table) with the start and the per-step blend of tests/test_gpu_joint_edit.py's ``_oracle_joint_edit``.  Relative L2 <=
1e-4, the split-policy latent bar both use.  Kept frames and kept samples are exact, a line region is
``edit_long(joint=True)``'s own call on the rolled recording bit for bit, and the seam of ``loop_from`` is consecutive
samples of one decode."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

T, OVERLAP, S = 40, 20, 2
FS = 512
STRENGTH_TS = {(2, 0.5): [499, 259]}  # scheduling_lcm.py:171 at strength 0.5
SEEDS = [5, 6]
PLANS = {60: [0, 20, 40], 70: [0, 17, 35, 52], 44: [0, 12, 28]}   # 70: the element path; 44: edit_loop's ring route


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
                z0=torch.randn((2, 20, 100), generator=torch.Generator().manual_seed(91)))


def _mask(L):
    """Clip 0 regenerates a run across the wrap (frames L - 8 .. L - 1 and 0 .. 9), clip 1 frames 25 .. 39."""
    m = torch.zeros((2, L))
    m[0, L - 8:] = 1.0
    m[0, :10] = 1.0
    m[1, 25:40] = 1.0
    return m


def _seam(L, m=4):
    from audiolcm_amd.windows import seam_mask
    return torch.from_numpy(seam_mask(L, m)).float().expand(2, L).contiguous()


def _oracle_ring_edit(Wd, ctx, z0, mask, n0, noise, starts, W, overlap, strength):
    """sample_ring_edit(init=z0, mask=mask) as a loop over the oracle's dit_forward / lcm_step_scalars / lcm_step on each
    window's frames (s + j) mod L."""
    from audiolcm_amd.pipeline import ring_weights
    from oracle import alcm_oracle as O
    B, _, L = z0.shape
    wn = torch.from_numpy(ring_weights(starts, W, L, overlap).copy())
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
                f = (s + torch.arange(W)) % L
                xs = img[:, :, f]
                _, dk = O.lcm_step(O.dit_forward(Wd, xs, tt, ctx, w_emb), xs, sc, None)
                den[:, :, f] += wn[k] * dk
            den = m * den + (1 - m) * z0
            img = sc["sqrt_a_prev"] * den + sc["sqrt_b_prev"] * noise[i] if i + 1 < len(ts) else den
    return den


@pytest.fixture(scope="module")
def refs(case):
    """The oracle composition per (ring length, strength, mask name), computed once."""
    from audiolcm_amd import recipe
    cache = {}

    def get(L, strength, seam=False):
        if (L, strength, seam) not in cache:
            n0, noise, _ = recipe.edit_noise(SEEDS, S, 20, L)
            cache[(L, strength, seam)] = _oracle_ring_edit(
                case["Wd"], case["ctx"], case["z0"][:, :, :L].contiguous(), _seam(L) if seam else _mask(L), n0, noise,
                PLANS[L], T, OVERLAP, strength)
        return cache[(L, strength, seam)]
    return get


def _ring_edit(pipe, ctx, z0, mask, strength=1.0, seeds=SEEDS, **kw):
    L = z0.shape[2]
    return pipe.sampler.sample_ring_edit(S=S, conditioning=ctx, init=z0, starts=PLANS[L], window=T, overlap=OVERLAP,
                                         mask=mask, strength=strength, seeds=seeds, **kw)


# ---------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("L", [60, 70], ids=["three-windows", "element-path"])
def test_sample_ring_edit_matches_oracle(pipe, case, refs, L, strength):
    z0, mask = case["z0"][:, :, :L].contiguous(), _mask(L)
    assert pipe.loop_windows(L, T, OVERLAP) == (PLANS[L], T, OVERLAP)
    z, last = _ring_edit(pipe, case["ctx"].cuda(), z0.cuda(), mask, strength)
    ref = refs(L, strength)
    z = z.cpu()
    regen = mask[:, None, :].expand_as(z) == 1
    err, err_regen = rel_l2(z.numpy(), ref.numpy()), rel_l2(z[regen].numpy(), ref[regen].numpy())
    print(f"sample_ring_edit L={L} strength={strength}: latent {err:.2e}, regenerated frames {err_regen:.2e}")
    assert err <= 1e-4 and err_regen <= 1e-4
    assert torch.equal(z[~regen], z0[~regen]) and torch.equal(z, last.cpu())   # kept frames are the input's bits
    assert rel_l2(z[regen].numpy(), z0[regen].numpy()) > 1e-2                   # and the others are regenerated
    if strength < 1.0:
        assert pipe.sampler.timesteps.tolist() == STRENGTH_TS[(S, strength)]


def test_rotating_the_recording_rotates_the_result(pipe, case, refs):
    """No frame of the ring is special: with init, mask and all noises rolled by 20 frames (the windows' spacing) every
    window sees the input of its neighbour, so the latent is the first one rolled by 20 up to fp32 summation order.
    Each run is within 1e-4 of the oracle composition, for which the rotation is exact up to that order: 2e-4, the
    argument of tests/test_gpu_loop.py::test_rotating_the_noise_rotates_the_loop."""
    from audiolcm_amd import recipe
    ctx = case["ctx"].cuda()
    z0, mask = case["z0"][:, :, :60].contiguous(), _mask(60)
    n0, noise, _ = recipe.edit_noise(SEEDS, S, 20, 60)
    roll = lambda t: torch.roll(t, 20, dims=-1).contiguous()   # noqa: E731
    a, _ = _ring_edit(pipe, ctx, z0.cuda(), mask, 0.5, init_noise=n0, noise=noise)
    b, _ = _ring_edit(pipe, ctx, roll(z0).cuda(), roll(mask), 0.5, init_noise=roll(n0), noise=roll(noise))
    e_ref = rel_l2(a.cpu().numpy(), refs(60, 0.5).numpy())
    err = rel_l2(b.cpu().numpy(), roll(a).cpu().numpy())
    print(f"ring edit L=60: rolled run against the rolled latent {err:.2e} (the run against the oracle {e_ref:.2e})")
    assert e_ref <= 1e-4 and err <= 2e-4
    kept = roll(mask)[:, None, :].expand_as(b) == 0
    assert torch.equal(b.cpu()[kept], roll(z0)[kept])


def test_no_mask_at_strength_one_is_plain_ring_sampling(pipe, case):
    from audiolcm_amd import _hip, recipe
    ctx, z0 = case["ctx"].cuda(), case["z0"][:, :, :70].contiguous().cuda()
    x_T, noise = recipe.prompt_noise(SEEDS, S, 20, 70)
    want = pipe.sampler.sample_joint(S=S, conditioning=ctx, length=70, starts=PLANS[70], window=T, overlap=OVERLAP,
                                     x_T=x_T, noise=noise, ring=True)
    _hip.profile_begin()
    got = _ring_edit(pipe, ctx, z0, None, 1.0, seeds=None, init_noise=x_T, noise=noise)
    rows = [(r["name"], r["launches"]) for r in _hip.profile_end() if "lcm_step" in r["name"]]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert rows == [("alcm::lcm_step_ring_kernel<1>", S)]            # without a mask the step is the ring's open entry
    _hip.profile_begin()
    _ring_edit(pipe, ctx, z0, _mask(70), 1.0)
    rows = [(r["name"], r["launches"]) for r in _hip.profile_end() if "lcm_step" in r["name"]]
    assert rows == [("alcm::lcm_step_ring_edit_kernel<1>", S)]       # with one, every step is the edit entry
    _hip.profile_begin()
    _ring_edit(pipe, ctx, case["z0"][:, :, :60].contiguous().cuda(), _mask(60), 0.5)
    rows = [(r["name"], r["launches"]) for r in _hip.profile_end() if "lcm_step" in r["name"] or "gather" in r["name"]]
    assert dict(rows) == {"alcm::ring_gather_kernel<4>": 1, "alcm::lcm_step_ring_edit_kernel<4>": S} and len(rows) == 2


def test_sample_ring_edit_argument_errors(pipe, case):
    ctx, z0 = case["ctx"].cuda(), case["z0"][:, :, :60].contiguous().cuda()
    with pytest.raises(ValueError, match="sample_ring_edit"):      # the line's entry still refuses a ring, and says where
        pipe.sampler.sample_joint(S=S, conditioning=ctx, length=60, starts=PLANS[60], window=T, overlap=OVERLAP,
                                  seeds=SEEDS, init=z0, ring=True)
    with pytest.raises(ValueError, match="mask"):
        _ring_edit(pipe, ctx, z0, torch.zeros((2, 61)))
    with pytest.raises(ValueError, match="strength"):
        _ring_edit(pipe, ctx, z0, None, 0.0)
    with pytest.raises(ValueError):
        pipe.sampler.sample_ring_edit(S=S, conditioning=ctx, init=z0, starts=[0], window=T, overlap=OVERLAP,
                                      seeds=SEEDS)         # one window cannot close a ring
    with pytest.raises(ValueError):
        pipe.sampler.sample_ring_edit(S=S, conditioning=ctx, init=z0, starts=[0, 10], window=T, overlap=OVERLAP,
                                      seeds=SEEDS)         # frames 50 .. 59 under no window


# ---------------------------------------------------------------------------- edit_loop from a latent
def _edit_loop(pipe, ctx, z, mask, seeds=SEEDS, **kw):
    return pipe.edit_loop(ctx, seeds, latent=z, mask=mask, window=T, overlap=OVERLAP, keep_original=False, **kw)


@pytest.fixture(scope="module")
def seam60(pipe, case):
    """One seam edit of a ring of 60 frames (the line route: one region of 48 frames across the wrap)."""
    z, m = case["z0"][:, :, :60].contiguous().cuda(), _seam(60)
    return z, m, _edit_loop(pipe, case["ctx"].cuda(), z, m)


def test_a_line_region_is_edit_longs_call_on_the_rolled_ring(pipe, case, seam60):
    from audiolcm_amd.windows import ring_edit_regions
    z, m, out = seam60
    assert ring_edit_regions((m > 0).any(0).tolist(), T, OVERLAP) == [("line", 36, 48, [0, 8], T)]
    roll = lambda t, k: torch.roll(t, k, dims=-1).contiguous()   # noqa: E731
    line = pipe.edit_long(case["ctx"].cuda(), SEEDS, latent=roll(z, 30), mask=roll(m, 30), window=T, overlap=OVERLAP,
                          joint=True)["latent"]
    assert torch.equal(out["latent"], roll(line, -30))
    kept = (m == 0)[:, None, :].expand(z.shape).cuda()
    assert torch.equal(out["latent"][kept], z[kept]) and not torch.equal(out["latent"][~kept], z[~kept])
    # the decode is generate_loop's: one period at 16 kHz, cut from the extended waveform
    assert out["wav"].shape == (2, 60 * FS) and out["rate"] == 16000 and out["ext"].shape == (2, (60 + 64) * FS)
    assert out["mel"].shape[-1] == 120 and torch.isfinite(out["wav"]).all()


def test_rolling_the_ring_rolls_the_edit(pipe, case, seam60):
    """One region, and its noise is drawn at the region's length: bit for bit."""
    z, m, out = seam60
    roll = lambda t: torch.roll(t, 7, dims=-1).contiguous()   # noqa: E731
    got = _edit_loop(pipe, case["ctx"].cuda(), roll(z), roll(m))
    assert torch.equal(got["latent"], roll(out["latent"]))


def test_regions_that_cover_the_ring_match_oracle(pipe, case, refs):
    from audiolcm_amd.windows import ring_edit_regions
    z, m = case["z0"][:, :, :44].contiguous(), _seam(44)
    assert ring_edit_regions((m > 0).any(0).tolist(), T, OVERLAP) == [("ring", PLANS[44], T, OVERLAP)]
    out = _edit_loop(pipe, case["ctx"].cuda(), z.cuda(), m)
    got = out["latent"].cpu()
    err = rel_l2(got.numpy(), refs(44, 0.5, seam=True).numpy())
    print(f"edit_loop L=44, the ring route: {err:.2e}")
    assert err <= 1e-4
    assert torch.equal(got[:, :, 4:40], z[:, :, 4:40]) and out["wav"].shape == (2, 44 * FS)


def test_edit_loop_dit_calls(pipe, case, monkeypatch):
    """S calls of K rows per region and clip; none for an empty mask."""
    calls = []
    dit = pipe.model.unet.diffusion_model
    fwd = dit.forward_cached
    monkeypatch.setattr(dit, "forward_cached", lambda x, *a, **k: (calls.append(x.shape[0]), fwd(x, *a, **k))[1])
    ctx, z0 = case["ctx"].cuda(), case["z0"].cuda()
    _edit_loop(pipe, ctx, z0[:, :, :60].contiguous(), _seam(60))
    assert calls == [2] * S * 2                                     # one region of two windows, two clips
    del calls[:]
    two = torch.zeros((1, 100))
    two[0, 10:15] = two[0, 60:65] = 1.0                             # two regions of 45 frames: [40, 85) and [90, 135)
    out = _edit_loop(pipe, ctx[:1], z0[:1], two, seeds=SEEDS[:1])
    assert calls == [2] * S + [2] * S and not torch.equal(out["latent"], z0[:1])
    del calls[:]
    _edit_loop(pipe, ctx[:1], z0[:1, :, :44].contiguous(), _seam(44)[:1], seeds=SEEDS[:1])
    assert calls == [3] * S                                         # the ring route: one call of three windows a step
    del calls[:]
    out = _edit_loop(pipe, ctx, z0, torch.zeros((2, 100)))
    assert calls == [] and torch.equal(out["latent"], z0)


def test_edit_loop_of_a_loop_decodes_as_generate_loop(pipe, case):
    """A variation of a generated loop (mask None: the ring route): one period, and the decode of the circularly padded
    latent continues past the period's end with its start, tests/test_gpu_loop.py's check at its bar of 1e-3."""
    from audiolcm_amd import kernels
    from audiolcm_amd.windows import ring_edit_regions
    ctx = case["ctx"].cuda()
    L, h = 24, 16
    z = pipe.generate_loop(ctx, SEEDS, L, halo_frames=h)["latent"]
    assert [e[0] for e in ring_edit_regions([True] * L, L)] == ["ring"]
    out = pipe.edit_loop(ctx, SEEDS, latent=z, halo_frames=h)
    assert set(out) == {"latent", "mel", "wav", "rate", "ext"} and out["rate"] == 16000
    assert out["wav"].shape == (2, L * FS) and out["ext"].shape == (2, (L + 2 * h) * FS)
    assert rel_l2(out["latent"].cpu().numpy(), z.cpu().numpy()) > 1e-2
    a, b = h * FS, (h + L) * FS
    err = rel_l2(out["ext"][:, b:b + FS].cpu().numpy(), out["ext"][:, a:a + FS].cpu().numpy())
    print(f"edit_loop L=24 h=16: continuation against the start {err:.2e}")
    assert err <= 1e-3
    assert torch.equal(out["wav"], kernels.wave_loop(out["ext"], a, L * FS, 512))
    tail = pipe._decode_loop(out["latent"], 16000, h, 512)
    assert torch.equal(tail["wav"], out["wav"]) and torch.equal(tail["ext"], out["ext"])


# ---------------------------------------------------------------------------- loop_from a waveform
def _recording(L):
    g = torch.Generator().manual_seed(93)
    return torch.rand((2, L * FS), generator=g) - 0.5


@pytest.mark.parametrize("L,halo,route", [(60, 8, "region"), (44, 32, "ring")])
def test_loop_from_keeps_the_recording(pipe, case, L, halo, route):
    from audiolcm_amd.windows import ring_paste_regions, seam_mask
    m, R = 4, 512
    wav = _recording(L)
    out = pipe.loop_from(case["ctx"].cuda(), SEEDS, wav, seam_frames=m, window=T, overlap=OVERLAP, halo_frames=halo)
    got, z = out["wav"].cpu(), out["latent"]
    assert set(out) == {"latent", "wav", "regions"} and got.shape == wav.shape and z.shape == (2, 20, L)
    assert out["regions"] == ring_paste_regions(seam_mask(L, m), halo)
    assert out["regions"] == ([(L - m - halo, 2 * (m + halo))] if route == "region" else [("ring",)])
    # every sample at least R from a regenerated frame, round the ring, is the recording's
    lo, hi = m * FS + R - 1, (L - m) * FS - R + 1
    assert hi > lo and torch.equal(got[:, lo:hi], wav[:, lo:hi])
    assert not torch.equal(got[:, m * FS:lo], wav[:, m * FS:lo]) and not torch.equal(got[:, hi:hi + R], wav[:, hi:hi + R])
    # the seam is consecutive samples of one decode: the last m frames, then the first m
    if route == "region":
        a = L - m - halo
        idx = (a + torch.arange(2 * (m + halo), device="cuda")) % L
        first = halo
    else:       # the ring is cut open in the middle of the kept frames and decoded from there with the circular halo
        from audiolcm_amd.windows import ring_paste_cut
        a = ring_paste_cut(seam_mask(L, m), 1)
        assert a == L // 2
        idx = (torch.arange(L + 2 * halo, device="cuda") + a - halo) % L
        first = halo + L - m - a
    gen = pipe.decode(z[:, :, idx].contiguous())["wav"].cpu()
    seam = torch.cat([got[:, (L - m) * FS:], got[:, :m * FS]], 1)
    assert torch.equal(seam, gen[:, first * FS:(first + 2 * m) * FS])
    assert not torch.equal(seam, torch.cat([wav[:, (L - m) * FS:], wav[:, :m * FS]], 1))
    # the latent outside the seam is the ring encoding of the recording
    z_rec = pipe._encode_ring(wav.cuda(), SEEDS, S, True, halo)
    assert torch.equal(z[:, :, m:L - m], z_rec[:, :, m:L - m]) and not torch.equal(z, z_rec)


def test_loop_from_takes_further_spans(pipe, case):
    wav = _recording(60)
    extra = torch.zeros((2, 60))
    extra[0, 30:32] = 1.0
    out = pipe.loop_from(case["ctx"].cuda(), SEEDS, wav, seam_frames=4, mask=extra, window=T, overlap=OVERLAP,
                         halo_frames=4)
    got = out["wav"].cpu()
    assert out["regions"] == [(26, 10), (52, 16)]
    assert torch.equal(got[1, 5 * FS:55 * FS], wav[1, 5 * FS:55 * FS])          # clip 1 has only the seam
    assert not torch.equal(got[0, 30 * FS:32 * FS], wav[0, 30 * FS:32 * FS])
    assert torch.equal(got[0, 5 * FS:29 * FS], wav[0, 5 * FS:29 * FS])


@pytest.mark.parametrize("name", ["seam-as-wide-as-the-halo", "span-where-the-cut-would-be", "all-regenerated"])
def test_whole_ring_paste_has_the_halo_round_every_sample(pipe, case, name):
    """The ("ring",) paste at m = h and L >= 2h, where a decode of L + 2h frames has no room for gen to go on into its
    halo: the ring is cut open among kept frames (``ring_paste_cut``) and decoded from there, so every pasted sample has
    h frames of context either side: the pasted samples are, bit for bit, the centre N samples of a decode of L + 2h
    frames.  (The decoder normalises and attends over the whole length, so decodes of different extents are different
    renderings, 0.23 apart here; the check is therefore made inside the one decode.)  Where that decode's two ends meet
    they are two renderings of neighbouring frames: the FS samples after the centre's end against the centre's first
    FS, 1e-3 as in tests/test_gpu_loop.py::test_circular_decode_continues_with_the_clips_start at the same halo.  A
    regenerated span elsewhere moves the cut, so no span holds that place; with every frame regenerated the cut is the
    wrap, the centre N samples at gen_start 0."""
    from audiolcm_amd.windows import ring_paste_cut, ring_paste_regions, seam_mask
    L, h, m, R = 64, 16, 16, 512
    wav = _recording(L)
    union = seam_mask(L, m).copy()
    extra = None
    if name == "span-where-the-cut-would-be":
        union[30:35] = True                         # frame 32 is where the seam alone puts the cut
    elif name == "all-regenerated":
        union[:] = True
    if name != "seam-as-wide-as-the-halo":
        extra = torch.from_numpy(union).float().expand(2, L).contiguous()
    a = ring_paste_cut(union, 1)
    assert a == {"seam-as-wide-as-the-halo": 32, "span-where-the-cut-would-be": 23, "all-regenerated": 0}[name]
    assert ring_paste_regions(union, h) == [("ring",)]
    out = pipe.loop_from(case["ctx"].cuda(), SEEDS, wav, seam_frames=m, mask=extra, window=T, overlap=OVERLAP,
                         halo_frames=h)
    assert out["regions"] == [("ring",)]
    got, z = out["wav"].cpu(), out["latent"]

    idx = (torch.arange(L + 2 * h, device="cuda") + a - h) % L
    dec = pipe.decode(z[:, :, idx].contiguous())["wav"].cpu()
    assert dec.shape == (2, (L + 2 * h) * FS)
    gen = torch.roll(dec[:, h * FS:(h + L) * FS], a * FS, dims=1)               # sample n of the ring
    regen = torch.from_numpy(np.repeat(union, FS))
    assert torch.equal(got[:, regen], gen[:, regen])                            # gen's bits inside regenerated frames
    err = rel_l2(dec[:, (h + L) * FS:(h + L + 1) * FS].numpy(), dec[:, h * FS:(h + 1) * FS].numpy())
    print(f"whole-ring paste, {name}: the decode's continuation past its centre against the centre's start {err:.2e}")
    assert err <= 1e-3
    if name == "all-regenerated":
        assert torch.equal(got, gen)
        return
    # the decode's two ends meet between frames a - 1 and a, among kept frames: the recording's bits, a frame either side
    lo, hi = (a - 1) * FS, (a + 1) * FS
    assert not union[a - 1] and not union[a] and torch.equal(got[:, lo:hi], wav[:, lo:hi])
    d = torch.from_numpy(np.repeat(~union, FS))     # kept frames: the recording's bits at least R from a regenerated one
    edge = torch.from_numpy(np.repeat(np.roll(union, 1) | np.roll(union, -1), FS))
    assert torch.equal(got[:, d & ~edge], wav[:, d & ~edge])


def test_encode_ring_is_the_centre_of_the_padded_encode(pipe):
    from audiolcm_amd import kernels, recipe
    L = 24
    wav = _recording(L).cuda()
    scale = float(pipe.model.scale_factor)
    for halo in (8, 32):                # 32 > L: the halo is the whole recording either side
        he = min(halo, L)
        padded = torch.cat([wav[:, (L - he) * FS:], wav, wav[:, :he * FS]], 1).contiguous()
        moments = pipe._encode(padded).parameters[:, :, he:he + L].float().contiguous()
        e0 = recipe.edit_noise(SEEDS, S, 20, L)[2].cuda()
        want = kernels.latent_init(None, moments=moments, e0=e0, scale=scale, want_x=False)[0]
        assert torch.equal(pipe._encode_ring(wav, SEEDS, S, True, halo), want)
        mode = kernels.latent_init(None, moments=moments, scale=scale, want_x=False)[0]
        assert torch.equal(pipe._encode_ring(wav, SEEDS, S, False, halo), mode)
    assert not torch.equal(want, pipe._encode_latent(wav, SEEDS, S))       # the line's encoding has two ends


def test_edit_loop_argument_errors(pipe, case):
    ctx, z = case["ctx"].cuda(), case["z0"][:, :, :60].contiguous().cuda()
    wav = _recording(60)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.edit_loop(ctx, SEEDS)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.edit_loop(ctx, SEEDS, wav=wav, latent=z)
    with pytest.raises(ValueError, match="at least 2"):
        pipe.edit_loop(ctx, SEEDS, latent=z[:, :, :1].contiguous())
    with pytest.raises(ValueError, match="at least 2"):
        pipe.loop_from(ctx, SEEDS, wav[:, :FS], seam_frames=1)
    with pytest.raises(ValueError, match="seam"):
        pipe.loop_from(ctx, SEEDS, wav, seam_frames=31)             # 2 * 31 > 60
    with pytest.raises(ValueError, match="seam"):
        pipe.loop_from(ctx, SEEDS, wav, seam_frames=0)
    with pytest.raises(ValueError, match="halo_frames"):
        pipe.loop_from(ctx, SEEDS, wav, seam_frames=4, halo_frames=1, fade_samples=513)
    with pytest.raises(ValueError, match="fade_samples"):
        pipe.loop_from(ctx, SEEDS, wav, seam_frames=4, fade_samples=16 * FS + 1)
    with pytest.raises(ValueError, match="keep_original"):
        pipe.edit_loop(ctx, SEEDS, latent=z, keep_original=True)
    from audiolcm_amd.audio_in import check_level
    for kw in (dict(out_sample_rate=48000), dict(level=check_level(-16.0)), dict(loop_fade_samples=64)):
        with pytest.raises(ValueError, match="keep_original"):
            pipe.edit_loop(ctx, SEEDS, wav=wav, mask=_seam(60), keep_original=True, **kw)
    with pytest.raises(ValueError, match="multiple of 5"):
        pipe.edit_loop(ctx, SEEDS, latent=z[:, :, :44].contiguous(), out_sample_rate=44100)
    with pytest.raises(ValueError, match="mask"):
        pipe.edit_loop(ctx, SEEDS, latent=z, mask=torch.zeros((2, 61)))
    with pytest.raises(ValueError, match="512"):
        pipe.edit_loop(ctx, SEEDS, wav=wav[:, :1000])
