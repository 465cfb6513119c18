"""The two device entry points of audio-conditioned generation, through the C-ABI: alcm_lcm_step_edit (the LCM step
blended per latent frame with a known latent) and alcm_latent_init (encoder moments -> the sampler's start).

Exact where the kernel must reproduce a value (mask 1: the plain step; mask 0: the known latent; pass-through), and
relative L2 <= 1e-6 against the fp32 torch expression where one fused multiply-add stands against two roundings
(<= 2^-24 per term) or expf against torch.exp (a few ulp)."""
import ctypes as C

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

# (B, C, T): 16-byte path, element path with a ragged tail, the smallest case, and two shapes that exceed one pass of the
# edit kernels' grid (1024 blocks x 64 items; an item is 4 frames, or 1 on the element path, of up to 4 channels: 150,000
# and 600,003 items) and of alcm_lcm_step's (4096 x 256 elements): the grid-stride loops of both, on either path
SHAPES = [(3, 20, 40), (3, 20, 37), (1, 1, 1), (3, 2, 200000), (3, 2, 200001)]
COEFFS = (0.7071, 0.7071, 0.99995, 2.5e-5, 0.9, 0.43589)  # sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


@pytest.fixture(scope="module")
def data():
    """Per shape, once: x, eps, eps_u, noise, z0 and the plain / guided step results they are compared with."""
    cache = {}

    def get(K, shape):
        if shape not in cache:
            g = torch.Generator(device="cuda").manual_seed(sum(shape))
            x, eps, eu, nz, z0 = (torch.randn(shape, device="cuda", generator=g) for _ in range(5))
            d = dict(x=x, eps=eps, eu=eu, nz=nz, z0=z0, g=g)
            d["plain"] = K.lcm_step(x, eps, nz, COEFFS)
            d["plain_last"] = K.lcm_step(x, eps, None, COEFFS)
            d["cfg"] = _step_cfg(x, eps, eu, 3.0, nz)
            cache[shape] = d
        return cache[shape]
    return get


def _step_cfg(x, ec, eu, scale, nz):
    from audiolcm_amd._hip import check, lib, ptr, stream_handle
    prev, den = torch.empty_like(x), torch.empty_like(x)
    arr = (C.c_float * 6)(*COEFFS)
    check(lib().alcm_lcm_step_cfg(ptr(x), ptr(ec), ptr(eu), scale, ptr(nz), arr, ptr(prev), ptr(den), x.numel(),
                                  stream_handle()), "lcm_step_cfg")
    return prev, den


@pytest.mark.parametrize("shape", SHAPES)
def test_step_edit_mask_one_is_the_plain_step(K, data, shape):
    d = data(K, shape)
    ones = torch.ones((shape[0], shape[2]), device="cuda")
    prev, den = K.lcm_step_edit(d["x"], d["eps"], d["nz"], COEFFS, d["z0"], ones)
    assert torch.equal(prev, d["plain"][0]) and torch.equal(den, d["plain"][1])
    prev, den = K.lcm_step_edit(d["x"], d["eps"], None, COEFFS, d["z0"], ones)   # the final step: no noise
    assert torch.equal(prev, d["plain_last"][0]) and torch.equal(den, d["plain_last"][1]) and torch.equal(prev, den)
    prev, den = K.lcm_step_edit(d["x"], d["eps"], d["nz"], COEFFS, d["z0"], ones, eps_uncond=d["eu"], cfg_scale=3.0)
    assert torch.equal(prev, d["cfg"][0]) and torch.equal(den, d["cfg"][1])
    assert not torch.equal(d["cfg"][1], d["plain"][1])


@pytest.mark.parametrize("shape", SHAPES)
def test_step_edit_mask_zero_keeps_z0(K, data, shape):
    d = data(K, shape)
    zeros = torch.zeros((shape[0], shape[2]), device="cuda")
    prev, den = K.lcm_step_edit(d["x"], d["eps"], d["nz"], COEFFS, d["z0"], zeros)
    assert torch.equal(den, d["z0"])
    ref = COEFFS[4] * d["z0"] + COEFFS[5] * d["nz"]
    err = rel_l2(prev.cpu().numpy(), ref.cpu().numpy())
    print(f"{shape} mask 0 prev: {err:.2e}")
    assert err <= 1e-6
    prev, den = K.lcm_step_edit(d["x"], d["eps"], None, COEFFS, d["z0"], zeros)
    assert torch.equal(den, d["z0"]) and torch.equal(prev, d["z0"])


@pytest.mark.parametrize("shape", SHAPES)
def test_step_edit_binary_mask(K, data, shape):
    d = data(K, shape)
    B, _, T = shape
    m = (torch.rand((B, T), device="cuda", generator=d["g"]) < 0.5).float()
    if T > 1:
        m[:, 0], m[:, -1] = 0.0, 1.0   # both values present, at the row edges
    for eu, ref in ((None, d["plain"]), (d["eu"], d["cfg"])):
        prev, den = K.lcm_step_edit(d["x"], d["eps"], d["nz"], COEFFS, d["z0"], m, eps_uncond=eu, cfg_scale=3.0)
        regen = (m == 1)[:, None, :].expand(shape)
        assert torch.equal(den[~regen], d["z0"][~regen])
        assert torch.equal(den[regen], ref[1][regen]) and torch.equal(prev[regen], ref[0][regen])


@pytest.mark.parametrize("shape", SHAPES)
def test_step_edit_fractional_mask(K, data, shape):
    d = data(K, shape)
    B, _, T = shape
    m = torch.where(torch.rand((B, T), device="cuda", generator=d["g"]) < 0.5, 0.25, 0.5)
    prev, den = K.lcm_step_edit(d["x"], d["eps"], d["nz"], COEFFS, d["z0"], m)
    mm = m[:, None, :]
    den_ref = mm * d["plain"][1] + (1 - mm) * d["z0"]
    prev_ref = COEFFS[4] * den_ref + COEFFS[5] * d["nz"]
    e_den = rel_l2(den.cpu().numpy(), den_ref.cpu().numpy())
    e_prev = rel_l2(prev.cpu().numpy(), prev_ref.cpu().numpy())
    print(f"{shape} fractional mask: den {e_den:.2e} prev {e_prev:.2e}")
    assert e_den <= 1e-6 and e_prev <= 1e-6


def test_step_edit_single_output_and_unaligned_views(K, data):
    """One output pointer null; and 4-byte-aligned views of a T % 4 == 0 shape take the element path with the same
    results."""
    from audiolcm_amd._hip import check, lib, ptr, stream_handle
    shape = (3, 20, 40)
    d = data(K, shape)
    m = (torch.rand((3, 40), device="cuda", generator=d["g"]) < 0.5).float()
    want = K.lcm_step_edit(d["x"], d["eps"], d["nz"], COEFFS, d["z0"], m)
    arr = (C.c_float * 6)(*COEFFS)
    for which in (0, 1):
        out = torch.empty_like(d["x"])
        check(lib().alcm_lcm_step_edit(ptr(d["x"]), ptr(d["eps"]), None, 1.0, ptr(d["nz"]), arr, ptr(d["z0"]), ptr(m),
                                       ptr(out) if which == 0 else None, ptr(out) if which == 1 else None, 3, 20, 40,
                                       stream_handle()), "lcm_step_edit")
        assert torch.equal(out, want[which])

    def shifted(t):  # the same values at an address that is 4 mod 16
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(t.shape)
    xs = shifted(d["x"])
    assert xs.data_ptr() % 16 == 4
    got = K.lcm_step_edit(xs, d["eps"], d["nz"], COEFFS, d["z0"], m)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_step_edit_bad_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd._hip import lib, ptr, stream_handle
    x = torch.zeros((1, 2, 4), device="cuda")
    m = torch.zeros((1, 4), device="cuda")
    arr = (C.c_float * 6)(*COEFFS)
    L, s, p = lib(), stream_handle(), ptr(x)
    assert L.alcm_lcm_step_edit(None, p, None, 1.0, None, arr, p, ptr(m), p, p, 1, 2, 4, s) != 0
    assert L.alcm_lcm_step_edit(p, None, None, 1.0, None, arr, p, ptr(m), p, p, 1, 2, 4, s) != 0
    assert L.alcm_lcm_step_edit(p, p, None, 1.0, None, None, p, ptr(m), p, p, 1, 2, 4, s) != 0
    assert L.alcm_lcm_step_edit(p, p, None, 1.0, None, arr, None, ptr(m), p, p, 1, 2, 4, s) != 0
    assert L.alcm_lcm_step_edit(p, p, None, 1.0, None, arr, p, None, p, p, 1, 2, 4, s) != 0
    assert L.alcm_lcm_step_edit(p, p, None, 1.0, None, arr, p, ptr(m), None, None, 1, 2, 4, s) != 0
    assert b"lcm_step_edit" in L.alcm_last_error()
    for bct in ((-1, 2, 4), (1, -2, 4), (1, 2, -4)):
        assert L.alcm_lcm_step_edit(p, p, None, 1.0, None, arr, p, ptr(m), p, p, *bct, s) != 0
    assert L.alcm_lcm_step_edit(p, p, None, 1.0, None, arr, p, ptr(m), p, p, 0, 2, 4, s) == 0   # empty: no launch


# ---------------------------------------------------------------------------- alcm_latent_init
def _moments(shape, g):
    """Encoder-like moments (B, 2C, T) whose logvar leaves [-30, 20] on both sides."""
    B, Cc, T = shape
    mom = torch.randn((B, 2 * Cc, T), device="cuda", generator=g)
    lv = mom[:, Cc:]
    lv.mul_(3.0)
    flat = lv.reshape(-1)
    idx = torch.arange(flat.numel(), device="cuda")
    lo, hi = idx % 7 == 0, idx % 7 == 3
    vals = torch.where(lo, torch.full_like(flat, -41.0), torch.where(hi, torch.full_like(flat, 23.5), flat))
    mom[:, Cc:] = vals.view(B, Cc, T)
    return mom


@pytest.mark.parametrize("shape", SHAPES)
def test_latent_init_matches_the_posterior_math(K, data, shape):
    from audiolcm_amd.models import DiagonalGaussianDistribution
    d = data(K, shape)
    B, Cc, T = shape
    mom = _moments(shape, d["g"])
    assert (mom[:, Cc:] < -30).any() and (mom[:, Cc:] > 20).any() or shape == (1, 1, 1)
    post = DiagonalGaussianDistribution(mom)
    e0, n0 = d["eps"], d["nz"]
    scale, keep, regen = 0.75, (0.6, 0.8), (0.3, 0.95)
    m = torch.where(torch.rand((B, T), device="cuda", generator=d["g"]) < 0.5, 0.0, 1.0)
    if T > 1:
        m[:, 1] = 0.25
    z_ref = scale * (post.mean + post.std * e0)
    mm = m[:, None, :]
    x_ref = mm * (regen[0] * z_ref + regen[1] * n0) + (1 - mm) * (keep[0] * z_ref + keep[1] * n0)
    z0, x = K.latent_init(n0, keep, regen, moments=mom, e0=e0, scale=scale, mask=m)
    ez, ex = rel_l2(z0.cpu().numpy(), z_ref.cpu().numpy()), rel_l2(x.cpu().numpy(), x_ref.cpu().numpy())
    print(f"{shape} latent_init: z0 {ez:.2e} x {ex:.2e}")
    assert ez <= 1e-6 and ex <= 1e-6
    # no mask: the kept pair everywhere
    _, x = K.latent_init(n0, keep, regen, moments=mom, e0=e0, scale=scale)
    assert rel_l2(x.cpu().numpy(), (keep[0] * z_ref + keep[1] * n0).cpu().numpy()) <= 1e-6
    # e0 NULL: the posterior mode, one multiply
    z0, x = K.latent_init(n0, keep, regen, moments=mom, scale=scale, mask=m)
    assert torch.equal(z0, scale * post.mode())
    # either output alone
    z_only, none = K.latent_init(None, moments=mom, scale=scale, want_x=False)
    assert none is None and torch.equal(z_only, z0)
    none, x_only = K.latent_init(n0, keep, regen, moments=mom, scale=scale, mask=m, want_z0=False)
    assert none is None and torch.equal(x_only, x)


@pytest.mark.parametrize("shape", SHAPES)
def test_latent_init_pass_through_and_pure_noise(K, data, shape):
    d = data(K, shape)
    B, _, T = shape
    n0 = d["nz"]
    ones = torch.ones((B, T), device="cuda")
    # a given latent passes through bit for bit (e0 and scale are ignored); mask 1 with (0, 1) gives the noise itself
    z0, x = K.latent_init(n0, (0.6, 0.8), (0.0, 1.0), z0=d["z0"], e0=d["eps"], scale=0.75, mask=ones)
    assert torch.equal(z0, d["z0"]) and torch.equal(x, n0)
    zeros = torch.zeros((B, T), device="cuda")
    _, x = K.latent_init(n0, (0.6, 0.8), (0.0, 1.0), z0=d["z0"], mask=zeros)
    assert rel_l2(x.cpu().numpy(), (0.6 * d["z0"] + 0.8 * n0).cpu().numpy()) <= 1e-6


def test_latent_init_bad_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd._hip import lib, ptr, stream_handle
    mom = torch.zeros((1, 4, 4), device="cuda")
    z = torch.zeros((1, 2, 4), device="cuda")
    L, s, pm, pz = lib(), stream_handle(), ptr(mom), ptr(z)
    co = (1.0, 0.0, 0.0, 1.0)
    assert L.alcm_latent_init(None, None, None, 1.0, pz, None, *co, pz, pz, 1, 2, 4, s) != 0      # no input
    assert L.alcm_latent_init(pm, pz, None, 1.0, pz, None, *co, pz, pz, 1, 2, 4, s) != 0          # both inputs
    assert L.alcm_latent_init(pm, None, None, 1.0, pz, None, *co, None, None, 1, 2, 4, s) != 0    # no output
    assert L.alcm_latent_init(pm, None, None, 1.0, None, None, *co, None, pz, 1, 2, 4, s) != 0    # x without noise
    assert b"latent_init" in L.alcm_last_error()
    for bct in ((-1, 2, 4), (1, -2, 4), (1, 2, -4)):
        assert L.alcm_latent_init(pm, None, None, 1.0, pz, None, *co, pz, pz, *bct, s) != 0
    assert L.alcm_latent_init(pm, None, None, 1.0, pz, None, *co, pz, pz, 1, 2, 0, s) == 0        # empty: no launch
