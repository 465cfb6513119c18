"""alcm_lcm_step_ring_edit through the C-ABI: the joint LCM step on a ring of L frames with a known latent blended in per
frame, the step of a loop made from a recording.

As tests/test_gpu_loop_ops.py for the ring and tests/test_gpu_joint_edit_ops.py for the line's edit form: exact where the
kernel must reproduce a value (xw: prev gathered with the wrap; frames of mask 0: z0; a mask of ones: the ring entry; an
open plan: the line's edit entry; either access width; any batch split), and relative L2 <= 1e-6 against a float64
restatement of the definition where weighted sums stand against fp32 roundings (the bar both siblings state)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

B = 2
COEFFS = (0.7071, 0.7071, 0.99995, 2.5e-5, 0.9, 0.43589)  # sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev
# (L, W, overlap, starts): the 16-byte path with a last window that wraps; the element path; a ring of one window's
# length, every frame under both windows
LAYOUTS = {"vec": (24, 16, 8, (0, 8, 16)), "elem": (23, 15, 7, (0, 7, 15)), "full": (16, 16, 8, (0, 8))}
CHANNELS = [20, 5]   # 5: a channel group of 4 and a remainder of 1


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


def _mask(L):
    """(B, L): zeros, ones and a fractional value; clip 0 regenerates a run across the wrap, clip 1 one inside."""
    m = np.zeros((B, L), dtype=np.float32)
    m[0, L - 5:] = 1.0
    m[0, :4] = 1.0
    m[0, 4] = 0.25
    m[1, 6:13] = 1.0
    m[1, 13] = 0.625
    return m


@pytest.fixture(scope="module")
def data():
    """Per (channels, layout), once: x, eps, eps_u, noise, z0, the mask, the weights, the ring's frames per window."""
    cache = {}

    def get(Cc, name):
        if (Cc, name) not in cache:
            from audiolcm_amd.pipeline import ring_weights
            L, W, ov, starts = LAYOUTS[name]
            g = torch.Generator(device="cuda").manual_seed(100 * Cc + L + 1)
            x, nz, z0 = (torch.randn((B, Cc, L), device="cuda", generator=g) for _ in range(3))
            eps, eu = (torch.randn((len(starts) * B, Cc, W), device="cuda", generator=g) for _ in range(2))
            wn = ring_weights(starts, W, L, ov)
            frames = [(s + np.arange(W)) % L for s in starts]
            m = _mask(L)
            cache[(Cc, name)] = dict(x=x, nz=nz, z0=z0, eps=eps, eu=eu, wn=torch.from_numpy(wn.copy()).cuda(), wn_h=wn,
                                     starts=starts, L=L, W=W, frames=frames, m_h=m, m=torch.from_numpy(m).cuda(),
                                     frames_d=[torch.from_numpy(f).cuda() for f in frames])
        return cache[(Cc, name)]
    return get


def _restated(d, use_nz, use_eu, cfg=3.0):
    """The definition in float64 numpy: (den, prev, xw)."""
    c = [float(np.float32(v)) for v in COEFFS]
    x, eps = d["x"].cpu().numpy().astype(np.float64), d["eps"].cpu().numpy().astype(np.float64)
    if use_eu:
        eu = d["eu"].cpu().numpy().astype(np.float64)
        eps = eu + float(np.float32(cfg)) * (eps - eu)
    den = np.zeros_like(x)
    for k, f in enumerate(d["frames"]):
        xs = x[:, :, f]
        x0 = (xs - c[1] * eps[k * B:(k + 1) * B]) / c[0]
        den[:, :, f] += d["wn_h"][k].astype(np.float64) * (c[3] * xs + c[2] * x0)
    m = d["m_h"].astype(np.float64)[:, None, :]
    den = m * den + (1.0 - m) * d["z0"].cpu().numpy().astype(np.float64)
    prev = c[4] * den + c[5] * d["nz"].cpu().numpy().astype(np.float64) if use_nz else den
    xw = np.concatenate([prev[:, :, f] for f in d["frames"]], 0)
    return den, prev, xw


def _gathered(t, d):
    """t (B, C, L) in window layout (K * B, C, W), with the wrap."""
    return torch.cat([t[:, :, f] for f in d["frames_d"]], 0)


def _edit(K, d, nz, mask=None, **kw):
    return K.lcm_step_ring_edit(d["x"], d["eps"], nz, COEFFS, d["starts"], d["wn"], d["z0"],
                                d["m"] if mask is None else mask, **kw)


def _rows(_hip):
    return [r["name"] for r in _hip.profile_end() if "lcm_step" in r["name"] or "gather" in r["name"]]


@pytest.mark.parametrize("use_eu", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("use_nz", [True, False], ids=["noise", "last"])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_ring_edit_step_matches_the_definition(K, data, Cc, name, use_nz, use_eu):
    d = data(Cc, name)
    nz, eu = (d["nz"] if use_nz else None), (d["eu"] if use_eu else None)
    prev, den, xw = _edit(K, d, nz, eps_uncond=eu, cfg_scale=3.0)
    torch.cuda.synchronize()
    den_r, prev_r, xw_r = _restated(d, use_nz, use_eu)
    errs = [rel_l2(a.cpu().numpy(), r) for a, r in ((den, den_r), (prev, prev_r), (xw, xw_r))]
    print(f"ring edit C={Cc} {name} noise={use_nz} cfg={use_eu}: den {errs[0]:.2e} prev {errs[1]:.2e} xw {errs[2]:.2e}")
    assert max(errs) <= 1e-6
    assert torch.equal(xw, _gathered(prev, d))              # xw is prev gathered with the wrap, bit for bit
    if not use_nz:
        assert torch.equal(prev, den)
    kept = (d["m"] == 0)[:, None, :].expand_as(den)          # frames of mask 0 are z0, bit for bit
    assert bool(kept.any()) and torch.equal(den[kept], d["z0"][kept])
    ones = (d["m"] == 1)[:, None, :].expand_as(den)          # frames of mask 1 are the ring entry's, bit for bit
    ring = K.lcm_step_joint(d["x"], d["eps"], nz, COEFFS, d["starts"], d["wn"], eps_uncond=eu, cfg_scale=3.0, ring=True)
    assert bool(ones.any()) and torch.equal(den[ones], ring[1][ones]) and torch.equal(prev[ones], ring[0][ones])
    frac = ((d["m"] > 0) & (d["m"] < 1))[:, None, :].expand_as(den)
    assert bool(frac.any()) and not torch.equal(den[frac], ring[1][frac]) and not torch.equal(den[frac], d["z0"][frac])


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_a_mask_of_ones_is_the_ring_entry(K, data, Cc, name):
    d = data(Cc, name)
    got = _edit(K, d, d["nz"], mask=torch.ones_like(d["m"]), eps_uncond=d["eu"], cfg_scale=3.0)
    want = K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"], eps_uncond=d["eu"], cfg_scale=3.0,
                            ring=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    full = _edit(K, d, d["nz"])
    for i in range(3):      # any single output
        want1 = [j == i for j in range(3)]
        one = _edit(K, d, d["nz"], want_prev=want1[0], want_den=want1[1], want_xw=want1[2])
        assert [o is not None for o in one] == want1 and torch.equal(one[i], full[i])


@pytest.mark.parametrize("Cc", CHANNELS)
def test_an_open_plan_gives_the_lines_edit_entrys_bits(K, Cc):
    """Where no window wraps (the last one ends at L) the ring's edit entry and the line's run the same chain: on the
    16-byte path and on the element path."""
    from audiolcm_amd.pipeline import joint_weights
    for L, W, ov, starts in ((24, 16, 8, (0, 8)), (23, 15, 7, (0, 8))):
        g = torch.Generator(device="cuda").manual_seed(7 + L)
        x, nz, z0 = (torch.randn((B, Cc, L), device="cuda", generator=g) for _ in range(3))
        eps = torch.randn((2 * B, Cc, W), device="cuda", generator=g)
        wn = torch.from_numpy(joint_weights(starts, W, L, ov).copy()).cuda()
        m = torch.from_numpy(_mask(L)).cuda()
        a = K.lcm_step_joint_edit(x, eps, nz, COEFFS, starts, wn, z0, m)
        b = K.lcm_step_ring_edit(x, eps, nz, COEFFS, starts, wn, z0, m)
        assert all(torch.equal(p, q) for p, q in zip(a, b))


def _shifted(t):
    """The same values at an address that is 4 mod 16."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("name", ["vec", "full"])
@pytest.mark.parametrize("Cc", CHANNELS)
def test_vector_and_element_paths_agree(K, data, Cc, name):
    from audiolcm_amd import _hip
    d = data(Cc, name)
    _hip.profile_begin()
    want = _edit(K, d, d["nz"], eps_uncond=d["eu"], cfg_scale=3.0)
    assert _rows(_hip) == ["alcm::lcm_step_ring_edit_kernel<4>"]
    sh = {k: _shifted(d[k]) for k in ("x", "eps", "eu", "nz", "z0", "m")}
    assert all(t.data_ptr() % 16 == 4 for t in sh.values())
    outs = [_shifted(torch.zeros_like(w)) for w in want]
    _hip.profile_begin()
    got = K.lcm_step_ring_edit(sh["x"], sh["eps"], sh["nz"], COEFFS, d["starts"], d["wn"], sh["z0"], sh["m"],
                               eps_uncond=sh["eu"], cfg_scale=3.0, prev=outs[0], den=outs[1], xw=outs[2])
    assert _rows(_hip) == ["alcm::lcm_step_ring_edit_kernel<1>"]
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    for key in ("z0", "m"):     # one shifted pointer is enough to leave the 16-byte path
        _hip.profile_begin()
        got = K.lcm_step_ring_edit(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"],
                                   sh["z0"] if key == "z0" else d["z0"], sh["m"] if key == "m" else d["m"],
                                   eps_uncond=d["eu"], cfg_scale=3.0)
        assert _rows(_hip) == ["alcm::lcm_step_ring_edit_kernel<1>"]
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    _hip.profile_begin()
    _edit(K, data(Cc, "elem"), None)
    assert _rows(_hip) == ["alcm::lcm_step_ring_edit_kernel<1>"]


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_batch_of_two_is_two_batches_of_one(K, data, Cc, name):
    d = data(Cc, name)
    nk, W = len(d["starts"]), d["W"]
    full = _edit(K, d, d["nz"], eps_uncond=d["eu"], cfg_scale=3.0)
    for b in range(B):
        rows = lambda t: t.view(nk, B, Cc, W)[:, b].contiguous()   # noqa: E731  (row k * B + b of every window)
        cut = lambda t: t[b:b + 1].contiguous()                    # noqa: E731
        one = K.lcm_step_ring_edit(cut(d["x"]), rows(d["eps"]), cut(d["nz"]), COEFFS, d["starts"], d["wn"],
                                   cut(d["z0"]), cut(d["m"]), eps_uncond=rows(d["eu"]), cfg_scale=3.0)
        assert torch.equal(one[0], full[0][b:b + 1]) and torch.equal(one[1], full[1][b:b + 1])
        assert torch.equal(one[2], rows(full[2]))


def test_profile_row_counts_what_is_touched(K, data):
    from audiolcm_amd import _hip
    d = data(20, "vec")
    nk, L, W = len(d["starts"]), d["L"], d["W"]
    nl, nw = B * 20 * L, nk * B * 20 * W
    _hip.profile_begin()
    _edit(K, d, d["nz"])
    row, = [r for r in _hip.profile_end() if "lcm_step" in r["name"] or "gather" in r["name"]]
    # x, noise, prev, den and z0 at the ring's length; eps and xw per window; the weights per window, frame and channel
    # group, and the mask per frame and channel group (5 groups of 4 channels)
    assert row["name"] == "alcm::lcm_step_ring_edit_kernel<4>" and row["launches"] == 1
    assert row["bytes"] == 4.0 * (5 * nl + 2 * nw + nk * W * B * 5 + B * L * 5)
    assert row["flops"] == 10.0 * nw + 3.0 * nl
    _hip.profile_begin()
    _edit(K, d, None, eps_uncond=d["eu"], cfg_scale=3.0, want_xw=False)
    row, = [r for r in _hip.profile_end() if "lcm_step" in r["name"]]
    assert row["bytes"] == 4.0 * (4 * nl + 2 * nw + nk * W * B * 5 + B * L * 5) and row["flops"] == 10.0 * nw


def test_ring_edit_step_bad_arguments(K):
    from audiolcm_amd._hip import lib, ptr, stream_handle
    Cc, L = 2, 12
    x = torch.zeros((1, Cc, L), device="cuda")
    e = torch.zeros((2, Cc, 8), device="cuda")
    wn = torch.ones((2, 8), device="cuda")
    m = torch.ones((1, L), device="cuda")
    out = torch.full((1, Cc, L), 7.0, device="cuda")
    ow = torch.full((2, Cc, 8), 7.0, device="cuda")
    arr = (C.c_float * 6)(*COEFFS)
    Lb, s = lib(), stream_handle()
    px, pe, pw, pm, po, pow_ = ptr(x), ptr(e), ptr(wn), ptr(m), ptr(out), ptr(ow)

    def st(*v):
        return (C.c_int * len(v))(*v)

    def call(x=px, eps=pe, eu=None, nz=None, co=arr, starts=st(0, 6), nk=2, wn=pw, z0=px, mask=pm, prev=po, den=po,
             xw=pow_, dims=(1, Cc, L, 8)):
        return Lb.alcm_lcm_step_ring_edit(x, eps, eu, 1.0, nz, co, starts, nk, wn, z0, mask, prev, den, xw, *dims, s)

    def refused(**kw):
        return call(**kw) != 0 and b"lcm_step_ring_edit" in Lb.alcm_last_error()

    # the edit form's rules
    assert refused(z0=None) and refused(mask=None) and refused(eps=None)
    assert refused(eps=None, prev=None, den=None)                        # no gather-only form
    assert refused(x=None) and refused(wn=None) and refused(co=None) and refused(starts=None)
    assert refused(prev=None, den=None, xw=None)                         # no output
    for dims in ((-1, Cc, L, 8), (1, -Cc, L, 8), (1, Cc, -L, 8), (1, Cc, L, -8)):
        assert refused(dims=dims)
    # the ring's rules
    assert refused(nk=1, starts=st(0))                                   # one window cannot close a ring
    assert refused(nk=0) and refused(nk=33, starts=st(*range(0, 132, 4)), dims=(1, Cc, 136, 8))
    assert refused(dims=(1, Cc, 7, 8))                                   # a window longer than the ring
    assert refused(starts=st(4, 8))                                      # does not start at 0
    assert refused(starts=st(0, 0))                                      # not strictly ascending
    assert refused(starts=st(0, 12))                                     # a start on L
    assert refused(starts=st(0, 9), dims=(1, Cc, 17, 8))                 # frame 8 under no window
    assert refused(starts=st(0, 4), dims=(1, Cc, 13, 8))                 # frame 12 under no window: across the wrap
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())          # nothing was launched
    for dims in ((0, Cc, L, 8), (1, 0, L, 8), (1, Cc, 0, 8), (1, Cc, L, 0)):
        assert call(dims=dims) == 0                                      # empty: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())
    assert call() == 0 and call(starts=st(0, 4)) == 0                    # and the valid forms run
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((ow == 0.0).all())
    # the Python wrappers: the open entry keeps refusing a ring with z0, the new one takes it
    with pytest.raises(ValueError, match="ring"):
        K.lcm_step_joint(x, e, None, COEFFS, (0, 6), wn, ring=True, z0=x, mask=m)
    assert K.lcm_step_ring_edit(x, e, None, COEFFS, (0, 6), wn, x, m)[0].shape == x.shape
