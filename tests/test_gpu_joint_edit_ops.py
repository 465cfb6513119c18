"""alcm_lcm_step_joint_edit through the C-ABI: the joint LCM step of overlapping windows with a known latent blended in
per frame.

Exact where the kernel must reproduce a value (mask 1: alcm_lcm_step_joint; one window: alcm_lcm_step_edit; mask 0: z0
and its re-noise; xw: prev's slices; either access width; any batch split), and relative L2 <= 1e-6 against a float64
restatement of the definition where weighted sums and the blend stand against fp32 roundings (the bar
tests/test_gpu_edit_ops.py and tests/test_gpu_joint_ops.py state for the step kernels).  Shapes and layouts are
tests/test_gpu_joint_ops.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

B, W, OVERLAP = 2, 40, 20
COEFFS = (0.7071, 0.7071, 0.99995, 2.5e-5, 0.9, 0.43589)  # sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev
# (L, starts): 16-byte path, element path with three windows on frames 30 .. 39, one window
LAYOUTS = {"vec": (72, (0, 20, 32)), "elem": (70, (0, 20, 30)), "one": (40, (0,))}
CHANNELS = [20, 5]   # 5: a channel group of 4 and a remainder of 1


def _mask(L):
    """Per clip.  Row 0: runs of 0 and 1 whose edges are no multiples of 4, so a 16-byte group mixes the two, and which
    cross the windows' overlaps; row 1: 0, 1 and 0.25."""
    m = np.zeros((B, L), dtype=np.float32)
    m[0, 3:17] = 1.0
    m[0, 22:35] = 1.0
    m[0, L - 5:L - 2] = 1.0
    m[1, :] = 0.25
    m[1, 6:13] = 0.0
    m[1, 25:38] = 1.0
    return m


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


@pytest.fixture(scope="module")
def data():
    """Per (channels, layout), once: x, eps, eps_u, noise, z0, the mask, the weights."""
    cache = {}

    def get(Cc, name):
        if (Cc, name) not in cache:
            from audiolcm_amd.pipeline import joint_weights
            L, starts = LAYOUTS[name]
            g = torch.Generator(device="cuda").manual_seed(100 * Cc + L)
            x, nz, z0 = (torch.randn((B, Cc, L), device="cuda", generator=g) for _ in range(3))
            eps, eu = (torch.randn((len(starts) * B, Cc, W), device="cuda", generator=g) for _ in range(2))
            wn = joint_weights(starts, W, L, OVERLAP)
            m = _mask(L)
            cache[(Cc, name)] = dict(x=x, nz=nz, z0=z0, eps=eps, eu=eu, wn=torch.from_numpy(wn.copy()).cuda(), wn_h=wn,
                                     starts=starts, L=L, m=torch.from_numpy(m).cuda(), m_h=m)
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
    for k, s in enumerate(d["starts"]):
        xs = x[:, :, s:s + W]
        x0 = (xs - c[1] * eps[k * B:(k + 1) * B]) / c[0]
        den[:, :, s:s + W] += d["wn_h"][k].astype(np.float64) * (c[3] * xs + c[2] * x0)
    m = d["m_h"].astype(np.float64)[:, None, :]
    den = m * den + (1.0 - m) * d["z0"].cpu().numpy().astype(np.float64)
    prev = c[4] * den + c[5] * d["nz"].cpu().numpy().astype(np.float64) if use_nz else den
    xw = np.concatenate([prev[:, :, s:s + W] for s in d["starts"]], 0)
    return den, prev, xw


def _slices(t, starts):
    return torch.cat([t[:, :, s:s + W] for s in starts], 0)


def _call(K, d, use_nz=True, use_eu=True, **kw):
    z0, mask = kw.pop("z0", d["z0"]), kw.pop("mask", d["m"])
    return K.lcm_step_joint_edit(d["x"], d["eps"], d["nz"] if use_nz else None, COEFFS, d["starts"], d["wn"], z0, mask,
                                 eps_uncond=d["eu"] if use_eu else None, cfg_scale=3.0, **kw)


@pytest.mark.parametrize("use_eu", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("use_nz", [True, False], ids=["noise", "last"])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_joint_edit_step_matches_the_definition(K, data, Cc, name, use_nz, use_eu):
    d = data(Cc, name)
    prev, den, xw = _call(K, d, use_nz, use_eu)
    torch.cuda.synchronize()
    den_r, prev_r, xw_r = _restated(d, use_nz, use_eu)
    errs = [rel_l2(a.cpu().numpy(), r) for a, r in ((den, den_r), (prev, prev_r), (xw, xw_r))]
    print(f"C={Cc} {name} noise={use_nz} cfg={use_eu}: den {errs[0]:.2e} prev {errs[1]:.2e} xw {errs[2]:.2e}")
    assert max(errs) <= 1e-6
    # xw is prev, window by window, bit for bit; without noise prev is den
    assert torch.equal(xw, _slices(prev, d["starts"]))
    if not use_nz:
        assert torch.equal(prev, den)
    # frames of mask 0: den is z0 and prev its re-noise, which is lcm_step_edit's value there, bit for bit
    keep = (d["m"] == 0)[:, None, :].expand_as(den)
    assert int(keep.sum()) > 0 and torch.equal(den[keep], d["z0"][keep])
    nz = d["nz"] if use_nz else None
    want_prev, _ = K.lcm_step_edit(d["z0"], torch.zeros_like(d["z0"]), nz, COEFFS, d["z0"], torch.zeros_like(d["m"]))
    assert torch.equal(prev[keep], want_prev[keep])
    # frames of mask 1: the open joint entry's value, bit for bit
    open_prev, open_den, _ = K.lcm_step_joint(d["x"], d["eps"], nz, COEFFS, d["starts"], d["wn"],
                                              eps_uncond=d["eu"] if use_eu else None, cfg_scale=3.0)
    regen = (d["m"] == 1)[:, None, :].expand_as(den)
    assert int(regen.sum()) > 0 and torch.equal(den[regen], open_den[regen]) and torch.equal(prev[regen], open_prev[regen])


@pytest.mark.parametrize("use_nz", [True, False], ids=["noise", "last"])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_mask_of_ones_is_the_open_joint_step(K, data, Cc, name, use_nz):
    d = data(Cc, name)
    got = _call(K, d, use_nz, True, mask=torch.ones_like(d["m"]))
    want = K.lcm_step_joint(d["x"], d["eps"], d["nz"] if use_nz else None, COEFFS, d["starts"], d["wn"],
                            eps_uncond=d["eu"], cfg_scale=3.0)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("use_eu", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("Cc", CHANNELS)
def test_one_window_is_the_edit_step(K, data, Cc, use_eu):
    d = data(Cc, "one")
    for nz in (True, False):
        prev, den, xw = _call(K, d, nz, use_eu)
        want_prev, want_den = K.lcm_step_edit(d["x"], d["eps"], d["nz"] if nz else None, COEFFS, d["z0"], d["m"],
                                              eps_uncond=d["eu"] if use_eu else None, cfg_scale=3.0)
        assert torch.equal(prev, want_prev) and torch.equal(den, want_den) and torch.equal(xw, prev)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_single_outputs(K, data, name):
    d = data(5, name)
    full = _call(K, d)
    for i in range(3):
        want = [j == i for j in range(3)]
        got = _call(K, d, want_prev=want[0], want_den=want[1], want_xw=want[2])
        assert [g is not None for g in got] == want and torch.equal(got[i], full[i])


def _shifted(t):
    """The same values at an address that is 4 mod 16."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def _rows(_hip):
    return [r["name"] for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]


@pytest.mark.parametrize("Cc", CHANNELS)
def test_vector_and_element_paths_agree(K, data, Cc):
    from audiolcm_amd import _hip
    d = data(Cc, "vec")
    _hip.profile_begin()
    want = _call(K, d)
    assert _rows(_hip) == ["alcm::lcm_step_joint_edit_kernel<4>"]
    # every input off the 16-byte grid
    sh = {k: _shifted(d[k]) for k in ("x", "eps", "eu", "nz", "z0", "m")}
    assert all(t.data_ptr() % 16 == 4 for t in sh.values())
    outs = [_shifted(torch.zeros_like(w)) for w in want]
    _hip.profile_begin()
    got = K.lcm_step_joint_edit(sh["x"], sh["eps"], sh["nz"], COEFFS, d["starts"], d["wn"], sh["z0"], sh["m"],
                                eps_uncond=sh["eu"], cfg_scale=3.0, prev=outs[0], den=outs[1], xw=outs[2])
    assert _rows(_hip) == ["alcm::lcm_step_joint_edit_kernel<1>"]
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # z0 or the mask alone off the grid takes the element path too, with the same bits
    for key in ("z0", "m"):
        _hip.profile_begin()
        got = _call(K, d, **{"z0" if key == "z0" else "mask": sh[key]})
        assert _rows(_hip) == ["alcm::lcm_step_joint_edit_kernel<1>"]
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    # and so does a layout whose starts are no multiples of 4
    _hip.profile_begin()
    _call(K, data(Cc, "elem"))
    assert _rows(_hip) == ["alcm::lcm_step_joint_edit_kernel<1>"]


@pytest.mark.parametrize("name", ["vec", "elem"])
@pytest.mark.parametrize("Cc", CHANNELS)
def test_batch_of_two_is_two_batches_of_one(K, data, Cc, name):
    d = data(Cc, name)
    nk = len(d["starts"])
    full = _call(K, d)
    for b in range(B):
        rows = lambda t: t.view(nk, B, Cc, W)[:, b].contiguous()   # noqa: E731  (row k * B + b of every window)
        cut = lambda t: t[b:b + 1].contiguous()                    # noqa: E731
        one = K.lcm_step_joint_edit(cut(d["x"]), rows(d["eps"]), cut(d["nz"]), COEFFS, d["starts"], d["wn"],
                                    cut(d["z0"]), cut(d["m"]), eps_uncond=rows(d["eu"]), cfg_scale=3.0)
        assert torch.equal(one[0], full[0][b:b + 1]) and torch.equal(one[1], full[1][b:b + 1])
        assert torch.equal(one[2], rows(full[2]))


@pytest.mark.parametrize("Cc", CHANNELS)
def test_profile_row_counts_what_is_touched(K, data, Cc):
    from audiolcm_amd import _hip
    d = data(Cc, "vec")
    nk, L = len(d["starts"]), d["L"]
    _hip.profile_begin()
    _call(K, d, True, False)
    row, = [r for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]
    nl, nw, cg = B * Cc * L, nk * B * Cc * W, -(-Cc // 4)
    # the open entry's bytes (x, noise, prev, den at the clip's length; eps and xw per window; the weights per window,
    # frame and channel group), plus z0 at the clip's length, plus the mask per frame and channel group
    assert row["name"] == "alcm::lcm_step_joint_edit_kernel<4>" and row["launches"] == 1
    assert row["bytes"] == 4.0 * (4 * nl + 2 * nw + nk * W * B * cg) + 4.0 * nl + 4.0 * B * L * cg
    assert row["flops"] == 10.0 * nw + 3.0 * nl


def test_joint_edit_step_bad_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
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

    def call(x=px, eps=pe, eu=None, nz=None, co=arr, starts=st(0, 4), nk=2, wn=pw, z0=px, mask=pm, prev=po, den=po,
             xw=pow_, dims=(1, Cc, L, 8)):
        return Lb.alcm_lcm_step_joint_edit(x, eps, eu, 1.0, nz, co, starts, nk, wn, z0, mask, prev, den, xw, *dims, s)

    def refused(**kw):
        return call(**kw) != 0 and b"lcm_step_joint_edit" in Lb.alcm_last_error()

    assert refused(x=None) and refused(wn=None) and refused(co=None) and refused(starts=None)
    assert refused(eps=None) and refused(z0=None) and refused(mask=None)     # no gather-only form, and what it adds
    assert refused(eps=None, prev=None, den=None)
    assert refused(prev=None, den=None, xw=None)                             # no output
    for dims in ((-1, Cc, L, 8), (1, -Cc, L, 8), (1, Cc, -L, 8), (1, Cc, L, -8)):
        assert refused(dims=dims)
    assert refused(nk=0) and refused(nk=33, starts=st(*range(0, 132, 4)))
    assert refused(starts=st(4, 8))                                          # does not start at 0
    assert refused(starts=st(0, 0))                                          # not strictly ascending
    assert refused(starts=st(0, 9), dims=(1, Cc, 17, 8))                     # frame 8 under no window
    assert refused(starts=st(0, 4), dims=(1, Cc, 13, 8))                     # does not end at L
    assert refused(starts=st(0, 2))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())              # nothing was launched
    for dims in ((0, Cc, L, 8), (1, 0, L, 8), (1, Cc, 0, 8), (1, Cc, L, 0)):
        assert call(dims=dims) == 0                                          # empty: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())
    assert call(prev=None, den=None) == 0                                    # and the valid form runs
    torch.cuda.synchronize()
    assert bool((ow == 0.0).all())
