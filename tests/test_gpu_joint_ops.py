"""alcm_lcm_step_joint through the C-ABI: the LCM step on one long latent whose overlapping windows went through the
DiT as one batch.

Exact where the kernel must reproduce a value (a frame under one window: the plain step; xw: prev's slices; the
gather-only form; either access width; any batch split), and relative L2 <= 1e-6 against a float64 restatement of the
definition where weighted sums stand against fp32 roundings (the bar tests/test_gpu_edit_ops.py states for the step
kernels)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

B, W, OVERLAP = 2, 40, 20
COEFFS = (0.7071, 0.7071, 0.99995, 2.5e-5, 0.9, 0.43589)  # sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev
# (L, starts): 16-byte path (every start a multiple of 4), element path with three windows on frames 30 .. 39, one window
LAYOUTS = {"vec": (72, (0, 20, 32)), "elem": (70, (0, 20, 30)), "one": (40, (0,))}
CHANNELS = [20, 5]   # 5: a channel group of 4 and a remainder of 1


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


@pytest.fixture(scope="module")
def data():
    """Per (channels, layout), once: x, eps, eps_u, noise, the weights, and the float64 restatement's inputs."""
    cache = {}

    def get(Cc, name):
        if (Cc, name) not in cache:
            from audiolcm_amd.pipeline import joint_weights
            L, starts = LAYOUTS[name]
            g = torch.Generator(device="cuda").manual_seed(100 * Cc + L)
            x, nz = (torch.randn((B, Cc, L), device="cuda", generator=g) for _ in range(2))
            eps, eu = (torch.randn((len(starts) * B, Cc, W), device="cuda", generator=g) for _ in range(2))
            wn = joint_weights(starts, W, L, OVERLAP)
            cover = np.zeros(L, dtype=np.int64)
            for s in starts:
                cover[s:s + W] += 1
            cache[(Cc, name)] = dict(x=x, nz=nz, eps=eps, eu=eu, wn=torch.from_numpy(wn.copy()).cuda(), wn_h=wn,
                                     starts=starts, L=L, cover=cover)
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
    prev = c[4] * den + c[5] * d["nz"].cpu().numpy().astype(np.float64) if use_nz else den
    xw = np.concatenate([prev[:, :, s:s + W] for s in d["starts"]], 0)
    return den, prev, xw


def _step_cfg(x, ec, eu, scale, nz):
    from audiolcm_amd._hip import check, lib, ptr, stream_handle
    prev, den = torch.empty_like(x), torch.empty_like(x)
    arr = (C.c_float * 6)(*COEFFS)
    check(lib().alcm_lcm_step_cfg(ptr(x), ptr(ec), ptr(eu), scale, ptr(nz), arr, ptr(prev), ptr(den), x.numel(),
                                  stream_handle()), "lcm_step_cfg")
    return prev, den


def _slices(t, starts):
    return torch.cat([t[:, :, s:s + W] for s in starts], 0)


@pytest.mark.parametrize("use_eu", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("use_nz", [True, False], ids=["noise", "last"])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_joint_step_matches_the_definition(K, data, Cc, name, use_nz, use_eu):
    d = data(Cc, name)
    nz, eu = (d["nz"] if use_nz else None), (d["eu"] if use_eu else None)
    prev, den, xw = K.lcm_step_joint(d["x"], d["eps"], nz, COEFFS, d["starts"], d["wn"], eps_uncond=eu, cfg_scale=3.0)
    torch.cuda.synchronize()
    den_r, prev_r, xw_r = _restated(d, use_nz, use_eu)
    errs = [rel_l2(a.cpu().numpy(), r) for a, r in ((den, den_r), (prev, prev_r), (xw, xw_r))]
    print(f"C={Cc} {name} noise={use_nz} cfg={use_eu}: den {errs[0]:.2e} prev {errs[1]:.2e} xw {errs[2]:.2e}")
    assert max(errs) <= 1e-6
    # xw is prev, window by window, bit for bit
    assert torch.equal(xw, _slices(prev, d["starts"]))
    if not use_nz:
        assert torch.equal(prev, den)
    # a frame under one window is that window's plain step, bit for bit
    seen = 0
    for k, s in enumerate(d["starts"]):
        single = torch.from_numpy(d["cover"][s:s + W] == 1).cuda()
        xs, ek = d["x"][:, :, s:s + W].contiguous(), d["eps"][k * B:(k + 1) * B]
        if use_eu:
            _, den_k = _step_cfg(xs, ek, d["eu"][k * B:(k + 1) * B], 3.0, None)
        else:
            _, den_k = K.lcm_step(xs, ek, None, COEFFS)
        assert torch.equal(den[:, :, s:s + W][:, :, single], den_k[:, :, single])
        seen += int(single.sum())
    assert seen == int((d["cover"] == 1).sum()) > 0


@pytest.mark.parametrize("Cc", CHANNELS)
def test_one_window_is_the_plain_step(K, data, Cc):
    d = data(Cc, "one")
    for nz in (d["nz"], None):
        prev, den, xw = K.lcm_step_joint(d["x"], d["eps"], nz, COEFFS, d["starts"], d["wn"])
        want_prev, want_den = K.lcm_step(d["x"], d["eps"], nz, COEFFS)
        assert torch.equal(prev, want_prev) and torch.equal(den, want_den) and torch.equal(xw, prev)
    prev, den, _ = K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"], eps_uncond=d["eu"],
                                    cfg_scale=3.0)
    want_prev, want_den = _step_cfg(d["x"], d["eps"], d["eu"], 3.0, d["nz"])
    assert torch.equal(prev, want_prev) and torch.equal(den, want_den)


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_gather_only_and_single_outputs(K, data, Cc, name):
    d = data(Cc, name)
    prev, den, xw = K.lcm_step_joint(d["x"], None, None, COEFFS, d["starts"], d["wn"])
    assert prev is None and den is None and torch.equal(xw, _slices(d["x"], d["starts"]))
    full = K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"])
    for i in range(3):
        want = [j == i for j in range(3)]
        got = K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"], want_prev=want[0],
                               want_den=want[1], want_xw=want[2])
        assert [g is not None for g in got] == want and torch.equal(got[i], full[i])


def _shifted(t):
    """The same values at an address that is 4 mod 16."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("Cc", CHANNELS)
def test_vector_and_element_paths_agree(K, data, Cc):
    from audiolcm_amd import _hip
    d = data(Cc, "vec")
    _hip.profile_begin()
    want = K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"], eps_uncond=d["eu"], cfg_scale=3.0)
    rows = [r["name"] for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]
    assert rows == ["alcm::lcm_step_joint_kernel<4>"]
    xs, es, us, ns = (_shifted(d[k]) for k in ("x", "eps", "eu", "nz"))
    assert all(t.data_ptr() % 16 == 4 for t in (xs, es, us, ns))
    outs = [_shifted(torch.zeros_like(w)) for w in want]
    _hip.profile_begin()
    got = K.lcm_step_joint(xs, es, ns, COEFFS, d["starts"], d["wn"], eps_uncond=us, cfg_scale=3.0, prev=outs[0],
                           den=outs[1], xw=outs[2])
    rows = [r["name"] for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]
    assert rows == ["alcm::lcm_step_joint_kernel<1>"]
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # the gather-only form too
    assert torch.equal(K.lcm_step_joint(xs, None, None, COEFFS, d["starts"], d["wn"])[2],
                       K.lcm_step_joint(d["x"], None, None, COEFFS, d["starts"], d["wn"])[2])


@pytest.mark.parametrize("name", ["vec", "elem"])
@pytest.mark.parametrize("Cc", CHANNELS)
def test_batch_of_two_is_two_batches_of_one(K, data, Cc, name):
    d = data(Cc, name)
    nk = len(d["starts"])
    full = K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"], eps_uncond=d["eu"], cfg_scale=3.0)
    for b in range(B):
        rows = lambda t: t.view(nk, B, Cc, W)[:, b].contiguous()   # noqa: E731  (row k * B + b of every window)
        one = K.lcm_step_joint(d["x"][b:b + 1].contiguous(), rows(d["eps"]), d["nz"][b:b + 1].contiguous(), COEFFS,
                               d["starts"], d["wn"], eps_uncond=rows(d["eu"]), cfg_scale=3.0)
        assert torch.equal(one[0], full[0][b:b + 1]) and torch.equal(one[1], full[1][b:b + 1])
        assert torch.equal(one[2], rows(full[2]))


def test_profile_row_counts_what_is_touched(K, data):
    from audiolcm_amd import _hip
    d = data(20, "vec")
    nk, L = len(d["starts"]), d["L"]
    _hip.profile_begin()
    K.lcm_step_joint(d["x"], d["eps"], d["nz"], COEFFS, d["starts"], d["wn"])
    row, = [r for r in _hip.profile_end() if "lcm_step_joint" in r["name"]]
    nl, nw = B * 20 * L, nk * B * 20 * W
    # x, noise, prev, den at the clip's length; eps and xw per window; the weights per window, frame and channel group
    assert row["launches"] == 1 and row["bytes"] == 4.0 * (4 * nl + 2 * nw + nk * W * B * 5)
    assert row["flops"] == 10.0 * nw + 3.0 * nl


def test_joint_step_bad_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd._hip import lib, ptr, stream_handle
    Cc, L = 2, 12
    x = torch.zeros((1, Cc, L), device="cuda")
    e = torch.zeros((2, Cc, 8), device="cuda")
    wn = torch.ones((2, 8), device="cuda")
    out = torch.full((1, Cc, L), 7.0, device="cuda")
    ow = torch.full((2, Cc, 8), 7.0, device="cuda")
    arr = (C.c_float * 6)(*COEFFS)
    Lb, s = lib(), stream_handle()
    px, pe, pw, po, pow_ = ptr(x), ptr(e), ptr(wn), ptr(out), ptr(ow)

    def st(*v):
        return (C.c_int * len(v))(*v)

    def call(x=px, eps=pe, eu=None, nz=None, co=arr, starts=st(0, 4), nk=2, wn=pw, prev=po, den=po, xw=pow_,
             dims=(1, Cc, L, 8)):
        return Lb.alcm_lcm_step_joint(x, eps, eu, 1.0, nz, co, starts, nk, wn, prev, den, xw, *dims, s)

    assert call(x=None) != 0 and call(wn=None) != 0 and call(co=None) != 0 and call(starts=None) != 0
    assert call(prev=None, den=None, xw=None) != 0                       # no output
    assert b"lcm_step_joint" in Lb.alcm_last_error()
    assert call(eps=None) != 0                                           # gather-only with prev / den
    assert call(eps=None, prev=None, den=None, nz=px) != 0               # gather-only with noise
    assert call(eps=None, prev=None, den=None, eu=pe) != 0               # gather-only with eps_u
    assert call(eps=None, prev=None, den=None, xw=None) != 0             # gather-only without xw
    for dims in ((-1, Cc, L, 8), (1, -Cc, L, 8), (1, Cc, -L, 8), (1, Cc, L, -8)):
        assert call(dims=dims) != 0
    assert call(nk=0) != 0 and call(nk=33, starts=st(*range(0, 132, 4))) != 0
    assert call(starts=st(4, 8)) != 0                                    # does not start at 0
    assert call(starts=st(0, 0)) != 0                                    # not strictly ascending
    assert call(starts=st(0, 9), dims=(1, Cc, 17, 8)) != 0               # frame 8 under no window
    assert call(starts=st(0, 4), dims=(1, Cc, 13, 8)) != 0               # does not end at L
    assert call(starts=st(0, 2)) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())          # nothing was launched
    for dims in ((0, Cc, L, 8), (1, 0, L, 8), (1, Cc, 0, 8), (1, Cc, L, 0)):
        assert call(dims=dims) == 0                                      # empty: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())
    assert call(prev=None, den=None) == 0                                # and the valid form runs
    torch.cuda.synchronize()
    assert bool((ow == 0.0).all())
