"""alcm_lcm_step_ring and alcm_wave_loop through the C-ABI: the joint LCM step on a ring of L frames, and the crop that
closes a loop's seam.

As tests/test_gpu_joint_ops.py for the open entry: exact where the kernel must reproduce a value (xw: prev gathered
with the wrap; a frame under one window: the plain step; the gather-only form; either access width; any batch split),
and relative L2 <= 1e-6 against a float64 restatement of the definition where weighted sums stand against fp32
roundings.  wave_loop: the copied samples and out[0] bit for bit, the fade within 1e-6 absolute of float64 on magnitudes
<= 1 (three fp32 roundings: the bar tests/test_gpu_paste_ops.py states for the same fma form)."""
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


@pytest.fixture(scope="module")
def data():
    """Per (channels, layout), once: x, eps, eps_u, noise, the weights, and the ring's frame indices per window."""
    cache = {}

    def get(Cc, name):
        if (Cc, name) not in cache:
            from audiolcm_amd.pipeline import ring_weights
            L, W, ov, starts = LAYOUTS[name]
            g = torch.Generator(device="cuda").manual_seed(100 * Cc + L)
            x, nz = (torch.randn((B, Cc, L), device="cuda", generator=g) for _ in range(2))
            eps, eu = (torch.randn((len(starts) * B, Cc, W), device="cuda", generator=g) for _ in range(2))
            wn = ring_weights(starts, W, L, ov)
            frames = [(s + np.arange(W)) % L for s in starts]
            cover = np.zeros(L, dtype=np.int64)
            for f in frames:
                cover[f] += 1
            cache[(Cc, name)] = dict(x=x, nz=nz, eps=eps, eu=eu, wn=torch.from_numpy(wn.copy()).cuda(), wn_h=wn,
                                     starts=starts, L=L, W=W, cover=cover, frames=frames,
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
    prev = c[4] * den + c[5] * d["nz"].cpu().numpy().astype(np.float64) if use_nz else den
    xw = np.concatenate([prev[:, :, f] for f in d["frames"]], 0)
    return den, prev, xw


def _step_cfg(x, ec, eu, scale, nz):
    from audiolcm_amd._hip import check, lib, ptr, stream_handle
    prev, den = torch.empty_like(x), torch.empty_like(x)
    arr = (C.c_float * 6)(*COEFFS)
    check(lib().alcm_lcm_step_cfg(ptr(x), ptr(ec), ptr(eu), scale, ptr(nz), arr, ptr(prev), ptr(den), x.numel(),
                                  stream_handle()), "lcm_step_cfg")
    return prev, den


def _gathered(t, d):
    """t (B, C, L) in window layout (K * B, C, W), with the wrap."""
    return torch.cat([t[:, :, f] for f in d["frames_d"]], 0)


def _ring(K, d, eps, nz, **kw):
    return K.lcm_step_joint(d["x"], eps, nz, COEFFS, d["starts"], d["wn"], ring=True, **kw)


@pytest.mark.parametrize("use_eu", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("use_nz", [True, False], ids=["noise", "last"])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_ring_step_matches_the_definition(K, data, Cc, name, use_nz, use_eu):
    d = data(Cc, name)
    nz, eu = (d["nz"] if use_nz else None), (d["eu"] if use_eu else None)
    prev, den, xw = _ring(K, d, d["eps"], nz, eps_uncond=eu, cfg_scale=3.0)
    torch.cuda.synchronize()
    den_r, prev_r, xw_r = _restated(d, use_nz, use_eu)
    errs = [rel_l2(a.cpu().numpy(), r) for a, r in ((den, den_r), (prev, prev_r), (xw, xw_r))]
    print(f"ring C={Cc} {name} noise={use_nz} cfg={use_eu}: den {errs[0]:.2e} prev {errs[1]:.2e} xw {errs[2]:.2e}")
    assert max(errs) <= 1e-6
    # xw is prev gathered with the wrap, bit for bit
    assert torch.equal(xw, _gathered(prev, d))
    if not use_nz:
        assert torch.equal(prev, den)
    # a frame under one window is that window's plain step, bit for bit
    seen = 0
    for k, f in enumerate(d["frames_d"]):
        single = torch.from_numpy(d["cover"][d["frames"][k]] == 1).cuda()
        xs, ek = d["x"][:, :, f].contiguous(), d["eps"][k * B:(k + 1) * B]
        if use_eu:
            _, den_k = _step_cfg(xs, ek, d["eu"][k * B:(k + 1) * B], 3.0, None)
        else:
            _, den_k = K.lcm_step(xs, ek, None, COEFFS)
        assert torch.equal(den[:, :, f][:, :, single], den_k[:, :, single])
        seen += int(single.sum())
    assert seen == int((d["cover"] == 1).sum())
    assert (seen > 0) == (name == "elem")        # "vec" and "full": every frame is under two windows


def test_layouts_cover_what_they_claim(data):
    assert (data(5, "full")["cover"] == 2).all()
    vec = data(5, "vec")
    assert vec["frames"][2].tolist() == list(range(16, 24)) + list(range(0, 8))     # the last window wraps
    assert (vec["cover"] == 2).all()
    elem = data(5, "elem")
    assert elem["frames"][2][-1] == 6 and set(elem["cover"].tolist()) == {1, 2}


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_gather_only_and_single_outputs(K, data, Cc, name):
    d = data(Cc, name)
    prev, den, xw = _ring(K, d, None, None)
    assert prev is None and den is None and torch.equal(xw, _gathered(d["x"], d))
    full = _ring(K, d, d["eps"], d["nz"])
    for i in range(3):
        want = [j == i for j in range(3)]
        got = _ring(K, d, d["eps"], d["nz"], want_prev=want[0], want_den=want[1], want_xw=want[2])
        assert [g is not None for g in got] == want and torch.equal(got[i], full[i])


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
    want = _ring(K, d, d["eps"], d["nz"], eps_uncond=d["eu"], cfg_scale=3.0)
    rows = [r["name"] for r in _hip.profile_end() if "lcm_step" in r["name"]]
    assert rows == ["alcm::lcm_step_ring_kernel<4>"]
    xs, es, us, ns = (_shifted(d[k]) for k in ("x", "eps", "eu", "nz"))
    assert all(t.data_ptr() % 16 == 4 for t in (xs, es, us, ns))
    outs = [_shifted(torch.zeros_like(w)) for w in want]
    _hip.profile_begin()
    got = K.lcm_step_joint(xs, es, ns, COEFFS, d["starts"], d["wn"], eps_uncond=us, cfg_scale=3.0, prev=outs[0],
                           den=outs[1], xw=outs[2], ring=True)
    rows = [r["name"] for r in _hip.profile_end() if "lcm_step" in r["name"]]
    assert rows == ["alcm::lcm_step_ring_kernel<1>"]
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # the gather-only form too
    assert torch.equal(K.lcm_step_joint(xs, None, None, COEFFS, d["starts"], d["wn"], ring=True)[2],
                       _ring(K, d, None, None)[2])


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("Cc", CHANNELS)
def test_batch_of_two_is_two_batches_of_one(K, data, Cc, name):
    d = data(Cc, name)
    nk, W = len(d["starts"]), d["W"]
    full = _ring(K, d, d["eps"], d["nz"], eps_uncond=d["eu"], cfg_scale=3.0)
    for b in range(B):
        rows = lambda t: t.view(nk, B, Cc, W)[:, b].contiguous()   # noqa: E731  (row k * B + b of every window)
        one = K.lcm_step_joint(d["x"][b:b + 1].contiguous(), rows(d["eps"]), d["nz"][b:b + 1].contiguous(), COEFFS,
                               d["starts"], d["wn"], eps_uncond=rows(d["eu"]), cfg_scale=3.0, ring=True)
        assert torch.equal(one[0], full[0][b:b + 1]) and torch.equal(one[1], full[1][b:b + 1])
        assert torch.equal(one[2], rows(full[2]))


def test_an_open_plan_gives_the_open_entrys_bits(K):
    """Where no window wraps (the last one ends at L) the ring entry and the open one run the same chain; here on the
    16-byte path, with frames under one window (the open entry's own test holds those to the plain step's bits)."""
    from audiolcm_amd.pipeline import joint_weights
    g = torch.Generator(device="cuda").manual_seed(7)
    x, nz = (torch.randn((B, 5, 24), device="cuda", generator=g) for _ in range(2))
    eps = torch.randn((2 * B, 5, 16), device="cuda", generator=g)
    wn = torch.from_numpy(joint_weights((0, 8), 16, 24, 8).copy()).cuda()
    a = K.lcm_step_joint(x, eps, nz, COEFFS, (0, 8), wn)
    b = K.lcm_step_joint(x, eps, nz, COEFFS, (0, 8), wn, ring=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_profile_rows_count_what_is_touched(K, data):
    from audiolcm_amd import _hip
    d = data(20, "vec")
    nk, L, W = len(d["starts"]), d["L"], d["W"]
    nl, nw = B * 20 * L, nk * B * 20 * W
    _hip.profile_begin()
    _ring(K, d, d["eps"], d["nz"])
    rows = _hip.profile_end()
    row, = [r for r in rows if "lcm_step" in r["name"] or "gather" in r["name"]]
    # x, noise, prev, den at the ring's length; eps and xw per window; the weights per window, frame and channel group
    assert row["name"] == "alcm::lcm_step_ring_kernel<4>" and row["launches"] == 1
    assert row["bytes"] == 4.0 * (4 * nl + 2 * nw + nk * W * B * 5)
    assert row["flops"] == 10.0 * nw + 3.0 * nl
    _hip.profile_begin()
    _ring(K, d, None, None)
    _ring(K, data(20, "elem"), None, None)
    rows = {r["name"]: r for r in _hip.profile_end() if "lcm_step" in r["name"] or "gather" in r["name"]}
    assert sorted(rows) == ["alcm::ring_gather_kernel<1>", "alcm::ring_gather_kernel<4>"]
    assert rows["alcm::ring_gather_kernel<4>"]["launches"] == 1
    assert rows["alcm::ring_gather_kernel<4>"]["bytes"] == 4.0 * (nl + nw)
    assert rows["alcm::ring_gather_kernel<4>"]["flops"] == 0.0


def test_ring_step_bad_arguments():
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

    def call(x=px, eps=pe, eu=None, nz=None, co=arr, starts=st(0, 6), nk=2, wn=pw, prev=po, den=po, xw=pow_,
             dims=(1, Cc, L, 8)):
        return Lb.alcm_lcm_step_ring(x, eps, eu, 1.0, nz, co, starts, nk, wn, prev, den, xw, *dims, s)

    assert call(x=None) != 0 and call(wn=None) != 0 and call(co=None) != 0 and call(starts=None) != 0
    assert call(prev=None, den=None, xw=None) != 0                       # no output
    assert b"lcm_step_ring" in Lb.alcm_last_error()
    assert call(eps=None) != 0                                           # gather-only with prev / den
    assert call(eps=None, prev=None, den=None, nz=px) != 0               # gather-only with noise
    assert call(eps=None, prev=None, den=None, eu=pe) != 0               # gather-only with eps_u
    assert call(eps=None, prev=None, den=None, xw=None) != 0             # gather-only without xw
    for dims in ((-1, Cc, L, 8), (1, -Cc, L, 8), (1, Cc, -L, 8), (1, Cc, L, -8)):
        assert call(dims=dims) != 0
    assert call(nk=1, starts=st(0)) != 0                                 # one window cannot close a ring
    assert call(nk=0) != 0 and call(nk=33, starts=st(*range(0, 132, 4)), dims=(1, Cc, 136, 8)) != 0
    assert call(dims=(1, Cc, 7, 8)) != 0                                 # a window longer than the ring
    assert call(starts=st(4, 8)) != 0                                    # does not start at 0
    assert call(starts=st(0, 0)) != 0                                    # not strictly ascending
    assert call(starts=st(0, 12)) != 0                                   # a start on L
    assert call(starts=st(0, 9), dims=(1, Cc, 17, 8)) != 0               # frame 8 under no window
    assert call(starts=st(0, 4), dims=(1, Cc, 13, 8)) != 0               # frame 12 under no window: across the wrap
    assert b"lcm_step_ring" in Lb.alcm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())          # nothing was launched
    for dims in ((0, Cc, L, 8), (1, 0, L, 8), (1, Cc, 0, 8), (1, Cc, L, 0)):
        assert call(dims=dims) == 0                                      # empty: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ow == 7.0).all())
    assert call(prev=None, den=None) == 0                                # and the valid forms run
    assert call(starts=st(0, 4), prev=None, den=None) == 0               # the last window ends on L
    torch.cuda.synchronize()
    assert bool((ow == 0.0).all())


# ---------------------------------------------------------------------------------------------------- wave_loop
N_LOOP = 2048
FADES = [0, 7, 512]
# (start, row length): 16-byte accesses; a start that is no multiple of 4 (the element path)
CROPS = {"aligned": (1024, 1024 + N_LOOP + 1024), "misaligned": (1023, 1023 + N_LOOP + 513)}


@pytest.fixture(scope="module")
def ext():
    out = {}
    for name, (start, n) in CROPS.items():
        h = np.random.default_rng(n).uniform(-1, 1, (B, n)).astype(np.float32)
        out[name] = (h, torch.from_numpy(h).cuda())
    return out


@pytest.mark.parametrize("R", FADES)
@pytest.mark.parametrize("name", list(CROPS))
def test_wave_loop_matches_the_definition(K, ext, name, R):
    from audiolcm_amd import _hip
    from audiolcm_amd.kernels import paste_ramp_host
    start, _ = CROPS[name]
    h, d = ext[name]
    _hip.profile_begin()
    got = K.wave_loop(d, start, N_LOOP, R)
    rows = [r for r in _hip.profile_end() if "wave_loop" in r["name"]]
    assert [r["name"] for r in rows] == [f"alcm::wave_loop_kernel<{4 if name == 'aligned' else 1}>"]
    assert rows[0]["launches"] == 1
    assert rows[0]["bytes"] == 4.0 * (2 * B * N_LOOP + 2 * B * max(R - 1, 0) + (B if R else 0))
    assert rows[0]["flops"] == 3.0 * B * max(R - 1, 0)
    got = got.cpu().numpy()
    assert got.shape == (B, N_LOOP)
    own = h[:, start:start + N_LOOP]
    assert np.array_equal(got[:, max(R, 0):], own[:, max(R, 0):])       # the copy region, bit for bit
    if R == 0:
        assert np.array_equal(got, own)                                  # a plain crop
        return
    assert np.array_equal(got[:, 0], h[:, start + N_LOOP])               # the sample after the period's last one
    ramp = paste_ramp_host(R).numpy().astype(np.float64)
    a = own[:, :R].astype(np.float64)
    c = h[:, start + N_LOOP:start + N_LOOP + R].astype(np.float64)
    want = a + ramp * (c - a)
    worst = float(np.abs(got[:, 1:R] - want[:, 1:R]).max())
    print(f"wave_loop {name} R={R}: max abs error of the fade {worst:.2e}")
    assert worst <= 1e-6
    assert not np.array_equal(got[:, 1:R], own[:, 1:R])                  # and the fade does something


def test_wave_loop_paths_agree_and_rows_are_independent(K, ext):
    h, d = ext["aligned"]
    start = CROPS["aligned"][0]
    want = K.wave_loop(d, start, N_LOOP, 512)
    buf = torch.empty(d.numel() + 1, device="cuda")
    buf[1:].copy_(d.reshape(-1))
    shifted = buf[1:].view(d.shape)                                      # the same values at an address 4 mod 16
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(K.wave_loop(shifted, start, N_LOOP, 512), want)
    for b in range(B):
        assert torch.equal(K.wave_loop(d[b:b + 1].contiguous(), start, N_LOOP, 512), want[b:b + 1])
    # the fade may take the whole period, and may end on the row's last sample
    whole = K.wave_loop(d[:, :2 * N_LOOP].contiguous(), 0, N_LOOP, N_LOOP).cpu().numpy()
    assert np.array_equal(whole[:, 0], h[:, N_LOOP])


def test_wave_loop_bad_arguments(K, ext):
    from audiolcm_amd._hip import lib, ptr, stream_handle
    from audiolcm_amd.kernels import paste_ramp
    _, d = ext["aligned"]
    n = d.shape[1]
    out = torch.full((B, N_LOOP), 7.0, device="cuda")
    ramp = paste_ramp(512, "cuda")
    Lb, s = lib(), stream_handle()

    def call(e=ptr(d), r=ptr(ramp), o=ptr(out), b=B, row=n, start=1024, N=N_LOOP, R=512):
        return Lb.alcm_wave_loop(e, r, o, b, row, start, N, R, s)

    assert call(e=None) != 0 and call(o=None) != 0 and call(r=None) != 0
    assert b"wave_loop" in Lb.alcm_last_error()
    assert call(b=-1) != 0 and call(row=-1) != 0 and call(N=-1) != 0 and call(R=-1) != 0
    assert call(start=-4) != 0                                           # start >= 0
    assert call(N=256, R=257) != 0                                       # R <= N
    assert call(R=1025) != 0                                             # start + N + R <= row length
    assert call(start=2048, R=4) != 0
    assert call(start=n + 4, N=0, R=0) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # nothing was launched
    assert call(b=0) == 0 and call(N=0, R=0) == 0                        # empty: no launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0 and call(r=None, R=1) == 0 and call(r=None, R=0) == 0   # and the valid forms run
    torch.cuda.synchronize()
    assert torch.equal(out, d[:, 1024:1024 + N_LOOP])
    for bad in (dict(start=-1), dict(fade_samples=N_LOOP + 1), dict(start=n - N_LOOP, fade_samples=1)):
        with pytest.raises(ValueError, match="wave_loop"):
            K.wave_loop(d, **{"start": 1024, "N": N_LOOP, "fade_samples": 0, **bad})
