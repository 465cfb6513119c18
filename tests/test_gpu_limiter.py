"""alcm_limiter through ``kernels.limit`` against the float64 restatement of ``tests/_limiter_ref.py``: steps 1 to 7 of
the definition as plain NumPy with a Python loop for the release.

Bar: |gpu - ref| <= 4 * 2^-24 * |ref| per sample, plus the smallest normal.  The kernel's fp64 curve differs from the
loop's only by association (the attack is a prefix sum over a tile, the release a scan of composed maps), at about
1e-13; that can flip fl32(y) by one ulp and the product by one or two more; 4 ulp is that plus margin.  Also: no |out|
exceeds the ceiling, exactly; the output is fl32(x g) bit for bit before the first ramp begins; a clip that never
passes the ceiling has alcm_wave_gain's bits; a clip's bits depend on neither B, the strides, the alignment nor its
neighbours; in place equals out of place.

Shapes are the smallest that meet every path: N = 2 SPAN + 37 (three workgroups per clip, a partial last chunk), with
peaks at both ends of the clip and either side of a span's edge, N of 1, of 50 (under the look-ahead) and of SPAN
exactly, La of 0, 1 and 1024 (the kernel's limit), a of 0 and of exp(-1 / 160000).

Measured on an MI355X: in every case here, the batched, late-peak and oversampled ones included, no sample's bits
differ from the restatement's at all (share 0, worst error 0); the share is printed per case (``pytest -s``).  The
kernel's tile arithmetic restated in NumPy (``_limiter_ref.tile_attack``, checked in ``test_limiter_host.py``) puts its
attack curve within 1.0e-13 of the restatement's, which at these lengths never moved an fp32 rounding."""
import functools
import math

import numpy as np
import pytest
import torch

import _limiter_ref as ref

pytestmark = pytest.mark.gpu

RATE = 16000
A0 = math.exp(-1.0 / 1600.0)
G = np.float32(2.5)
C = ref.ceiling_of(-1.0)


def _span():
    from audiolcm_amd import limiter
    return limiter.SPAN


@functools.lru_cache(maxsize=None)
def _case(n, La, a):
    """Once per shape: the clip, the restatement's output and curves (read-only)."""
    x, spikes = ref.edge_signal(n, _span(), 80)
    out, d = ref.limiter(x, G, C, La, a)
    for v in (x, out, d["u"], d["e"]):
        v.setflags(write=False)
    return x, out, d


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip
    _hip.require_device(0)
    return torch.device("cuda")


def _limit(dev, x, g, La, a, **kw):
    from audiolcm_amd import kernels
    xs = torch.from_numpy(np.atleast_2d(x).copy()).to(dev)
    gs = torch.from_numpy(np.atleast_1d(np.asarray(g, np.float32)).copy()).to(dev)
    return kernels.limit(xs, gs, float(C), La, a, **kw).cpu().numpy()


def _check(name, got, want):
    ok = ref.within(got, want)
    diff = float((got.view(np.uint32) != want.view(np.uint32)).mean())
    worst = float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want.astype(np.float64)), 1e-30)).max())
    print(f"{name}: {diff:.2e} of the samples differ in bits, worst {worst / 2.0 ** -24:.2f} ulp-units of 2^-24")
    assert ok.all(), (name, int((~ok).sum()), worst)
    assert np.abs(got).max() <= C


def _cases():
    S = 2048
    big = 2 * S + 37
    return [("main", big, 80, A0), ("n1", 1, 80, A0), ("n50", 50, 80, A0), ("span", S, 80, A0), ("la0", big, 0, A0),
            ("la1", big, 1, A0), ("la1024", big, 1024, A0), ("a0", big, 80, 0.0),
            ("slow", big, 80, math.exp(-1.0 / 160000.0))]


@pytest.mark.parametrize("name,n,La,a", _cases(), ids=[c[0] for c in _cases()])
def test_limit_matches_the_float64_restatement(dev, name, n, La, a):
    assert _span() == 2048                                      # _cases spells the span out for the ids
    x, want, d = _case(n, La, a)
    if name == "main":                                          # the issue's prototype: 408 over, lowest gain 0.396
        assert abs(int((d["e"] > C).sum()) - 408) <= 12 and abs(d["y"].min() - 0.396) < 1e-3
    got = _limit(dev, x, G, La, a)[0]
    _check(name, got, want)


def test_untouched_until_the_first_ramp_and_a_quiet_clip_is_wave_gain(dev):
    """Two spans of ones before a peak in the third: bit-equal to fl32(x g) up to La before it.  And a clip that never
    passes the ceiling: alcm_wave_gain's bits, which are fl32(x g)."""
    from audiolcm_amd import _hip, kernels
    n, La = 2 * _span() + 37, 80
    t = np.arange(n) / RATE
    x = (0.2 * np.sin(2 * np.pi * 220.0 * t) + 0.02 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    quiet = x.copy()
    first = 2 * _span() + 5
    x[first] = -0.9
    want, d = ref.limiter(x, G, C, La, A0)
    assert int(np.argmax(d["e"] > C)) == first and (d["e"] > C).sum() == 1
    got = _limit(dev, x, G, La, A0)[0]
    _check("late", got, want)
    assert (got[:first - La].view(np.uint32) == d["u"][:first - La].view(np.uint32)).all()

    xs, gs = torch.from_numpy(quiet[None]).to(dev), torch.tensor([2.5], device=dev)
    wg = torch.empty_like(xs)
    _hip.check(_hip.lib().alcm_wave_gain(_hip.ptr(xs), _hip.ptr(gs), _hip.ptr(wg), 1, n, n, n, _hip.stream_handle()))
    lim = kernels.limit(xs, gs, float(C), La, A0)
    assert torch.equal(lim.view(torch.int32), wg.view(torch.int32))
    assert (wg.cpu().numpy().view(np.uint32) == (quiet * G).view(np.uint32)).all()


def test_a_clip_depends_on_neither_batch_stride_nor_alignment(dev):
    """B = 3 with three gains, one of which never limits, rows n + 7 apart from a base one element off 16 bytes, into an
    output laid out the same way: each clip bit-equal to its own B = 1 aligned run.  And in place equals out of place."""
    from audiolcm_amd import kernels
    n, La = 2 * _span() + 37, 80
    x = _case(n, La, A0)[0].copy()
    gains = np.array([2.5, 0.5, 1.7], np.float32)
    assert np.abs(x * gains[1]).max() <= C < np.abs(x * gains[2]).max()
    alone = [_limit(dev, x, g, La, A0)[0] for g in gains]
    ld = n + 7
    buf = torch.zeros(3 * ld + 1, device=dev)
    obuf = torch.full((3 * ld + 1,), 7.0, device=dev)
    xs = buf[1:].as_strided((3, n), (ld, 1))
    xs.copy_(torch.from_numpy(x).to(dev).expand(3, n))
    out = obuf[1:].as_strided((3, n), (ld, 1))
    assert xs.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    gs = torch.from_numpy(gains).to(dev)
    kernels.limit(xs, gs, float(C), La, A0, out=out)
    got = out.cpu().numpy()
    for b in range(3):
        assert (got[b].view(np.uint32) == alone[b].view(np.uint32)).all(), b
    assert (alone[1].view(np.uint32) == (x * gains[1]).view(np.uint32)).all()
    pad = obuf.cpu().numpy()
    assert pad[0] == 7.0 and (pad[1:].reshape(3, ld)[:, n:] == 7.0).all()           # nothing written between the rows
    # aligned and batched: the 16-byte path gives the same bits
    xa = torch.from_numpy(x).to(dev).expand(3, n).contiguous()
    assert n % 4 != 0                                                               # rows of an odd length: element path
    xa4 = torch.zeros((3, n + 3), device=dev)[:, :n]
    xa4.copy_(xa)
    assert xa4.stride(0) % 4 == 0 and xa4.data_ptr() % 16 == 0
    got4 = kernels.limit(xa4, gs, float(C), La, A0).cpu().numpy()
    for b in range(3):
        assert (got4[b].view(np.uint32) == alone[b].view(np.uint32)).all(), b
    # in place
    kernels.limit(xa4, gs, float(C), La, A0, out=xa4)
    assert (xa4.cpu().numpy().view(np.uint32) == got4.view(np.uint32)).all()
    kernels.limit(xs, gs, float(C), La, A0, out=xs)
    assert (xs.cpu().numpy().view(np.uint32) == got4.view(np.uint32)).all()


@pytest.mark.parametrize("os_", [1, 4])
def test_an_oversampled_copy_raises_the_envelope(dev, os_):
    """env exceeds |u| between the samples at chosen places: the limiter turns down there, as the restatement does."""
    from audiolcm_amd import kernels
    n, La = 2 * _span() + 37, 80
    x = _case(n, La, A0)[0]
    g = np.float32(1.7)
    env = np.repeat(x, os_).astype(np.float32)
    for p in (3, _span() - 2, _span() + 1, 3000, n - 1):
        env[p * os_ + os_ - 1] = 0.75 if p % 2 else -0.75                          # 0.75 * 1.7 = 1.275 > c
    want, d = ref.limiter(x, g, C, La, A0, env, os_)
    plain = ref.limiter(x, g, C, La, A0)[0]
    assert (d["e"] > np.abs(d["u"])).sum() >= 4 and (want != plain).sum() > 5 * La
    xs, gs = torch.from_numpy(x[None].copy()).to(dev), torch.tensor([float(g)], device=dev)
    got = kernels.limit(xs, gs, float(C), La, A0, env=torch.from_numpy(env[None]).to(dev)).cpu().numpy()[0]
    _check(f"env os={os_}", got, want)
    # the copy one element off alignment: element loads, same bits
    ebuf = torch.zeros(env.size + 1, device=dev)
    ebuf[1:].copy_(torch.from_numpy(env).to(dev))
    got1 = kernels.limit(xs, gs, float(C), La, A0, env=ebuf[1:][None]).cpu().numpy()[0]
    assert (got1.view(np.uint32) == got.view(np.uint32)).all()
