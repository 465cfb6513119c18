"""alcm_resample through the C-ABI and ``kernels.resample`` against a float64 numpy restatement of its definition
(include/audiolcm_hip.h, audiolcm_amd/resample.py), written here:

  y[n] = sum_k h(k + first - r / up) * xm[floor(n * down / up) + first + k],  r = (n * down) mod up,
  xm the channel mean of x and 0 outside [0, N_in), N_out = ceil(N_in * up / down).

Every output, edges included, is held to 1e-5 * max|x|.  The kernel's arithmetic (fp32 taps, one fp32 fmaf chain in
rising k) differs from float64 by at most 8e-7 for |x| <= 1 (tests/test_resample_host.py restates it on the host); the
worst case of any fp32 summation order is ntaps * 2^-24 * sum|h| ~ 3e-5; a wrong tap, phase or offset shows at 1e-3 or
more.  With a channel mean the input gains one more fp32 rounding (6e-8 * sum|h| ~ 1.4e-7), inside the same bound."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (32000, 16000), (8000, 16000), (16000, 22050),
         (16000, 44100), (16000, 48000)]
ZEROS, BETA, ROLLOFF = 32, 9.0, 0.92
TILE = 1024          # outputs per workgroup for every pair here (alcm_resample.hip: 256 threads x 4)
TOL = 1e-5


def _params(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    fcn = ROLLOFF * min(rate_in, rate_out) / (2.0 * rate_in)
    hw = ZEROS / (2.0 * fcn)
    return up, down, fcn, hw, -math.floor(hw), 2 * math.floor(hw) + 2


def _h(t, fcn, hw):
    inside = np.abs(t) <= hw
    u = np.where(inside, t / hw, 0.0)
    return np.where(inside, 2.0 * fcn * np.sinc(2.0 * fcn * t) * np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA), 0.0)


def _ref(xm, pair, n=None):
    """float64 outputs ``n`` (default: all) of the mono float64 clip xm (N_in,)."""
    up, down, fcn, hw, first, ntaps = _params(*pair)
    n_in = xm.shape[0]
    n = np.arange(-(-n_in * up // down), dtype=np.int64) if n is None else np.asarray(n, dtype=np.int64)
    pos, r = n * down // up, n * down % up
    k = np.arange(ntaps, dtype=np.int64)[None, :]
    taps = _h(k + first - r[:, None].astype(np.float64) / up, fcn, hw)
    idx = pos[:, None] + first + k
    ok = (idx >= 0) & (idx < n_in)
    return np.einsum("nk,nk->n", taps, np.where(ok, xm[np.clip(idx, 0, n_in - 1)], 0.0))


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


def _clip(B, n_in, ch, seed):
    x = np.random.default_rng(seed).uniform(-1, 1, (B, n_in, ch)).astype(np.float32)
    return x, x.astype(np.float64).mean(2)


def _run(K, x, pair, ch):
    xd = torch.from_numpy(x).cuda()
    return K.resample(xd if ch > 1 else xd[:, :, 0].contiguous(), pair[0], pair[1], channels=ch).cpu().numpy()


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("pair", PAIRS)
def test_matches_the_definition(K, pair, ch):
    up, down, fcn, hw, first, ntaps = _params(*pair)
    n_in = 5003 * down // up
    n_out = -(-n_in * up // down)
    assert 4 * TILE < n_out < 5 * TILE and n_out % 4 and n_out % TILE       # several tiles and a partial one
    x, xm = _clip(2, n_in, ch, 11)
    got = _run(K, x, pair, ch)
    assert got.shape == (2, n_out) and got.dtype == np.float32
    err = max(float(np.abs(got[b] - _ref(xm[b], pair)).max()) for b in range(2))
    print(f"resample {pair} ch={ch}: max abs error {err:.2e} (bound {TOL * np.abs(x).max():.2e})")
    assert err <= TOL * np.abs(x).max()


@pytest.mark.parametrize("pair", [(48000, 16000), (16000, 44100)])
def test_inputs_shorter_than_the_filter(K, pair):
    ntaps = _params(*pair)[5]
    for n_in in (1, 2, ntaps // 2, ntaps + 1):
        x, xm = _clip(2, n_in, 1, n_in)
        got = _run(K, x, pair, 1)
        ref = np.stack([_ref(xm[b], pair) for b in range(2)])
        assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL * np.abs(x).max(), (pair, n_in)
        assert np.abs(ref).max() > 1e-3


def test_indices_past_2_to_the_31(K):
    pair, n_in = (44100, 16000), 13_500_000
    up, down = _params(*pair)[:2]
    n_out = -(-n_in * up // down)
    assert n_out == 4_897_960
    cross = (2 ** 31) // down                      # n * 441 passes 2^31 here
    assert abs(cross - 4_869_600) < 100 and cross + 1000 < n_out
    x = np.random.default_rng(2).uniform(-1, 1, n_in).astype(np.float32)
    got = K.resample(torch.from_numpy(x).cuda()[None], *pair)[0].cpu().numpy()
    assert got.shape == (n_out,)
    xm = x.astype(np.float64)
    for n in (np.arange(2000), np.arange(n_out - 2000, n_out), np.arange(cross - 1000, cross + 1000)):
        err = float(np.abs(got[n] - _ref(xm, pair, n)).max())
        print(f"resample 13.5M samples, outputs {n[0]}..{n[-1]}: {err:.2e}")
        assert err <= TOL


def _shifted(t):
    """The same values one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, device="cuda")
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    v = buf[off:off + t.numel()]
    assert v.data_ptr() % 16 == 4
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


@pytest.mark.parametrize("ch", [1, 2])
def test_alignment_batch_and_repeat_invariance(K, ch):
    for pair in ((48000, 16000), (16000, 44100), (44100, 16000)):
        x, _ = _clip(3, 3001, ch, 4)
        xd = torch.from_numpy(x).cuda()
        xd = xd if ch > 1 else xd[:, :, 0].contiguous()
        assert xd.data_ptr() % 16 == 0
        want = K.resample(xd, *pair, channels=ch)
        assert torch.equal(K.resample(xd, *pair, channels=ch), want)             # two identical calls
        assert torch.equal(K.resample(_shifted(xd), *pair, channels=ch), want)   # x one float off a 16-byte boundary
        for b in range(3):
            assert torch.equal(K.resample(xd[b:b + 1].contiguous(), *pair, channels=ch)[0], want[b])


def test_same_rate_returns_the_input_and_the_table_is_cached(K):
    x = torch.rand((2, 100), device="cuda")
    assert K.resample(x, 16000, 16000) is x
    a = K.resample_taps(48000, 16000, x.device)
    assert K.resample_taps(48000, 16000, x.device)[1] is a[1] and tuple(a[1].shape) == (1, 210)
    with pytest.raises(ValueError):
        K.resample(x, 48000, 16000, channels=2)
    assert K.resample(torch.empty((0, 100), device="cuda"), 48000, 16000).shape == (0, 34)
    assert K.resample(torch.empty((2, 0), device="cuda"), 48000, 16000).shape == (2, 0)


def test_bad_and_empty_calls():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd._hip import lib, ptr, stream_handle
    from audiolcm_amd.kernels import resample_taps
    pl, taps = resample_taps(48000, 16000, "cuda")
    x = torch.full((1, 3000, 2), 0.25, device="cuda")
    y = torch.full((1, 1000), 7.0, device="cuda")
    L, s = lib(), stream_handle()
    px, py, pt = ptr(x), ptr(y), ptr(taps)

    def call(x=px, y=py, B=1, N_in=3000, ch=1, N_out=1000, up=1, down=3, t=pt, ntaps=pl.ntaps, first=pl.first):
        return L.alcm_resample(x, y, B, N_in, ch, N_out, up, down, t, ntaps, first, s)
    assert call(x=None) != 0 and call(y=None) != 0 and call(t=None) != 0
    assert b"resample" in L.alcm_last_error()
    assert call(up=0) != 0 and call(down=0) != 0 and call(ntaps=0) != 0 and call(up=-1) != 0
    assert call(ch=0) != 0 and call(ch=9) != 0
    assert call(N_out=999) != 0 and call(N_out=1001) != 0 and call(N_in=2998, N_out=999) != 0
    assert call(B=-1) != 0 and call(N_in=-3, N_out=-1) != 0 and call(N_out=-1) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                  # none of these launched
    assert call(B=0) == 0 and call(N_in=0, N_out=0) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call(ch=2, N_in=2998, N_out=1000) == 0  # and a good call does launch
    torch.cuda.synchronize()
    assert bool((y != 7.0).all())
