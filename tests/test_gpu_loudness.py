"""alcm_loudness_hops, alcm_loudness_gain and alcm_wave_gain through ``kernels.loudness`` / ``normalize_loudness``
against a float64 restatement of ITU-R BS.1770-4 written here: K-weighting as a sample-by-sample recursion over the two
biquads (coefficients by the bilinear transform of the analog prototypes), y^2 summed per 100 ms hop, 400 ms blocks, the
absolute gate at -70 LUFS and the relative gate 10 LU under the mean of what the absolute gate kept.

Bars.  Hop sums: the relative error per hop is at most 4 x the worst relative error of an fp32 recursion of the same
input (computed here, ``_recursion32``), with a floor of 1e-5: the kernel may order its arithmetic
differently from the loop but has no reason to be an order worse.  Integrated loudness: 0.01 LU, a tenth of the 0.1 LU
EBU Tech 3341 allows a meter; that is 1.2e-3 relative in the gain.  Every case first asserts on the float64 reference
alone that each block lies 0.5 LU or more from both gates, so that no gate decision hangs on rounding.

Measured on an MI355X (fp64 state and sums, y^2 rounded to fp32 once): worst hop-sum error 9.6e-9 over all shapes and
recipes, the DC case included (1.2e-9 to 6.9e-9), where the fp32 recursion's own worst per case is 4.6e-7 (8 kHz) to
2.2e-2 (44.1 kHz, recipe D); loudness within 1.1e-6 LU of float64."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RECIPES = {"A": (0, (0.1, 0.001, 0.1)),     # the relative gate drops blocks
           "C": (2, (0.3, 0.3, 0.003)),
           "D": (1, (0.2, 1e-6, 0.2))}      # the absolute gate drops blocks
SHAPES = [(16000, 3.0), (44100, 2.37), (8000, 1.9), (48000, 3.0), (16000, 30.0)]
SIGNALS = ("A", "C", "D", "A+dc")
MARGIN = 0.5
LU_TOL = 0.01
GAIN_RTOL = 1.2e-3


def _coefs(rate):
    """((b0, b1, b2, a1, a2) of the high shelf, of the high pass) in float64."""
    def a_of(f0, Q):
        K = math.tan(math.pi * f0 / rate)
        a0 = 1.0 + K / Q + K * K
        return K, a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0
    Q = 0.7071752369554196
    K, a0, a1, a2 = a_of(1681.974450955533, Q)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, a1, a2)
    _, _, a1, a2 = a_of(38.13547087602444, 0.5003270373238773)
    return shelf, (1.0, -2.0, 1.0, a1, a2)


def _biquad64(x, b0, b1, b2, a1, a2):
    """y[n] = (b0 x[n] + b1 x[n-1] + b2 x[n-2]) - a1 y[n-1] - a2 y[n-2], a plain loop on Python floats (float64)."""
    xp = np.concatenate([np.zeros(2), x])
    f = (b0 * xp[2:] + b1 * xp[1:-1] + b2 * xp[:-2]).tolist()
    y1 = y2 = 0.0
    out = []
    put = out.append
    for v in f:
        v = v - a1 * y1 - a2 * y2
        y2 = y1
        y1 = v
        put(v)
    return np.array(out)


def _recursion32(xs, rate):
    """The same recursion with every coefficient, product and sum in fp32, the clips of xs (R, N) side by side."""
    y = xs.astype(np.float32)
    for c in _coefs(rate):
        b0, b1, b2, a1, a2 = (np.float32(v) for v in c)
        xp = np.concatenate([np.zeros((y.shape[0], 2), np.float32), y], axis=1)
        f = np.ascontiguousarray(((b0 * xp[:, 2:] + b1 * xp[:, 1:-1]) + b2 * xp[:, :-2]).T)
        assert f.dtype == np.float32
        out = np.empty_like(f)
        y1 = np.zeros(y.shape[0], np.float32)
        y2 = np.zeros(y.shape[0], np.float32)
        t = np.empty_like(y1)
        for n in range(f.shape[0]):
            v = out[n]
            np.multiply(a1, y1, out=t)
            np.subtract(f[n], t, out=v)
            np.multiply(a2, y2, out=t)
            np.subtract(v, t, out=v)
            y2, y1 = y1, v
        y = out.T
    return y


def _hop_sums(y, hop):
    nh = y.shape[-1] // hop
    return (y[..., :nh * hop].astype(np.float64) ** 2).reshape(y.shape[:-1] + (nh, hop)).sum(-1)


def _k64(x, rate):
    shelf, highpass = _coefs(rate)
    return _biquad64(_biquad64(np.asarray(x, np.float64), *shelf), *highpass)


def _gated(sums, hop):
    """(integrated loudness, the least distance of a block from a gate that decides about it) from float64 hop sums."""
    S = np.asarray(sums, np.float64)
    if S.size < 4:
        return -math.inf, math.inf
    z = (S[:-3] + S[1:-2] + S[2:-1] + S[3:]) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    margin = np.abs(l + 70.0).min()
    if not keep.any():
        return -math.inf, margin
    rel = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    margin = min(margin, np.abs(l[keep] - rel).min())
    keep &= l > rel
    return -0.691 + 10.0 * np.log10(z[keep].mean()), margin


def _lufs64(x, rate):
    hop = (rate + 5) // 10
    return _gated(_hop_sums(_k64(x, rate), hop), hop)


def _signal(name, n):
    base, _, dc = name.partition("+")
    seed, levels = RECIPES[base]
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    for part, level in zip(np.array_split(x, 3), levels):
        part *= np.float32(level)
    return x + np.float32(0.25) if dc else x


@functools.lru_cache(maxsize=None)
def _case(rate, seconds):
    """Per shape, once: the four signals, their float64 hop sums, loudness and gate margin, and the worst relative
    hop-sum error of the fp32 recursion per signal."""
    n, hop = int(round(rate * seconds)), (rate + 5) // 10
    xs = np.stack([_signal(s, n) for s in SIGNALS])
    ref = np.stack([_hop_sums(_k64(x, rate), hop) for x in xs])
    err32 = np.abs(_hop_sums(_recursion32(xs, rate), hop) / ref - 1.0).max(1)
    gated = [_gated(r, hop) for r in ref]
    for a in (xs, ref, err32):
        a.setflags(write=False)
    return dict(n=n, hop=hop, x=xs, sums=ref, err32=err32, lufs=[g[0] for g in gated], margin=[g[1] for g in gated])


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}Hz-{s[1]}s")
def test_hop_sums_and_loudness_match_float64(K, shape):
    """All four signals of a shape in one batch: the three recipes and recipe A on a DC offset of 0.25, whose long
    high-pass transient shows a wrong state carried between chunks or spans."""
    rate = shape[0]
    c = _case(*shape)
    for name, m in zip(SIGNALS, c["margin"]):
        assert m >= MARGIN, f"recipe {name} at {shape}: a block lies {m:.3f} LU from a gate"
    lufs, peak, sums = K.loudness(_dev(c["x"]), rate)
    sums, lufs, peak = sums.cpu().numpy(), lufs.cpu().numpy(), peak.cpu().numpy()
    assert sums.dtype == np.float64 and sums.shape == c["sums"].shape == (4, c["n"] // c["hop"])
    for i, name in enumerate(SIGNALS):
        err = np.abs(sums[i] / c["sums"][i] - 1.0).max()
        bar = max(4.0 * c["err32"][i], 1e-5)
        print(f"{shape} {name}: hop sums {err:.3e} (fp32 recursion {c['err32'][i]:.3e}, bar {bar:.3e}); "
              f"lufs {lufs[i]:.6f} vs {c['lufs'][i]:.6f}; gate margin {c['margin'][i]:.2f} LU")
        assert err <= bar, (name, err, bar)
        assert abs(float(lufs[i]) - c["lufs"][i]) <= LU_TOL, (name, lufs[i], c["lufs"][i])
    np.testing.assert_array_equal(peak, np.abs(c["x"]).max(1))


def test_gates_drop_blocks_in_these_recipes():
    """What the recipes are for, on the float64 reference alone: the relative gate drops blocks of A, the absolute gate
    blocks of D."""
    c = _case(16000, 3.0)
    for name, gate in (("A", "rel"), ("D", "abs")):
        S = c["sums"][SIGNALS.index(name)]
        z = (S[:-3] + S[1:-2] + S[2:-1] + S[3:]) / (4.0 * c["hop"])
        l = -0.691 + 10.0 * np.log10(z)
        keep = l > -70.0
        if gate == "abs":
            assert 0 < keep.sum() < keep.size
        else:
            assert keep.all() and (l <= -0.691 + 10.0 * np.log10(z.mean()) - 10.0).any()


@pytest.mark.parametrize("extra", ["0", "hop-1", "hop"])
def test_shortest_clips(K, extra):
    """N = block, block + hop - 1 (still one block) and block + hop (two), at a rate whose hop is odd."""
    rate, hop = 11025, 1103
    n = 4 * hop + {"0": 0, "hop-1": hop - 1, "hop": hop}[extra]
    x = np.float32(0.05) * np.random.default_rng(5).standard_normal(n).astype(np.float32)
    want, margin = _lufs64(x, rate)
    assert margin >= MARGIN
    lufs, peak, sums = K.loudness(_dev(x[None]), rate)
    assert sums.shape == (1, n // hop) and n // hop - 3 == (n - 4 * hop) // hop + 1
    assert np.abs(sums.cpu().numpy()[0] / _hop_sums(_k64(x, rate), hop) - 1.0).max() <= 1e-5
    assert abs(float(lufs[0]) - want) <= LU_TOL
    with pytest.raises(ValueError):
        K.loudness(_dev(x[None, :4 * hop - 1]), rate)


def test_length_that_is_no_multiple_of_a_chunk_and_a_strided_view(K):
    """N = 3 spans + 5 chunks + 7 samples; the same clips as rows of a wider tensor at an odd offset (element loads,
    another row stride) give the same bits as the contiguous ones (16-byte loads)."""
    rate, hop = 8000, 800
    n = 3 * 8192 + 5 * 32 + 7
    x = np.stack([_signal("A", n), _signal("C", n)])
    xd = _dev(x)
    lufs, peak, sums = K.loudness(xd, rate)
    for i in range(2):
        assert np.abs(sums[i].cpu().numpy() / _hop_sums(_k64(x[i], rate), hop) - 1.0).max() <= 1e-5
    wide = torch.full((2, n + 13), 7.0, device="cuda")
    view = wide[:, 3:3 + n]
    view.copy_(xd)
    assert not view.is_contiguous() and view.data_ptr() % 16
    lufs_v, peak_v, sums_v = K.loudness(view, rate)
    assert torch.equal(sums_v, sums) and torch.equal(lufs_v, lufs) and torch.equal(peak_v, peak)
    out = K.normalize_loudness(view, rate, target=-20.0, peak_dbfs=-1.0)
    ref = K.normalize_loudness(xd, rate, target=-20.0, peak_dbfs=-1.0)
    assert torch.equal(out["wav"], ref["wav"]) and torch.equal(out["gain"], ref["gain"])
    inplace = K.normalize_loudness(view, rate, target=-20.0, peak_dbfs=-1.0, out=view)["wav"]
    assert inplace.data_ptr() == view.data_ptr() and torch.equal(view, ref["wav"])
    assert float(wide[:, :3].min()) == 7.0 and float(wide[:, 3 + n:].max()) == 7.0      # nothing outside the view


def test_a_clip_does_not_depend_on_its_batch(K):
    """A, C and D stacked against each clip alone: hop sums, loudness, gain and output bit for bit."""
    rate = 16000
    x = _dev(_case(rate, 3.0)["x"][:3])
    both = K.normalize_loudness(x, rate, target=-18.0, peak_dbfs=-2.0)
    sums = K.loudness(x, rate)[2]
    for i in range(3):
        one = K.normalize_loudness(x[i:i + 1].clone(), rate, target=-18.0, peak_dbfs=-2.0)
        for key in ("wav", "lufs", "gain", "peak"):
            assert torch.equal(one[key][0], both[key][i]), (i, key)
        assert torch.equal(K.loudness(x[i:i + 1].clone(), rate)[2][0], sums[i])


def test_silence(K):
    """An all-zero clip beside a live one: -inf LUFS, gain 1, the input's bits."""
    rate = 16000
    x = _dev(np.stack([np.zeros(48000, np.float32), _signal("C", 48000)]))
    out = K.normalize_loudness(x, rate, target=-23.0, peak_dbfs=-1.0)
    assert float(out["lufs"][0]) == -math.inf and float(out["gain"][0]) == 1.0 and float(out["peak"][0]) == 0.0
    assert torch.equal(out["wav"][0].view(torch.int32), x[0].view(torch.int32))
    assert math.isfinite(float(out["lufs"][1])) and float(out["gain"][1]) != 1.0


@pytest.mark.parametrize("rate", [16000, 44100])
def test_peak_and_true_peak(K, rate):
    n = int(rate * 1.3) + 3
    x = _dev(np.stack([_signal("A", n), _signal("C", n), _signal("D", n)]))
    lufs, peak, _ = K.loudness(x, rate)
    assert torch.equal(peak, x.abs().amax(1))
    lufs_t, peak_t, _ = K.loudness(x, rate, true_peak=True)
    assert torch.equal(peak_t, K.resample(x, rate, 4 * rate).abs().amax(1))
    assert torch.equal(lufs_t, lufs) and bool((peak_t != peak).any())


def test_normalize_to_a_target(K):
    """-23 LUFS without a ceiling on recipe A: the output, measured by the float64 reference, sits at -23 +- 0.02 LU,
    and the gain is the float64 one to 1.2e-3."""
    rate = 16000
    c = _case(rate, 3.0)
    x = c["x"][0]
    out = K.normalize_loudness(_dev(x[None]), rate, target=-23.0)
    want_gain = 10.0 ** ((-23.0 - c["lufs"][0]) / 20.0)
    assert abs(float(out["gain"][0]) / want_gain - 1.0) <= GAIN_RTOL
    y = out["wav"][0].cpu().numpy()
    np.testing.assert_array_equal(y, x * np.float32(float(out["gain"][0])))     # one fp32 rounding per sample
    got, margin = _lufs64(y, rate)
    assert margin >= MARGIN and abs(got + 23.0) <= 0.02, got


@pytest.mark.parametrize("target", [-14.0, -8.0])
def test_normalize_under_a_ceiling(K, target):
    """Recipe C (peak 1.276, -8.02 LUFS) under a ceiling of -1 dBFS: no sample above fp32(10^(-1/20)), exactly, and the
    loudness does not pass the target.  At -14 LUFS the gain of 0.50 leaves the peak at 0.64, under the ceiling, so the
    target is met; at -8 LUFS the peak binds (the target alone would leave it at 1.28) and the loudness stays under
    the target by what the ceiling takes."""
    rate = 16000
    c = _case(rate, 3.0)
    x = c["x"][1]
    peak = float(np.abs(x).max())
    ceiling = np.float32(10.0 ** (-1.0 / 20.0))
    want = 10.0 ** ((target - c["lufs"][1]) / 20.0)
    binds = peak * want > float(ceiling)
    assert binds == (target == -8.0)
    out = K.normalize_loudness(_dev(x[None]), rate, target=target, peak_dbfs=-1.0)
    y = out["wav"][0].cpu().numpy()
    assert np.abs(y).max() <= ceiling
    g = float(out["gain"][0])
    got = _lufs64(y, rate)[0]
    if binds:
        assert float(ceiling) / peak * (1.0 - 3e-7) <= g <= float(ceiling) / peak     # no lower than it has to be
        assert got < target - 1.0 and abs(got - (c["lufs"][1] + 20.0 * math.log10(g))) <= 0.02
    else:
        assert abs(g / want - 1.0) <= GAIN_RTOL and abs(got - target) <= 0.02
    tp = K.normalize_loudness(_dev(x[None]), rate, target=target, peak_dbfs=-1.0, true_peak=True)
    assert float(tp["gain"][0]) <= g and float(tp["peak"][0]) >= peak


def test_gain_of_one_returns_the_inputs_bits(K):
    """No target and a ceiling the peak stays under: gain 1, and every bit of the input, denormals and signed zeros
    included."""
    rate = 16000
    x = _signal("A", 16000)
    x[:4] = np.array([1e-42, -1e-42, -0.0, 0.0], np.float32)
    assert np.abs(x).max() < 0.9
    out = K.normalize_loudness(_dev(x[None]), rate, peak_dbfs=-0.5)
    assert float(out["gain"][0]) == 1.0
    np.testing.assert_array_equal(out["wav"][0].cpu().numpy().view(np.int32), x.view(np.int32))
    over = K.normalize_loudness(_dev(x[None] * np.float32(4.0)), rate, peak_dbfs=-0.5)
    assert float(over["gain"][0]) < 1.0 and float(over["wav"].abs().max()) <= np.float32(10.0 ** (-0.5 / 20.0))


def test_c_abi_refusals(K):
    from audiolcm_amd import _hip
    L = _hip.lib()
    x = torch.zeros((2, 8000), device="cuda")
    coef = K.loudness_coef(16000, x.device)
    sums = torch.empty((2, 5), device="cuda", dtype=torch.float64)
    peak = torch.empty((2,), device="cuda")
    ws = torch.empty(L.alcm_loudness_workspace_bytes(2, 8000, 1600) // 8 + 1, device="cuda", dtype=torch.float64)
    p, s = _hip.ptr, _hip.stream_handle()
    ok = (p(x), 2, 8000, 8000, p(coef), 1600, p(sums), p(peak), p(ws), ws.numel() * 8, s)
    assert L.alcm_loudness_hops(*ok) == 0

    def hops(**kw):
        names = ("x", "B", "N", "ld", "coef", "hop", "sums", "peak", "ws", "ws_bytes", "stream")
        return L.alcm_loudness_hops(*[kw.get(n, v) for n, v in zip(names, ok)])
    assert L.alcm_loudness_workspace_bytes(2, 8000, 0) == 0
    for bad in (dict(x=None), dict(sums=None, peak=None), dict(coef=None), dict(B=-1), dict(N=-1), dict(hop=0),
                dict(ld=7999), dict(ws=None), dict(ws_bytes=ws.numel() * 8 // 2)):
        assert hops(**bad) != 0, bad
    assert hops(B=0) == 0 and hops(N=0, ld=0) == 0 and hops(sums=None, coef=None) == 0
    lufs = torch.empty((2,), device="cuda")
    gain = torch.empty((2,), device="cuda")
    nan = float("nan")
    assert L.alcm_loudness_gain(p(sums), p(peak), 2, 5, 1600, nan, 0.0, p(lufs), p(gain), s) == 0
    assert L.alcm_loudness_gain(p(sums), p(peak), 2, 5, 1600, nan, 0.0, None, None, s) != 0
    assert L.alcm_loudness_gain(None, p(peak), 2, 5, 1600, nan, 0.0, p(lufs), p(gain), s) != 0
    assert L.alcm_loudness_gain(p(sums), None, 2, 5, 1600, nan, 0.5, p(lufs), p(gain), s) != 0
    assert L.alcm_loudness_gain(p(sums), p(peak), 2, 5, 0, nan, 0.0, p(lufs), p(gain), s) != 0
    assert L.alcm_wave_gain(p(x), p(gain), p(x), 2, 8000, 8000, 8000, s) == 0
    assert L.alcm_wave_gain(p(x), None, p(x), 2, 8000, 8000, 8000, s) != 0
    assert L.alcm_wave_gain(p(x), p(gain), p(x), 2, 8000, 7999, 8000, s) != 0
    assert L.alcm_wave_gain(p(x), p(gain), p(x), -1, 8000, 8000, 8000, s) != 0
    assert L.alcm_wave_gain(p(x), p(gain), p(x), 0, 8000, 8000, 8000, s) == 0
    torch.cuda.synchronize()
