"""Float64 restatements for the limiter's tests: the limiter's definition (include/audiolcm_hip.h, alcm_limiter) as plain
NumPy with a Python loop for the release, the release again as a scan of its maps, the ITU-R BS.1770-4 meter of
``test_gpu_loudness.py`` restated, and the level stage built from the two (``pipeline64``).  Nothing here touches the
GPU or the package's kernels."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def ceiling_of(dbfs):
    return np.float32(10.0 ** (dbfs / 20.0))


def envelope(x, g, env=None, os=1):
    """(u, e) of steps 1 and 2, both fp32: u = fl32(x g), e = |u| or the larger of it and the oversampled copy's."""
    u = np.asarray(x, np.float32) * np.float32(g)
    assert u.dtype == np.float32
    e = np.abs(u)
    if env is not None:
        ue = np.abs(np.asarray(env, np.float32) * np.float32(g)).reshape(u.size, os)
        e = np.maximum(e, ue.max(1))
    return u, e


def curve(e, c, La):
    """(r, s) of steps 3 to 5 in float64 from the fp32 envelope e."""
    e64 = e.astype(np.float64)
    over = e > np.float32(c)
    r = np.ones(e.size, np.float64)
    r[over] = float(np.float32(c)) / e64[over]
    rp = np.concatenate([np.ones(La), r, np.ones(La)])
    m = sliding_window_view(rp, La + 1).min(-1)          # m[j], j = -La .. N - 1
    s = sliding_window_view(m, La + 1).mean(-1)          # s[n] = mean m[n - La .. n]
    assert m.size == e.size + La and s.size == e.size
    return r, s


def tile_attack(e, c, La, span=2048):
    """The attack curve s as alcm_limiter's first kernel computes it, tile by tile, with the kernel's indices: per span
    of ``span`` samples the envelope over the span and a halo of H = La rounded up to 4 either side (zero outside the
    clip); the hold as a sliding maximum of e by doubling (floor(log2(La + 1)) steps, then two overlapping windows of
    2^p); m = c / max where it exceeds c, else 1; an inclusive prefix sum P of m over the tile that starts at the tile;
    s[n0 + q] = (P[q + La] - P[q - 1]) / (La + 1).  The kernel sums each thread's 12 values and scans the totals where
    this uses one running sum; both are prefix sums of the same values in float64."""
    e = np.asarray(e, np.float32)
    c = np.float32(c)
    N, w = e.size, La + 1
    H = (La + 3) & ~3
    W = span + 2 * H
    p = 0
    while (2 << p) <= w:
        p += 1
    rest = w - (1 << p)
    out = np.ones(-(-N // span) * span)
    for n0 in range(0, N, span):
        idx = np.arange(W) + n0 - H
        t = np.where((idx >= 0) & (idx < N), e[np.clip(idx, 0, N - 1)], np.float32(0)).astype(np.float32)
        for j in range(p):
            d = 1 << j
            v = t.copy()
            v[:W - d] = np.maximum(t[:W - d], t[d:])
            t = v
        i = np.arange(span + La) + H - La
        top = np.maximum(t[i], t[i + rest])
        m = np.ones(top.size)
        m[top > c] = float(c) / top[top > c].astype(np.float64)
        P = np.cumsum(m)
        q = np.arange(span)
        out[n0:n0 + span] = (P[q + La] - np.where(q > 0, P[q - 1], 0.0)) / float(w)
    return out[:N]


def release_loop(s, a):
    """Step 6 as it is written: y[n] = min(s[n], a y[n-1] + (1 - a) s[n]), y[-1] = 1."""
    y, out = 1.0, []
    oma = 1.0 - a
    for v in s.tolist():
        y = min(v, a * y + oma * v)
        out.append(y)
    return np.array(out, np.float64)


def release_scan(s, a):
    """Step 6 as an inclusive Hillis-Steele scan of the maps y -> min(C, A y + D), applied to y[-1] = 1:
    f2 o f1 = min(min(C2, A2 C1 + D2), A2 A1 y + A2 D1 + D2)."""
    C, A, D = s.copy(), np.full(s.size, a, np.float64), (1.0 - a) * s
    d = 1
    while d < s.size:
        C2, A2, D2 = C[d:], A[d:], D[d:]
        C1, A1, D1 = C[:-d], A[:-d], D[:-d]
        nC, nA, nD = np.minimum(C2, A2 * C1 + D2), A2 * A1, A2 * D1 + D2
        C, A, D = (np.concatenate([v[:d], n]) for v, n in ((C, nC), (A, nA), (D, nD)))
        d *= 2
    return np.minimum(C, A * 1.0 + D)


def limiter(x, g, c, La, a, env=None, os=1):
    """Steps 1 to 7: (out fp32, dict(u, e, r, s, y))."""
    c = np.float32(c)
    u, e = envelope(x, g, env, os)
    r, s = curve(e, c, La)
    y = release_loop(s, a)
    v = np.abs(u * y.astype(np.float32))
    assert v.dtype == np.float32
    out = np.copysign(np.minimum(v, c), u)
    return out, dict(u=u, e=e, r=r, s=s, y=y)


def within(got, ref, ulps=4):
    """|got - ref| <= ulps * 2^-24 * |ref| + the smallest normal, per sample, in float64."""
    got64, ref64 = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got64 - ref64) <= ulps * 2.0 ** -24 * np.abs(ref64) + float(np.finfo(np.float32).tiny)


# ---------------------------------------------------------------------------- the meter, as test_gpu_loudness.py
def _coefs(rate):
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


def lufs64(x, rate):
    """(integrated loudness, the least distance of a block from a gate that decides about it) of the clip x."""
    shelf, highpass = _coefs(rate)
    y = _biquad64(_biquad64(np.asarray(x, np.float64), *shelf), *highpass)
    hop = (rate + 5) // 10
    nh = y.size // hop
    S = (y[:nh * hop] ** 2).reshape(nh, hop).sum(-1)
    z = (S[:-3] + S[1:-2] + S[2:-1] + S[3:]) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    margin = np.abs(l + 70.0).min()
    rel = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    margin = min(margin, np.abs(l[keep] - rel).min())
    keep &= l > rel
    return -0.691 + 10.0 * np.log10(z[keep].mean()), margin


def gain_to(target, L):
    return np.float32(10.0 ** ((target - L) / 20.0))


def static64(x, rate, target, c):
    """Today's level stage: the gain to the target, or the smaller one that keeps the peak at the ceiling:
    dict(wav, lufs_out, margin)."""
    L, margin = lufs64(x, rate)
    g = gain_to(target, L)
    peak = np.abs(np.asarray(x, np.float32)).max()
    if peak * g > np.float32(c):
        g = np.float32(float(np.float32(c)) / float(peak))
        while peak * g > np.float32(c):
            g = np.nextafter(g, np.float32(0))
    wav = np.asarray(x, np.float32) * g
    L1, m1 = lufs64(wav, rate)
    return dict(wav=wav, gain=g, lufs_out=L1, margin=min(margin, m1))


def pipeline64(x, rate, target, c, La, a, passes=3, env=None, os=1):
    """``normalize_loudness(limiter=...)`` restated: measure, the gain to the target with no ceiling, limit; then, where
    the peak passes the ceiling, measure the limited clip, multiply the pre-gain by the gain that asks for and limit the
    original again, ``passes`` runs in all: dict(wav, gain, lufs, lufs_out, margin (the least over every measurement),
    binds)."""
    x = np.asarray(x, np.float32)
    L0, margin = lufs64(x, rate)
    g = gain_to(target, L0)
    peak = np.abs(x if env is None else np.asarray(env, np.float32)).max()      # with env: the oversampled estimate
    binds = bool(np.float32(peak) * g > np.float32(c))
    wav = limiter(x, g, c, La, a, env, os)[0]
    for _ in range(passes - 1):
        if not binds:
            break
        Lk, mk = lufs64(wav, rate)
        margin = min(margin, mk)
        g = g * gain_to(target, Lk)
        assert g.dtype == np.float32
        wav = limiter(x, g, c, La, a, env, os)[0]
    L1, m1 = lufs64(wav, rate)
    return dict(wav=wav, gain=g, lufs=L0, lufs_out=L1, margin=min(margin, m1), binds=binds)


# ---------------------------------------------------------------------------- signals
def edge_signal(n, span, La, seed=0):
    """The kernel tests' clip at 16 kHz, before the pre-gain of 2.5: a 220 Hz tone at 0.2, noise at 0.05, spikes of
    +-0.9 at sample 0, at n - 1, at the last sample of a span and the first of the next, two more within La of those,
    one isolated, and a 400-sample plateau at 0.8.  -> (x fp32, the spike positions)."""
    t = np.arange(n) / 16000.0
    x = 0.2 * np.sin(2 * np.pi * 220.0 * t) + 0.05 * np.random.default_rng(seed).standard_normal(n)
    spikes = [p for p in (0, n - 1, span - 1, span, span - 1 - La // 2, span + La - 10, span // 2) if 0 <= p < n]
    for i, p in enumerate(sorted(set(spikes))):
        x[p] = 0.9 if i % 2 == 0 else -0.9
    p0 = span + span // 2
    if p0 + 400 <= n:
        x[p0:p0 + 400] = 0.8
    return x.astype(np.float32), sorted(set(spikes))


def burst_signal(rate, seconds=2.0, burst=0.6, seed=1):
    """A 330 Hz tone at 0.05, noise at 0.02 and every 250 ms a 20 ms burst of 90 Hz that starts at ``burst`` and decays
    (time constant 5 ms): the impacts, drums and door slams a static gain under a ceiling leaves too quiet."""
    n = int(round(rate * seconds))
    t = np.arange(n) / rate
    x = 0.05 * np.sin(2 * np.pi * 330.0 * t) + 0.02 * np.random.default_rng(seed).standard_normal(n)
    nb = int(round(0.020 * rate))
    tb = np.arange(nb) / rate
    shot = burst * np.exp(-tb / 0.005) * np.cos(2 * np.pi * 90.0 * tb)
    for k in range(int(seconds / 0.25)):
        p = int(round((0.05 + 0.25 * k) * rate))
        x[p:p + nb] += shot[:max(0, min(nb, n - p))]
    return x.astype(np.float32)
