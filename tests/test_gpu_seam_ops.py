"""alcm_seam_stats and alcm_wave_paste_law through the C-ABI against the float64 restatement of tests/_seam_ref.py.

Bars.  Stats: the fp64 sums carry a relative error of at most N 2^-53 (sum |x y| <= sqrt(Sxx Syy)), so rho and gam are
the restatement's up to their own rounding to fp32: |rho - ref| <= 2^-23, gam within 2^-23 relative, and the degenerate
values (1 at an edge without a junction, for an empty or silent zone, for a run without a junction) exact.
Blend: against the restatement fed the device's tables, |out - ref| <= 32 * 2^-24 * max(|orig|, gam |gen|) per sample:
about a dozen fp32 roundings on terms bounded by sqrt(2) max, doubled.  Samples of g = 0 are orig's bits, samples of
g = 1 gen's where gam is 1.  The blend is also compared bit for bit with the same operations done in NumPy fp32 in the
order include/audiolcm_hip.h states, and the element path with the 16-byte path on the same data."""
import numpy as np
import pytest
import torch

import _seam_ref as ref

pytestmark = pytest.mark.gpu

B = 2
EPS_TAB = 2.0 ** -23
BLEND_BAR = 32 * 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    # the package's own table, so that the fp32 restatement sees the ramp's bits (both are float64 cosines rounded to fp32)
    assert all(np.array_equal(kernels.paste_ramp_host(R).numpy(), ref.ramp_table(R)) for R in (1, 6, 7, 259, 4096))
    return kernels


_waves = {}


def waves(N):
    """Per N, once: orig and a full-length gen, uniform in [-1, 1]."""
    if N not in _waves:
        g = np.random.default_rng(N + 7)
        _waves[N] = (g.uniform(-1, 1, (B, N)).astype(np.float32), g.uniform(-1, 1, (B, N)).astype(np.float32))
    return _waves[N]


def masks(T, ring):
    def m(*rows):
        out = np.zeros((B, T), np.float32)
        for b, f in enumerate(rows):
            out[b, list(f)] = 1.0
        return out
    cases = {
        "gap1_and_ends": m((3, 5), (0, 1, T - 1)),          # a one-frame kept gap; runs touching frame 0 and frame T - 1
        "interior": m((6, 7, 8), (2, 9, 10)),
        "kept_and_full": m((), range(T)),
        "full_and_first": m(range(T), (0,)),
        "last": m((T - 1,), (T - 3, T - 2)),
    }
    if ring:
        cases["wrap"] = m((T - 2, T - 1, 0), (5,))           # one run across the wrap
        cases["one_kept"] = m(set(range(T)) - {4}, (0, T - 1))
    return cases


def gens(fs, T, ring):
    """(gen_start, Ng): the whole clip; a part whose edges cut zones short (multiples of 4 where fs is one); the same
    part off by one and shorter (the element path); on a ring a gen across the wrap."""
    N = T * fs
    out = [(0, N), (2 * fs + fs // 2, 6 * fs), (2 * fs + fs // 2 + 1, 6 * fs - 3)]
    if ring:
        out += [((T - 3) * fs, 5 * fs), ((T - 3) * fs + 1, 5 * fs + 2), (3 * fs, N)]
    return out


def part(gen, gen_start, Ng, ring):
    N = gen.shape[1]
    idx = (gen_start + np.arange(Ng)) % N if ring else gen_start + np.arange(Ng)
    return np.ascontiguousarray(gen[:, idx])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_stats(K, orig, gp, mask, fs, gs, R, ring):
    rho_d, gam_d, sums_d = K.seam_stats(dev(orig), dev(gp), dev(mask), gs, R, fs, ring)
    rho, gam, sums = rho_d.cpu().numpy(), gam_d.cpu().numpy(), sums_d.cpu().numpy()
    r_rho, r_gam, r_sums = ref.stats(orig, gp, mask, fs, gs, R, ring)
    assert np.abs(sums - r_sums).max() <= 1e-12 * max(r_sums.max(), 1e-300)
    assert ((sums == 0) == (r_sums == 0)).all()
    assert np.abs(rho.astype(np.float64) - r_rho).max() <= EPS_TAB
    assert (np.abs(gam.astype(np.float64) - r_gam) <= EPS_TAB * r_gam).all()
    degenerate = (r_sums[..., 0] == 0) | (r_sums[..., 1] == 0)
    assert (rho[degenerate] == 1.0).all() and (rho >= 0).all() and (rho <= 1).all()
    assert (gam[r_gam == 1.0] == 1.0).all() and (gam[mask <= 0] == 1.0).all()
    assert (gam >= 0.5).all() and (gam <= 2.0).all()
    if ring:
        assert (rho[:, -1] == rho[:, 0]).all() and (sums[:, -1] == sums[:, 0]).all()
    return rho_d, gam_d


def check_blend(K, orig, gp, mask, fs, gs, R, ring, rho_d, gam_d):
    """Out of place and in place against the restatement; returns the worst error in units of the bar's scale."""
    orig_d, gp_d, mask_d = dev(orig), dev(gp), dev(mask)
    rho = None if rho_d is None else rho_d.cpu().numpy()
    gam = None if gam_d is None else gam_d.cpu().numpy()
    want, g, scale = ref.blend(orig, gp, mask, fs, gs, R, ring, rho, gam)
    out = K.wave_paste_law(orig_d, gp_d, mask_d, gs, R, fs, None, ring, rho_d, gam_d).cpu().numpy()
    err = np.abs(out.astype(np.float64) - want)
    assert (err <= BLEND_BAR * scale).all(), float((err / np.maximum(scale, 1e-30)).max() / 2.0 ** -24)
    keep, take = g == 0.0, g == 1.0
    assert np.array_equal(out[keep].view(np.uint32), orig[keep].view(np.uint32))
    inside, gi = ref.in_gen(orig.shape[1], gs, gp.shape[1], ring)
    full = np.zeros_like(orig)
    full[:, inside] = gp[:, gi[inside]]
    if gam is None or (gam[mask > 0] == 1.0).all():
        assert np.array_equal(out[take].view(np.uint32), full[take].view(np.uint32))
    # the same fp32 operations in the stated order give the same bits
    want32 = ref.blend32(orig, gp, mask, fs, gs, R, ring, rho, gam)
    assert np.array_equal(out.view(np.uint32), want32.view(np.uint32))
    # in place: the same bits, and a sample of g = 0 is not written (a guard value survives there)
    guard = orig.copy()
    guard[keep] = np.float32(123.0)
    inplace = dev(guard)
    K.wave_paste_law(inplace, gp_d, mask_d, gs, R, fs, inplace, ring, rho_d, gam_d)
    got = inplace.cpu().numpy()
    assert (got[keep] == np.float32(123.0)).all()
    assert np.array_equal(got[~keep].view(np.uint32), out[~keep].view(np.uint32))
    # the element path on the same data: orig and out one float off a 16-byte boundary
    flat = torch.zeros(orig.size + 1, device="cuda")
    flat[1:] = orig_d.reshape(-1)
    out_un = torch.zeros(orig.size + 1, device="cuda")
    K.wave_paste_law(flat[1:].view(orig.shape), gp_d, mask_d, gs, R, fs, out_un[1:].view(orig.shape), ring, rho_d, gam_d)
    assert np.array_equal(out_un[1:].cpu().numpy().view(np.uint32), out.reshape(-1).view(np.uint32))
    live = scale > 0
    return float((err[live] / scale[live]).max() / 2.0 ** -24) if live.any() else 0.0


def radius(Rf, fs):
    return {"0": 0, "1": 1, "half": fs // 2 + 3, "16 frames": 16 * fs}[Rf]


@pytest.mark.parametrize("ring", [False, True], ids=["line", "ring"])
@pytest.mark.parametrize("Rf", ["0", "1", "half", "16 frames"])
@pytest.mark.parametrize("fs,T", [(8, 12), (8, 20), (512, 12), (512, 20), (7, 12)])
def test_stats_and_blend_match_the_restatement(K, fs, T, Rf, ring):
    """Every mask and gen placement of ``masks`` and ``gens``; 7 samples per frame gives the one-frame gap a tie sample.
    On the ring T = 12 with R of 16 frames has H > T."""
    R = radius(Rf, fs)
    N = T * fs
    orig, gen = waves(N)
    worst = 0.0
    for name, mask in masks(T, ring).items():
        for gs, Ng in gens(fs, T, ring):
            gp = part(gen, gs, Ng, ring)
            rho_d, gam_d = check_stats(K, orig, gp, mask, fs, gs, R, ring)
            worst = max(worst, check_blend(K, orig, gp, mask, fs, gs, R, ring, rho_d, gam_d))
        gp = part(gen, 0, N, ring)
        worst = max(worst, check_blend(K, orig, gp, mask, fs, 0, R, ring, None, None))       # equal power, no gain
    print(f"fs {fs} T {T} R {R} ring {ring}: worst blend error {worst:.2f} x 2^-24 of max(|orig|, gam |gen|)")


def test_the_tie_sample_goes_to_the_right_run(K):
    """7 samples per frame, frames 3 and 5 regenerated: sample 31 of the gap 28 .. 34 is 4 from either run.  With rho 1
    on the left junction and 0 on the right one the sample shows which entry it took."""
    fs, T, R = 7, 12, 6
    orig, gen = waves(T * fs)
    mask = np.zeros((B, T), np.float32)
    mask[:, [3, 5]] = 1.0
    d, edge, _ = ref.geometry(mask[0], fs, T * fs, False)
    assert d[31] == 4 and edge[31] == 5 and edge[30] == 4
    rho = np.ones((B, T + 1), np.float32)
    rho[:, 5] = 0.0
    out = K.wave_paste_law(dev(orig), dev(gen), dev(mask), 0, R, fs, None, False, dev(rho), None).cpu().numpy()
    want, _, _ = ref.blend(orig, gen, mask, fs, 0, R, False, rho, None)
    other, _, _ = ref.blend(orig, gen, mask, fs, 0, R, False, np.ones_like(rho), None)
    assert abs(out[0, 31] - want[0, 31]) < 1e-6 < abs(want[0, 31] - other[0, 31])
    assert abs(out[0, 31] - other[0, 31]) > 1e-6


@pytest.mark.parametrize("ring", [False, True], ids=["line", "ring"])
def test_degenerate_signals(K, ring):
    fs, T, R = 512, 12, 512 // 2 + 3
    N = T * fs
    orig, _ = waves(N)
    mask = np.zeros((B, T), np.float32)
    mask[0, [3, 5]] = 1.0
    mask[1, [T - 1, 0] if ring else [T - 1]] = 1.0
    # gen == orig: rho 1 at every junction, gam 1, and out within the bar of orig
    rho_d, gam_d = check_stats(K, orig, orig, mask, fs, 0, R, ring)
    sums = ref.stats(orig, orig, mask, fs, 0, R, ring)[2]
    assert (rho_d.cpu().numpy() == 1.0).all() and (gam_d.cpu().numpy() == 1.0).all() and sums[0, 3, 0] > 0
    out = K.wave_paste_law(dev(orig), dev(orig), dev(mask), 0, R, fs, None, ring, rho_d, gam_d).cpu().numpy()
    assert (np.abs(out.astype(np.float64) - orig) <= BLEND_BAR * np.abs(orig)).all()
    check_blend(K, orig, orig, mask, fs, 0, R, ring, rho_d, gam_d)
    # gen = -orig: rho clamps to 0
    neg = (-orig).astype(np.float32)
    rho_d, gam_d = check_stats(K, orig, neg, mask, fs, 0, R, ring)
    has_zone = sums[..., 0] > 0
    assert (rho_d.cpu().numpy()[has_zone] == 0.0).all() and (gam_d.cpu().numpy() == 1.0).all()
    check_blend(K, orig, neg, mask, fs, 0, R, ring, rho_d, gam_d)
    # gen = 0.5 * orig shifted by a sample: gam about 2; 0.25 *: at the clamp of 2 exactly
    for scale, exact in ((0.5, False), (0.25, True)):
        half = (scale * np.roll(orig, 1, axis=1)).astype(np.float32)
        rho_d, gam_d = check_stats(K, orig, half, mask, fs, 0, R, ring)
        gam = gam_d.cpu().numpy()
        assert np.allclose(gam[mask > 0], 2.0, rtol=0.05) and (not exact or (gam[mask > 0] == 2.0).all())
        check_blend(K, orig, half, mask, fs, 0, R, ring, rho_d, gam_d)
    # a silent zone: orig silent round clip 0's frame 3, gen silent round its frame 5
    quiet, gq = orig.copy(), waves(N)[1].copy()
    quiet[0, 2 * fs:5 * fs - fs // 2] = 0.0
    gq[0, 4 * fs + fs // 2:7 * fs] = 0.0
    rho_d, gam_d = check_stats(K, quiet, gq, mask, fs, 0, R, ring)
    assert (rho_d.cpu().numpy()[0, 3:7] == 1.0).all() and (gam_d.cpu().numpy()[0] == 1.0).all()
    check_blend(K, quiet, gq, mask, fs, 0, R, ring, rho_d, gam_d)


def test_noise_keeps_its_power_through_the_matched_fade(K):
    """Independent equal-power noise, 512 samples per frame, R = 4096: the mean square over the fade zones relative to
    outside them is 0.75 under the linear law (below 0.85) and 1 under the matched one (within [0.9, 1.1])."""
    import test_seam_host as host
    orig, gen, mask, fs = host._noise(*host.NOISE_SEEDS)
    R = host.NOISE_R
    o_d, g_d, m_d = dev(orig), dev(gen), dev(mask)
    lin = K.wave_paste(o_d, g_d, m_d, 0, R, fs).cpu().numpy().astype(np.float64)
    rho_d, gam_d, _ = K.seam_stats(o_d, g_d, m_d, 0, R, fs)
    matched = K.wave_paste_law(o_d, g_d, m_d, 0, R, fs, None, False, rho_d, None).cpu().numpy().astype(np.float64)
    both = K.wave_paste_law(o_d, g_d, m_d, 0, R, fs, None, False, rho_d, gam_d).cpu().numpy().astype(np.float64)
    _, g = ref.blend_linear(orig, gen, mask, fs, 0, R)
    outside = (g == 0) | (g == 1)
    p_lin, p_matched, p_both = (ref.zone_power(x, g, outside) for x in (lin, matched, both))
    print(f"zone power: linear {p_lin:.4f}, matched {p_matched:.4f}, matched with gain {p_both:.4f}")
    assert p_lin < 0.85
    assert 0.9 <= p_matched <= 1.1 and 0.9 <= p_both <= 1.1


def test_paste_dispatch(K):
    """``kernels.paste``: "linear" alone is ``wave_paste``'s bytes; the other forms are ``seam_stats`` and
    ``wave_paste_law`` with the tables the law asks for."""
    fs, T, R = 8, 20, 7
    orig, gen = waves(T * fs)
    mask = masks(T, False)["interior"]
    o_d, g_d, m_d = dev(orig), dev(gen), dev(mask)
    rho_d, gam_d, _ = K.seam_stats(o_d, g_d, m_d, 0, R, fs)
    eq = lambda a, b: np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))    # noqa: E731
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs), K.wave_paste(o_d, g_d, m_d, 0, R, fs))
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs, ring=True), K.wave_paste_ring(o_d, g_d, m_d, 0, R, fs))
    law = lambda **kw: K.wave_paste_law(o_d, g_d, m_d, 0, R, fs, **kw)                                   # noqa: E731
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs, fade_law="equal-power"), law())
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs, fade_law="matched"), law(rho=rho_d))
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs, fade_law="matched", match_gain=True), law(rho=rho_d, gam=gam_d))
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs, fade_law="equal-power", match_gain=True), law(gam=gam_d))
    assert eq(K.paste(o_d, g_d, m_d, 0, R, fs, match_gain=True), law(rho=torch.ones_like(rho_d), gam=gam_d))
    with pytest.raises(ValueError, match="fade_law"):
        K.paste(o_d, g_d, m_d, 0, R, fs, fade_law="cubic")
