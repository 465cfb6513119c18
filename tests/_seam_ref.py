"""Float64 restatements for the fade-law tests: the junctions, zones, sums, rho and gam of alcm_seam_stats and the blend
of alcm_wave_paste_law (include/audiolcm_hip.h) as plain NumPy.  Distances are measured sample by sample on the
regenerated samples' positions (a sorted search), not frame by frame as the kernels do, and the owner of a kept sample
is decided from those two distances alone.  ``blend32`` is the blend once more in fp32, operation by operation in the
order the header states.  Nothing here touches the GPU or the package's kernels."""
import numpy as np

FAR = 1 << 40


def ramp_table(R):
    """The fade weights as the package builds them: 0.5 (1 + cos(pi d / R)) in float64, rounded to fp32."""
    d = np.arange(R, dtype=np.float64)
    return (0.5 * (1.0 + np.cos(np.pi * d / max(R, 1)))).astype(np.float32)


def geometry(mask_row, fs, N, ring):
    """Per sample n of one clip: d (0 inside a regenerated frame, FAR if there is none to measure from), ``edge`` (the
    frame edge d is measured from, -1 at d = 0 or FAR) and ``frame`` (the regenerated frame at that edge; the sample's
    own frame at d = 0, -1 at FAR).  Ties between the left and the right run go to the right one."""
    T = mask_row.size
    reg = np.repeat(mask_row > 0, fs)                     # per sample of the T frames
    n = np.arange(N)
    d = np.full(N, FAR, np.int64)
    edge = np.full(N, -1, np.int64)
    frame = np.full(N, -1, np.int64)
    if not reg.any():
        return d, edge, frame
    if ring:
        assert N == T * fs
        pos = np.flatnonzero(np.tile(reg, 3)) - N         # the ring unrolled three times, this turn at 0 .. N - 1
    else:
        pos = np.flatnonzero(reg)
    k = np.searchsorted(pos, n)                           # pos[k - 1] < n <= pos[k]
    has_l, has_r = k > 0, k < pos.size
    left = pos[np.clip(k - 1, 0, pos.size - 1)]
    right = pos[np.clip(k, 0, pos.size - 1)]
    dl = np.where(has_l, n - left, FAR)
    dr = np.where(has_r, right - n, FAR)
    inside = has_r & (dr == 0)
    go_left = ~inside & (dl < dr)
    go_right = ~inside & ~go_left & has_r
    d[inside] = 0
    frame[inside] = n[inside] // fs
    d[go_left] = dl[go_left]
    fl = np.floor_divide(left, fs)                        # the regenerated frame on the left, maybe on the turn before
    edge[go_left] = (fl[go_left] + 1) % T if ring else fl[go_left] + 1
    frame[go_left] = fl[go_left] % T if ring else fl[go_left]
    d[go_right] = dr[go_right]
    fr = np.floor_divide(right, fs)
    edge[go_right] = fr[go_right] % T if ring else fr[go_right]
    frame[go_right] = fr[go_right] % T if ring else fr[go_right]
    return d, edge, frame


def in_gen(N, gen_start, Ng, ring):
    """(inside (N,) bool, gi (N,) the sample's index in gen)."""
    gi = np.arange(N) - gen_start
    if ring:
        gi = gi % N
    return (gi >= 0) & (gi < Ng), gi


def runs(mask_row, ring):
    """The maximal runs of regenerated frames as (frames, edges): edges are the run's junctions, none for a ring
    regenerated all round; a run across the wrap of a ring is one run."""
    T = mask_row.size
    reg = mask_row > 0
    out = []
    if reg.all():
        return [(list(range(T)), [] if ring else [0, T])] if T else []
    start = 0
    if ring:
        while reg[start]:                                 # start the walk on a kept frame
            start += 1
    f = 0
    while f < T:
        if reg[(start + f) % T] if ring else reg[f]:
            g = f
            while g < T and (reg[(start + g) % T] if ring else reg[g]):
                g += 1
            frames = [(start + q) % T if ring else q for q in range(f, g)]
            edges = [frames[0], (frames[-1] + 1) % T if ring else frames[-1] + 1]
            out.append((frames, edges))
            f = g
        else:
            f += 1
    return out


def stats(orig, gen, mask, fs, gen_start, R, ring=False):
    """(rho (B, T + 1), gam (B, T), sums (B, T + 1, 3)) in float64 from orig (B, N), gen (B, Ng) and mask (B, T)."""
    B, N = orig.shape
    T, Ng = mask.shape[1], gen.shape[1]
    rho = np.ones((B, T + 1))
    gam = np.ones((B, T))
    sums = np.zeros((B, T + 1, 3))
    inside, gi = in_gen(N, gen_start, Ng, ring)
    for b in range(B):
        d, edge, _ = geometry(mask[b], fs, N, ring)
        zone = (d > 0) & (d < R) & inside
        x = orig[b].astype(np.float64)
        y = np.zeros(N)
        y[inside] = gen[b].astype(np.float64)[gi[inside]]
        for e in np.unique(edge[zone]):
            z = zone & (edge == e)
            sums[b, e] = [np.sum(x[z] * x[z]), np.sum(y[z] * y[z]), np.sum(x[z] * y[z])]
        for e in range(T + 1):
            sxx, syy, sxy = sums[b, e]
            if sxx > 0 and syy > 0:
                rho[b, e] = min(max(sxy / (np.sqrt(sxx) * np.sqrt(syy)), 0.0), 1.0)
        for frames, edges in runs(mask[b], ring):
            sxx = sum(sums[b, e, 0] for e in edges)
            syy = sum(sums[b, e, 1] for e in edges)
            if sxx > 0 and syy > 0:
                gam[b, frames] = min(max(np.sqrt(sxx / syy), 0.5), 2.0)
        if ring:
            rho[b, T], sums[b, T] = rho[b, 0], sums[b, 0]
    return rho, gam, sums


def _per_sample(orig, gen, mask, fs, gen_start, R, ring, rho, gam):
    """Per sample, float64: g, the gen sample y0 (0 outside gen), rho and gam as the paste looks them up."""
    B, N = orig.shape
    T, Ng = mask.shape[1], gen.shape[1]
    ramp = ramp_table(R).astype(np.float64)
    inside, gi = in_gen(N, gen_start, Ng, ring)
    g = np.zeros((B, N))
    y0 = np.zeros((B, N))
    rs = np.zeros((B, N))
    gs = np.ones((B, N))
    for b in range(B):
        d, edge, frame = geometry(mask[b], fs, N, ring)
        g[b] = np.where(d == 0, 1.0, 0.0)
        fade = (d > 0) & (d < R)
        g[b, fade] = ramp[d[fade]]
        g[b, ~inside] = 0.0
        y0[b, inside] = gen[b].astype(np.float64)[gi[inside]]
        live = g[b] > 0
        if rho is not None:
            rs[b, live & fade] = np.asarray(rho, np.float64)[b, edge[live & fade]]
        if gam is not None:
            gs[b, live] = np.asarray(gam, np.float64)[b, frame[live]]
    return g, y0, rs, gs


def blend(orig, gen, mask, fs, gen_start, R, ring=False, rho=None, gam=None):
    """float64 (out, g, scale): out = n ((1 - g) orig + g gam gen) with n = 1 / sqrt((1 - g)^2 + g^2 + 2 (1 - g) g rho)
    in the fade, orig at g = 0, gam gen at g = 1; scale = max(|orig|, gam |gen|) per sample, what the bar is stated on.
    rho None: 0; gam None: 1."""
    g, y0, rs, gs = _per_sample(orig, gen, mask, fs, gen_start, R, ring, rho, gam)
    o = orig.astype(np.float64)
    y = gs * y0
    a = 1.0 - g
    n = 1.0 / np.sqrt(a * a + g * g + 2.0 * a * g * rs)
    out = np.where(g == 0.0, o, np.where(g == 1.0, y, n * (a * o + g * y)))
    return out, g, np.maximum(np.abs(o), np.abs(y))


def blend_linear(orig, gen, mask, fs, gen_start, R, ring=False):
    """float64 out of the linear law, orig + g (gen - orig)."""
    g, y0, _, _ = _per_sample(orig, gen, mask, fs, gen_start, R, ring, None, None)
    o = orig.astype(np.float64)
    return o + g * (y0 - o), g


def blend32(orig, gen, mask, fs, gen_start, R, ring=False, rho=None, gam=None):
    """fp32 out, every operation rounded on its own in the header's order."""
    g, y0, rs, gs = _per_sample(orig, gen, mask, fs, gen_start, R, ring, rho, gam)
    f = np.float32
    g, y0, rs, gs, o = g.astype(f), y0.astype(f), rs.astype(f), gs.astype(f), orig.astype(f)
    y = gs * y0 if gam is not None else y0
    a = f(1.0) - g
    s = (a * o) + (g * y)
    p = ((a * a) + (g * g)) + (((a + a) * g) * rs)
    out = (f(1.0) / np.sqrt(p)) * s
    assert out.dtype == f
    return np.where(g == 0, o, np.where(g == 1, y, out))


def zone_power(out, g, outside):
    """Mean square of ``out`` over the samples of 0 < g < 1 relative to its mean square over ``outside`` (bool)."""
    z = (g > 0) & (g < 1)
    return float(np.mean(out[z] ** 2) / np.mean(out[outside] ** 2))
