"""The fused attention's production variants and length edges, element by element.

alcm_flash_attention_ex reaches every form the models launch (fp32 rows or an fp16 / bf16 plane in, fp32 or a plane
out, T5's score bias with its pitch, an explicit scale); alcm_softmax_rows_bias / alcm_softmax_rows with ld > n are the
split policy's softmax of the same scores.  The reference is plain fp64 torch on the CPU:

    q, k, v = the operands rounded to the kernel's format, per (b, head)
    S = scale * q k^T (+ bias[h, :L, :L]);  P = softmax(S, -1);  R = P v;  A = P |v|

Per-element bound (derived, not measured).  The kernels round only the unnormalised probabilities p in (0, 1] to the
operand format before the P.V MFMA; the normaliser l is summed from the unrounded fp32 p.  With u = 2^-11 (fp16) or
2^-8 (bf16) the first-order error of an element is u * A; a plane output rounds the result once more, u * |R|; an
fp16 p below 2^-14 is subnormal (absolute error <= 2^-25 a key, and l >= 1), which adds L * 2^-25 * max|v|:

    |got - R| <= 2 u (A + [plane out] |R|) + [fp16] L 2^-25 max|v| + 1e-6 max|v|

The factor 2 is margin over the first-order term (the fp32 score accumulation, the hardware exp2); the last term is
fp32 output noise.  The factor was derived and validated against a CPU emulation of the kernels' arithmetic only
(64-key tiles, running max in the log2 domain, p rounded per tile, l from the unrounded p: under half the bound).

test_mutants_exceed_the_bound (no GPU) proves that these inputs tell a wrong kernel from a right one: a transposed
bias, the next head's bias, a dropped last key, scale 1 for dh^-1/2 and one phantom key (a mask off by one, an
unzeroed LDS row) each exceed the bound at least tenfold at some element.

Worst |got - R| / bound measured on an MI355X, per (kernel, prec, output format) over every case of this file:
    resident  fp16  fp32 out   0.445   B2 L64 heads3 dh64 plain, fp32 in, bias pitch 64
    resident  fp16  plane out  0.390   B2 L64 heads3 dh64 plain, fp32 in, bias pitch 64
    resident  bf16  fp32 out   0.415   B2 L77 heads3 dh64 plain, fp32 in, scale 0.25
    resident  bf16  plane out  0.411   B2 L449 heads3 dh64 steep, plane in
    tiled     fp16  fp32 out   0.250   B1 L576 heads2 dh64 mixed
    tiled     fp16  plane out  0.274   B1 L577 heads2 dh64 low
    tiled     bf16  fp32 out   0.315   B2 L845 heads3 dh64 mixed
    tiled     bf16  plane out  0.279   B1 L577 heads2 dh64 mixed
(the module prints them again, per case and as a table when it is done, under pytest -s)
"""
import functools

import pytest
import torch

U = {2: 2.0 ** -11, 0: 2.0 ** -8}       # _hip.PREC_F16, PREC_BF16: unit roundoff of the operand format
PRECS = [2, 0]
RES_L = [1, 15, 16, 17, 63, 64, 65, 77, 449, 511, 512]     # resident-K/V kernel: key-tile / query-block edges, the cap
TILED_L = [513, 575, 576, 577, 845, 1024]                  # tiled kernel: the switch, 64-query tile edges, the DiT cap
TILED_BH = {513: (1, 1), 1024: (1, 2), 845: (2, 3)}        # workgroups mod 8: 9 -> 1, 32 -> 0, 84 -> 4 (XCD remap)
PATTERN_L = [200, 449]
MASK_L = [1, 15, 17, 63, 65, 511]       # the "all scores low" input at the key-mask edges of the resident kernel


def rnd(x, prec):
    return x.half().float() if prec == 2 else x.bfloat16().float()


def to_plane(x, prec):
    return (x.half() if prec == 2 else x.bfloat16()).view(torch.int16)


def from_plane(p, prec):
    return p.view(torch.float16 if prec == 2 else torch.bfloat16).float()


def _randn(shape, seed, std):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


@functools.lru_cache(maxsize=None)
def make_qkv(B, L, heads, dh, pattern="plain", scale=0.0):
    """q, k, v (B, heads, L, dh) fp32 ~ N(0, 1.5^2), one seed per tensor, distinct per head and per clip."""
    sc = scale if scale > 0 else dh ** -0.5
    w = 4.5 if pattern == "large" else 1.5          # large: |S| of several hundred at scale 1, far inside fp16's range
    q, k, v = (_randn((B, heads, L, dh), 7000 + 13 * L + i, s) for i, s in enumerate((w, w, 1.5)))
    trend = (torch.arange(L, dtype=torch.float32) / L - 0.5)
    alt = 1.0 - 2.0 * (torch.arange(L) % 2).float()
    if pattern in ("ascending", "descending", "mixed", "steep", "steep_mixed"):
        # ascending: the running max moves in every key tile; descending: (mostly) never after tile 0, the resident
        # kernel's skip-the-rescale branch; mixed: within one 16-query block some maxima move and some do not.
        # steep*: the descending trend at 32x, so that no maximum moves after tile 0 whatever the other dims draw
        # (k[..., 0] within +-133, scores within +-90)
        slope = {"ascending": 8.0, "descending": -8.0, "mixed": 8.0, "steep": -256.0, "steep_mixed": -256.0}[pattern]
        q[..., 0] = q[..., 0].abs() + 1
        if pattern in ("mixed", "steep_mixed"):
            q[..., 0] *= alt
        k[..., 0] += slope * trend
    elif pattern == "low":      # all scores about -12: one phantom key of score 0 would take most of the softmax mass
        c = (12.0 / sc) ** 0.5
        q[..., 0] = c
        k[..., 0] = -c
    else:
        assert pattern in ("plain", "large"), pattern
    return q, k, v


@functools.lru_cache(maxsize=None)
def make_bias(heads, bld, offset=0.0):
    """[heads][bld][bld] ~ N(0, 2^2): not symmetric, different per head."""
    return (_randn((heads, bld, bld), 7900 + bld, 2.0) + offset).contiguous()


def pack(q, k, v):
    """(B, heads, L, dh) x 3 -> (B, L, 3H) rows [q | k | v], head h at columns h * dh."""
    f = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)
    return torch.cat([f(q), f(k), f(v)], -1).contiguous()


def attend(q, k, v, scale, bias=None):
    """fp64 attention of (B, heads, L, dh) operands -> R, A as (B, L, H); bias (heads, L, Lk) or None."""
    q, k, v = q.double(), k.double(), v.double()
    S = scale * q @ k.transpose(-1, -2)
    if bias is not None:
        S = S + bias.double()
    P = torch.softmax(S, -1)
    f = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)
    return f(P @ v), f(P @ v.abs())


@functools.lru_cache(maxsize=None)
def reference(B, L, heads, dh, pattern, prec, scale=0.0, bld=0, boff=0.0):
    """R, A, max|v| of the case (computed once, shared by the forms and tests that use the case)."""
    q, k, v = (rnd(t, prec) for t in make_qkv(B, L, heads, dh, pattern, scale))
    bias = make_bias(heads, bld, boff)[:, :L, :L] if bld else None
    R, A = attend(q, k, v, scale if scale > 0 else dh ** -0.5, bias)
    return R, A, float(v.abs().max())


def bound(R, A, vmax, prec, plane_out, L):
    b = 2 * U[prec] * (A + (R.abs() if plane_out else 0)) + 1e-6 * vmax
    return b + L * 2.0 ** -25 * vmax if prec == 2 else b


# ------------------------------------------------------------------------------------------------ CPU: mutants
def _mutants(q, k, v, scale, bias, heads):
    """name -> (R of a reference that is wrong in one way).  bias: (heads, L, L) or None."""
    out = {}
    if q.shape[2] == 1:         # one key: the softmax is 1 whatever the score
        return out
    if bias is not None:
        out["bias transposed"] = attend(q, k, v, scale, bias.transpose(-1, -2))[0]
        if heads > 1:
            out["bias of head h+1"] = attend(q, k, v, scale, bias.roll(-1, 0))[0]
    out["last key dropped"] = attend(q, k[:, :, :-1], v[:, :, :-1], scale,
                                     None if bias is None else bias[:, :, :-1])[0]
    out["scale 1.0"] = attend(q, k, v, 1.0, bias)[0]
    return out


def _phantom(q, k, v, scale, bias):
    """One more key at index L with k = v = 0 and the bias of column L - 1."""
    z = torch.zeros_like(k[:, :, :1])
    b = None if bias is None else torch.cat([bias, bias[:, :, -1:]], -1)
    return attend(q, torch.cat([k, z], 2), torch.cat([v, z], 2), scale, b)[0]


def _worst(mut, R, A, vmax, prec, L):
    return float(((mut - R).abs() / bound(R, A, vmax, prec, True, L)).max())   # plane out: the wider of the bounds


@pytest.mark.parametrize("prec", PRECS)
def test_mutants_exceed_the_bound(prec):
    """On the inputs of the GPU cases a reference that is wrong in one way exceeds the bound >= 10x at some element,
    for every L and both precs.  (At L = 1 the softmax is 1 whatever the score: only the phantom key can show.)"""
    B, heads, dh = 2, 3, 64
    low = []
    for L in RES_L + TILED_L:
        bh = TILED_BH.get(L, (1, 2)) if L > 512 else (B, heads)
        bld = L if L <= 512 else 0                      # the bias exists only on the resident kernel
        q, k, v = (rnd(t, prec) for t in make_qkv(bh[0], L, bh[1], dh, "plain", 0.0))
        bias = make_bias(bh[1], bld)[:, :L, :L] if bld else None
        R, A, vmax = reference(bh[0], L, bh[1], dh, "plain", prec, 0.0, bld, 0.0)
        for name, mut in _mutants(q, k, v, dh ** -0.5, bias, bh[1]).items():
            low.append((name, L, _worst(mut, R, A, vmax, prec, L)))
    # the phantom key on the "all scores low" input, with and without the bias (offset -12), where the GPU runs it
    for L in MASK_L + PATTERN_L + TILED_L:
        bh = TILED_BH.get(L, (1, 2)) if L > 512 else (B, heads)
        for bld, boff in ((0, 0.0), (L, -12.0)) if L <= 512 else ((0, 0.0),):
            q, k, v = (rnd(t, prec) for t in make_qkv(bh[0], L, bh[1], dh, "low", 0.0))
            bias = make_bias(bh[1], bld, boff)[:, :L, :L] if bld else None
            R, A, vmax = reference(bh[0], L, bh[1], dh, "low", prec, 0.0, bld, boff)
            low.append(("phantom key" + (" + bias" if bld else ""), L,
                        _worst(_phantom(q, k, v, dh ** -0.5, bias), R, A, vmax, prec, L)))
    print(f"prec {prec}: weakest mutants", sorted(low, key=lambda t: t[2])[:5])
    assert not [t for t in low if t[2] < 10], [t for t in low if t[2] < 10]


@functools.lru_cache(maxsize=None)
def softmax_case(n, bld, ld, L):
    """scores (rows, ld) with NaN in [n, ld), the bias table, and the scores as fp64 (B, heads, L, n)."""
    B, heads = 2, 3
    x = _randn((B * heads * L, ld), 8100 + n, 2.0)
    x[:, n:] = float("nan")
    bias = make_bias(heads, bld)
    xs = x[:, :n].double().reshape(B, heads, L, n)
    return x, bias, xs


# (n keys, bias pitch, row pitch, L query rows per (clip, head)): square as the models launch it, and one case with
# L != n, where a row -> (z, i, h) decomposition by n instead of L would show
SOFTMAX_CASES = [(n, bld, ld, n) for n in (1, 20, 63, 64, 65, 77) for bld in (n, 80)
                 for ld in ((n + 7) // 8 * 8, n + 13)] + [(20, 80, 24, 33)]


@pytest.mark.parametrize("n,bld,ld,L", [c for c in SOFTMAX_CASES if c[0] > 1])
def test_softmax_mutants_exceed_the_tolerance(n, bld, ld, L):
    """The softmax_rows_bias reference with the bias transposed / of the next head misses rtol 1e-5, atol 1e-7 by
    >= 10x at some element (n = 1: the softmax is 1 whatever the bias)."""
    _, bias, xs = softmax_case(n, bld, ld, L)
    b = bias[:, :L, :n].double()
    ref = torch.softmax(xs + b, -1)
    for name, mb in (("transposed", bias[:, :n, :L].double().transpose(-1, -2)), ("head h+1", b.roll(-1, 0))):
        mut = torch.softmax(xs + mb, -1)
        assert float(((mut - ref).abs() / (1e-7 + 1e-5 * ref.abs())).max()) >= 10, name


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


@pytest.fixture(scope="module")
def worst():
    """Worst |got - R| / bound per (kernel, prec, output format), printed when the module is done."""
    w = {}
    yield w
    for key in sorted(w):
        print(f"\nworst |d|/bound {key}: {w[key][0]:.3f} at {w[key][1]}", end="")
    print()


def launch(K, qkv, heads, prec, in_plane=False, out_plane=False, bias=None, scale=0.0):
    """One fused-attention call -> (fp32 (B, L, H) result on the CPU, the raw output); asserts which kernel
    instantiation ran (the profile's kernel names)."""
    from audiolcm_amd import _hip
    L = qkv.shape[1]
    kw = dict(bias=None if bias is None else bias.cuda(), scale=scale, out_plane=out_plane)
    _hip.profile_begin()
    if in_plane:
        y = K.flash_attention(None, heads, prec, qkv_plane=to_plane(qkv, prec).cuda(), **kw)
    else:
        y = K.flash_attention(qkv.cuda(), heads, prec, **kw)
    torch.cuda.synchronize()
    names = [p["name"] for p in _hip.profile_end()]
    tf = lambda b: "true" if b else "false"
    want = (f"alcm::flash_attn_res_kernel<{prec}, {tf(bias is not None)}, {tf(in_plane)}>" if L <= 512
            else f"alcm::flash_attn_kernel<{prec}>")
    assert names == [want], (names, want)
    y = y.cpu()
    return (from_plane(y, prec) if out_plane else y), y


def check(K, worst, B, L, heads, dh, pattern, prec, in_plane, out_plane, bld=0, boff=0.0, scale=0.0):
    q, k, v = make_qkv(B, L, heads, dh, pattern, scale)
    R, A, vmax = reference(B, L, heads, dh, pattern, prec, scale, bld, boff)
    got, _ = launch(K, pack(q, k, v), heads, prec, in_plane, out_plane, make_bias(heads, bld, boff) if bld else None,
                    scale)
    assert got.shape == R.shape and bool(torch.isfinite(got).all())
    ratio = (got.double() - R).abs() / bound(R, A, vmax, prec, out_plane, L)
    r = float(ratio.max())
    case = (f"B{B} L{L} heads{heads} dh{dh} {pattern} in={'plane' if in_plane else 'fp32'} bld={bld} scale={scale}")
    key = ("resident" if L <= 512 else "tiled", "fp16" if prec == 2 else "bf16", "plane" if out_plane else "fp32")
    print(f"{key} {case}: worst |d|/bound {r:.3f}")
    if r > worst.get(key, (0.0, ""))[0]:
        worst[key] = (r, case)
    idx = divmod(int(ratio.argmax()), ratio.shape[-1])
    assert r <= 1.0, (key, case, r, "at (row, column)", idx)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("L", RES_L)
def test_resident_forms(K, worst, L, biased, prec):
    """Every input form {fp32, plane} x output form {fp32, plane}, with and without the bias (pitch = L)."""
    for in_plane in (False, True):
        for out_plane in (False, True):
            check(K, worst, 2, L, 3, 64, "plain", prec, in_plane, out_plane, bld=L if biased else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L,bld", [(20, 77), (77, 77), (77, 80)])
def test_resident_bias_pitch(K, worst, L, bld, prec):
    """The bias is the full [heads][bld][bld] table with bld >= L (T5: bld = max_len); the corner [:L, :L] counts."""
    for in_plane, out_plane in ((True, True), (False, False)):
        check(K, worst, 2, L, 3, 64, "plain", prec, in_plane, out_plane, bld=bld)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L", [77, 130])
@pytest.mark.parametrize("dh", [4, 36, 64, 68, 72])
def test_head_dims(K, worst, dh, L, prec):
    """dh = 4 .. 72: the zero-padded K dims and the masked V rows."""
    for in_plane, out_plane in ((True, True), (False, False)):
        check(K, worst, 2, L, 2, dh, "plain", prec, in_plane, out_plane)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L", PATTERN_L)
@pytest.mark.parametrize("pattern", ["ascending", "descending", "mixed", "steep", "steep_mixed", "low", "large"])
def test_data_patterns(K, worst, pattern, L, prec):
    """Running maxima that move in every tile, in none (the skipped rescale), in some lanes of a block only; scores
    all low; T5's unscaled large scores.  Plane in, plane out; low and large with the bias.  Whether the resident
    kernel takes its skip-the-rescale branch cannot be seen from outside: descending / steep / steep_mixed reach it by
    construction of the data only (steep and steep_mixed make the trend dominate the other 63 dims)."""
    if pattern == "low":
        check(K, worst, 2, L, 3, 64, pattern, prec, True, True, bld=L, boff=-12.0)
    elif pattern == "large":
        check(K, worst, 2, L, 3, 64, pattern, prec, True, True, bld=L, scale=1.0)
    else:
        check(K, worst, 2, L, 3, 64, pattern, prec, True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L", MASK_L)
def test_resident_key_mask(K, worst, L, prec):
    """All scores low at the key-mask edges: a key >= L left in the softmax (score 0) would take most of its mass."""
    check(K, worst, 2, L, 3, 64, "low", prec, True, True)
    check(K, worst, 2, L, 3, 64, "low", prec, False, False, bld=L, boff=-12.0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_explicit_scale(K, worst, prec):
    """scale = 0.25 at dh = 64 (not the default 0.125: a dropped argument shows); scale = 0 equals an explicit
    dh^-1/2 bit for bit."""
    for in_plane, out_plane in ((True, True), (False, False)):
        check(K, worst, 2, 77, 3, 64, "plain", prec, in_plane, out_plane, scale=0.25)
    for dh in (64, 36):
        qkv = pack(*make_qkv(2, 77, 3, dh))
        for in_plane in (False, True):
            a = launch(K, qkv, 3, prec, in_plane, False)[1]
            b = launch(K, qkv, 3, prec, in_plane, False, scale=dh ** -0.5)[1]
            assert torch.equal(a, b), (dh, in_plane)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pattern", ["plain", "mixed", "low"])
@pytest.mark.parametrize("L", TILED_L)
def test_tiled(K, worst, L, pattern, prec):
    """The 64-query tiled kernel (L > 512), fp32 and plane out; (B, heads) put its grid at 1, 0 and 4 mod 8 for the
    XCD work-id remap."""
    B, heads = TILED_BH.get(L, (1, 2))
    for out_plane in (False, True):
        check(K, worst, B, L, heads, 64, pattern, prec, False, out_plane)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L,in_plane,biased", [(77, True, True), (449, False, False), (577, False, False)])
def test_clips_are_independent(K, L, in_plane, biased, prec):
    """Each (b, head) is its own workgroup(s): clip 1 of a B = 3 call equals the same clip run alone."""
    heads = 2
    qkv = pack(*make_qkv(3, L, heads, 64))
    bias = make_bias(heads, 80) if biased else None
    for out_plane in (False, True):
        full = launch(K, qkv, heads, prec, in_plane, out_plane, bias)[1]
        one = launch(K, qkv[1:2].contiguous(), heads, prec, in_plane, out_plane, bias)[1]
        assert torch.equal(full[1:2], one), (L, out_plane)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L,biased", [(77, True), (449, False), (845, False)])
def test_plane_forms_agree_bitwise(K, L, biased, prec):
    """The plane output is the fp32 output rounded to the format, and the plane input gives what the fp32 input
    holding exactly the plane's values gives, bit for bit."""
    heads = 2
    qkv = rnd(pack(*make_qkv(2, L, heads, 64)), prec)          # exactly representable in the format
    bias = make_bias(heads, L) if biased else None
    f32 = launch(K, qkv, heads, prec, False, False, bias)[1]
    pl = launch(K, qkv, heads, prec, False, True, bias)[1]
    assert torch.equal(pl, to_plane(f32, prec))
    if L <= 512:
        assert torch.equal(launch(K, qkv, heads, prec, True, False, bias)[1], f32)
        assert torch.equal(launch(K, qkv, heads, prec, True, True, bias)[1], pl)


@pytest.mark.gpu
def test_error_returns(K):
    """Shapes the host checks reject before any launch."""
    def call(B, L, heads, dh, prec=2, in_plane=False, both=False, bld=0, scale=0.0):
        H = heads * dh
        x = torch.zeros((B, L, 3 * H), device="cuda")
        p = torch.zeros((B, L, 3 * H), device="cuda", dtype=torch.int16) if (in_plane or both) else None
        bias = torch.zeros((heads, bld, bld), device="cuda") if bld else None
        with pytest.raises(RuntimeError):
            K.flash_attention(None if in_plane else x, heads, prec, bias=bias, scale=scale, qkv_plane=p,
                              out_plane=True)
    call(1, 20, 2, 76)                          # dh > 72
    call(1, 20, 2, 76, in_plane=True)
    call(1, 20, 2, 70)                          # dh % 4
    call(1, 20, 2, 70, in_plane=True)
    call(1, 20, 2, 64, prec=1)                  # the split format has no fused attention
    call(1, 20, 2, 64, prec=1, in_plane=True)
    call(1, 513, 2, 64, bld=513)                # bias, scale, plane input: the resident kernel only (L <= 512)
    call(1, 513, 2, 64, scale=0.125)
    call(1, 513, 2, 64, in_plane=True)
    call(1, 20, 2, 64, both=True)               # qkv and qkv_plane
    call(1, 20, 2, 64, bld=19)                  # bias pitch < L
    call(1, 20, 2, 64, bld=19, in_plane=True)
    x = torch.zeros((2 * 3 * 20, 24), device="cuda")
    with pytest.raises(RuntimeError):           # bias rows i < L need bld >= L
        K.softmax_bias_(x[:, :10], torch.zeros((3, 16, 16), device="cuda"), 20, ld=24)
    with pytest.raises(RuntimeError):           # bld < n
        K.softmax_bias_(x[:, :20], torch.zeros((3, 16, 16), device="cuda"), 20, ld=24)


@pytest.mark.gpu
@pytest.mark.parametrize("n,bld,ld,L", SOFTMAX_CASES)
def test_softmax_rows_bias_and_padding(K, n, bld, ld, L):
    """softmax_rows_bias and softmax_rows on (rows, ld) buffers with ld > n vs the fp64 softmax of x + bias[h, i, :n]
    (of x); the columns [n, ld), NaN before the call, come back exactly 0."""
    import numpy as np
    x, bias, xs = softmax_case(n, bld, ld, L)
    for biased in (True, False):
        buf = x.cuda()
        if biased:
            K.softmax_bias_(buf[:, :n], bias.cuda(), L, ld=ld)
            ref = torch.softmax(xs + bias[:, :L, :n].double(), -1)
        else:
            K.softmax_(buf[:, :n], ld=ld)
            ref = torch.softmax(xs, -1)
        got = buf.cpu()
        np.testing.assert_allclose(got[:, :n].numpy(), ref.reshape(-1, n).numpy(), rtol=1e-5, atol=1e-7)
        assert ld == n or bool((got[:, n:] == 0).all())
