"""alcm_wave_paste through the C-ABI against a float64 numpy restatement of its definition (include/audiolcm_hip.h):
with d the distance in samples to the nearest sample of a regenerated frame of the same clip, out is gen at d = 0, orig
from d = R on and outside gen, both bit for bit, and orig + ramp[d] * (gen - orig) in between.

The blended samples are held to 1e-6 absolute: three fp32 roundings on magnitudes <= 2 against the float64 evaluation
of the same fp32 table is <= 4e-7 (the bar test_gpu_edit_ops.py uses for blended values)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, FS = 2, 12, 512
N_FULL = T * FS            # 6144
RS = [0, 1, 64, 512, 700, 2048]


def _mask(*rows):
    m = np.zeros((B, T), dtype=np.float32)
    for b, frames in enumerate(rows):
        m[b, list(frames)] = 1.0
    return m


MASKS = {
    "empty": _mask((), ()),
    "full": _mask(range(T), range(T)),
    "interior": _mask((5, 6), (5, 6)),
    "start": _mask((0, 1), (0, 1)),
    "end": _mask((10, 11), (10, 11)),
    "two_close": _mask((3, 5), (3, 5)),          # one kept frame between them: closer than 2R from R = 257 on
    "per_clip": _mask((2, 3, 9), ()),            # a different mask per clip, one clip all zero
}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


@pytest.fixture(scope="module")
def waves():
    """Per N, once: orig and a whole-clip gen, uniform in [-1, 1], on the host and on the device."""
    out = {}
    for N in (N_FULL, N_FULL - 37):
        g = np.random.default_rng(N)
        orig = g.uniform(-1, 1, (B, N)).astype(np.float32)
        gen = g.uniform(-1, 1, (B, N)).astype(np.float32)
        out[N] = (orig, gen, torch.from_numpy(orig).cuda(), torch.from_numpy(gen).cuda())
    return out


def _distance(mask, N):
    """(B, N) int64: samples to the nearest sample of a regenerated frame of the same clip (a large value if none)."""
    d = np.full((mask.shape[0], N), 1 << 40, dtype=np.int64)
    n = np.arange(N)
    for b in range(mask.shape[0]):
        idx = np.flatnonzero(np.repeat(mask[b] > 0, FS)[:N])
        if idx.size:
            pos = np.searchsorted(idx, n)
            left, right = idx[np.clip(pos - 1, 0, idx.size - 1)], idx[np.clip(pos, 0, idx.size - 1)]
            d[b] = np.minimum(np.abs(n - left), np.abs(n - right))
    return d


def _reference(orig, gen_part, mask, gen_start, R):
    """float64 out, and the two exact sets: keep (orig bit for bit) and take (gen bit for bit)."""
    from audiolcm_amd.kernels import paste_ramp_host
    N, Ng = orig.shape[1], gen_part.shape[1]
    d = _distance(mask, N)
    ramp = paste_ramp_host(R).numpy().astype(np.float64)
    g = np.where(d == 0, 1.0, 0.0)
    if R:
        g = np.where((d > 0) & (d < R), ramp[np.minimum(d, R - 1)], g)
    inside = np.zeros_like(d, dtype=bool)
    inside[:, gen_start:gen_start + Ng] = True
    g = np.where(inside, g, 0.0)
    gen = np.zeros(orig.shape, dtype=np.float64)
    gen[:, gen_start:gen_start + Ng] = gen_part
    o = orig.astype(np.float64)
    return o + g * (gen - o), g == 0.0, g == 1.0


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("name", list(MASKS))
def test_wave_paste_matches_the_definition(K, waves, name, R):
    mask = MASKS[name]
    mask_d = torch.from_numpy(mask).cuda()
    if name == "two_close" and R >= 512:
        d = _distance(mask, N_FULL)[0, 4 * FS:5 * FS]      # the kept frame between the spans: the nearer span wins
        assert d.max() == FS // 2 and d[0] == 1 and d[-1] == 1
    worst = 0.0
    # gen covers the whole clip; a sub-range at a start that is no multiple of 4; a 16-byte aligned sub-range
    for N in (N_FULL, N_FULL - 37):
        orig, gen, orig_d, gen_d = waves[N]
        for gen_start, Ng in ((0, N), (1021, 3001), (1024, 3072)):
            part, part_d = gen[:, gen_start:gen_start + Ng], gen_d[:, gen_start:gen_start + Ng].contiguous()
            ref, keep, take = _reference(orig, part, mask, gen_start, R)
            if gen_start == 0:
                assert take.any() == bool(mask.any()) and (name != "full" or take.all())
            full_gen = np.zeros_like(orig)
            full_gen[:, gen_start:gen_start + Ng] = part
            for inplace in (False, True):
                if inplace:
                    dst = orig_d.clone()
                    got = K.wave_paste(dst, part_d, mask_d, gen_start, R, FS, out=dst)
                    assert got.data_ptr() == dst.data_ptr()
                else:
                    got = K.wave_paste(orig_d, part_d, mask_d, gen_start, R, FS)
                    assert got.data_ptr() != orig_d.data_ptr()
                got = got.cpu().numpy()
                assert np.array_equal(got[keep], orig[keep]), (name, R, N, gen_start, inplace)
                assert np.array_equal(got[take], full_gen[take]), (name, R, N, gen_start, inplace)
                worst = max(worst, float(np.abs(got - ref).max()))
        assert torch.equal(orig_d, torch.from_numpy(orig).cuda())     # the out-of-place form leaves orig alone
    print(f"wave_paste {name} R={R}: max abs error {worst:.2e}")
    assert worst <= 1e-6


def test_wave_paste_unaligned_views_take_the_element_path(K, waves):
    """The same values at addresses that are 4 mod 16 give the same bits."""
    orig, gen, orig_d, gen_d = waves[N_FULL]
    mask_d = torch.from_numpy(MASKS["interior"]).cuda()
    want = K.wave_paste(orig_d, gen_d, mask_d, 0, 700, FS)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(t.shape)
    for o, g in ((shifted(orig_d), gen_d), (orig_d, shifted(gen_d))):
        assert torch.equal(K.wave_paste(o, g, mask_d, 0, 700, FS), want)


def test_wave_paste_bad_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd._hip import lib, ptr, stream_handle
    from audiolcm_amd.kernels import paste_ramp
    orig = torch.full((1, 2048), 0.25, device="cuda")
    gen = torch.full((1, 2048), -0.5, device="cuda")
    out = torch.full((1, 2048), 7.0, device="cuda")
    mask = torch.ones((1, 4), device="cuda")
    L, s = lib(), stream_handle()
    po, pg, pm, pr, pd = ptr(orig), ptr(gen), ptr(mask), ptr(paste_ramp(64, "cuda")), ptr(out)

    def call(o=po, g=pg, m=pm, r=pr, d=pd, B=1, N=2048, start=0, Ng=2048, T=4, fs=512, R=64):
        return L.alcm_wave_paste(o, g, m, r, d, B, N, start, Ng, T, fs, R, s)
    assert call(o=None) != 0 and call(g=None) != 0 and call(m=None) != 0 and call(r=None) != 0 and call(d=None) != 0
    assert b"wave_paste" in L.alcm_last_error()
    assert call(B=-1) != 0 and call(N=-1) != 0 and call(start=-1) != 0 and call(Ng=-1) != 0 and call(T=-1) != 0
    assert call(fs=0) != 0 and call(fs=-512) != 0 and call(R=-1) != 0
    assert call(T=3) != 0                      # T * frame_samples < N
    assert call(start=1, Ng=2048) != 0         # gen reaches past the clip
    assert call(R=16 * 512 + 1) != 0           # R is limited to 16 frames
    assert call(fs=4, T=512, R=65) != 0        # ... of the frame length in use
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())            # none of these launched
    # the empty cases return 0 without a launch
    assert call(B=0) == 0 and call(N=0, Ng=0, T=0) == 0
    assert call(d=po, Ng=0, g=None) == 0       # in place with nothing to blend
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((orig == 0.25).all())
    assert call(R=0, r=None) == 0              # R = 0 needs no table: a hard switch
    torch.cuda.synchronize()
    assert bool((out == -0.5).all())
