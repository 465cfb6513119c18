"""alcm_wave_paste_ring through the C-ABI against a float64 numpy restatement of its definition
(include/audiolcm_hip.h): alcm_wave_paste on one period of a loop.  With d the distance in samples, measured round the
ring, to the nearest sample of a regenerated frame of the same clip, out is gen at d = 0, orig from d = R on and outside
gen, both bit for bit, and orig + ramp[d] * (gen - orig) in between; gen holds the ring's samples (gen_start + i) mod N.

The blended samples are held to 1e-6 absolute on magnitudes <= 1: three fp32 roundings against the float64 evaluation of
the same fp32 table, the bar tests/test_gpu_paste_ops.py states for the same fma form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 2, 24
FRAME = [512, 6]           # 6: no multiple of 4, the element path


def _mask(*rows, frames=T):
    m = np.zeros((B, frames), dtype=np.float32)
    for b, f in enumerate(rows):
        m[b, list(f)] = 1.0
    return m


MASKS = {
    "empty": _mask((), ()),
    "full": _mask(range(T), range(T)),
    "seam": _mask((T - 2, T - 1, 0, 1), (T - 1, 0)),
    "last": _mask((T - 1,), (T - 1,)),          # fades into the first samples of frame 0
    "first": _mask((0,), (0,)),                 # fades into the end of frame T - 1
    "interior": _mask((10, 11), (10, 11)),
    "per_clip": _mask((2, 3, 21), ()),          # a different mask per clip, one clip all zero
}


def _gens(fs):
    """(gen_start, Ng): the whole ring; a gen that wraps, 16-byte aligned at 512 samples per frame; one that wraps at a
    start and a length that are no multiples of 4; the whole ring from the middle of it on."""
    N = T * fs
    return [(0, N), (20 * fs, 8 * fs), (20 * fs + 1, 8 * fs - 3), (3 * fs, N)]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from audiolcm_amd import _hip, kernels
    _hip.require_device(0)
    return kernels


@pytest.fixture(scope="module")
def waves():
    """Per N, once: orig and a ring of gen samples, uniform in [-1, 1], on the host and on the device."""
    cache = {}

    def get(N):
        if N not in cache:
            g = np.random.default_rng(N)
            orig = g.uniform(-1, 1, (B, N)).astype(np.float32)
            gen = g.uniform(-1, 1, (B, N)).astype(np.float32)
            cache[N] = (orig, gen, torch.from_numpy(orig).cuda(), torch.from_numpy(gen).cuda())
        return cache[N]
    return get


def _ring_distance(mask, fs):
    """(B, N) int64: samples round the ring to the nearest sample of a regenerated frame (a large value if none)."""
    N = mask.shape[1] * fs
    d = np.full((mask.shape[0], N), 1 << 40, dtype=np.int64)
    n = np.arange(N, 2 * N)
    for b in range(mask.shape[0]):
        idx = np.flatnonzero(np.tile(np.repeat(mask[b] > 0, fs), 3))        # the ring unrolled three times
        if idx.size:
            pos = np.searchsorted(idx, n)
            left, right = idx[np.clip(pos - 1, 0, idx.size - 1)], idx[np.clip(pos, 0, idx.size - 1)]
            d[b] = np.minimum(np.abs(n - left), np.abs(n - right))
    return d


def _part(gen, gen_start, Ng):
    """The gen argument (B, Ng): the ring's samples (gen_start + i) mod N."""
    return np.ascontiguousarray(gen[:, (gen_start + np.arange(Ng)) % gen.shape[1]])


def _reference(orig, gen, mask, fs, gen_start, Ng, R):
    """float64 out, the two exact sets keep (orig bit for bit) and take (gen bit for bit), and the ring's gen."""
    from audiolcm_amd.kernels import paste_ramp_host
    N = orig.shape[1]
    d = _ring_distance(mask, fs)
    ramp = paste_ramp_host(R).numpy().astype(np.float64)
    g = np.where(d == 0, 1.0, 0.0)
    if R:
        g = np.where((d > 0) & (d < R), ramp[np.minimum(d, R - 1)], g)
    inside = ((np.arange(N) - gen_start) % N) < Ng
    g = np.where(inside[None], g, 0.0)
    o = orig.astype(np.float64)
    return o + g * (gen.astype(np.float64) - o), g == 0.0, g == 1.0


@pytest.mark.parametrize("fs", FRAME)
@pytest.mark.parametrize("Rf", [0, 7, 512, "16 frames"])
@pytest.mark.parametrize("name", list(MASKS))
def test_wave_paste_ring_matches_the_definition(K, waves, name, Rf, fs):
    R = 16 * fs if Rf == "16 frames" else min(Rf, 16 * fs)     # at 6 samples per frame 512 is past the limit of 96
    N = T * fs
    mask = MASKS[name]
    mask_d = torch.from_numpy(mask).cuda()
    orig, gen, orig_d, gen_d = waves(N)
    d = _ring_distance(mask, fs)
    if name == "last" and R > 1:        # frame T - 1 regenerated: the first R - 1 samples of frame 0 are faded
        assert d[0, 0] == 1 and d[0, min(R, 2 * fs) - 2] == min(R, 2 * fs) - 1
    if name == "first" and R > 1:       # and a regenerated frame 0 fades into the end of frame T - 1
        assert d[0, N - 1] == 1 and d[0, N - (min(R, 2 * fs) - 1)] == min(R, 2 * fs) - 1
    worst = 0.0
    for gen_start, Ng in _gens(fs):
        part_d = torch.from_numpy(_part(gen, gen_start, Ng)).cuda()
        ref, keep, take = _reference(orig, gen, mask, fs, gen_start, Ng, R)
        if Ng == N:
            assert take.any() == bool(mask.any()) and (name != "full" or take.all())
            if name in ("last", "first") and R > 1:
                faded = ~keep & ~take
                assert faded[0, :R - 1].all() if name == "last" else faded[0, N - R + 1:].all()
        for inplace in (False, True):
            if inplace:
                dst = orig_d.clone()
                got = K.wave_paste_ring(dst, part_d, mask_d, gen_start, R, fs, out=dst)
                assert got.data_ptr() == dst.data_ptr()
            else:
                got = K.wave_paste_ring(orig_d, part_d, mask_d, gen_start, R, fs)
                assert got.data_ptr() != orig_d.data_ptr()
            got = got.cpu().numpy()
            assert np.array_equal(got[keep], orig[keep]), (name, R, gen_start, inplace)
            assert np.array_equal(got[take], gen[take]), (name, R, gen_start, inplace)
            worst = max(worst, float(np.abs(got - ref).max()))
    assert torch.equal(orig_d, torch.from_numpy(orig).cuda())     # the out-of-place form leaves orig alone
    print(f"wave_paste_ring {name} R={R} fs={fs}: max abs error {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("fs", FRAME)
def test_in_place_visits_only_the_frames_gen_covers(K, waves, fs):
    """In place the frames gen does not cover are neither read nor written: NaNs there stay and spread nowhere."""
    N = T * fs
    orig, gen, orig_d, gen_d = waves(N)
    mask_d = torch.from_numpy(MASKS["seam"]).cuda()
    for gen_start, Ng in _gens(fs)[1:3]:
        part_d = torch.from_numpy(_part(gen, gen_start, Ng)).cuda()
        want = K.wave_paste_ring(orig_d, part_d, mask_d, gen_start, 7 * fs, fs)
        frames = np.arange(gen_start // fs, -(-(gen_start + Ng) // fs)) % T
        covered = np.zeros(T, dtype=bool)
        covered[frames] = True
        assert 0 < covered.sum() < T
        outside = torch.from_numpy(np.repeat(~covered, fs)).cuda()
        dst = orig_d.clone()
        dst[:, outside] = float("nan")
        got = K.wave_paste_ring(dst, part_d, mask_d, gen_start, 7 * fs, fs, out=dst)
        assert bool(torch.isnan(got[:, outside]).all()) and not bool(torch.isnan(got[:, ~outside]).any())
        assert torch.equal(got[:, ~outside], want[:, ~outside])
        assert not torch.equal(want, orig_d)


@pytest.mark.parametrize("R", [0, 7, 512])
def test_away_from_the_wrap_it_is_wave_paste(K, waves, R):
    """gen does not wrap and the fade of no regenerated frame reaches the wrap: the line's bits."""
    fs, N = 512, T * 512
    orig, gen, orig_d, gen_d = waves(N)
    mask_d = torch.from_numpy(MASKS["interior"]).cuda()
    for gen_start, Ng in ((0, N), (4 * fs, 14 * fs), (4 * fs + 1, 14 * fs - 3)):
        part_d = gen_d[:, gen_start:gen_start + Ng].contiguous()
        assert torch.equal(K.wave_paste_ring(orig_d, part_d, mask_d, gen_start, R, fs),
                           K.wave_paste(orig_d, part_d, mask_d, gen_start, R, fs))


def test_away_from_the_wrap_it_is_wave_paste_at_the_longest_fade(K):
    """The same at R = 16 frames: a ring of 48 frames whose regenerated frames are 23 frames from the wrap."""
    fs, frames = 512, 48
    N = frames * fs
    g = torch.Generator(device="cuda").manual_seed(48)
    orig_d, gen_d = (torch.rand((B, N), device="cuda", generator=g) * 2 - 1 for _ in range(2))
    mask_d = torch.from_numpy(_mask((23, 24), (24,), frames=frames)).cuda()
    for dst in (None, "in place"):
        a, b = orig_d.clone(), orig_d.clone()
        ring = K.wave_paste_ring(a, gen_d, mask_d, 0, 16 * fs, fs, out=a if dst else None)
        line = K.wave_paste(b, gen_d, mask_d, 0, 16 * fs, fs, out=b if dst else None)
        assert torch.equal(ring, line) and not torch.equal(ring, orig_d)


@pytest.mark.parametrize("fs", FRAME)
@pytest.mark.parametrize("k", [1, T - 1, 5])
def test_rotating_the_ring_rotates_the_output(K, waves, k, fs):
    N = T * fs
    orig, gen, orig_d, gen_d = waves(N)
    for name in ("seam", "per_clip"):
        mask_d = torch.from_numpy(MASKS[name]).cuda()
        for gen_start, Ng in _gens(fs):
            part_d = torch.from_numpy(_part(gen, gen_start, Ng)).cuda()
            want = K.wave_paste_ring(orig_d, part_d, mask_d, gen_start, 7 * fs, fs)
            got = K.wave_paste_ring(torch.roll(orig_d, k * fs, 1).contiguous(), part_d,
                                    torch.roll(mask_d, k, 1).contiguous(), (gen_start + k * fs) % N, 7 * fs, fs)
            assert torch.equal(got, torch.roll(want, k * fs, 1)), (name, gen_start)


def _shifted(t):
    """The same values at an address that is 4 mod 16."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def test_vector_and_element_paths_agree_and_rows_are_independent(K, waves):
    from audiolcm_amd import _hip
    fs, N = 512, T * 512
    orig, gen, orig_d, gen_d = waves(N)
    mask_d = torch.from_numpy(MASKS["seam"]).cuda()
    gen_start, Ng = 20 * fs, 8 * fs
    part_d = torch.from_numpy(_part(gen, gen_start, Ng)).cuda()

    def rows():
        return [r["name"] for r in _hip.profile_end() if "wave_paste" in r["name"]]
    _hip.profile_begin()
    want = K.wave_paste_ring(orig_d, part_d, mask_d, gen_start, 700, fs)
    assert rows() == ["alcm::wave_paste_ring_kernel<4>"]
    for o, g in ((_shifted(orig_d), part_d), (orig_d, _shifted(part_d))):
        _hip.profile_begin()
        got = K.wave_paste_ring(o, g, mask_d, gen_start, 700, fs)
        assert rows() == ["alcm::wave_paste_ring_kernel<1>"]
        assert torch.equal(got, want)
    for b in range(B):
        one = K.wave_paste_ring(orig_d[b:b + 1].contiguous(), part_d[b:b + 1].contiguous(),
                                mask_d[b:b + 1].contiguous(), gen_start, 700, fs)
        assert torch.equal(one, want[b:b + 1])


def test_profile_rows_count_what_is_touched(K, waves):
    """R = 0: the samples of g > 0 are those of the regenerated frames gen covers, 2 frames per clip here."""
    from audiolcm_amd import _hip
    fs, N = 512, T * 512
    orig, gen, orig_d, gen_d = waves(N)
    mask_d = torch.from_numpy(_mask((T - 1, 0), (T - 1, 0))).cuda()
    blended = B * 2 * fs
    for gen_start, Ng, tiles in ((0, N, 3), (20 * fs, 8 * fs, 1)):
        part_d = torch.from_numpy(_part(gen, gen_start, Ng)).cuda()
        for inplace in (False, True):
            dst = orig_d.clone()
            _hip.profile_begin()
            K.wave_paste_ring(dst, part_d, mask_d, gen_start, 0, fs, out=dst if inplace else None)
            row, = [r for r in _hip.profile_end() if "wave_paste" in r["name"]]
            assert row["name"] == "alcm::wave_paste_ring_kernel<4>" and row["launches"] == 1
            n_tiles = tiles if inplace else 3       # out of place every frame is at least copied
            copied = 0 if inplace else 2 * (B * N - blended)
            assert row["bytes"] == 4.0 * (3 * blended + copied + n_tiles * B * 8)
            assert row["flops"] == 3.0 * blended
    _hip.profile_begin()
    K.wave_paste_ring(orig_d[:, :T * 6].contiguous(), gen_d[:, :T * 6].contiguous(), mask_d, 0, 0, 6)
    assert [r["name"] for r in _hip.profile_end() if "wave_paste" in r["name"]] == ["alcm::wave_paste_ring_kernel<1>"]


def test_wave_paste_ring_bad_arguments(K):
    from audiolcm_amd._hip import lib, ptr, stream_handle
    from audiolcm_amd.kernels import paste_ramp
    orig = torch.full((1, 2048), 0.25, device="cuda")
    gen = torch.full((1, 2048), -0.5, device="cuda")
    out = torch.full((1, 2048), 7.0, device="cuda")
    mask = torch.ones((1, 4), device="cuda")
    L, s = lib(), stream_handle()
    po, pg, pm, pr, pd = ptr(orig), ptr(gen), ptr(mask), ptr(paste_ramp(64, "cuda")), ptr(out)

    def call(o=po, g=pg, m=pm, r=pr, d=pd, B=1, N=2048, start=0, Ng=2048, T=4, fs=512, R=64):
        return L.alcm_wave_paste_ring(o, g, m, r, d, B, N, start, Ng, T, fs, R, s)

    def refused(**kw):
        return call(**kw) != 0 and b"wave_paste_ring" in L.alcm_last_error()
    assert refused(o=None) and refused(g=None) and refused(m=None) and refused(r=None) and refused(d=None)
    assert refused(B=-1) and refused(N=-1) and refused(start=-1) and refused(Ng=-1) and refused(T=-1)
    assert refused(fs=0) and refused(fs=-512) and refused(R=-1)
    assert refused(T=3) and refused(T=5)       # N is T * frame_samples exactly, one period
    assert refused(N=2047) and refused(N=2049)
    assert refused(Ng=2049)                    # gen is no longer than the ring
    assert refused(start=2048) and refused(start=4096, Ng=4)   # gen starts inside the ring
    assert refused(R=16 * 512 + 1)             # R is limited to 16 frames
    assert refused(fs=4, T=512, R=65)          # ... of the frame length in use
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())            # none of these launched
    # the empty cases return 0 without a launch
    assert call(B=0) == 0 and call(N=0, Ng=0, T=0) == 0
    assert call(d=po, Ng=0, g=None) == 0       # in place with nothing to blend
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((orig == 0.25).all())
    assert call(start=2044, Ng=2048, R=0, r=None) == 0     # a whole ring of gen from its last samples on; no table
    torch.cuda.synchronize()
    assert bool((out == -0.5).all())
