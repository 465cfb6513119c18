"""The resampler's filter (audiolcm_amd/resample.py), ``wavio.read_audio`` and the new command-line flags, without a GPU.

The filter is checked against a float64 restatement of its definition written here (``_h`` / ``_ref_resample``): the
plan values per rate pair, the fp32 table against the formula, and what the design promises of a tone: a pass-band tone
comes out within -85 dB (max abs) of the analytic tone at the new rate and a tone above the new Nyquist comes out
below -95 dB, with the product's own table put through the float64 sum.  Both limits are conditions on the filter (zeros 32, beta 9, rolloff 0.92): they sit 6 and 4 dB inside
what it measures in float64 (-91 dB and -99 dB)."""
import math
import os
import struct

import numpy as np
import pytest

from conftest import REPO

PAIRS = {
    (44100, 16000): (160, 441, 192, -95),
    (48000, 16000): (1, 3, 210, -104),
    (22050, 16000): (320, 441, 96, -47),
    (32000, 16000): (1, 2, 140, -69),
    (8000, 16000): (2, 1, 70, -34),
    (16000, 22050): (441, 320, 70, -34),
    (16000, 44100): (441, 160, 70, -34),
    (16000, 48000): (3, 1, 70, -34),
}
ZEROS, BETA, ROLLOFF = 32, 9.0, 0.92


def _h(t, fcn, hw):
    """h(t) = 2 fcn sinc(2 fcn t) I0(beta sqrt(1 - (t / Hw)^2)) / I0(beta) for |t| <= Hw, else 0 (float64)."""
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) <= hw
    u = np.where(inside, t / hw, 0.0)
    a = np.pi * 2.0 * fcn * t
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return np.where(inside, 2.0 * fcn * sinc * np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA), 0.0)


def _params(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    fcn = ROLLOFF * min(rate_in, rate_out) / (2.0 * rate_in)
    hw = ZEROS / (2.0 * fcn)
    return up, down, fcn, hw, -math.floor(hw), 2 * math.floor(hw) + 2


def _table64(rate_in, rate_out):
    up, down, fcn, hw, first, ntaps = _params(rate_in, rate_out)
    k = np.arange(ntaps, dtype=np.float64)[None, :]
    r = np.arange(up, dtype=np.float64)[:, None]
    return _h(k + first - r / up, fcn, hw)


def _ref_resample(x, rate_in, rate_out, table=None):
    """float64 y[n] = sum_k h(k + first - r / up) x[floor(n down / up) + first + k], x = 0 outside, N_out = ceil;
    ``table`` (up, ntaps): another table in place of the formula's own."""
    up, down, fcn, hw, first, ntaps = _params(rate_in, rate_out)
    T = _table64(rate_in, rate_out) if table is None else np.asarray(table, dtype=np.float64)
    assert T.shape == (up, ntaps)
    n_in = x.shape[0]
    n = np.arange(-(-n_in * up // down), dtype=np.int64)
    pos, r = n * down // up, n * down % up
    xp = np.concatenate([np.zeros(ntaps + 1), x.astype(np.float64), np.zeros(ntaps + 1)])
    idx = pos[:, None] + first + np.arange(ntaps)[None, :] + ntaps + 1
    return np.einsum("nk,nk->n", T[r], xp[np.clip(idx, 0, xp.size - 1)])


@pytest.mark.parametrize("pair", list(PAIRS))
def test_plan_values(pair):
    from audiolcm_amd import resample
    pl = resample.plan(*pair)
    assert (pl.up, pl.down, pl.ntaps, pl.first) == PAIRS[pair]
    assert pl.taps.shape == (pl.up, pl.ntaps) and pl.taps.dtype == np.float32
    assert resample.plan(*pair) is pl                      # cached per rate pair
    assert pl.out_len(1000) == -(-1000 * pl.up // pl.down)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_tap_table(pair):
    from audiolcm_amd import resample
    taps = resample.plan(*pair).taps
    t64 = _table64(*pair)
    rows = taps.astype(np.float64).sum(1)
    print(f"{pair}: row sums in [{rows.min():.7f}, {rows.max():.7f}], max sum|taps| {np.abs(taps).sum(1).max():.3f}")
    assert np.abs(rows - 1.0).max() <= 1e-5
    assert np.abs(taps.astype(np.float64)).sum(1).max() <= 2.4
    # the fp32 table is the float64 formula rounded to nearest: within half an fp32 ulp of it (2^-24 relative; the
    # 1e-15 covers a last-bit difference between two float64 evaluations of the formula)
    assert (np.abs(taps.astype(np.float64) - t64) <= 2.0 ** -24 * np.abs(t64) + 1e-15).all()


def _product_table(pair):
    """The table the kernel is given, which the tone tests put through the float64 reference."""
    from audiolcm_amd import resample
    return resample.plan(*pair).taps


def _interior(n_out, n_in, up, down, hw):
    """Outputs whose filter support lies inside the clip."""
    pos = np.arange(n_out) * down / up
    return (pos >= hw + 1) & (pos <= n_in - hw - 2)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_pass_band_tones(pair):
    rate_in, rate_out = pair
    up, down, fcn, hw, first, ntaps = _params(*pair)
    n_in = rate_in // 2                                    # 0.5 s
    for f in (1000.0, 0.8 * min(rate_in, rate_out) / 2):
        x = np.sin(2 * np.pi * f * np.arange(n_in) / rate_in + 0.3)
        y = _ref_resample(x, rate_in, rate_out, _product_table(pair))
        want = np.sin(2 * np.pi * f * np.arange(y.size) / rate_out + 0.3)
        keep = _interior(y.size, n_in, up, down, hw)
        assert keep.sum() > y.size // 2
        err = np.abs(y - want)[keep].max()
        print(f"{pair} pass {f:.0f} Hz: {20 * np.log10(err):.1f} dB")
        assert 20 * np.log10(err) <= -85.0


@pytest.mark.parametrize("pair", [p for p in PAIRS if p[1] < p[0]])
def test_stop_band_tones(pair):
    rate_in, rate_out = pair
    up, down, fcn, hw, first, ntaps = _params(*pair)
    n_in = rate_in // 2
    factors = [m for m in (1.172, 1.3, 2.7, 2.8) if m * rate_out / 2 < rate_in / 2]
    assert len(factors) >= 2
    for m in factors:
        f = m * rate_out / 2
        x = np.sin(2 * np.pi * f * np.arange(n_in) / rate_in + 0.3)
        y = _ref_resample(x, rate_in, rate_out, _product_table(pair))
        keep = _interior(y.size, n_in, up, down, hw)
        out = np.abs(y)[keep].max()
        print(f"{pair} stop {m} x Nyquist ({f:.0f} Hz): {20 * np.log10(out):.1f} dB")
        assert 20 * np.log10(out) <= -95.0


def test_fp32_restatement_is_within_8e7_of_float64():
    """The bound the GPU parity test's 1e-5 rests on: fp32 taps and fp32 accumulation in rising k against float64."""
    from audiolcm_amd import resample
    for pair in ((48000, 16000), (16000, 44100)):
        pl = resample.plan(*pair)
        x = np.random.default_rng(1).uniform(-1, 1, 4000).astype(np.float32)
        ref = _ref_resample(x, *pair)
        n = np.arange(ref.size, dtype=np.int64)
        pos, r = n * pl.down // pl.up, n * pl.down % pl.up
        xp = np.concatenate([np.zeros(pl.ntaps + 1, np.float32), x, np.zeros(pl.ntaps + 1, np.float32)])
        acc = np.zeros(ref.size, dtype=np.float32)
        for k in range(pl.ntaps):
            acc = (acc.astype(np.float64) + pl.taps[r, k].astype(np.float64) *
                   xp[pos + pl.first + k + pl.ntaps + 1].astype(np.float64)).astype(np.float32)   # one rounding: fmaf
        err = np.abs(acc.astype(np.float64) - ref).max()
        print(f"{pair}: fp32 vs float64 {err:.2e}")
        assert err <= 8e-7


# ---------------------------------------------------------------------------- read_audio
def _wav_bytes(x, rate, bits, tag=1, extensible=False, extra=b""):
    """x (N, channels) float in [-1, 1) -> a RIFF/WAVE file's bytes (and the floats a reader should return)."""
    x = np.asarray(x, dtype=np.float64)
    ch = x.shape[1]
    if tag == 3:
        data, want = x.astype("<f4").tobytes(), x.astype(np.float32)
    elif bits == 16:
        q = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
        data, want = q.tobytes(), q.astype(np.float32) / np.float32(32768.0)
    elif bits == 24:
        q = np.clip(np.rint(x * 8388608.0), -8388608, 8388607).astype("<i4")
        data = q.reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
        want = q.astype(np.float32) / np.float32(8388608.0)
    else:
        q = np.clip(np.rint(x * 128.0 + 128), 0, 255).astype(np.uint8)
        data, want = q.tobytes(), None
    block = ch * bits // 8
    if extensible:
        guid = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * block, block, bits, 22, bits, (1 << ch) - 1) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * block, block, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body, want


def _write(path, blob):
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


LIST = b"LIST" + struct.pack("<I", 7) + b"INFOabc" + b"\x00"      # odd size: padded to a word


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("fmt", ["pcm16", "pcm24", "float32", "extensible24"])
def test_read_audio_formats(tmp_path, fmt, ch):
    from audiolcm_amd.wavio import read_audio
    x = np.random.default_rng(5).uniform(-1, 1, (301, ch))
    x[0, 0], x[1, 0] = -1.0, 0.999999
    bits, tag, ext, extra = {"pcm16": (16, 1, False, b""), "pcm24": (24, 1, False, b""), "float32": (32, 3, False, b""),
                             "extensible24": (24, 1, True, LIST)}[fmt]
    blob, want = _wav_bytes(x, 44100, bits, tag, ext, extra)
    got, sr = read_audio(_write(tmp_path / "a.wav", blob))
    assert sr == 44100 and got.dtype == np.float32 and got.shape == (301, ch)
    assert np.array_equal(got, want)
    assert got[0, 0] == -1.0


def test_read_audio_extensible_float_and_list_chunk(tmp_path):
    from audiolcm_amd.wavio import read_audio
    x = np.random.default_rng(6).uniform(-1, 1, (50, 2))
    blob, want = _wav_bytes(x, 48000, 32, 3, True, LIST)
    got, sr = read_audio(_write(tmp_path / "a.wav", blob))
    assert sr == 48000 and np.array_equal(got, want)


def test_read_audio_mono_pcm16_equals_read_wav(tmp_path):
    from audiolcm_amd.wavio import read_audio, read_wav
    x = np.random.default_rng(7).uniform(-1, 1, (1000, 1))
    p = _write(tmp_path / "a.wav", _wav_bytes(x, 16000, 16, extra=LIST)[0])
    a, sa = read_audio(p)
    b, sb = read_wav(p)
    assert sa == sb == 16000 and a.shape == (1000, 1) and np.array_equal(a[:, 0], b)


def test_read_audio_refusals(tmp_path):
    from audiolcm_amd.wavio import read_audio
    x = np.zeros((10, 1))
    with pytest.raises(ValueError, match="16- and 24-bit"):
        read_audio(_write(tmp_path / "u8.wav", _wav_bytes(x, 16000, 8)[0]))
    with pytest.raises(ValueError, match="channels"):
        read_audio(_write(tmp_path / "c9.wav", _wav_bytes(np.zeros((10, 9)), 16000, 16)[0]))
    with pytest.raises(ValueError, match="RIFF"):
        read_audio(_write(tmp_path / "junk.wav", b"not a wav file at all"))
    blob = _wav_bytes(x, 16000, 16)[0]
    with pytest.raises(ValueError, match="data"):
        read_audio(_write(tmp_path / "nodata.wav", blob[:blob.index(b"data")]))
    # read_wav keeps its own refusals
    from audiolcm_amd.wavio import read_wav
    with pytest.raises(ValueError):
        read_wav(_write(tmp_path / "st.wav", _wav_bytes(np.zeros((10, 2)), 16000, 16)[0]))


# ---------------------------------------------------------------------------- loaders and the command line
def test_loader_error_names_the_new_keyword(tmp_path):
    from audiolcm_amd.infer_api import load_init_audio
    p = _write(tmp_path / "a.wav", _wav_bytes(np.zeros((100, 1)), 44100, 16)[0])
    with pytest.raises(ValueError, match="sample rate") as e:
        load_init_audio(p, 4)
    assert "resample=True" in str(e.value)


def test_cli_flags_parse():
    from audiolcm_amd.cli import parse_args
    opt = parse_args([])
    assert opt.resample is False and opt.out_sample_rate is None and opt.sample_rate == 22050
    opt = parse_args(["--resample", "--out-sample-rate", "48000", "--init-audio", "x.wav"])
    assert opt.resample is True and opt.out_sample_rate == 48000 and opt.sample_rate == 22050


def _keep_args(path, *more):
    return ["--init-audio", path, "--inpaint", "--mask-spans", "0.5-1.0", "--keep-original", "--resample",
            "--synthetic-seed", "0", "-b", os.path.join(REPO, "configs", "audiolcm.yaml"), *more]


def test_cli_build_refuses_what_keep_original_cannot_do(tmp_path, monkeypatch):
    from audiolcm_amd import cli

    def no_model(*a, **k):
        raise AssertionError("a refused input must not reach the model")
    monkeypatch.setattr(cli, "build_models", no_model)
    mono = np.zeros((4000, 1))
    p441 = _write(tmp_path / "a441.wav", _wav_bytes(mono, 44100, 16)[0])
    with pytest.raises(ValueError, match="48000") as e:
        cli.build(cli.parse_args(_keep_args(p441)))
    assert "44100" in str(e.value) and "32000" in str(e.value)
    st = _write(tmp_path / "st.wav", _wav_bytes(np.zeros((4000, 2)), 48000, 16)[0])
    with pytest.raises(ValueError, match="channels"):
        cli.build(cli.parse_args(_keep_args(st)))
    p48 = _write(tmp_path / "a48.wav", _wav_bytes(mono, 48000, 16)[0])
    with pytest.raises(ValueError, match="out_sample_rate"):
        cli.build(cli.parse_args(_keep_args(p48, "--out-sample-rate", "16000")))
    # the same refusals from the Python entry point, before any model is built
    from audiolcm_amd import infer_api
    monkeypatch.setattr(infer_api, "_build", no_model)
    for path, kw, what in ((p441, {}, "48000"), (st, {}, "channels"), (p48, dict(out_sample_rate=44100), "44100")):
        with pytest.raises(ValueError, match=what):
            infer_api.AudioLCMEditInfer("a dog barks", path, mask_spans=[(0.05, 0.08)], keep_original=True,
                                        resample=True, synthetic_seed=0, **kw)
    with pytest.raises(ValueError, match="--resample"):
        cli.build(cli.parse_args(["--resample"]))
