"""``audio_in.plan_edit``: the one place that decides what an audio-conditioned request is and that refuses one.  Every
field of the plan per mode, every refusal from ``plan_edit`` itself and the same refusals through the two front ends
before any model is built, and one read of the file per request.  No GPU: the inputs are 16 kHz mono, or keep-original
ones, which are not resampled on the way in."""
import os
import struct

import numpy as np
import pytest

from conftest import REPO

CONFIG = os.path.join(REPO, "configs", "audiolcm.yaml")


def _wav(path, n, rate, ch=1, bits=16):
    """n frames of a ramp -> a PCM file; returns (path, the float32 samples of channel 0 as a reader gives them)."""
    full = 1 << (bits - 1)
    q = ((np.arange(n * ch, dtype=np.int64) * 7919) % 4001 - 2000).reshape(n, ch).astype("<i4")
    data = q.astype("<i2").tobytes() if bits == 16 else q.reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    block = ch * bits // 8
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * block, block, bits))
        f.write(b"data" + struct.pack("<I", len(data)) + data)
    return str(path), q[:, 0].astype(np.float32) / np.float32(full)


SPANS = [(0.5, 1.0)]
# mode, keywords -> the plan's scalar fields, the spans, the regenerated frames
MODES = [
    ("variation", {}, None, None),
    ("inpaint", dict(mask_spans=SPANS), ((0.5, 1.0),), None),
    ("keep_original", dict(mask_spans=SPANS, keep_original=True, fade_ms=32), None, list(range(16, 31))),
]


@pytest.mark.parametrize("mode,kw,spans,frames", MODES, ids=[m[0] for m in MODES])
def test_plan_fields_16k(tmp_path, mode, kw, spans, frames):
    from audiolcm_amd.audio_in import EditPlan, plan_edit
    path, x = _wav(tmp_path / "a.wav", 24000, 16000)
    plan = plan_edit(path, **kw)
    assert isinstance(plan, EditPlan) and plan.mode == mode
    assert plan.samples.dtype == np.float32 and plan.samples.shape == (47 * 512,)      # 24000 -> 24064
    assert np.array_equal(plan.samples[:24000], x) and not plan.samples[24000:].any()
    assert (plan.n_samples, plan.rate, plan.frame_samples, plan.fade) == (24000, 16000, 512, 512)
    assert plan.spans == spans
    if frames is None:
        assert plan.mask is None
    else:
        assert plan.mask.dtype == np.float32 and plan.mask.shape == (47,)
        assert np.flatnonzero(plan.mask).tolist() == frames
    keep = mode == "keep_original"
    assert (plan.out_rate, plan.resample_out, plan.native) == (16000, False, False)
    assert plan.pcm_scale == (32768.0 if keep else 32767.0)
    with pytest.raises(Exception):                                  # frozen
        plan.mode = "other"


def test_plan_fields_other_keywords(tmp_path):
    from audiolcm_amd.audio_in import plan_edit
    path, x = _wav(tmp_path / "a.wav", 24000, 16000)
    plan = plan_edit(path, max_frames=3, out_sample_rate=44100, fade_ms=10)
    assert plan.samples.shape == (3 * 512,) and np.array_equal(plan.samples, x[:1536]) and plan.n_samples == 24000
    assert (plan.mode, plan.rate, plan.out_rate, plan.resample_out, plan.fade) == ("variation", 16000, 44100, True, 160)
    assert plan_edit(path, mask_spans=[]).mode == "inpaint"         # an empty list is a mask of zeros, as before
    plan = plan_edit(path, SPANS, keep_original=True, out_sample_rate=16000, max_frames=3)   # the input's own rate
    assert (plan.out_rate, plan.resample_out, plan.samples.size) == (16000, False, 47 * 512)  # and never cropped


def test_plan_keep_original_at_48k(tmp_path):
    from audiolcm_amd.audio_in import plan_edit
    path, x = _wav(tmp_path / "a48.wav", 72000, 48000)
    plan = plan_edit(path, SPANS, keep_original=True, fade_ms=32, resample=True)
    assert (plan.mode, plan.rate, plan.frame_samples, plan.fade) == ("keep_original", 48000, 1536, 1536)
    assert (plan.out_rate, plan.resample_out, plan.pcm_scale, plan.native) == (48000, False, 32768.0, True)
    assert plan.n_samples == 72000 and plan.samples.shape == (47 * 1536,) and np.array_equal(plan.samples[:72000], x)
    assert plan.spans is None and np.flatnonzero(plan.mask).tolist() == list(range(16, 31))
    # a 16 kHz mono file under resample=True is read by read_audio and needs no resampling
    path, x = _wav(tmp_path / "a16.wav", 3000, 16000)
    plan = plan_edit(path, resample=True)
    assert plan.samples.shape == (6 * 512,) and np.array_equal(plan.samples[:3000], x) and plan.native is False


def _refusals(tmp_path):
    """[(what, the file, plan_edit keywords, a substring of the message)]: every refusal about the file and keywords."""
    a16 = _wav(tmp_path / "a16.wav", 4000, 16000)[0]
    a22 = _wav(tmp_path / "a22.wav", 4000, 22050)[0]
    a441 = _wav(tmp_path / "a441.wav", 4000, 44100)[0]
    a48 = _wav(tmp_path / "a48.wav", 4000, 48000)[0]
    st48 = _wav(tmp_path / "st48.wav", 4000, 48000, ch=2)[0]
    e16 = _wav(tmp_path / "e16.wav", 0, 16000)[0]
    e48 = _wav(tmp_path / "e48.wav", 0, 48000)[0]
    keep = dict(mask_spans=[(0.05, 0.2)], keep_original=True)
    return [
        ("keep-original without spans", a16, dict(keep_original=True), "mask_spans"),
        ("no whole frame inside the spans", a16, dict(mask_spans=[(0.05, 0.07)], keep_original=True),
         "whole latent frame"),
        ("wrong rate without resample", a22, {}, "resample=True"),
        ("wrong rate without resample, keep-original", a48, keep, "resample=True"),
        ("more than one channel with keep-original", st48, dict(keep, resample=True), "channels"),
        ("a rate at which a latent frame is not whole", a441, dict(keep, resample=True), "125 Hz"),
        ("out_sample_rate that is not the input's, 48 kHz", a48, dict(keep, resample=True, out_sample_rate=16000),
         "own sample rate 48000"),
        ("out_sample_rate that is not the input's, 16 kHz", a16, dict(keep, out_sample_rate=48000),
         "own sample rate 16000"),
        ("an empty file", e16, {}, "no samples"),
        ("an empty file, resample", e16, dict(resample=True), "no samples"),
        ("an empty file, keep-original at its own rate", e48, dict(keep, resample=True), "no samples"),
        ("a bad out_sample_rate", a16, dict(out_sample_rate=0), "positive whole number"),
        ("a bad out_sample_rate, fractional", a16, dict(out_sample_rate=44100.5), "positive whole number"),
    ]


def test_plan_edit_refuses(tmp_path):
    from audiolcm_amd.audio_in import plan_edit
    for what, path, kw, text in _refusals(tmp_path):
        with pytest.raises(ValueError) as e:
            plan_edit(path, **kw)
        assert text in str(e.value), what
    # the whole-frame-rate message is one text, here and in the pipeline: the rate, the rule and the rates that do
    with pytest.raises(ValueError) as e:
        plan_edit(_wav(tmp_path / "b441.wav", 4000, 44100)[0], [(0.05, 0.2)], keep_original=True, resample=True)
    assert all(s in str(e.value) for s in ("44100", "125 Hz", "8000", "16000", "32000", "48000"))
    from audiolcm_amd.audio_in import frame_samples_of
    with pytest.raises(ValueError) as e2:
        frame_samples_of(44100)
    assert str(e2.value) == str(e.value)
    assert (frame_samples_of(16000), frame_samples_of(48000), frame_samples_of(8000)) == (512, 1536, 256)


def _cli_args(path, kw):
    """The command line of ``plan_edit(path, **kw)``, or None where its flags cannot say it."""
    if isinstance(kw.get("out_sample_rate"), float):
        return None                                                 # argparse takes whole numbers only
    args = ["--init-audio", path, "--synthetic-seed", "0", "-b", CONFIG]
    if kw.get("mask_spans"):
        args += ["--inpaint", "--mask-spans", ",".join(f"{a}-{b}" for a, b in kw["mask_spans"])]
    elif kw.get("keep_original"):
        return None                                                 # --keep-original without --inpaint: a flag error
    args += ["--keep-original"] * bool(kw.get("keep_original")) + ["--resample"] * bool(kw.get("resample"))
    if kw.get("out_sample_rate") is not None:
        args += ["--out-sample-rate", str(kw["out_sample_rate"])]
    return args


def test_front_ends_refuse_the_same_before_any_model(tmp_path, monkeypatch):
    from audiolcm_amd import cli, infer_api

    def no_model(*a, **k):
        raise AssertionError("a refused input must not reach the model")
    monkeypatch.setattr(cli, "build_models", no_model)
    monkeypatch.setattr(infer_api, "build_models", no_model)
    monkeypatch.setattr(infer_api, "_build", no_model)
    through_cli = 0
    for what, path, kw, text in _refusals(tmp_path):
        with pytest.raises(ValueError) as e:
            infer_api.AudioLCMEditInfer("a dog barks", path, synthetic_seed=0, config_path=CONFIG,
                                        outpath=str(tmp_path / "out"), **kw)
        assert text in str(e.value), what
        args = _cli_args(path, kw)
        if args is not None:
            with pytest.raises(ValueError) as e:
                cli.build(cli.parse_args(args))
            assert text in str(e.value), what
            through_cli += 1
    assert through_cli == len(_refusals(tmp_path)) - 2
    assert not os.path.exists(tmp_path / "out")


def test_the_file_is_read_once_per_request(tmp_path, monkeypatch):
    from audiolcm_amd import audio_in, cli, infer_api
    reads = []

    def counted(fn):
        def wrapper(path, *a, **k):
            reads.append(path)
            return fn(path, *a, **k)
        return wrapper
    monkeypatch.setattr(audio_in, "read_wav", counted(audio_in.read_wav))
    monkeypatch.setattr(audio_in, "read_audio", counted(audio_in.read_audio))
    a16 = _wav(tmp_path / "a16.wav", 24000, 16000)[0]
    a48 = _wav(tmp_path / "a48.wav", 72000, 48000)[0]
    for path, kw in ((a16, {}), (a16, dict(mask_spans=SPANS)), (a16, dict(mask_spans=SPANS, keep_original=True)),
                     (a48, dict(mask_spans=SPANS, keep_original=True, resample=True))):
        del reads[:]
        audio_in.plan_edit(path, **kw)
        assert reads == [path]

    # through the front ends, up to the model build: the plan is made, and the file read, exactly once
    class Built(Exception):
        pass

    def stop(*a, **k):
        raise Built
    monkeypatch.setattr(cli, "build_models", stop)
    monkeypatch.setattr(infer_api, "_build", stop)
    for path, kw in ((a16, dict(mask_spans=SPANS)), (a48, dict(mask_spans=SPANS, keep_original=True, resample=True))):
        del reads[:]
        with pytest.raises(Built):
            infer_api.AudioLCMEditInfer("a dog barks", path, synthetic_seed=0, config_path=CONFIG, **kw)
        assert reads == [path]
        del reads[:]
        with pytest.raises(Built):
            cli.build(cli.parse_args(_cli_args(path, kw)))
        assert reads == [path]


def test_gen_samples_takes_the_plan_and_reads_nothing(tmp_path, monkeypatch):
    """``GenSamples`` uses ``build``'s plan: constructing it opens no file (and builds no pipeline)."""
    from audiolcm_amd import audio_in, cli
    a16 = _wav(tmp_path / "a16.wav", 24000, 16000)[0]
    opt = cli.parse_args(_cli_args(a16, dict(mask_spans=SPANS, keep_original=True)))
    plan = audio_in.plan_edit(a16, SPANS, keep_original=True)

    def no_read(*a, **k):
        raise AssertionError("the file was read again")
    monkeypatch.setattr(audio_in, "read_wav", no_read)
    monkeypatch.setattr(audio_in, "read_audio", no_read)

    class Model:
        channels = 0
    gen = cli.GenSamples(opt, None, Model(), str(tmp_path), None, plan=plan)
    assert gen.plan is plan and "pipeline" not in vars(gen)


def test_importing_audio_in_does_not_load_the_library():
    import subprocess
    import sys
    code = ("import sys; import audiolcm_amd.audio_in; from audiolcm_amd import _hip; "
            "assert _hip._lib is None and 'audiolcm_amd.kernels' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)
