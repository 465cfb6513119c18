"""Config-1 command line: ``scripts/txt2audio_for_lcm.py`` on the MI355X path.

Mirrors the reference CLI (scripts/txt2audio_for_lcm.py:48-152 arguments, :209-270 main) — the same flags,
output names and ``result.csv`` — with every model stage in libaudiolcm_hip.  Differences, all deliberate:
  * prompts are generated in batches (``--batch-size``, the reference loops at batch 1) with per-clip RNG
    seeds derived from the global prompt index, the iteration and the sample
    (``--seed + (prompt * n_iter + iteration) * n_samples + sample``; the reference draws from the global RNG),
    so outputs do not depend on the batching;
  * ``--prompt_txt`` lines become ``{'ori_caption': p, 'struct_caption': '<p& all>'}`` as InferAPI.py:137 builds
    them (the reference passes the raw string to ``gen_test_sample``, which fails on ``prompt.items()``);
  * the unused unconditional embedding (``uc``, computed when ``--scale != 1`` and never passed to the LCM
    sampler, :90-92) is skipped;
  * ``--plms`` (teacher sampler, out of the hot-path scope and broken for LCM_audio, plms.py:185) raises;
  * ``--inpaint`` (parsed and never read by the reference) is text-guided inpainting of ``--init-audio PATH`` on the
    spans of ``--mask-spans "2.0-4.5,7-8"`` (seconds); without both it raises.  ``--init-audio`` alone is a variation
    of that clip at ``--strength F``; ``--duration SECONDS`` generates long-form clips by windowed continuation
    (DESIGN.md §5), with ``--long-joint`` by denoising all windows jointly, one DiT call per clip and LCM step.
    ``--keep-original`` (with ``--inpaint``) takes a recording of any length, regenerates only the
    whole latent frames inside the spans window by window and fades them into the input over ``--fade-ms F`` (default
    32) either side: every sample further than F ms from a span is written back as it was read, and each output has
    the input's sample count.  Without it the clip is cropped to the DiT's 845 frames and synthesised again as a whole.
    ``--long-joint`` with ``--init-audio`` denoises the frames to regenerate jointly (S DiT calls per region instead
    of S per window), and a variation or a plain ``--inpaint`` then works on the whole recording instead of a crop;
  * ``--extend SECONDS`` (with ``--init-audio``) continues the recording at 16 kHz: the file holds the recording,
    as it was read up to ``--fade-ms`` before the junction, and SECONDS of generated continuation.  It does not combine
    with ``--inpaint``, ``--mask-spans``, ``--keep-original``, ``--loop``, ``--duration``, the level options or
    ``--out-sample-rate``;
  * ``--loop-from PATH`` makes the recording PATH loop.  It is trimmed at its end to L whole latent frames.  Alone, only
    the frames within ``--loop-seam SECONDS`` (default 1.0, rounded up to whole frames) either side of the wrap are
    generated (from pure noise: ``--strength`` defaults to 1.0 here), conditioned on the recording across the wrap, and
    faded in over ``--fade-ms``; ``--mask-spans`` adds further spans (a span whose end is not after its start goes
    across the wrap).  The file holds L * 512 samples at 16 kHz: the recording's own bits outside the fades and spans.
    With ``--loop-vary`` the whole ring is regenerated from the recording as a hint at ``--strength`` (default 0.5),
    and ``--out-sample-rate``, ``--loudness``, ``--peak``, ``--true-peak`` and ``--loop-fade-ms`` apply as for
    ``--loop``.  ``--resample`` brings any input to 16 kHz first.  It does not combine with ``--loop``,
    ``--init-audio``, ``--inpaint``, ``--keep-original``, ``--duration`` or ``--extend``, and without ``--loop-vary``
    not with the level options or ``--out-sample-rate`` either;
  * ``--fade-law {linear,equal-power,matched}`` and ``--match-gain`` (with ``--keep-original``, ``--extend`` or
    ``--loop-from``; refused elsewhere and with ``--loop-vary``): the law of that fade, the linear crossfade, one that
    keeps the power of uncorrelated signals, or of signals with the correlation measured at each junction on the GPU;
    and each regenerated run scaled to the recording's level at its junctions (Fade laws);
  * ``--resample``: ``--init-audio`` may have any sample rate, 1 to 8 channels and PCM16, PCM24 or float32 samples; it
    is downmixed and resampled to 16 kHz on the GPU (alcm_resample; without the flag only 16 kHz mono PCM16 is read).
    With ``--keep-original`` the edit is done at the recording's own rate: mono, and a rate at which a latent frame is a
    whole number of samples (48000, 32000, 8000, ...); the output has the input's rate and sample count;
  * ``--out-sample-rate R`` resamples every output from 16 kHz to R on the GPU and writes R into the header.
    ``--sample_rate`` (default 22050, the reference's) only labels the header of the 16 kHz samples, as in the
    reference, and is ignored when ``--out-sample-rate`` is given;
  * ``--loudness LUFS`` brings every output to that ITU-R BS.1770 integrated loudness, measured on the GPU on the
    samples that are written; ``--peak DBFS`` scales a clip down where its peak would pass that ceiling (-1 dBFS when
    only ``--loudness`` is given); ``--true-peak`` lets the ceiling act on the 4x oversampled peak estimate.  Refused
    with ``--keep-original``, whose kept samples they would scale;
  * ``--limiter`` (with ``--loudness`` or ``--peak``) keeps the ceiling with a look-ahead peak limiter on the GPU
    instead of a smaller gain for the whole clip, so that a clip with short loud peaks still reaches ``--loudness``;
    ``--limiter-lookahead-ms`` (5) and ``--limiter-release-ms`` (100) are its times.  Refused wherever a level is, and
    with ``--loop`` and ``--loop-from``: a gain that varies in time would break the period;
  * ``--synthetic-seed N`` runs on the seeded recipe weights (no checkpoints offline).
"""
from __future__ import annotations

import argparse
import functools
import math
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .audio_in import (FRAME_SAMPLES, SAMPLE_RATE, EditPlan, check_level, check_out_rate, fade_samples_of,
                       finish_output, loop_frames, loop_multiple, parse_spans, plan_edit)
from .config import instantiate_from_config, load_config
from .infer_api import build_models, struct_caption
from .lcm import LCMSampler
from .wavio import write_pcm16


def parse_args(argv: Optional[Sequence[str]] = None):
    p = argparse.ArgumentParser(description="AudioLCM text-to-audio on MI355X (scripts/txt2audio_for_lcm.py)")
    p.add_argument("--prompt_txt", type=str, nargs="?", default="prompt.txt", help="txt file with prompts in it")
    p.add_argument("--sample_rate", type=int, default=22050, help="sample rate of wav")
    p.add_argument("--inpaint", action="store_true", help="if test txt guided inpaint task")
    p.add_argument("--test-dataset", default="none", help="test which dataset: audiocaps/clotho/fsd50k")
    p.add_argument("--outdir", type=str, nargs="?", default="outputs/txt2audio-samples", help="dir to write results to")
    p.add_argument("--ddim_steps", type=int, default=100, help="number of ddim sampling steps")
    p.add_argument("--plms", action="store_true", help="use plms sampling")
    p.add_argument("--n_iter", type=int, default=1, help="sample this often")
    p.add_argument("--H", type=int, default=20, help="image height, in pixel space")
    p.add_argument("--W", type=int, default=312, help="image width, in pixel space")
    p.add_argument("--n_samples", type=int, default=1, help="how many samples to produce for the given prompt")
    p.add_argument("--scale", type=float, default=5.0, help="guidance scale (LCM w-embedding: w = scale - 1)")
    p.add_argument("-r", "--resume", type=str, const=True, default="", nargs="?", help="checkpoint to load")
    p.add_argument("-b", "--base", type=str, default="configs/audiolcm.yaml", help="path to the base config")
    p.add_argument("--vocoder-ckpt", type=str, default="vocoder/logs/audioset", help="path to vocoder checkpoint")
    # MI355X build options
    p.add_argument("--synthetic-seed", type=int, default=None, help="run on the seeded synthetic recipe weights")
    p.add_argument("--synthetic-tokenizer", action="store_true",
                   help="with -r: use the hash-id tokenizer stand-in when the tokenizer directories are absent")
    p.add_argument("--batch-size", type=int, default=32, help="prompts per batched generation")
    p.add_argument("--seed", type=int, default=0, help="per-clip RNG seeds: seed + (prompt * n_iter + iteration) * n_samples + sample")
    p.add_argument("--precision", choices=["split", "mixed", "bf16"], default="mixed",
                   help="MFMA precision policy (DESIGN.md §3)")
    p.add_argument("--init-audio", type=str, default=None,
                   help="16 kHz mono PCM16 WAV every prompt starts from: a variation, or with --inpaint an inpainting")
    p.add_argument("--strength", type=float, default=None,
                   help="with --init-audio: how far the clip is noised before sampling, in (0, 1] (default 0.5; with "
                        "--loop-from alone 1.0)")
    p.add_argument("--mask-spans", type=str, default=None,
                   help='with --inpaint: the time spans to regenerate, in seconds, e.g. "2.0-4.5,7-8"')
    p.add_argument("--keep-original", action="store_true",
                   help="with --inpaint: any clip length; keep the input waveform outside the spans bit for bit")
    p.add_argument("--fade-ms", type=float, default=32.0,
                   help="with --keep-original: the fade between the input and the regenerated audio, either side")
    p.add_argument("--fade-law", type=str, default="linear", choices=["linear", "equal-power", "matched"],
                   help="with --keep-original, --extend or --loop-from: the law of that fade: the linear crossfade, one "
                        "that keeps the power of uncorrelated signals, or of signals with the correlation measured at "
                        "each junction on the GPU (DESIGN.md §5)")
    p.add_argument("--match-gain", action="store_true",
                   help="with --keep-original, --extend or --loop-from: scale each regenerated run to the level of the "
                        "recording, measured at the run's junctions on the GPU (DESIGN.md §5)")
    p.add_argument("--resample", action="store_true",
                   help="with --init-audio: read any rate, 1-8 channels, PCM16/PCM24/float32; resample to 16 kHz on "
                        "the GPU (with --keep-original: edit at the recording's own rate)")
    p.add_argument("--out-sample-rate", type=int, default=None,
                   help="resample the output from 16 kHz to this rate on the GPU and write it into the header "
                        "(--sample_rate only labels the header and is then ignored)")
    p.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                   help="bring every output to this ITU-R BS.1770 integrated loudness (-70 .. 0) on the GPU")
    p.add_argument("--peak", type=float, default=None, metavar="DBFS",
                   help="peak ceiling of every output in dBFS, at most 0 (default with --loudness: -1)")
    p.add_argument("--true-peak", action="store_true",
                   help="with --loudness or --peak: the ceiling acts on the 4x oversampled peak estimate")
    p.add_argument("--limiter", action="store_true",
                   help="with --loudness or --peak: keep the ceiling with a look-ahead limiter on the GPU instead of a "
                        "smaller gain for the whole clip, so that the clip still reaches --loudness (DESIGN.md §5)")
    p.add_argument("--limiter-lookahead-ms", type=float, default=5.0, metavar="MS",
                   help="with --limiter: the look-ahead, at most 1024 samples at the rate written (default 5)")
    p.add_argument("--limiter-release-ms", type=float, default=100.0, metavar="MS",
                   help="with --limiter: the release time, above 0 (default 100)")
    p.add_argument("--duration", type=float, default=None,
                   help="clip length in seconds, generated by windowed continuation (default: one window of --W frames)")
    p.add_argument("--long-joint", action="store_true",
                   help="with --duration: denoise the windows jointly, one DiT call per clip and LCM step; with "
                        "--init-audio: denoise the frames to regenerate jointly, on the whole recording (DESIGN.md §5)")
    p.add_argument("--extend", type=float, default=None, metavar="SECONDS",
                   help="with --init-audio: continue the recording by this many seconds (DESIGN.md §5)")
    p.add_argument("--loop", action="store_true",
                   help="write clips that loop without a seam: one period of --duration seconds (rounded up to whole "
                        "latent frames), or of --W frames without --duration (DESIGN.md §5)")
    p.add_argument("--loop-fade-ms", type=float, default=32.0,
                   help="with --loop: the fade that closes the seam at the start of the period")
    p.add_argument("--loop-from", type=str, default=None, metavar="PATH",
                   help="make the recording PATH loop: regenerate only the seam either side of the wrap and keep every "
                        "other sample (DESIGN.md §5)")
    p.add_argument("--loop-seam", type=float, default=1.0, metavar="SECONDS",
                   help="with --loop-from: the audio made anew either side of the wrap, rounded up to whole frames")
    p.add_argument("--loop-vary", action="store_true",
                   help="with --loop-from: regenerate the whole ring from the recording as a hint at --strength")
    p.add_argument("--test-dataset-tsv", type=str, default=None, help="override the config's test_dataset tsv_path")
    opt = p.parse_args(argv)
    if opt.strength is None:
        opt.strength = 1.0 if opt.loop_from and not opt.loop_vary else 0.5
    return opt


class GenSamples:
    """scripts/txt2audio_for_lcm.py:96-147 (GenSamples.gen_test_sample), batched over prompts."""

    def __init__(self, opt, sampler: LCMSampler, model, outpath: str, vocoder, save_mel: bool = True,
                 save_wav: bool = True, original_inference_steps: Optional[int] = None,
                 plan: Optional[EditPlan] = None):
        """``plan``: ``build``'s plan of the ``--init-audio`` request every prompt starts from."""
        self.opt, self.sampler, self.model, self.outpath = opt, sampler, model, outpath
        self.vocoder = vocoder
        self.save_mel, self.save_wav = save_mel, save_wav
        self.channel_dim = model.channels
        self.original_inference_steps = original_inference_steps
        self.plan = plan
        self.level = check_level(opt.loudness, opt.peak, opt.true_peak, opt.limiter, opt.limiter_lookahead_ms,
                                 opt.limiter_release_ms)

    @functools.cached_property
    def pipeline(self):
        """Built at the first long-form or audio-conditioned batch; plain text-to-audio runs on ``sampler`` alone."""
        from .pipeline import AudioLCMPipeline
        return AudioLCMPipeline(self.model, self.vocoder.generator, steps=self.opt.ddim_steps,
                                guidance_scale=self.opt.scale, latent_shape=(self.opt.H, self.opt.W),
                                original_inference_steps=self.original_inference_steps)

    def generate(self, c, seeds):
        """Conditioning (B, ...) and per-clip seeds -> (mel or None, waveform (B, L) on the device or None, the rate for
        the header, the PCM16 scale)."""
        label = self.opt.out_sample_rate is None  # --sample_rate labels 16 kHz samples, as in the reference
        if self.plan is not None:
            wav, rate, mel = self.pipeline.run_edit(self.plan, c, seeds, self.opt.strength)
            return mel, wav, self.opt.sample_rate if label and not self.plan.native else rate, self.plan.pcm_scale
        if self.opt.loop:
            out = self.pipeline.generate_loop(c, seeds, loop_period(self.opt), out_sample_rate=self.opt.out_sample_rate,
                                              fade_samples=fade_samples_of(self.opt.loop_fade_ms,
                                                                           self.opt.out_sample_rate or SAMPLE_RATE),
                                              level=self.level)
            return out["mel"], out["wav"], self.opt.sample_rate if label else out["rate"], 32767.0
        if self.opt.duration is not None:
            out = self.pipeline.generate_long(c, seeds, math.ceil(self.opt.duration * SAMPLE_RATE / FRAME_SAMPLES),
                                              joint=self.opt.long_joint)
            mel, wav = out["mel"], out["wav"]
        else:
            B = c.shape[0]
            shape = [self.channel_dim, self.opt.H, self.opt.W] if self.channel_dim > 0 else [self.opt.H, self.opt.W]
            z, _ = self.sampler.sample(S=self.opt.ddim_steps, conditioning=c, batch_size=B, shape=shape,
                                       verbose=False, seeds=seeds, guidance_scale=self.opt.scale,
                                       original_inference_steps=self.original_inference_steps)
            mel = self.model.decode_first_stage(z)
            wav = self.vocoder.vocode(mel).squeeze(1) if self.save_wav else None
        rate = self.opt.sample_rate
        if wav is not None and (not label or self.level is not None):
            wav, out_rate = finish_output(wav, self.opt.out_sample_rate, self.level)
            rate = rate if label else out_rate
        return mel, wav, rate, 32767.0

    def clip_seed(self, prompt_index: int, it: int, j: int) -> int:
        """RNG seed of sample j of iteration `it` of the prompt at global index `prompt_index` (batch-invariant)."""
        return self.opt.seed + (prompt_index * self.opt.n_iter + it) * self.opt.n_samples + j

    def gen_batch(self, prompts: List[Dict[str, str]], names: List[str], first_index: int = 0) -> List[Dict[str, str]]:
        """prompts[i] (global prompt index first_index + i) -> n_iter x n_samples clips named <names[i]>_<idx>;
        returns the records in the reference's order (per prompt, per iteration, per sample)."""
        n = self.opt.n_samples
        records: List[List[Dict[str, str]]] = [[] for _ in prompts]
        for it in range(self.opt.n_iter):
            text = {"ori_caption": [p["ori_caption"] for p in prompts for _ in range(n)],
                    "struct_caption": [p["struct_caption"] for p in prompts for _ in range(n)]}
            c = self.model.get_learned_conditioning(text)
            seeds = [self.clip_seed(first_index + i, it, j) for i in range(len(prompts)) for j in range(n)]
            mel, wav, rate, scale = self.generate(c, seeds)
            wav = wav.cpu().numpy() if self.save_wav else None
            mel_np = mel.cpu().numpy() if mel is not None else None
            for i in range(len(prompts)):
                for j in range(n):
                    idx = it * n + j  # the reference restarts idx per iteration (overwriting files); keep them apart
                    k = i * n + j
                    rec = {"caption": prompts[i]["ori_caption"]}
                    if self.save_mel and mel_np is not None:  # --keep-original decodes no whole-clip mel
                        mp = os.path.join(self.outpath, f"{names[i]}_{idx}.npy")
                        np.save(mp, mel_np[k])
                        rec["mel_path"] = mp
                    if self.save_wav:
                        wp = os.path.join(self.outpath, f"{names[i]}_{idx}.wav")
                        write_pcm16(wp, wav[k], rate, scale=scale)
                        rec["audio_path"] = wp
                    records[i].append(rec)
        return [r for rs in records for r in rs]


def loop_period(opt) -> int:
    """The period of ``--loop`` in latent frames: ``--duration`` rounded up (``audio_in.loop_frames``), else ``--W``."""
    if opt.duration is not None:
        return loop_frames(opt.duration, opt.out_sample_rate)
    return opt.W


def check_loop_from(opt) -> None:
    """The refusals of ``--loop-from`` that the flags alone decide; the file decides the rest (``audio_in.plan_loop``)."""
    if opt.loop_vary and not opt.loop_from:
        raise ValueError("--loop-vary is used with --loop-from")
    if not opt.loop_from:
        return
    if opt.limiter:
        raise ValueError("--limiter does not combine with --loop-from, with or without --loop-vary: a gain that varies "
                         "in time and starts from 1 at the first sample would break the period")
    for flag, given in (("--loop", opt.loop), ("--init-audio", opt.init_audio), ("--inpaint", opt.inpaint),
                        ("--keep-original", opt.keep_original), ("--duration", opt.duration is not None),
                        ("--extend", opt.extend is not None)):
        if given:
            raise ValueError(f"--loop-from does not combine with {flag}: it takes its length from the recording, reads "
                             "it itself and keeps every sample outside the seam")
    if not opt.loop_vary:
        for flag, given in (("--loudness", opt.loudness is not None), ("--peak", opt.peak is not None),
                            ("--true-peak", opt.true_peak), ("--out-sample-rate", opt.out_sample_rate is not None)):
            if given:
                raise ValueError(f"--loop-from keeps the recording's samples bit for bit at 16 kHz: {flag} is used with "
                                 "--loop-vary")
    elif opt.mask_spans:
        raise ValueError("--loop-from --loop-vary regenerates the whole ring: it does not take --mask-spans")


def check_fade_law_flags(opt) -> None:
    """``--fade-law`` and ``--match-gain`` are refused wherever nothing is pasted into a recording."""
    if opt.fade_law == "linear" and not opt.match_gain:
        return
    if opt.loop_from and opt.loop_vary:
        raise ValueError("--fade-law and --match-gain do not combine with --loop-from --loop-vary: the whole ring is "
                         "decoded and nothing is pasted")
    if not (opt.keep_original or opt.extend is not None or opt.loop_from):
        raise ValueError("--fade-law and --match-gain act where regenerated audio is pasted into a recording: they are "
                         "used with --keep-original, --extend or --loop-from")


def build(opt):
    check_loop_from(opt)
    check_fade_law_flags(opt)
    if opt.extend is not None:
        if not opt.init_audio:
            raise ValueError("--extend continues a recording: it needs --init-audio PATH")
        if opt.inpaint or opt.mask_spans or opt.keep_original:
            raise ValueError("--extend does not combine with --inpaint, --mask-spans or --keep-original: it regenerates "
                             "nothing of the recording")
        if opt.loop:
            raise ValueError("--extend does not combine with --loop: a continued recording does not loop")
        if opt.duration is not None:
            raise ValueError("--extend does not combine with --duration: the length is the recording's plus --extend")
        if opt.loudness is not None or opt.peak is not None or opt.true_peak:
            raise ValueError("--extend keeps the recording's samples bit for bit; --loudness, --peak and --true-peak "
                             "would scale them")
        if opt.limiter:
            raise ValueError("--extend keeps the recording's samples bit for bit; --limiter would scale them")
        if opt.out_sample_rate is not None:
            raise ValueError("--extend writes 16 kHz, the rate it keeps the recording at: it does not combine with "
                             "--out-sample-rate")
    if opt.loop:
        if opt.init_audio or opt.inpaint or opt.keep_original:
            raise ValueError("--loop generates from text: it does not combine with --init-audio, --inpaint or "
                             "--keep-original")
        if opt.loop_fade_ms < 0:
            raise ValueError("--loop-fade-ms must not be negative")
        if opt.limiter:
            raise ValueError("--limiter does not combine with --loop: a gain that varies in time and starts from 1 at "
                             "the first sample would break the period that a static gain keeps")
        mult = loop_multiple(check_out_rate(opt.out_sample_rate) or SAMPLE_RATE)
        if loop_period(opt) < 2 or loop_period(opt) % mult:
            raise ValueError(f"--loop without --duration: the period of --W {opt.W} frames must be at least 2 and, at "
                             f"this output rate, a multiple of {mult}")
    if opt.plms:
        raise NotImplementedError("--plms: the teacher PLMS sampler is outside the LCM hot path (and calls the 3-arg "
                                  "apply_model, plms.py:185, which LCM_audio does not have)")
    if opt.inpaint and not (opt.init_audio and opt.mask_spans):
        raise NotImplementedError("--inpaint needs --init-audio PATH and --mask-spans: the clip to inpaint and the "
                                  "time spans to regenerate")
    if opt.keep_original and not opt.inpaint:
        raise ValueError("--keep-original is used with --inpaint")
    if opt.mask_spans and not opt.inpaint and not opt.loop_from:
        raise ValueError("--mask-spans is used with --inpaint")
    if opt.init_audio and opt.duration is not None:
        raise ValueError("--init-audio and --duration do not combine")
    if opt.long_joint and opt.duration is None and not opt.loop and not opt.init_audio:
        raise ValueError("--long-joint is used with --duration or with --init-audio")
    if opt.resample and not opt.init_audio and not opt.loop_from:
        raise ValueError("--resample is used with --init-audio")
    check_out_rate(opt.out_sample_rate)
    if opt.limiter and opt.keep_original:
        raise ValueError("--keep-original keeps the input's samples bit for bit outside the spans; --limiter would "
                         "scale them")
    level = check_level(opt.loudness, opt.peak, opt.true_peak, opt.limiter, opt.limiter_lookahead_ms,
                        opt.limiter_release_ms)
    if level is not None and level.limiter:   # the look-ahead must fit the kernel at the rate that is written
        from . import limiter as _lm
        _lm.plan(check_out_rate(opt.out_sample_rate) or SAMPLE_RATE, 0, level.lookahead_ms, level.release_ms)
    # the file and the flags decide: a refused request fails before the models are built
    plan = plan_edit(opt.init_audio, parse_spans(opt.mask_spans) if opt.inpaint else None, opt.keep_original,
                     opt.fade_ms, opt.resample, opt.out_sample_rate, loudness=opt.loudness, peak_dbfs=opt.peak,
                     true_peak=opt.true_peak, joint=opt.long_joint, extend_s=opt.extend, limiter=opt.limiter,
                     limiter_lookahead_ms=opt.limiter_lookahead_ms, limiter_release_ms=opt.limiter_release_ms,
                     fade_law=opt.fade_law, match_gain=opt.match_gain) if opt.init_audio else None
    if opt.loop_from:
        plan = plan_edit(opt.loop_from, parse_spans(opt.mask_spans) if opt.mask_spans else None, False, opt.fade_ms,
                         opt.resample, opt.out_sample_rate, loudness=opt.loudness, peak_dbfs=opt.peak,
                         true_peak=opt.true_peak, loop_from=True, loop_seam_s=opt.loop_seam, loop_vary=opt.loop_vary,
                         loop_fade_ms=opt.loop_fade_ms, fade_law=opt.fade_law, match_gain=opt.match_gain)
        if plan.dropped:
            print(f"--loop-from: the last {plan.dropped} samples of {opt.loop_from} are left out: the period is "
                  f"{plan.samples.size // plan.frame_samples} whole latent frames")
    config = load_config(opt.base)
    split = {"split": True, "bf16": "bf16", "mixed": "mixed"}[opt.precision]
    if opt.synthetic_seed is None:
        if not opt.resume or not os.path.exists(str(opt.resume)):
            raise FileNotFoundError(f"checkpoint {opt.resume!r} not found (pass --synthetic-seed N to run on the "
                                    "seeded synthetic weights)")
        if "bigv" not in opt.vocoder_ckpt:
            raise NotImplementedError(f"vocoder {opt.vocoder_ckpt!r}: only BigVGAN checkpoints are on the path")
    model, vocoder = build_models(config, opt.resume, opt.vocoder_ckpt, opt.synthetic_seed, split,
                                  opt.synthetic_tokenizer, encoder=plan is not None)
    return config, model, LCMSampler(model), vocoder, plan


def main(argv: Optional[Sequence[str]] = None) -> List[Dict[str, str]]:
    opt = parse_args(argv)
    config, model, sampler, vocoder, plan = build(opt)
    os.makedirs(opt.outdir, exist_ok=True)
    gen = GenSamples(opt, sampler, model, opt.outdir, vocoder, save_mel=False, save_wav=True,
                     original_inference_steps=config.model.params.num_ddim_timesteps, plan=plan)
    csv_dicts: List[Dict[str, str]] = []
    bs = max(1, opt.batch_size // max(1, opt.n_samples))
    with torch.no_grad():
        if opt.test_dataset != "none":
            if opt.test_dataset not in ("audiocaps", "clotho", "fsd50k"):
                raise ValueError(f"unknown test dataset {opt.test_dataset!r}")
            key = "test_dataset3" if opt.test_dataset == "fsd50k" else "test_dataset"
            dcfg = dict(config[key])
            if opt.test_dataset_tsv:
                dcfg["params"] = dict(dcfg.get("params", {}), tsv_path=opt.test_dataset_tsv)
            test_dataset = instantiate_from_config(dcfg)
            test_dataset.load_mel = False  # ground-truth mels are for evaluation only
            print(f"Dataset: {type(test_dataset)} LEN: {len(test_dataset)}")
            for lo in range(0, len(test_dataset), bs):
                prompts, names = [], []
                for item in (test_dataset[i] for i in range(lo, min(lo + bs, len(test_dataset)))):
                    f_name = item["f_name"]
                    cut = f_name.rfind("_")  # file name = video_name + '_' + num
                    v_n, num = f_name[:cut], f_name[cut + 1:]
                    prompts.append(dict(item["caption"]))
                    names.append(f"{v_n}_sample_{num}")
                csv_dicts.extend(gen.gen_batch(prompts, names, lo))
            import pandas as pd
            pd.DataFrame.from_dict(csv_dicts).to_csv(os.path.join(opt.outdir, "result.csv"), sep="\t", index=False)
        else:
            with open(opt.prompt_txt) as f:
                lines = [l.strip() for l in f.readlines() if l.strip()]
            for lo in range(0, len(lines), bs):
                chunk = lines[lo:lo + bs]
                csv_dicts.extend(gen.gen_batch([dict(ori_caption=p, struct_caption=struct_caption(p)) for p in chunk],
                                               [p.replace(" ", "-") for p in chunk], lo))
    print(f"Your samples are ready and waiting four you here: \n{opt.outdir} \nEnjoy.")
    return csv_dicts


if __name__ == "__main__":
    main(sys.argv[1:])
