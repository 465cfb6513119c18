"""Public inference API with the reference signatures (pythonscripts/InferAPI.py:26-166).

``AudioLCMInfer`` / ``AudioLCMBatchInfer`` build the model from the YAML config surface,
generate 2-step LCM samples, vocode them and write PCM16 16 kHz WAVs to
``results/test/<prompt-with-dashes>_0.wav``, returning the (last) path like the reference.
Prompts are batched (the reference loops at batch 1); everything on the path runs in the HIP
library.  Checkpoints are read with safe loaders only (audiolcm_amd/ckpt.py: ``weights_only=True`` with inert
placeholders for a Lightning checkpoint's non-tensor objects; yaml.safe_load).
"""
from __future__ import annotations

import os
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import recipe
from .audio_in import (FRAME_SAMPLES, SAMPLE_RATE, EditPlan, Level, check_level,  # noqa: F401
                       check_native_keep_original, check_out_rate, fade_samples_of, finish_output, keep_original_mask,
                       load_init_audio, load_init_audio_whole, load_native_audio, loop_frames, parse_spans, plan_edit,
                       spans_to_mask, to_out_rate)
from .ckpt import load_checkpoint, state_dict_of
from .config import instantiate_from_config, load_config
from .lcm import LCM_audio, LCMSampler
from .models import VocoderBigVGAN
from .wavio import write_pcm16


def load_model_from_config(config, ckpt: Optional[str] = None, verbose: bool = True, split: bool = True,
                           synthetic_seed: Optional[int] = None, encoder: bool = False) -> LCM_audio:
    """InferAPI.py:26-45: instantiate LCM_audio and load the Lightning ``state_dict`` (``encoder``: the synthetic
    weights include the VAE encoder; a checkpoint's ``first_stage_model.encoder.*`` is always loaded)."""
    model = instantiate_from_config(config.model, split=split)
    if ckpt:
        print(f"Loading model from {ckpt}")
        model.load_state_dict(state_dict_of(load_checkpoint(ckpt)), strict=False)
    elif synthetic_seed is not None:
        model.load_recipe(synthetic_seed, encoder=encoder)
    else:
        print("Note chat no ckpt is loaded !!!")
    return model


def struct_caption(p: str) -> str:
    return f"<{p}& all>"


def wav_name_for(prompt: str) -> str:
    return prompt.strip().replace(" ", "-")


class GenSamples:
    """InferAPI.py:49-101, batched."""

    def __init__(self, sampler: LCMSampler, model: LCM_audio, outpath: str, vocoder=None, save_mel=True,
                 save_wav=True, original_inference_steps=None, steps: int = 2, guidance_scale: float = 5.0,
                 out_sample_rate: Optional[int] = None, loudness: Optional[float] = None,
                 peak_dbfs: Optional[float] = None, true_peak: bool = False, limiter: bool = False,
                 limiter_lookahead_ms: float = 5.0, limiter_release_ms: float = 100.0):
        self.sampler, self.model, self.outpath = sampler, model, outpath
        self.out_sample_rate = check_out_rate(out_sample_rate)
        self.level = check_level(loudness, peak_dbfs, true_peak, limiter, limiter_lookahead_ms, limiter_release_ms)
        if save_wav:
            assert vocoder is not None
        self.vocoder = vocoder
        self.save_mel, self.save_wav = save_mel, save_wav
        self.channel_dim = model.channels
        self.original_inference_steps = original_inference_steps or 50
        self.steps, self.guidance_scale = steps, guidance_scale

    def gen_batch(self, prompts: List[Dict[str, str]], names: List[str], seeds=None) -> List[Dict[str, str]]:
        c = self.model.get_learned_conditioning({"ori_caption": [p["ori_caption"] for p in prompts],
                                                 "struct_caption": [p["struct_caption"] for p in prompts]})
        shape = [self.model.mel_dim, self.model.mel_length]
        z, _ = self.sampler.sample(S=self.steps, conditioning=c, batch_size=len(prompts), shape=shape,
                                   verbose=False, guidance_scale=self.guidance_scale,
                                   original_inference_steps=self.original_inference_steps, seeds=seeds)
        mel = self.model.decode_first_stage(z)
        wav, rate = None, SAMPLE_RATE
        if self.save_wav:
            wav, rate = finish_output(self.vocoder.vocode(mel).squeeze(1), self.out_sample_rate, self.level)
            wav = wav.cpu().numpy()
        mel_np = mel.cpu().numpy()
        records = []
        for i, p in enumerate(prompts):
            rec = {"caption": p["ori_caption"]}
            if self.save_mel:
                mp = os.path.join(self.outpath, names[i] + "_0.npy")
                np.save(mp, mel_np[i])
                rec["mel_path"] = mp
            if self.save_wav:
                wp = os.path.join(self.outpath, names[i] + "_0.wav")
                write_pcm16(wp, wav[i], rate)
                rec["audio_path"] = wp
            records.append(rec)
        return records

    def gen_test_sample(self, prompt: Dict[str, str], mel_name=None, wav_name=None):
        name = wav_name or mel_name or wav_name_for(prompt["ori_caption"])
        return self.gen_batch([prompt], [name])


def build_models(config, model_path, vocoder_path, synthetic_seed, split, synthetic_tokenizer=False, encoder=False):
    """(LCM_audio, VocoderBigVGAN) as both front ends build them: the checkpoints' weights (``synthetic_tokenizer``:
    on the hash-id tokenizer stand-in), or with ``synthetic_seed`` the seeded synthetic ones (``encoder``: with the VAE
    encoder's).  The callers check that the checkpoints exist."""
    if synthetic_seed is not None:
        model = load_model_from_config(config, None, split=split, synthetic_seed=synthetic_seed, encoder=encoder)
        return model, VocoderBigVGAN(state=recipe.bigvgan_state(synthetic_seed), split=split)
    model = load_model_from_config(config, model_path, split=split)
    if synthetic_tokenizer and model.cond_stage_model is not None:
        model.cond_stage_model.use_synthetic_tokenizer()
    return model, VocoderBigVGAN(vocoder_path, split=split)


def _build(config_path, model_path, vocoder_path, synthetic_seed, split, synthetic_tokenizer=False, encoder=False):
    config = load_config(config_path)
    if synthetic_seed is None:
        if not model_path or not os.path.exists(model_path):
            raise FileNotFoundError(f"model checkpoint {model_path!r} not found (pass synthetic_seed=... to run "
                                    "on the seeded synthetic weights)")
        if not vocoder_path or not os.path.exists(os.path.join(vocoder_path, "best_netG.pt")):
            raise FileNotFoundError(f"vocoder checkpoint dir {vocoder_path!r} not found")
    model, vocoder = build_models(config, model_path, vocoder_path, synthetic_seed, split, synthetic_tokenizer, encoder)
    sampler = LCMSampler(model)
    steps_cfg = config.model.params.get("num_ddim_timesteps", 50)
    return model, sampler, vocoder, steps_cfg


def _check_limiter_rate(out_sample_rate: Optional[int], limiter: bool, lookahead_ms: float, release_ms: float) -> None:
    """Refuses, before any model is built, limiter times that do not fit the rate that is written."""
    if limiter:
        from .limiter import plan
        plan(out_sample_rate or SAMPLE_RATE, 0, lookahead_ms, release_ms)


def AudioLCMBatchInfer(ori_prompts: List[str], config_path: str = "configs/audiolcm.yaml",
                       model_path: str = "./model/000184.ckpt", vocoder_path: str = "./model/vocoder",
                       batch_size: int = 32, synthetic_seed: Optional[int] = None, split: bool = True,
                       outpath: str = "results/test", seed: Optional[int] = None,
                       synthetic_tokenizer: bool = False, out_sample_rate: Optional[int] = None,
                       loudness: Optional[float] = None, peak_dbfs: Optional[float] = None,
                       true_peak: bool = False, limiter: bool = False, limiter_lookahead_ms: float = 5.0,
                       limiter_release_ms: float = 100.0) -> str:
    """InferAPI.py:135-166. Returns the path of the last prompt's WAV.  ``seed``: per-prompt RNG seeds
    seed + i (default None: the global device RNG, as the reference).  ``synthetic_tokenizer``: run checkpoint
    weights on the hash-id tokenizer stand-in when the tokenizer directories are absent (tests only).
    ``out_sample_rate``: resample the 16 kHz waveform to that rate on the GPU and write it under that rate.
    ``loudness``: bring each clip to that ITU-R BS.1770 integrated loudness in LUFS (-70 .. 0), measured on the GPU on
    the samples that are written; ``peak_dbfs``: scale a clip down where its peak would pass that ceiling (at most 0
    dBFS; -1 when only ``loudness`` is given, so a normalised file never clips); ``true_peak``: the ceiling acts on the
    4x oversampled peak estimate.  Without the three the samples are written as generated.  ``limiter`` (with
    ``loudness`` or ``peak_dbfs``): the ceiling is kept by a look-ahead limiter on the GPU (``audiolcm_amd/limiter.py``)
    instead of a smaller gain for the whole clip, so a clip with a binding ceiling still reaches ``loudness``;
    ``limiter_lookahead_ms`` (at most 1024 samples at the rate written) and ``limiter_release_ms`` (above 0) are its
    times, 5 and 100 ms by choice, not by a listening test."""
    check_out_rate(out_sample_rate)
    check_level(loudness, peak_dbfs, true_peak, limiter, limiter_lookahead_ms, limiter_release_ms)
    _check_limiter_rate(out_sample_rate, limiter, limiter_lookahead_ms, limiter_release_ms)
    prompts = [dict(ori_caption=p, struct_caption=struct_caption(p)) for p in ori_prompts]
    model, sampler, vocoder, orig_steps = _build(config_path, model_path, vocoder_path, synthetic_seed, split,
                                                 synthetic_tokenizer)
    os.makedirs(outpath, exist_ok=True)
    gen = GenSamples(sampler, model, outpath, vocoder, save_mel=False, save_wav=True,
                     original_inference_steps=orig_steps, out_sample_rate=out_sample_rate, loudness=loudness,
                     peak_dbfs=peak_dbfs, true_peak=true_peak, limiter=limiter,
                     limiter_lookahead_ms=limiter_lookahead_ms, limiter_release_ms=limiter_release_ms)
    names = [wav_name_for(p["ori_caption"]) for p in prompts]
    with torch.no_grad():
        for lo in range(0, len(prompts), batch_size):
            n = len(prompts[lo:lo + batch_size])
            gen.gen_batch(prompts[lo:lo + batch_size], names[lo:lo + batch_size],
                          seeds=None if seed is None else list(range(seed + lo, seed + lo + n)))
    print(f"Your samples are ready and waiting four you here: \n{outpath} \nEnjoy.")
    return os.path.join(outpath, names[-1] + "_0.wav")


def AudioLCMInfer(ori_prompt: str, config_path: str = "configs/audiolcm.yaml",
                  model_path: str = "./model/000184.ckpt", vocoder_path: str = "./model/vocoder",
                  synthetic_seed: Optional[int] = None, split: bool = True, outpath: str = "results/test",
                  seed: Optional[int] = None, out_sample_rate: Optional[int] = None,
                  loudness: Optional[float] = None, peak_dbfs: Optional[float] = None, true_peak: bool = False,
                  limiter: bool = False, limiter_lookahead_ms: float = 5.0, limiter_release_ms: float = 100.0) -> str:
    """InferAPI.py:103-133.  ``loudness``, ``peak_dbfs``, ``true_peak`` and the limiter's three: as
    ``AudioLCMBatchInfer``."""
    return AudioLCMBatchInfer([ori_prompt], config_path, model_path, vocoder_path, 1, synthetic_seed, split, outpath,
                              seed, out_sample_rate=out_sample_rate, loudness=loudness, peak_dbfs=peak_dbfs,
                              true_peak=true_peak, limiter=limiter, limiter_lookahead_ms=limiter_lookahead_ms,
                              limiter_release_ms=limiter_release_ms)


# ---------------------------------------------------------------------------- audio-conditioned generation
def _seed_list(seed: Optional[int], n: int):
    return None if seed is None else list(range(seed, seed + n))


def AudioLCMEditInfer(ori_prompt: str, init_audio: str, strength: Optional[float] = None,
                      mask_spans: Optional[Sequence[Tuple[float, float]]] = None,
                      config_path: str = "configs/audiolcm.yaml", model_path: str = "./model/000184.ckpt",
                      vocoder_path: str = "./model/vocoder", synthetic_seed: Optional[int] = None, split: bool = True,
                      outpath: str = "results/test", seed: Optional[int] = None, keep_original: bool = False,
                      fade_ms: float = 32.0, resample: bool = False, out_sample_rate: Optional[int] = None,
                      loudness: Optional[float] = None, peak_dbfs: Optional[float] = None,
                      true_peak: bool = False, joint: bool = False, extend_s: Optional[float] = None,
                      loop_from: bool = False, loop_seam_s: float = 1.0, loop_vary: bool = False,
                      loop_fade_ms: float = 32.0, limiter: bool = False, limiter_lookahead_ms: float = 5.0,
                      limiter_release_ms: float = 100.0, fade_law: str = "linear", match_gain: bool = False) -> str:
    """Text-guided variation of ``init_audio`` (16 kHz mono PCM16 WAV) at ``strength`` (default 0.5), or, with ``mask_spans``
    ([(t0, t1)] in seconds), inpainting: the spans are regenerated and the rest of the latent is kept.  The whole
    clip is synthesised again from the latent, cropped to the DiT's 845 frames.  ``keep_original`` (needs
    ``mask_spans``): the clip is not cropped, only the whole frames inside the spans are regenerated
    (``AudioLCMPipeline.edit_long``) and faded into the input over ``fade_ms`` either side; every sample further than
    ``fade_ms`` from a span is written back as it was read, and the file has the input's sample count.
    ``resample``: ``init_audio`` may have any sample rate, 1 to 8 channels and PCM16, PCM24 or float32 samples
    (``wavio.read_audio``); it is downmixed and resampled to 16 kHz on the GPU.  With ``keep_original`` the edit is
    then done at the recording's own rate (``AudioLCMPipeline.edit_long(rate=...)``; mono, and a rate at which a latent
    frame is a whole number of samples: 48000, 32000, 8000, ...) and the output has the input's rate and sample count.
    ``out_sample_rate``: the output is resampled from 16 kHz to that rate on the GPU and written under it (with
    ``keep_original`` it may only name the input's rate).  ``loudness``, ``peak_dbfs``, ``true_peak``: the level of the
    output, as ``AudioLCMBatchInfer``; refused with ``keep_original``, whose kept samples they would scale.
    ``limiter``, ``limiter_lookahead_ms``, ``limiter_release_ms``: as ``AudioLCMBatchInfer``; refused wherever a level
    is, and with ``loop_from`` in both its modes: its time-varying gain would break the period.
    ``joint``: the frames to regenerate are denoised jointly (``edit_long(joint=True)``: S DiT calls per region of
    regenerated frames instead of S per window); a variation or an inpainting without ``keep_original`` is then made
    from the whole recording, not from a crop to 845 frames.
    ``extend_s``: the recording is continued by that many seconds (``AudioLCMPipeline.extend``) at 16 kHz.  The file
    holds n + round(extend_s * 16000) samples, n the recording's; the recording comes back as it was read up to
    ``fade_ms`` before the junction at frame n // 512 (the samples of a last partial frame are generated again).
    ``resample`` brings any input to 16 kHz first.  Refused with ``mask_spans``, ``keep_original``, a level and
    ``out_sample_rate``, and for a recording shorter than one latent frame.
    ``loop_from``: the recording is made to loop (``AudioLCMPipeline.loop_from``).  It is trimmed at its end to L whole
    latent frames; only the frames within ``loop_seam_s`` seconds (rounded up to whole frames) either side of the wrap
    are generated, from pure noise by default (``strength`` 1.0 here), conditioned on the recording across the wrap,
    and faded in over ``fade_ms``; ``mask_spans`` adds further spans, and a span whose end is not after its start goes
    across the wrap.  The file holds L * 512 samples at 16 kHz: the recording's own outside the fades and spans.
    With ``loop_vary`` the whole ring is regenerated from the recording as a hint at ``strength`` (0.5) instead
    (``AudioLCMPipeline.edit_loop``), and ``out_sample_rate``, the level and ``loop_fade_ms`` apply as for
    ``AudioLCMLongInfer(loop=True)``.  ``loop_from`` is refused with ``keep_original`` and ``extend_s``, without
    ``loop_vary`` also with a level or ``out_sample_rate``, for a recording shorter than two frames and for a seam
    of more than half the recording.
    ``fade_law`` ("linear", "equal-power" or "matched") and ``match_gain``: how the regenerated audio is faded into the
    recording wherever one is kept (``keep_original``, ``extend_s``, ``loop_from`` without ``loop_vary``; refused
    elsewhere): the linear crossfade, one that keeps the power for uncorrelated signals, or for the correlation
    measured at each junction; and each regenerated run scaled to the recording's level at its junctions (DESIGN.md
    §5, Fade laws).  Returns the WAV path (``<prompt-with-dashes>_0.wav``)."""
    from .pipeline import AudioLCMPipeline
    if strength is None:
        strength = 1.0 if loop_from and not loop_vary else 0.5
    plan = plan_edit(init_audio, mask_spans, keep_original, fade_ms, resample, out_sample_rate, loudness=loudness,
                     peak_dbfs=peak_dbfs, true_peak=true_peak, joint=joint, extend_s=extend_s, loop_from=loop_from,
                     loop_seam_s=loop_seam_s, loop_vary=loop_vary, loop_fade_ms=loop_fade_ms, limiter=limiter,
                     limiter_lookahead_ms=limiter_lookahead_ms, limiter_release_ms=limiter_release_ms,
                     fade_law=fade_law, match_gain=match_gain)  # before any model
    _check_limiter_rate(None if plan.out_rate == SAMPLE_RATE else plan.out_rate, limiter, limiter_lookahead_ms,
                        limiter_release_ms)
    model, sampler, vocoder, orig_steps = _build(config_path, model_path, vocoder_path, synthetic_seed, split,
                                                 encoder=True)
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                            latent_shape=(model.mel_dim, model.mel_length))
    os.makedirs(outpath, exist_ok=True)
    with torch.no_grad():
        c = model.get_learned_conditioning({"ori_caption": [ori_prompt], "struct_caption": [struct_caption(ori_prompt)]})
        wav, rate, _ = pipe.run_edit(plan, c, _seed_list(seed, 1), strength)
    path = os.path.join(outpath, wav_name_for(ori_prompt) + "_0.wav")
    write_pcm16(path, wav[0].cpu().numpy(), rate, scale=plan.pcm_scale)
    return path


def AudioLCMLongInfer(ori_prompt: str, duration_s: float = 30.0, config_path: str = "configs/audiolcm.yaml",
                      model_path: str = "./model/000184.ckpt", vocoder_path: str = "./model/vocoder",
                      synthetic_seed: Optional[int] = None, split: bool = True, outpath: str = "results/test",
                      seed: Optional[int] = None, out_sample_rate: Optional[int] = None, joint: bool = False,
                      loudness: Optional[float] = None, peak_dbfs: Optional[float] = None,
                      true_peak: bool = False, loop: bool = False, loop_fade_ms: float = 32.0, limiter: bool = False,
                      limiter_lookahead_ms: float = 5.0, limiter_release_ms: float = 100.0) -> str:
    """A clip of ceil(duration_s * 16000 / 512) latent frames by long-form continuation
    (``AudioLCMPipeline.generate_long``).  ``seed`` None draws the clip's base seed from the global RNG.
    ``joint``: the windows are denoised jointly, one DiT call per LCM step (``generate_long(joint=True)``).
    ``out_sample_rate``: the clip is resampled from 16 kHz to that rate on the GPU, cropped to
    round(duration_s * out_sample_rate) samples and written under that rate (without it the file keeps every sample
    of the last latent frame, as before).  ``loudness``, ``peak_dbfs``, ``true_peak``: the level of the output, as
    ``AudioLCMBatchInfer``, measured at the output rate on the cropped clip.
    ``loop``: the clip loops without a seam (``AudioLCMPipeline.generate_loop``): the latent is denoised on a ring and
    decoded with a circular halo, and a fade of ``loop_fade_ms`` at the start of the period closes what is left.  The
    period is ``audio_in.loop_frames(duration_s, out_sample_rate)`` latent frames: ``duration_s`` rounded up to whole
    frames, and to a multiple of 5 frames at 44.1 and 22.05 kHz.  The file holds exactly one period at the output rate
    and is never cropped to ``duration_s``: a crop would cut the seam.  ``joint`` is then redundant.
    ``limiter``, ``limiter_lookahead_ms``, ``limiter_release_ms``: as ``AudioLCMBatchInfer``; refused with ``loop``: a
    gain that varies in time and starts from 1 at the first sample would break the period that a static gain keeps.
    Returns the WAV path."""
    from .pipeline import AudioLCMPipeline
    if loop and limiter:
        raise ValueError("limiter (--limiter) does not combine with loop (--loop): a gain that varies in time and "
                         "starts from 1 at the first sample would break the period that a static gain keeps")
    check_out_rate(out_sample_rate)
    level = check_level(loudness, peak_dbfs, true_peak, limiter, limiter_lookahead_ms, limiter_release_ms)
    _check_limiter_rate(out_sample_rate, limiter, limiter_lookahead_ms, limiter_release_ms)
    if loop and loop_fade_ms < 0:
        raise ValueError("loop_fade_ms must not be negative")
    model, sampler, vocoder, orig_steps = _build(config_path, model_path, vocoder_path, synthetic_seed, split)
    latent_len = math.ceil(duration_s * SAMPLE_RATE / FRAME_SAMPLES)
    if latent_len < 1:
        raise ValueError("duration_s must be positive")
    base = int(torch.randint(0, 2 ** 31 - 1, (1,))) if seed is None else seed
    pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                            latent_shape=(model.mel_dim, model.mel_length))
    os.makedirs(outpath, exist_ok=True)
    with torch.no_grad():
        c = model.get_learned_conditioning({"ori_caption": [ori_prompt], "struct_caption": [struct_caption(ori_prompt)]})
        if loop:
            out = pipe.generate_loop(c, [base], loop_frames(duration_s, out_sample_rate), level=level,
                                     out_sample_rate=out_sample_rate,
                                     fade_samples=fade_samples_of(loop_fade_ms, out_sample_rate or SAMPLE_RATE))
            wav, rate = out["wav"], out["rate"]
        else:
            n_out = None if out_sample_rate is None else int(round(duration_s * out_sample_rate))
            wav, rate = finish_output(pipe.generate_long(c, [base], latent_len, joint=joint)["wav"], out_sample_rate,
                                      level, n_out)
        wav = wav.cpu().numpy()
    path = os.path.join(outpath, wav_name_for(ori_prompt) + "_0.wav")
    write_pcm16(path, wav[0], rate)
    return path
