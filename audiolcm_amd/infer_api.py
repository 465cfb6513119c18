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
from .ckpt import load_checkpoint, state_dict_of
from .config import instantiate_from_config, load_config
from .lcm import LCM_audio, LCMSampler
from .models import BigVGAN, VocoderBigVGAN
from .wavio import read_audio, read_wav, write_pcm16


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
                 out_sample_rate: Optional[int] = None):
        self.sampler, self.model, self.outpath = sampler, model, outpath
        self.out_sample_rate = check_out_rate(out_sample_rate)
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
            wav, rate = to_out_rate(self.vocoder.vocode(mel).squeeze(1), self.out_sample_rate)
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


def _build(config_path, model_path, vocoder_path, synthetic_seed, split, synthetic_tokenizer=False, encoder=False):
    config = load_config(config_path)
    if synthetic_seed is None:
        if not model_path or not os.path.exists(model_path):
            raise FileNotFoundError(f"model checkpoint {model_path!r} not found (pass synthetic_seed=... to run "
                                    "on the seeded synthetic weights)")
        if not vocoder_path or not os.path.exists(os.path.join(vocoder_path, "best_netG.pt")):
            raise FileNotFoundError(f"vocoder checkpoint dir {vocoder_path!r} not found")
        model = load_model_from_config(config, model_path, split=split)
        if synthetic_tokenizer and model.cond_stage_model is not None:
            model.cond_stage_model.use_synthetic_tokenizer()
        vocoder = VocoderBigVGAN(vocoder_path, split=split)
    else:
        model = load_model_from_config(config, None, split=split, synthetic_seed=synthetic_seed, encoder=encoder)
        vocoder = VocoderBigVGAN(state=recipe.bigvgan_state(synthetic_seed), h=None, split=split)
    sampler = LCMSampler(model)
    steps_cfg = config.model.params.get("num_ddim_timesteps", 50)
    return model, sampler, vocoder, steps_cfg


def AudioLCMBatchInfer(ori_prompts: List[str], config_path: str = "configs/audiolcm.yaml",
                       model_path: str = "./model/000184.ckpt", vocoder_path: str = "./model/vocoder",
                       batch_size: int = 32, synthetic_seed: Optional[int] = None, split: bool = True,
                       outpath: str = "results/test", seed: Optional[int] = None,
                       synthetic_tokenizer: bool = False, out_sample_rate: Optional[int] = None) -> str:
    """InferAPI.py:135-166. Returns the path of the last prompt's WAV.  ``seed``: per-prompt RNG seeds
    seed + i (default None: the global device RNG, as the reference).  ``synthetic_tokenizer``: run checkpoint
    weights on the hash-id tokenizer stand-in when the tokenizer directories are absent (tests only).
    ``out_sample_rate``: resample the 16 kHz waveform to that rate on the GPU and write it under that rate."""
    check_out_rate(out_sample_rate)
    prompts = [dict(ori_caption=p, struct_caption=struct_caption(p)) for p in ori_prompts]
    model, sampler, vocoder, orig_steps = _build(config_path, model_path, vocoder_path, synthetic_seed, split,
                                                 synthetic_tokenizer)
    os.makedirs(outpath, exist_ok=True)
    gen = GenSamples(sampler, model, outpath, vocoder, save_mel=False, save_wav=True,
                     original_inference_steps=orig_steps, out_sample_rate=out_sample_rate)
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
                  seed: Optional[int] = None, out_sample_rate: Optional[int] = None) -> str:
    """InferAPI.py:103-133."""
    return AudioLCMBatchInfer([ori_prompt], config_path, model_path, vocoder_path, 1, synthetic_seed, split, outpath,
                              seed, out_sample_rate=out_sample_rate)


# ---------------------------------------------------------------------------- audio-conditioned generation
SAMPLE_RATE = 16000
FRAME_SAMPLES = 512  # one latent frame = 2 mel frames x hop 256


def parse_spans(text: str) -> List[Tuple[float, float]]:
    """``"2.0-4.5,7-8"`` -> [(2.0, 4.5), (7.0, 8.0)] (seconds)."""
    spans = []
    for part in text.split(","):
        if not part.strip():
            continue
        try:
            a, b = part.split("-")
            spans.append((float(a), float(b)))
        except ValueError:
            raise ValueError(f"bad span {part!r}: expected START-END in seconds") from None
    return spans


def spans_to_mask(spans: Optional[Sequence[Tuple[float, float]]], n_frames: int, sample_rate: int = SAMPLE_RATE,
                  frame_samples: int = FRAME_SAMPLES, inward: bool = False) -> np.ndarray:
    """(n_frames,) float32 regenerate-mask of the time spans [t0, t1) in seconds: span -> latent frames
    floor(sample_rate * t0 / frame_samples) up to (not including) ceil(sample_rate * t1 / frame_samples), so a span
    ending mid-frame takes that frame too; clipped to the clip.  ``inward``: only the frames that lie wholly inside a
    span (ceil at the start, floor at the end), so that nothing outside the span is regenerated."""
    mask = np.zeros((n_frames,), dtype=np.float32)
    first, last = (math.ceil, math.floor) if inward else (math.floor, math.ceil)
    for t0, t1 in spans or ():
        if t1 <= t0:
            continue
        lo = max(0, first(sample_rate * t0 / frame_samples))
        hi = min(n_frames, last(sample_rate * t1 / frame_samples))
        mask[lo:hi] = 1.0
    return mask


def keep_original_mask(spans: Sequence[Tuple[float, float]], n_frames: int) -> np.ndarray:
    """The mask of a keep-original inpainting: the whole frames inside the spans, so that with a fade of F samples no
    sample further than F from a span changes.  ValueError when no span holds a whole frame."""
    mask = spans_to_mask(spans, n_frames, inward=True)
    if not mask.any():
        raise ValueError(f"no whole latent frame ({1000 * FRAME_SAMPLES // SAMPLE_RATE} ms) lies inside the spans "
                         f"{list(spans)}")
    return mask


def fade_samples_of(fade_ms: float, sample_rate: int = SAMPLE_RATE) -> int:
    return int(round(fade_ms * sample_rate / 1000.0))


def load_init_audio(path: str, max_frames: Optional[int] = None, resample: bool = False) -> np.ndarray:
    """16 kHz mono PCM16 WAV -> float32 samples, zero-padded up to a whole number of latent frames (512 samples) and
    cropped to ``max_frames`` of them (the DiT's length limit) when given.  Another sample rate raises ValueError,
    unless ``resample``: then the file is read by ``read_audio`` (any rate, 1 to 8 channels, PCM16 / PCM24 / float32)
    and downmixed and resampled to 16 kHz on the GPU first."""
    x = _read_init_audio(path, resample)
    if max_frames is not None:
        x = x[:max_frames * FRAME_SAMPLES]
    return _pad_to_frames(x)


def _read_init_audio(path: str, resample: bool = False) -> np.ndarray:
    if resample:
        x, sr = read_audio(path)
        if x.shape[0] == 0:
            raise ValueError(f"{path}: no samples")
        return _to_16k_mono(x, sr)
    x, sr = read_wav(path)
    if sr != SAMPLE_RATE:
        raise ValueError(f"{path}: sample rate {sr}, need {SAMPLE_RATE} (resampling is not done here; pass "
                         "resample=True, --resample on the command line, to resample on the GPU)")
    if x.size == 0:
        raise ValueError(f"{path}: no samples")
    return x


def _to_16k_mono(x: np.ndarray, rate: int) -> np.ndarray:
    """(N, channels) at ``rate`` -> (N16,) at 16 kHz: the channel mean and the resampling in one ``kernels.resample``."""
    if rate == SAMPLE_RATE and x.shape[1] == 1:
        return np.ascontiguousarray(x[:, 0])
    from . import kernels
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()[None]
    return kernels.resample(xd, rate, SAMPLE_RATE, channels=x.shape[1])[0].cpu().numpy()


def _pad_to_frames(x: np.ndarray, frame_samples: int = FRAME_SAMPLES) -> np.ndarray:
    return np.pad(x, (0, -x.size % frame_samples))


def load_init_audio_whole(path: str, resample: bool = False) -> Tuple[np.ndarray, int]:
    """``load_init_audio`` without a crop, and the sample count before padding (a keep-original edit writes that
    many)."""
    x = _read_init_audio(path, resample)
    return _pad_to_frames(x), x.size


NATIVE_RATES = "8000, 16000, 32000, 48000, 96000 (any multiple of 125 Hz)"


def check_native_keep_original(path: str, rate: int, channels: int, out_sample_rate: Optional[int]) -> int:
    """What a keep-original edit at the recording's own rate needs; returns the samples F of one latent frame."""
    from .resample import frame_samples_at
    if channels != 1:
        raise ValueError(f"{path}: {channels} channels; keep_original keeps the input's samples bit for bit, which a "
                         "downmix cannot: pass a mono file")
    F = frame_samples_at(rate, SAMPLE_RATE, FRAME_SAMPLES)
    if F is None:
        raise ValueError(f"{path}: sample rate {rate}; keep_original pastes whole latent frames of "
                         f"{FRAME_SAMPLES} * rate / {SAMPLE_RATE} samples, so it takes {NATIVE_RATES}")
    if out_sample_rate is not None and out_sample_rate != rate:
        raise ValueError(f"{path}: keep_original writes the input's own sample rate {rate}, not out_sample_rate "
                         f"{out_sample_rate}")
    return F


def load_native_audio(path: str, out_sample_rate: Optional[int] = None) -> Tuple[np.ndarray, int, int, int]:
    """The input of a keep-original edit at the recording's own rate: (mono float32 samples zero-padded to whole latent
    frames, the file's sample count, its rate, the samples F of one latent frame at that rate).  ValueError for more
    than one channel, a rate at which F is not whole, or an ``out_sample_rate`` that is not the file's."""
    x, rate = read_audio(path)
    F = check_native_keep_original(path, rate, x.shape[1], out_sample_rate)
    if x.shape[0] == 0:
        raise ValueError(f"{path}: no samples")
    x = np.ascontiguousarray(x[:, 0])
    return _pad_to_frames(x, F), x.size, rate, F


def check_out_rate(out_sample_rate: Optional[int]) -> Optional[int]:
    if out_sample_rate is not None and (int(out_sample_rate) != out_sample_rate or out_sample_rate < 1):
        raise ValueError(f"out_sample_rate must be a positive whole number of Hz, got {out_sample_rate!r}")
    return None if out_sample_rate is None else int(out_sample_rate)


def to_out_rate(wav: torch.Tensor, out_sample_rate: Optional[int]) -> Tuple[torch.Tensor, int]:
    """(B, L) at 16 kHz on the device -> (the waveform at ``out_sample_rate``, that rate); None keeps 16 kHz."""
    if out_sample_rate is None or out_sample_rate == SAMPLE_RATE:
        return wav, SAMPLE_RATE
    from . import kernels
    return kernels.resample(wav.contiguous(), SAMPLE_RATE, out_sample_rate), out_sample_rate


def _seed_list(seed: Optional[int], n: int):
    return None if seed is None else list(range(seed, seed + n))


def AudioLCMEditInfer(ori_prompt: str, init_audio: str, strength: float = 0.5,
                      mask_spans: Optional[Sequence[Tuple[float, float]]] = None,
                      config_path: str = "configs/audiolcm.yaml", model_path: str = "./model/000184.ckpt",
                      vocoder_path: str = "./model/vocoder", synthetic_seed: Optional[int] = None, split: bool = True,
                      outpath: str = "results/test", seed: Optional[int] = None, keep_original: bool = False,
                      fade_ms: float = 32.0, resample: bool = False, out_sample_rate: Optional[int] = None) -> str:
    """Text-guided variation of ``init_audio`` (16 kHz mono PCM16 WAV) at ``strength``, or, with ``mask_spans``
    ([(t0, t1)] in seconds), inpainting: the spans are regenerated and the rest of the latent is kept.  The whole
    clip is synthesised again from the latent, cropped to the DiT's 845 frames.  ``keep_original`` (needs
    ``mask_spans``): the clip is not cropped, only the whole frames inside the spans are regenerated
    (``AudioLCMPipeline.edit_long``) and faded into the input over ``fade_ms`` either side; every sample further than
    ``fade_ms`` from a span is written back as it was read, and the file has the input's sample count.
    ``resample``: ``init_audio`` may have any sample rate, 1 to 8 channels and PCM16, PCM24 or float32 samples
    (``wavio.read_audio``); it is downmixed and resampled to 16 kHz on the GPU.  With ``keep_original`` the edit is
    then done at the recording's own rate (``AudioLCMPipeline.edit_long_native``; mono, and a rate at which a latent
    frame is a whole number of samples: 48000, 32000, 8000, ...) and the output has the input's rate and sample count.
    ``out_sample_rate``: the output is resampled from 16 kHz to that rate on the GPU and written under it (with
    ``keep_original`` it may only name the input's rate).  Returns the WAV path (``<prompt-with-dashes>_0.wav``)."""
    from .mel import MelNet
    if keep_original and not mask_spans:
        raise ValueError("keep_original needs mask_spans: the time spans to regenerate")
    check_out_rate(out_sample_rate)
    rate, F = SAMPLE_RATE, FRAME_SAMPLES
    if keep_original and resample:  # a bad input fails before the models are built
        wav_in, n_samples, rate, F = load_native_audio(init_audio, out_sample_rate)
    else:
        wav_in, n_samples = load_init_audio_whole(init_audio, resample)
    if keep_original:
        if out_sample_rate is not None and out_sample_rate != rate:
            raise ValueError(f"keep_original writes the input's own sample rate {rate}, not out_sample_rate "
                             f"{out_sample_rate}")
        mask = keep_original_mask(mask_spans, wav_in.size // F)
    model, sampler, vocoder, orig_steps = _build(config_path, model_path, vocoder_path, synthetic_seed, split,
                                                 encoder=True)
    path = os.path.join(outpath, wav_name_for(ori_prompt) + "_0.wav")
    if keep_original:
        from .pipeline import AudioLCMPipeline
        pipe = AudioLCMPipeline(model, vocoder.generator, steps=2, original_inference_steps=orig_steps,
                                latent_shape=(model.mel_dim, model.mel_length))
        os.makedirs(outpath, exist_ok=True)
        with torch.no_grad():
            c = model.get_learned_conditioning({"ori_caption": [ori_prompt],
                                                "struct_caption": [struct_caption(ori_prompt)]})
            if resample:
                out = pipe.edit_long_native(c, _seed_list(seed, 1), wav_in[None], rate, mask[None], strength=strength,
                                            fade_samples=fade_samples_of(fade_ms, rate))
            else:
                out = pipe.edit_long(c, _seed_list(seed, 1), wav=wav_in[None], mask=mask[None], strength=strength,
                                     keep_original=True, fade_samples=fade_samples_of(fade_ms))
        write_pcm16(path, out["wav"][0, :n_samples].cpu().numpy(), rate, scale=32768.0)
        return path
    wav_in = wav_in[:model.unet.diffusion_model.cfg.max_latent_len * FRAME_SAMPLES]
    os.makedirs(outpath, exist_ok=True)
    with torch.no_grad():
        c = model.get_learned_conditioning({"ori_caption": [ori_prompt], "struct_caption": [struct_caption(ori_prompt)]})
        post = model.encode_first_stage(MelNet()(wav_in))
        T = post.mean.shape[2]
        mask = torch.from_numpy(spans_to_mask(mask_spans, T))[None] if mask_spans is not None else None
        z, _ = sampler.sample_edit(S=2, conditioning=c, init=post, mask=mask, strength=strength,
                                   seeds=_seed_list(seed, 1), original_inference_steps=orig_steps)
        wav, rate = to_out_rate(vocoder.vocode(model.decode_first_stage(z)).squeeze(1), out_sample_rate)
        wav = wav.cpu().numpy()
    write_pcm16(path, wav[0], rate)
    return path


def AudioLCMLongInfer(ori_prompt: str, duration_s: float = 30.0, config_path: str = "configs/audiolcm.yaml",
                      model_path: str = "./model/000184.ckpt", vocoder_path: str = "./model/vocoder",
                      synthetic_seed: Optional[int] = None, split: bool = True, outpath: str = "results/test",
                      seed: Optional[int] = None, out_sample_rate: Optional[int] = None) -> str:
    """A clip of ceil(duration_s * 16000 / 512) latent frames by long-form continuation
    (``AudioLCMPipeline.generate_long``).  ``seed`` None draws the clip's base seed from the global RNG.
    ``out_sample_rate``: the clip is resampled from 16 kHz to that rate on the GPU, cropped to
    round(duration_s * out_sample_rate) samples and written under that rate (without it the file keeps every sample
    of the last latent frame, as before).  Returns the WAV path."""
    from .pipeline import AudioLCMPipeline
    check_out_rate(out_sample_rate)
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
        wav, rate = to_out_rate(pipe.generate_long(c, [base], latent_len)["wav"], out_sample_rate)
        if out_sample_rate is not None:
            wav = wav[:, :int(round(duration_s * rate))]
        wav = wav.cpu().numpy()
    path = os.path.join(outpath, wav_name_for(ori_prompt) + "_0.wav")
    write_pcm16(path, wav[0], rate)
    return path
