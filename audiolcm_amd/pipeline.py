"""Batched text-to-audio generation on one GPU: sampler -> decode_first_stage -> vocoder.

This is ``GenSamples.gen_test_sample`` (pythonscripts/InferAPI.py:63-101) without the
per-prompt batch-1 loop: a whole prompt batch goes through the LCM sampler, the VAE
decoder and BigVGAN as three batched HIP calls (the reference vocodes one clip at a time).
Inputs are device-resident conditioning embeddings (text encoders are out of scope,
SURVEY.md §8f) and per-prompt seeds.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import recipe
from .lcm import LCM_audio, LCMSampler
from .models import AutoencoderKL, BigVGAN, ConcatDiT2MLP


class AudioLCMPipeline:
    def __init__(self, model: LCM_audio, vocoder: BigVGAN, steps: int = 2, guidance_scale: float = 5.0,
                 original_inference_steps: int = 50, latent_shape=(20, 312)):
        self.model = model
        self.vocoder = vocoder
        self.sampler = LCMSampler(model)
        self.steps = steps
        self.guidance_scale = guidance_scale
        self.original_inference_steps = original_inference_steps
        self.latent_shape = tuple(latent_shape)
        self._mel_net = None

    @classmethod
    def from_recipe(cls, seed: int = 0, split: bool = True, encoder: bool = False, **kw) -> "AudioLCMPipeline":
        """``encoder``: also load the VAE encoder weights (``edit`` from a waveform needs them)."""
        lcm = LCM_audio(split=split)
        lcm.load_recipe(seed, encoder=encoder)
        voc = BigVGAN(split=split).load_state_dict(recipe.bigvgan_state(seed))
        return cls(lcm, voc, **kw)

    def set_split(self, split: bool):
        self.model.unet.diffusion_model.set_split(split)
        self.model.first_stage_model.set_split(split)
        self.vocoder.set_split(split)

    @torch.no_grad()
    def generate(self, cond: torch.Tensor, seeds: Sequence[int], steps: Optional[int] = None,
                 unconditional: Optional[torch.Tensor] = None, cfg_scale: float = 1.0,
                 latent_len: Optional[int] = None, noise=None, x_T=None) -> Dict[str, torch.Tensor]:
        B = cond.shape[0]
        S = steps or self.steps
        shape = (self.latent_shape[0], latent_len or self.latent_shape[1])
        z, _ = self.sampler.sample(S=S, batch_size=B, shape=shape, conditioning=cond, verbose=False,
                                   guidance_scale=self.guidance_scale,
                                   original_inference_steps=self.original_inference_steps, seeds=seeds,
                                   noise=noise, x_T=x_T, unconditional_conditioning=unconditional,
                                   unconditional_guidance_scale=cfg_scale)
        mel = self.model.decode_first_stage(z)
        wav = self.vocoder(mel)
        return dict(latent=z, mel=mel, wav=wav.squeeze(1))

    @torch.no_grad()
    def edit(self, cond: torch.Tensor, seeds: Sequence[int], wav=None, latent: Optional[torch.Tensor] = None,
             mask=None, strength: float = 0.5, sample_posterior: bool = True, steps: Optional[int] = None,
             unconditional: Optional[torch.Tensor] = None, cfg_scale: float = 1.0) -> Dict[str, torch.Tensor]:
        """Audio-conditioned generation (``LCMSampler.sample_edit``) from exactly one of ``wav`` (B, L) at 16 kHz, L a
        multiple of 512 (log-mel -> ``encode_first_stage``; needs the encoder weights) and ``latent`` (B, C, T) already
        scaled.  ``mask`` None: a variation of the whole clip at ``strength``; ``mask`` (B, T), 1 = regenerate: text-guided
        inpainting, the frames of mask 0 keep the input latent exactly.  The whole clip is decoded and vocoded again."""
        if (wav is None) == (latent is None):
            raise ValueError("pass exactly one of `wav` and `latent`")
        if wav is not None:
            if self._mel_net is None:
                from .mel import MelNet
                self._mel_net = MelNet()
            init = self.model.encode_first_stage(self._mel_net(wav))
        else:
            init = latent
        z, _ = self.sampler.sample_edit(S=steps or self.steps, conditioning=cond, init=init, mask=mask,
                                        strength=strength, seeds=seeds, sample_posterior=sample_posterior,
                                        guidance_scale=self.guidance_scale,
                                        original_inference_steps=self.original_inference_steps,
                                        unconditional_conditioning=unconditional,
                                        unconditional_guidance_scale=cfg_scale)
        out = self.decode(z)
        return dict(latent=z, **out)

    def long_windows(self, latent_len: int, window: Optional[int] = None, overlap: Optional[int] = None):
        """([(start, known)], window length) of ``generate_long``: window k covers frames start .. start + window, of
        which the first ``known`` are already generated.  The stride is window - overlap; the last window is shifted
        back to end at latent_len when the stride does not divide; a clip no longer than one window is that one window."""
        window = window or self.latent_shape[1]
        overlap = window // 2 if overlap is None else overlap
        if not 0 < overlap < window:
            raise ValueError("need 0 < overlap < window")
        if latent_len <= window:
            return [(0, 0)], latent_len
        spans, end = [(0, 0)], window
        while end < latent_len:
            start = min(end - overlap, latent_len - window)
            spans.append((start, end - start))
            end = start + window
        return spans, window

    @torch.no_grad()
    def generate_long(self, cond: torch.Tensor, seeds: Sequence[int], latent_len: int, window: Optional[int] = None,
                      overlap: Optional[int] = None, steps: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Long-form continuation past the DiT's length limit: window 0 is ``generate``'s latent for the prompt's own
        seeds; window k >= 1 is a ``sample_edit`` call at strength 1 whose known context (mask 0) is the previous
        ``overlap`` frames and whose remaining frames (mask 1) are new, with seeds ``recipe.window_seed(seed, k)``.
        The windows' new frames are concatenated into one (B, C, latent_len) latent, decoded and vocoded in one call
        each.  Defaults: window = latent_shape[1], overlap = window // 2."""
        B, Cc = cond.shape[0], self.latent_shape[0]
        S = steps or self.steps
        spans, W = self.long_windows(latent_len, window, overlap)
        kw = dict(guidance_scale=self.guidance_scale, original_inference_steps=self.original_inference_steps)
        z, _ = self.sampler.sample(S=S, batch_size=B, shape=(Cc, W), conditioning=cond, verbose=False, seeds=seeds,
                                   **kw)
        for k, (start, known) in enumerate(spans[1:], 1):
            init = torch.zeros((B, Cc, W), device=z.device, dtype=torch.float32)
            init[:, :, :known] = z[:, :, start:start + known]
            mask = torch.ones((B, W), device=z.device, dtype=torch.float32)
            mask[:, :known] = 0.0
            zk, _ = self.sampler.sample_edit(S=S, conditioning=cond, init=init, mask=mask, strength=1.0,
                                             seeds=[recipe.window_seed(s, k) for s in seeds], **kw)
            z = torch.cat([z, zk[:, :, known:]], 2)
        return dict(latent=z, **self.decode(z))

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Latent -> waveform only (config 5: long-form decode, the DiT caps at T <= 845)."""
        mel = self.model.decode_first_stage(z)
        return dict(mel=mel, wav=self.vocoder(mel).squeeze(1))
