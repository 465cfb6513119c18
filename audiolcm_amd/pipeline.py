"""Batched text-to-audio generation on one GPU: sampler -> decode_first_stage -> vocoder.

This is ``GenSamples.gen_test_sample`` (pythonscripts/InferAPI.py:63-101) without the
per-prompt batch-1 loop: a whole prompt batch goes through the LCM sampler, the VAE
decoder and BigVGAN as three batched HIP calls (the reference vocodes one clip at a time).
Inputs are device-resident conditioning embeddings (text encoders are out of scope,
SURVEY.md §8f) and per-prompt seeds.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import recipe, windows
from .audio_in import FRAME_SAMPLES, SAMPLE_RATE, EditPlan, finish_output, frame_samples_of, spans_to_mask
from .lcm import LCM_audio, LCMSampler
from .models import AutoencoderKL, BigVGAN, ConcatDiT2MLP, DiagonalGaussianDistribution
from .windows import JOINT_MAX_WINDOWS, edit_windows, joint_edit_regions, paste_regions  # noqa: F401  (public here too)
from .windows import long_windows as _long_windows  # noqa: F401  (the name the joint-edit tests import)


def joint_weights(starts, W: int, L: int, overlap: int) -> np.ndarray:
    """``windows.window_weights`` of a clip with two ends (``generate_long(joint=True)``, ``edit_long(joint=True)``)."""
    return windows.window_weights(starts, W, L, overlap)


def ring_weights(starts, W: int, L: int, overlap: int) -> np.ndarray:
    """``windows.window_weights`` of a ring (``generate_loop``)."""
    return windows.window_weights(starts, W, L, overlap, ring=True)


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
        scaled (or the encoder's posterior, as ``sample_edit`` takes it).  ``mask`` None: a variation of the whole clip
        at ``strength``; ``mask`` (B, T), 1 = regenerate: text-guided inpainting, the frames of mask 0 keep the input
        latent exactly.  The whole clip is decoded and vocoded again."""
        z = self._edit_latent(cond, seeds, wav, latent, mask, strength, sample_posterior, steps, unconditional,
                              cfg_scale)
        out = self.decode(z)
        return dict(latent=z, **out)

    def _encode(self, wav):
        if self._mel_net is None:
            from .mel import MelNet
            self._mel_net = MelNet()
        return self.model.encode_first_stage(self._mel_net(wav))

    def _edit_latent(self, cond, seeds, wav, latent, mask, strength, sample_posterior, steps, unconditional,
                     cfg_scale):
        """The latent of ``edit``: one ``sample_edit`` call on the whole clip."""
        if (wav is None) == (latent is None):
            raise ValueError("pass exactly one of `wav` and `latent`")
        init = self._encode(wav) if wav is not None else latent
        z, _ = self.sampler.sample_edit(S=steps or self.steps, conditioning=cond, init=init, mask=mask,
                                        strength=strength, seeds=seeds, sample_posterior=sample_posterior,
                                        guidance_scale=self.guidance_scale,
                                        original_inference_steps=self.original_inference_steps,
                                        unconditional_conditioning=unconditional,
                                        unconditional_guidance_scale=cfg_scale)
        return z

    @torch.no_grad()
    def edit_long(self, cond: torch.Tensor, seeds: Sequence[int], wav=None, latent: Optional[torch.Tensor] = None,
                  mask=None, strength: float = 0.5, window: Optional[int] = None, overlap: Optional[int] = None,
                  sample_posterior: bool = True, steps: Optional[int] = None,
                  unconditional: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, keep_original: bool = False,
                  fade_samples: Optional[int] = None, halo_frames: int = 32,
                  rate: int = SAMPLE_RATE, joint: bool = False,
                  joint_clips_per_call: int = 1, fade_law: str = "linear",
                  match_gain: bool = False) -> Dict[str, torch.Tensor]:
        """``edit`` for a clip of any length, optionally keeping the input waveform outside the regenerated frames.

        The input is exactly one of ``wav`` (B, N), N a multiple of 512, encoded once as a whole (z = the scaled
        posterior sample with e0 = ``recipe.edit_noise(seeds, S, C, L)[2]``, or the mode without ``sample_posterior``),
        and ``latent`` (B, C, L).  ``mask`` (B, L), 1 = regenerate; None = all ones.  A clip of L <= W frames (W =
        ``window`` or latent_shape[1]) takes ``edit``'s own path.  A longer one is edited window by window
        (``edit_windows`` on the batch's union mask, ``overlap`` = W // 2 by default): window k is one ``sample_edit``
        call on its W frames with the mask still to do and the seeds ``recipe.window_seed(seed, k)``; what it
        produces is known context to the next window.  Frames of mask 0 keep the input latent exactly; an empty mask
        runs no DiT call.

        ``joint=True``: the regenerated frames are denoised jointly instead (``joint_edit_regions`` on the union mask
        with the same W and overlap): region r of regenerated frames and their context is one
        ``sample_joint(init=z[:, :, a:b], mask=mask[:, a:b], ...)`` call with the seeds ``recipe.window_seed(seed, r)``:
        S DiT calls per region and clip whatever its length, and every window sees both neighbours.  It is another
        sampler, not another route to the same clip; a region of one window is ``sample_edit`` on that slice.
        ``joint_clips_per_call`` is ``sample_joint``'s ``clips_per_call``.  ValueError for a region of more than 32
        windows.  Everything after the latent (``keep_original``, ``rate``, halo and fade) is the same for both forms.

        ``keep_original=False``: the whole clip is decoded; returns latent, mel, wav.  ``keep_original=True`` (needs
        ``wav``): only ``paste_regions(union, halo_frames)`` are decoded, each blended into a copy of ``wav`` by one
        ``kernels.wave_paste`` with a raised-cosine fade of ``fade_samples`` either side of the regenerated frames;
        samples further away keep the input's bits.  Returns latent, wav (B, N) and regions.

        ``rate`` (with ``keep_original``): ``wav`` is a recording at its own rate, where one latent frame is a whole
        number F = 512 * rate / 16000 of samples (48000, 32000, 8000, ...; ValueError otherwise) and N a multiple of F.
        It is resampled to 16 kHz (``kernels.resample``) for the encoder only; each decoded region is resampled back
        up, to (b - a) * F samples exactly, and pasted with ``frame_samples`` = F.  ``fade_samples`` counts samples at
        ``rate``; None is 512 at 16 kHz and 1536 at any other rate.

        The halo: at 16 kHz ``halo_frames`` * 512 >= ``fade_samples`` is required unless every region is cut by the
        clip's ends, so that a fade never reaches the edge of a decoded region; at another rate ``halo_frames`` * 512 >=
        the fade in 16 kHz samples + |first| + 1 (``first`` of the 16000 -> rate filter, ``resample.plan``), whatever
        the regions, so that the upsampler's transient at a region's edges stays outside the fade too.  The default of
        32 frames (1 s) also keeps the fade away from the zero-padded edges of the region's decode; it is a choice,
        not a measurement (no trained weights here to listen to).

        ``fade_law`` and ``match_gain`` (with ``keep_original``; DESIGN.md §5, Fade laws): "linear" is the fade above;
        "equal-power" and "matched" keep the power through the fade for uncorrelated signals, or for the correlation
        measured at each junction; ``match_gain`` scales each regenerated run to the level of the recording at its
        junctions.  Each region is measured on its own decode (``kernels.paste``)."""
        from . import kernels, resample as rs
        self._check_law(fade_law, match_gain, keep_original)
        if (wav is None) == (latent is None):
            raise ValueError("pass exactly one of `wav` and `latent`")
        if keep_original and wav is None:
            raise ValueError("keep_original needs the input waveform `wav`")
        if rate != SAMPLE_RATE and not keep_original:
            raise ValueError("`rate` is used with keep_original: anything else is decoded at 16 kHz")
        F = frame_samples_of(rate)
        dev = torch.device("cuda")
        if wav is not None:
            wav = torch.as_tensor(wav, dtype=torch.float32).to(dev).contiguous()
            if wav.dim() != 2 or wav.shape[1] % F:
                raise ValueError(f"`wav` is (B, N) with N a multiple of {F}")
            B, L = wav.shape[0], wav.shape[1] // F
        else:
            B, L = latent.shape[0], latent.shape[2]
        W = min(window or self.latent_shape[1], L)
        if mask is None:
            union = [True] * L
        else:
            mask = torch.as_tensor(mask, dtype=torch.float32)
            if tuple(mask.shape) != (B, L):
                raise ValueError(f"mask must be (B, L) = {(B, L)}, got {tuple(mask.shape)}")
            union = (mask > 0).any(0).tolist()
        regions = paste_regions(union, halo_frames) if keep_original else None
        native = rate != SAMPLE_RATE
        if keep_original:
            if fade_samples is None:
                fade_samples = 1536 if native else 512
            reach = -(-fade_samples * SAMPLE_RATE // rate)      # the fade in 16 kHz samples
            if native:
                reach += abs(rs.plan(SAMPLE_RATE, rate).first) + 1
            self._check_fade(fade_samples, F, halo_frames, reach,
                             native or any(a > 0 or b < L for a, b in regions))
        wav16 = kernels.resample(wav, rate, SAMPLE_RATE) if native else wav     # for the encoder only
        assert wav16 is None or wav16.shape[1] == L * FRAME_SAMPLES
        z = self._edit_long_latent(cond, seeds, wav16, latent, mask, union, W, overlap, strength, sample_posterior,
                                   steps, unconditional, cfg_scale, joint, joint_clips_per_call)
        if not keep_original:
            return dict(latent=z, **self.decode(z))
        out = wav.clone()
        pm = torch.ones((B, L), device=dev) if mask is None else mask.to(dev).contiguous()
        self._paste_regions(out, z, pm, regions, fade_samples, rate, F, fade_law, match_gain)
        return dict(latent=z, wav=out, regions=regions)

    @staticmethod
    def _check_law(fade_law: str, match_gain: bool, pastes: bool = True):
        """``audio_in.check_fade_law``: a known law, and anything but the defaults needs a paste to act on."""
        from .audio_in import check_fade_law
        check_fade_law(fade_law, match_gain, pastes)

    @staticmethod
    def _check_fade(fade: int, frame_samples: int, halo_frames: int, reach: int, inside: bool):
        """The fade and halo rules of a paste: ``fade`` counts samples of ``frame_samples`` per latent frame and stays
        within ``wave_paste``'s ramp; ``reach`` 16 kHz samples past a regenerated frame must lie inside the decoded
        region wherever that region's edge is ``inside`` the clip."""
        from . import kernels
        if not 0 <= fade <= kernels.PASTE_MAX_FADE_FRAMES * frame_samples:
            raise ValueError(f"fade_samples must be in 0 .. {kernels.PASTE_MAX_FADE_FRAMES * frame_samples}")
        if inside and halo_frames * FRAME_SAMPLES < reach:
            raise ValueError(f"halo_frames * 512 must be at least {reach}: the fade, and at another rate the resampling "
                             "filter's reach, must end inside the decoded region")

    def _encode_latent(self, wav16, seeds, S, sample_posterior=True):
        """``wav16`` (B, L * 512) on the device -> the scaled latent z (B, C, L) of the whole recording: the posterior's
        sample with e0 = ``recipe.edit_noise(seeds, S, C, L)[2]`` (the global device RNG without seeds), or its mode
        without ``sample_posterior``."""
        return self._posterior_latent(self._encode(wav16).parameters, seeds, S, sample_posterior)

    def _posterior_latent(self, moments, seeds, S, sample_posterior=True):
        """The scaled latent z (B, C, L) of the encoder's ``moments`` (B, 2C, L), as ``_encode_latent`` states it."""
        from . import kernels
        e0 = None
        if sample_posterior:
            B, Cc, L = moments.shape[0], moments.shape[1] // 2, moments.shape[2]
            e0 = (recipe.edit_noise(seeds, S, Cc, L)[2].to(moments.device) if seeds is not None
                  else torch.randn((B, Cc, L), device=moments.device))
        return kernels.latent_init(None, moments=moments.float().contiguous(), e0=e0,
                                   scale=float(self.model.scale_factor), want_x=False)[0]

    def _encode_ring(self, wav16, seeds, S, sample_posterior=True, halo_frames: int = 32):
        """``_encode_latent`` of a recording that is about to loop: ``wav16`` (B, L * 512) is encoded as the periodic
        signal it becomes, cat(wav[:, -he * 512:], wav, wav[:, :he * 512]) with he = min(``halo_frames``, L), and the
        moments of the centre L frames are kept, so that the encoder's zero padding at a clip's edges stays he frames
        away from the wrap: the mirror of ``generate_loop``'s circular decode halo.  e0 is
        ``recipe.edit_noise(seeds, S, C, L)[2]``, drawn at the ring's length.  The 32 frames are the same choice as
        there, not a measurement (no trained weights here to listen to)."""
        L = wav16.shape[1] // FRAME_SAMPLES
        he = min(int(halo_frames), L)
        n = he * FRAME_SAMPLES
        padded = torch.cat([wav16[:, wav16.shape[1] - n:], wav16, wav16[:, :n]], 1).contiguous()
        moments = self._encode(padded).parameters[:, :, he:he + L]
        return self._posterior_latent(moments, seeds, S, sample_posterior)

    def _joint_region(self, z, m, region, r, cond, seeds, S, overlap, strength, clips_per_call, **kw):
        """Denoises ``region`` = (a, b, starts, W) of the latent ``z`` (B, C, L) jointly, in place: one ``sample_joint``
        call from z[:, :, a:b] under the mask m[:, a:b], with the seeds ``recipe.window_seed(seed, r)``; ``kw`` are the
        sampler's guidance arguments."""
        a, b, starts, W = region
        rseeds = None if seeds is None else [recipe.window_seed(sd, r) for sd in seeds]
        zr, _ = self.sampler.sample_joint(S=S, conditioning=cond, length=b - a, starts=starts, window=W,
                                          overlap=overlap, seeds=rseeds, clips_per_call=clips_per_call,
                                          init=z[:, :, a:b].contiguous(), mask=m[:, a:b], strength=strength, **kw)
        z[:, :, a:b] = zr

    def _edit_long_latent(self, cond, seeds, wav, latent, mask, union, W, overlap, strength, sample_posterior, steps,
                          unconditional, cfg_scale, joint=False, joint_clips_per_call=1):
        """The latent of ``edit_long``: ``wav`` (B, L * 512) on the device or ``latent`` (B, C, L), ``mask`` (B, L) on
        the host or None, ``union`` its per-frame any over the batch, W the window length.  ``joint``: one
        ``sample_joint`` call per region of ``joint_edit_regions`` instead of one ``sample_edit`` call per window."""
        S = steps or self.steps
        L = len(union)
        B = wav.shape[0] if wav is not None else latent.shape[0]
        if any(union) and L <= W:
            return self._edit_latent(cond, seeds, wav, latent, mask, strength, sample_posterior, steps, unconditional,
                                     cfg_scale)
        if wav is not None:
            z = self._encode_latent(wav, seeds, S, sample_posterior)
        else:
            z = latent.to(torch.device("cuda")).float().clone()
        kw = dict(guidance_scale=self.guidance_scale, original_inference_steps=self.original_inference_steps,
                  unconditional_conditioning=unconditional, unconditional_guidance_scale=cfg_scale)
        if joint:
            m = torch.ones((B, L)) if mask is None else mask.cpu()
            ov = W // 2 if overlap is None else overlap
            for r, region in enumerate(joint_edit_regions(union, W, ov)):
                self._joint_region(z, m, region, r, cond, seeds, S, ov, strength, joint_clips_per_call, **kw)
        elif any(union):
            m = torch.ones((B, L)) if mask is None else mask.cpu().clone()
            for k, s in enumerate(edit_windows(union, W, overlap)[0]):
                wseeds = None if seeds is None else [recipe.window_seed(sd, k) for sd in seeds]
                zk, _ = self.sampler.sample_edit(S=S, conditioning=cond, init=z[:, :, s:s + W].contiguous(),
                                                 mask=m[:, s:s + W], strength=strength, seeds=wseeds, **kw)
                z[:, :, s:s + W] = zk
                m[:, s:s + W] = 0.0
        return z

    def _paste_regions(self, out, z, pm, regions, fade_samples, rate: int = SAMPLE_RATE,
                       frame_samples: int = FRAME_SAMPLES, fade_law: str = "linear", match_gain: bool = False):
        """The paste of ``edit_long(keep_original=True)``: each region [a, b) of latent frames is decoded, resampled
        from 16 kHz to ``rate`` when that is another one ((b - a) * frame_samples samples exactly) and blended into
        ``out`` (B, N at ``rate``) in place by one ``kernels.paste``: ``kernels.wave_paste`` by default, else the
        region's own ``kernels.seam_stats`` and ``kernels.wave_paste_law``."""
        from . import kernels
        for a, b in regions:
            gen = self.decode(z[:, :, a:b].contiguous())["wav"].contiguous()
            if rate != SAMPLE_RATE:
                gen = kernels.resample(gen, SAMPLE_RATE, rate)
                assert gen.shape[1] == (b - a) * frame_samples
            kernels.paste(out, gen, pm, gen_start=a * frame_samples, fade_samples=fade_samples,
                          frame_samples=frame_samples, out=out, fade_law=fade_law, match_gain=match_gain)

    @torch.no_grad()
    def run_edit(self, plan: EditPlan, cond: torch.Tensor, seeds: Optional[Sequence[int]], strength: float = 0.5):
        """One clip per row of ``cond`` from the one recording of ``plan`` (``audio_in.plan_edit``) -> (the waveform
        (B, samples) on the device, the rate to write it under, the mel or None).  Variation and inpainting: the clip is
        cropped to the DiT's length limit and encoded once, the posterior is expanded to the batch, and ``edit`` makes
        the whole clip again, resampled to the plan's output rate and brought to the plan's level
        (``audio_in.finish_output``).  Keep-original: ``edit_long`` at the plan's rate on the whole recording, cropped
        to the input's sample count; no whole-clip mel is decoded.  With ``plan.joint`` the frames to regenerate are
        denoised jointly, and a variation or an inpainting is ``edit_long(joint=True)`` on the whole recording instead
        of a crop.  Extend: ``extend`` on the recording's whole frames, cropped to the plan's sample count.  Loops from
        the recording: ``loop_from`` on the plan's seam (and spans), or for "loop_vary" ``edit_loop`` without a mask at
        the plan's output rate, level and seam fade; one period each."""
        B = cond.shape[0]

        def span_mask(T):
            return None if plan.spans is None else torch.from_numpy(spans_to_mask(plan.spans, T)).expand(B, T)
        # the whole recording, once per clip
        if plan.mode in ("extend", "keep_original", "loop_from", "loop_vary") or plan.joint:
            wav = np.broadcast_to(plan.samples, (B, plan.samples.size)).copy()
            if plan.mode == "loop_from":
                mask = None if plan.mask is None else np.broadcast_to(plan.mask, (B, plan.mask.size)).copy()
                out = self.loop_from(cond, seeds, wav, plan.seam_frames, strength, mask, fade_samples=plan.fade,
                                     fade_law=plan.fade_law, match_gain=plan.match_gain)
                return out["wav"], plan.out_rate, None
            if plan.mode == "loop_vary":
                out = self.edit_loop(cond, seeds, wav=wav, strength=strength, level=plan.level,
                                     out_sample_rate=plan.out_rate, loop_fade_samples=plan.loop_fade)
                return out["wav"], out["rate"], out["mel"]
            if plan.mode == "extend":
                out = self.extend(cond, seeds, wav, plan.extend_frames, fade_samples=plan.fade,
                                  fade_law=plan.fade_law, match_gain=plan.match_gain)
                return out["wav"][:, :plan.n_out], plan.out_rate, None
            if plan.mode == "keep_original":
                mask = np.broadcast_to(plan.mask, (B, plan.mask.size)).copy()
                out = self.edit_long(cond, seeds, wav=wav, mask=mask, strength=strength, keep_original=True,
                                     rate=plan.rate, fade_samples=plan.fade, joint=plan.joint,
                                     fade_law=plan.fade_law, match_gain=plan.match_gain)
                return out["wav"][:, :plan.n_samples], plan.out_rate, None
            out = self.edit_long(cond, seeds, wav=wav, mask=span_mask(plan.samples.size // plan.frame_samples),
                                 strength=strength, joint=True)
        else:
            crop = self.model.unet.diffusion_model.cfg.max_latent_len * plan.frame_samples
            post = self._encode(plan.samples[:crop])
            init = DiagonalGaussianDistribution(post.parameters.expand(B, -1, -1).contiguous())
            out = self.edit(cond, seeds, latent=init, mask=span_mask(post.mean.shape[2]), strength=strength)
        wav, rate = finish_output(out["wav"], plan.out_rate, plan.level)
        return wav, rate, out["mel"]

    @torch.no_grad()
    def extend(self, cond: torch.Tensor, seeds: Optional[Sequence[int]], wav, extra_frames: int,
               context_frames: Optional[int] = None, window: Optional[int] = None, overlap: Optional[int] = None,
               fade_samples: Optional[int] = None, halo_frames: int = 32, steps: Optional[int] = None,
               joint_clips_per_call: int = 1, fade_law: str = "linear",
               match_gain: bool = False) -> Dict[str, torch.Tensor]:
        """Continues a recording: ``wav`` (B, N) at 16 kHz, N = L0 * 512, comes back followed by ``extra_frames`` new
        latent frames that continue it.

        The recording is encoded alone (z_rec = the scaled posterior sample with e0 =
        ``recipe.edit_noise(seeds, S, C, L0)[2]``, as in ``edit_long``) and followed by ``extra_frames`` frames of mask
        1.  One ``sample_joint(init=..., mask=..., strength=1.0)`` call denoises the region [max(L0 - context, 0),
        L0 + extra) jointly on ``long_windows``' plan (W = ``window`` or latent_shape[1], ``overlap`` = W // 2 by
        default, ``context_frames`` = ``overlap`` by default; seeds ``recipe.window_seed(seed, 0)``): the last
        ``context`` frames of the recording are known context to every window that covers them, the new frames start
        from pure noise, and a continuation of any length costs S DiT calls per clip.  The frames [max(L0 -
        ``halo_frames``, 0), L0 + extra) are decoded and blended into ``cat(wav, zeros)`` by one
        ``kernels.wave_paste``: the recording's samples are its own bit for bit up to ``fade_samples`` (default 512)
        before the junction at sample N, the raised-cosine fade closes the junction, and from the junction on
        everything is generated.  ``halo_frames`` * 512 >= ``fade_samples`` is required unless the decode starts at
        frame 0.  ``fade_law`` and ``match_gain`` are ``edit_long``'s; the one run has one junction, at sample N.

        Returns latent (B, C, L0 + extra; the first L0 frames are z_rec), wav (B, (L0 + extra) * 512) and region
        (a, L0 + extra).  ValueError for ``extra_frames`` < 1, an empty recording, or a region of more than 32
        windows."""
        from . import kernels
        dev = torch.device("cuda")
        S = steps or self.steps
        self._check_law(fade_law, match_gain)
        wav = torch.as_tensor(wav, dtype=torch.float32).to(dev).contiguous()
        if wav.dim() != 2 or wav.shape[1] % FRAME_SAMPLES or wav.shape[1] < FRAME_SAMPLES:
            raise ValueError(f"`wav` is (B, N) with N a multiple of {FRAME_SAMPLES} and at least one frame")
        extra = int(extra_frames)
        if extra < 1:
            raise ValueError(f"extra_frames must be at least 1, got {extra_frames}")
        B, L0 = wav.shape[0], wav.shape[1] // FRAME_SAMPLES
        L = L0 + extra
        W = window or self.latent_shape[1]
        ov = W // 2 if overlap is None else overlap
        context = ov if context_frames is None else int(context_frames)
        if context < 0:
            raise ValueError("context_frames must not be negative")
        a = max(L0 - context, 0)
        spans, Wr = windows.long_windows(L - a, W, ov)
        windows.check_region_windows(a, L, len(spans), Wr)
        fade = FRAME_SAMPLES if fade_samples is None else int(fade_samples)
        h0 = max(L0 - int(halo_frames), 0)
        self._check_fade(fade, FRAME_SAMPLES, halo_frames, fade, h0 > 0)
        z_rec = self._encode_latent(wav, seeds, S)
        z = torch.cat([z_rec, torch.zeros((B, z_rec.shape[1], extra), device=dev)], 2)
        m = torch.zeros((B, L), device=dev)
        m[:, L0:] = 1.0
        self._joint_region(z, m, (a, L, [s for s, _ in spans], Wr), 0, cond, seeds, S, ov, 1.0, joint_clips_per_call,
                           guidance_scale=self.guidance_scale, original_inference_steps=self.original_inference_steps)
        gen = self.decode(z[:, :, h0:].contiguous())["wav"].contiguous()
        out = torch.cat([wav, torch.zeros((B, extra * FRAME_SAMPLES), device=dev)], 1)
        kernels.paste(out, gen, m, gen_start=h0 * FRAME_SAMPLES, fade_samples=fade, out=out, fade_law=fade_law,
                      match_gain=match_gain)
        return dict(latent=z, wav=out, region=(a, L))

    @torch.no_grad()
    def edit_loop(self, cond: torch.Tensor, seeds: Optional[Sequence[int]], wav=None,
                  latent: Optional[torch.Tensor] = None, mask=None, strength: float = 0.5,
                  window: Optional[int] = None, overlap: Optional[int] = None, keep_original: bool = False,
                  fade_samples: Optional[int] = None, halo_frames: int = 32, out_sample_rate: Optional[int] = None,
                  level=None, loop_fade_samples: Optional[int] = None, sample_posterior: bool = True,
                  steps: Optional[int] = None, unconditional: Optional[torch.Tensor] = None, cfg_scale: float = 1.0,
                  joint_clips_per_call: int = 1, fade_law: str = "linear",
                  match_gain: bool = False) -> Dict[str, torch.Tensor]:
        """A loop from a recording: ``edit_long(joint=True)`` on a ring.  The input is exactly one of ``wav`` (B, N) at
        16 kHz, N = L * 512, encoded as the periodic signal it is about to become (``_encode_ring``), and ``latent``
        (B, C, L); its L >= 2 frames are one period, frame L - 1 the left neighbour of frame 0.  ``mask`` (B, L), 1 =
        regenerate; None = all ones, a variation of the whole ring at ``strength``.

        The latent follows ``windows.ring_edit_regions`` on the batch's union mask (W = min(``window`` or
        latent_shape[1], L), ``overlap`` = W // 2 by default).  A line region ("line", a, R, starts, W), which may lie
        across the wrap, is gathered as z[:, :, (a + arange(R)) % L], denoised by ``edit_long(joint=True)``'s own
        ``sample_joint(init=..., mask=...)`` call with the seeds ``recipe.window_seed(seed, r)`` and scattered back:
        the new frames either side of the wrap are conditioned on both neighbours.  When the regions cover the ring,
        the one entry ("ring", ...) is one ``sample_ring_edit`` call on the whole ring (r = 0).  Frames of mask 0
        keep the input latent exactly; S DiT calls per region and clip.

        ``keep_original=False``: the ring is decoded exactly as ``generate_loop`` decodes its latent (circular halo
        min(``halo_frames``, L), ``out_sample_rate``, ``kernels.wave_loop`` with ``loop_fade_samples``, ``level``), and L
        must be a multiple of ``audio_in.loop_multiple(rate)``; returns latent, mel, wav, rate and ext.

        ``keep_original=True`` (needs ``wav``; 16 kHz only, so ``out_sample_rate``, ``level`` and ``loop_fade_samples``
        are refused as ``edit_long`` refuses a rate): per entry of ``windows.ring_paste_regions(union, halo_frames)``
        the frames (a + j) mod L, j < n, are decoded in one call and blended into a copy of ``wav`` by one in-place
        ``kernels.wave_paste_ring`` with gen_start = a * 512; for ("ring",) the ring is cut open at frame a =
        ``windows.ring_paste_cut(union, ceil(fade_samples / 512))`` and decoded from there once round,
        z[:, :, (arange(L + 2h) + a - h) % L] with the circular halo h = min(``halo_frames``, L) either side, and the
        centre N samples are pasted at gen_start = a * 512: every sample of gen has h frames of context.  a is the
        middle of the longest run of kept frames when that leaves the fade's reach of kept frames either side of the
        cut: the paste then does not use the decode where its two ends meet, and the samples either side of the
        wrap are consecutive samples of the one decode, as they are for a region.  Without such a run (every frame
        regenerated, or only short gaps) a = 0: the centre N samples at gen_start = 0, whose two ends meet at the
        wrap as two renderings that agree to the halo's accuracy.  Samples further than ``fade_samples`` (default 512) from a
        regenerated frame, measured round the ring, keep the input's bits.  ``halo_frames`` * 512 >= ``fade_samples``
        always: a ring has no clip end that would exempt a region.  ``fade_law`` and ``match_gain`` are
        ``edit_long``'s, with ``keep_original`` only; junctions, zones and runs are taken round the ring, for a region as
        for the ring cut open.  Returns latent, wav (B, N) and regions."""
        from . import kernels
        self._check_law(fade_law, match_gain, keep_original)
        if (wav is None) == (latent is None):
            raise ValueError("pass exactly one of `wav` and `latent`")
        if keep_original and wav is None:
            raise ValueError("keep_original needs the input waveform `wav`")
        if keep_original and (out_sample_rate is not None or level is not None or loop_fade_samples is not None):
            raise ValueError("`out_sample_rate`, `level` and `loop_fade_samples` are used without keep_original: a kept "
                             "recording stays at 16 kHz and at its own level")
        dev = torch.device("cuda")
        S = steps or self.steps
        if wav is not None:
            wav = torch.as_tensor(wav, dtype=torch.float32).to(dev).contiguous()
            if wav.dim() != 2 or wav.shape[1] % FRAME_SAMPLES:
                raise ValueError(f"`wav` is (B, N) with N a multiple of {FRAME_SAMPLES}")
            B, L = wav.shape[0], wav.shape[1] // FRAME_SAMPLES
        else:
            B, L = latent.shape[0], latent.shape[2]
        if L < 2:
            raise ValueError(f"a loop has at least 2 latent frames, got {L}")
        halo = int(halo_frames)
        if keep_original:
            fade = FRAME_SAMPLES if fade_samples is None else int(fade_samples)
            self._check_fade(fade, FRAME_SAMPLES, halo, fade, True)
        else:
            tail = self._loop_tail_plan(L, min(halo, L), loop_fade_samples, out_sample_rate)
        if mask is None:
            union = [True] * L
        else:
            mask = torch.as_tensor(mask, dtype=torch.float32)
            if tuple(mask.shape) != (B, L):
                raise ValueError(f"mask must be (B, L) = {(B, L)}, got {tuple(mask.shape)}")
            union = (mask > 0).any(0).tolist()
        W = min(window or self.latent_shape[1], L)
        ov = W // 2 if overlap is None else overlap
        plan = windows.ring_edit_regions(union, W, ov)
        regions = windows.ring_paste_regions(union, halo) if keep_original else None

        if wav is not None:
            z = self._encode_ring(wav, seeds, S, sample_posterior, halo)
        else:
            z = latent.to(dev).float().clone()
        kw = dict(guidance_scale=self.guidance_scale, original_inference_steps=self.original_inference_steps,
                  unconditional_conditioning=unconditional, unconditional_guidance_scale=cfg_scale)
        m = torch.ones((B, L)) if mask is None else mask.cpu()
        for r, entry in enumerate(plan):
            if entry[0] == "ring":
                _, starts, Wr, ovr = entry
                rseeds = None if seeds is None else [recipe.window_seed(sd, r) for sd in seeds]
                z, _ = self.sampler.sample_ring_edit(S=S, conditioning=cond, init=z, starts=starts, window=Wr,
                                                     overlap=ovr, mask=None if mask is None else m,
                                                     strength=strength, seeds=rseeds,
                                                     clips_per_call=joint_clips_per_call, **kw)
            else:
                _, a, R, starts, Wr = entry
                idx = (a + torch.arange(R)) % L
                zr = z[:, :, idx.to(dev)].contiguous()
                self._joint_region(zr, m[:, idx], (0, R, starts, Wr), r, cond, seeds, S, ov, strength,
                                   joint_clips_per_call, **kw)
                z[:, :, idx.to(dev)] = zr
        if not keep_original:
            return dict(latent=z, **self._decode_loop(z, *tail, level))

        out = wav.clone()
        pm = m.to(dev).contiguous()
        for region in regions:
            if region == ("ring",):
                # the ring is cut open at frame a, among kept frames where it has them, and decoded from there once
                # round with the circular halo either side: every sample of gen has h frames of context
                h = min(halo, L)
                a = windows.ring_paste_cut(union, -(-fade // FRAME_SAMPLES))
                idx = (torch.arange(L + 2 * h, device=dev) + a - h) % L
                gen = self.decode(z[:, :, idx].contiguous())["wav"][:, h * FRAME_SAMPLES:(h + L) * FRAME_SAMPLES]
            else:
                a, n = region
                gen = self.decode(z[:, :, ((a + torch.arange(n, device=dev)) % L)].contiguous())["wav"]
            kernels.paste(out, gen.contiguous(), pm, gen_start=a * FRAME_SAMPLES, fade_samples=fade, out=out,
                          ring=True, fade_law=fade_law, match_gain=match_gain)
        return dict(latent=z, wav=out, regions=regions)

    @torch.no_grad()
    def loop_from(self, cond: torch.Tensor, seeds: Optional[Sequence[int]], wav, seam_frames: int = 32,
                  strength: float = 1.0, mask=None, **kw) -> Dict[str, torch.Tensor]:
        """Makes a recording loop: ``edit_loop(keep_original=True)`` under ``windows.seam_mask(L, seam_frames)``, OR-ed
        with ``mask`` (B, L) when one is given.  Only the ``seam_frames`` frames either side of the wrap are made anew,
        conditioned on the recording across the wrap on both sides; every other sample is the recording's own, bit for
        bit, up to the paste's fade.  The defaults are choices, not measurements (no trained weights here to listen
        to): a seam of 32 frames, about 1 s either side, and strength 1.0, so the seam frames start from pure noise.
        ``kw`` are ``edit_loop``'s further arguments, ``fade_law`` and ``match_gain`` among them.  ValueError unless 1 <= seam_frames and 2 * seam_frames <= L."""
        wav = torch.as_tensor(wav, dtype=torch.float32)
        if wav.dim() != 2 or wav.shape[1] % FRAME_SAMPLES:
            raise ValueError(f"`wav` is (B, N) with N a multiple of {FRAME_SAMPLES}")
        B, L = wav.shape[0], wav.shape[1] // FRAME_SAMPLES
        if L < 2:
            raise ValueError(f"a loop has at least 2 latent frames, got {L}")
        m = torch.from_numpy(windows.seam_mask(L, seam_frames)).float().expand(B, L)
        if mask is not None:
            mask = torch.as_tensor(mask, dtype=torch.float32).cpu()
            if tuple(mask.shape) != (B, L):
                raise ValueError(f"mask must be (B, L) = {(B, L)}, got {tuple(mask.shape)}")
            m = torch.maximum(m, mask)
        return self.edit_loop(cond, seeds, wav=wav, mask=m.contiguous(), strength=strength, keep_original=True, **kw)

    def long_windows(self, latent_len: int, window: Optional[int] = None, overlap: Optional[int] = None):
        """``windows.long_windows``, the plan of ``generate_long``; ``window`` defaults to latent_shape[1]."""
        return windows.long_windows(latent_len, window or self.latent_shape[1], overlap)

    @torch.no_grad()
    def generate_long(self, cond: torch.Tensor, seeds: Sequence[int], latent_len: int, window: Optional[int] = None,
                      overlap: Optional[int] = None, steps: Optional[int] = None,
                      joint: bool = False, joint_clips_per_call: int = 1) -> Dict[str, torch.Tensor]:
        """Long-form continuation past the DiT's length limit: window 0 is ``generate``'s latent for the prompt's own
        seeds; window k >= 1 is a ``sample_edit`` call at strength 1 whose known context (mask 0) is the previous
        ``overlap`` frames and whose remaining frames (mask 1) are new, with seeds ``recipe.window_seed(seed, k)``.
        The windows' new frames are concatenated into one (B, C, latent_len) latent, decoded and vocoded in one call
        each.  Defaults: window = latent_shape[1], overlap = window // 2.

        ``joint=True``: the same windows are denoised jointly instead of one after another
        (``LCMSampler.sample_joint``): every LCM step runs all windows of a clip through the DiT as one batch and
        averages their estimates where they overlap (``joint_weights``), with the noise of
        ``recipe.prompt_noise(seeds, S, C, latent_len)``.  It is another sampler, not another route to the same clip.
        ``joint_clips_per_call`` is ``sample_joint``'s ``clips_per_call``: 1 keeps a clip independent of its batch bit
        for bit, a larger value packs several clips' windows into a DiT call (faster from a few clips on; a clip then
        agrees across batch sizes to about 3e-6)."""
        B, Cc = cond.shape[0], self.latent_shape[0]
        S = steps or self.steps
        spans, W = self.long_windows(latent_len, window, overlap)
        kw = dict(guidance_scale=self.guidance_scale, original_inference_steps=self.original_inference_steps)
        if joint:
            ov = (window or self.latent_shape[1]) // 2 if overlap is None else overlap
            z, _ = self.sampler.sample_joint(S=S, conditioning=cond, length=latent_len, starts=[s for s, _ in spans],
                                             window=W, overlap=ov, seeds=seeds,
                                             clips_per_call=joint_clips_per_call, **kw)
            return dict(latent=z, **self.decode(z))
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

    def loop_windows(self, latent_len: int, window: Optional[int] = None, overlap: Optional[int] = None):
        """``windows.loop_windows``, the plan of ``generate_loop``; ``window`` defaults to latent_shape[1]."""
        return windows.loop_windows(latent_len, window or self.latent_shape[1], overlap)

    @torch.no_grad()
    def generate_loop(self, cond: torch.Tensor, seeds: Optional[Sequence[int]], latent_len: int,
                      window: Optional[int] = None, overlap: Optional[int] = None, steps: Optional[int] = None,
                      halo_frames: Optional[int] = None, fade_samples: Optional[int] = None,
                      out_sample_rate: Optional[int] = None, level=None, joint_clips_per_call: int = 1,
                      x_T: Optional[torch.Tensor] = None,
                      noise: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """A clip that loops: played end to start it has no seam.  The period is L = ``latent_len`` frames.

        The latent is denoised on a ring (``sample_joint(ring=True)`` on ``loop_windows``' plan): no frame is an end,
        and rotating the noise rotates the latent.  The decoders zero-pad at a clip's edges, so the ring is decoded with
        a circular halo: z_ext = z[:, :, (arange(L + 2h) - h) mod L], h = ``halo_frames`` (default min(32, L), 1 <= h <=
        L), in one ``decode`` call.  With ``out_sample_rate`` the whole extended waveform is resampled, as the one
        continuous signal it is.  ``kernels.wave_loop`` then cuts the period of N samples that starts h frames in: its
        first sample is the one that follows its last in the extended waveform, and what the halo leaves of a
        difference between that continuation and the period's own start is faded out over ``fade_samples`` (default
        32 ms at the output rate, at most h frames).  With ``level`` (``audio_in.check_level``) the N samples are
        brought to that level by one static gain (``kernels.normalize_loudness``), which keeps the period.

        The period is a whole number of frames and of output samples: L, and h after rounding up, are multiples of
        125 / gcd(125, rate) (``audio_in.loop_multiple``; ValueError for L otherwise).  ``x_T`` (B, C, L) and ``noise``
        (S - 1, B, C, L) replace ``recipe.prompt_noise(seeds, S, C, L)``.  Returns latent (B, C, L), mel (the centre 2L
        frames), wav (B, N), rate, and ext, the extended waveform at that rate that wav was cut from."""
        L = int(latent_len)
        tail = self._loop_tail_plan(L, halo_frames, fade_samples, out_sample_rate)
        starts, W, ov = self.loop_windows(L, window, overlap)
        z, _ = self.sampler.sample_joint(S=steps or self.steps, conditioning=cond, length=L, starts=starts, window=W,
                                         overlap=ov, seeds=seeds, x_T=x_T, noise=noise,
                                         guidance_scale=self.guidance_scale,
                                         original_inference_steps=self.original_inference_steps,
                                         clips_per_call=joint_clips_per_call, ring=True)
        return dict(latent=z, **self._decode_loop(z, *tail, level))

    @staticmethod
    def _loop_tail_plan(L: int, halo_frames, fade_samples, out_sample_rate):
        """(rate, h, fade) of a loop's decode, checked before any GPU work: the output rate, the circular halo in
        frames rounded up to ``audio_in.loop_multiple(rate)`` and the seam fade in output samples; ValueError as
        ``generate_loop`` states them."""
        from .audio_in import fade_samples_of, loop_multiple
        rate = SAMPLE_RATE if out_sample_rate is None else int(out_sample_rate)
        mult = loop_multiple(rate)
        if L < 2 or L % mult:
            raise ValueError(f"a loop at {rate} Hz is a multiple of {mult} latent frames and at least 2, got {L} "
                             "(audio_in.loop_frames)")
        per_frame = lambda n: n * FRAME_SAMPLES * rate // SAMPLE_RATE   # noqa: E731  (whole for multiples of mult)
        h = min(32, L) if halo_frames is None else int(halo_frames)
        if not 1 <= h <= L:
            raise ValueError(f"halo_frames must be in 1 .. {L}, got {h}")
        h = -(-h // mult) * mult
        fade = fade_samples_of(32.0, rate) if fade_samples is None else int(fade_samples)
        if not 0 <= fade <= min(per_frame(h), per_frame(L)):
            raise ValueError(f"fade_samples must be in 0 .. {min(per_frame(h), per_frame(L))}: the halo's {h} frames")
        return rate, h, fade

    def _decode_loop(self, z, rate: int, h: int, fade: int, level=None):
        """The tail of ``generate_loop`` and of ``edit_loop``: the ring latent z (B, C, L) decoded with a circular halo
        of h frames in one ``decode`` call, resampled to ``rate`` as one signal, the period cut and its seam closed by
        ``kernels.wave_loop`` and brought to ``level``: mel, wav, rate and ext."""
        from . import kernels
        L = z.shape[2]
        per_frame = lambda n: n * FRAME_SAMPLES * rate // SAMPLE_RATE   # noqa: E731
        idx = (torch.arange(L + 2 * h, device=z.device) - h) % L
        dec = self.decode(z[:, :, idx].contiguous())
        ext = dec["wav"].contiguous()
        if rate != SAMPLE_RATE:
            ext = kernels.resample(ext, SAMPLE_RATE, rate)
        if ext.shape[1] != per_frame(L + 2 * h):
            raise RuntimeError(f"the extended waveform has {ext.shape[1]} samples, not {per_frame(L + 2 * h)}")
        wav = kernels.wave_loop(ext, per_frame(h), per_frame(L), fade)
        if level is not None:
            if level.limiter:
                raise ValueError("a loop takes a static gain only: the limiter's gain varies in time and starts from 1 "
                                 "at the first sample, which would break the period")
            wav = kernels.normalize_loudness(wav, rate, level.loudness, level.peak_dbfs, level.true_peak)["wav"]
        return dict(mel=dec["mel"][..., 2 * h:2 * (h + L)], wav=wav, rate=rate, ext=ext)

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Latent -> waveform only (config 5: long-form decode, the DiT caps at T <= 845)."""
        mel = self.model.decode_first_stage(z)
        return dict(mel=mel, wav=self.vocoder(mel).squeeze(1))
