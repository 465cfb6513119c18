"""LCM_audio / LCMSampler mirrors: the sampler hot loop driving the HIP DiT + step kernels.

  LCM_audio    ldm/models/diffusion/lcm_audio.py:46-116 (inference members), apply_model :479-502,
               decode_first_stage :392-406, schedule buffers ddpm.py:116-168
  LCMSampler   ldm/models/diffusion/scheduling_lcm.py:13-496

Differences from the reference that are deliberate and documented in DESIGN.md:
  * RNG: x_T and the per-step noise are drawn per prompt from ``torch.Generator(seed)``
    (SURVEY.md §7 "RNG parity") when ``seeds`` are given, so results do not depend on
    how prompts are sharded over GPUs; without seeds the global device RNG is used as
    in the reference (scheduling_lcm.py:354,485).
  * the condition embedders are step-invariant and run once per ``sample`` call.
  * optional classifier-free guidance (BASELINE config 4): batch-doubled [uc; c] DiT call
    and the combine e_u + s(e_c - e_u) fused into the LCM step kernel.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List, Optional, Sequence, Tuple

import torch

from . import _hip, kernels, recipe, schedule, windows
from ._hip import check, lib, ptr, stream_handle
from .config import instantiate_from_config
from .models import AutoencoderKL, ConcatDiT2MLP, DiagonalGaussianDistribution


class DiffusionWrapper:
    """ddpm.py:1397-1437 (crossattn branch): holds ``diffusion_model``."""

    def __init__(self, diffusion_model, conditioning_key="crossattn"):
        self.diffusion_model = diffusion_model
        self.conditioning_key = conditioning_key

    def __call__(self, x, t, c_crossattn=None, w_cond=None, **kw):
        cc = torch.cat(c_crossattn, 1) if isinstance(c_crossattn, (list, tuple)) else c_crossattn
        return self.diffusion_model(x, t, context=cc, w_cond=w_cond)


class LCM_audio:
    """Inference surface of LCM_audio (lcm_audio.py) built from configs/audiolcm.yaml params."""

    def __init__(self, unet_config=None, first_stage_config=None, cond_stage_config=None, timesteps=1000,
                 linear_start=0.00085, linear_end=0.012, mel_dim=20, mel_length=312, conditioning_key="crossattn",
                 scale_factor=1.0, num_ddim_timesteps=50, split: bool = True, **unused):
        self.num_timesteps = int(timesteps)
        self.mel_dim, self.mel_length = mel_dim, mel_length
        self.channels = int(unused.get("channels", 0))
        self.alphas_cumprod = schedule.alphas_cumprod(timesteps, linear_start, linear_end)
        self.scale_factor = float(scale_factor)
        self.num_ddim_timesteps = num_ddim_timesteps
        self.split = split
        dit = instantiate_from_config(unet_config, split=split) if unet_config else ConcatDiT2MLP(split=split)
        self.unet = DiffusionWrapper(dit, conditioning_key)
        self.model = self.unet  # `model`, `unet`, `target_unet` share weights at inference (lcm_audio.py:98-114)
        self.first_stage_model = (instantiate_from_config(first_stage_config, split=split) if first_stage_config
                                  else AutoencoderKL(split=split))
        self.cond_stage_model = (instantiate_from_config(cond_stage_config, split=split) if cond_stage_config
                                 else None)

    # -- weights ---------------------------------------------------------------------------------
    def load_state_dict(self, sd, strict=False):
        """Lightning ``state_dict`` (Appendix A): ``unet.diffusion_model.*`` (the sampler's net; falls back
        to ``model.diffusion_model.*``), ``first_stage_model.*``, ``scale_factor``."""
        def sub(prefix):
            return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        dit = sub("unet.diffusion_model.") or sub("model.diffusion_model.")
        if dit:
            self.unet.diffusion_model.load_state_dict(dit)
        fs = sub("first_stage_model.")
        if fs:
            self.first_stage_model.load_state_dict(fs)
        cs = sub("cond_stage_model.")
        if cs and self.cond_stage_model is not None and hasattr(self.cond_stage_model, "load_state_dict"):
            self.cond_stage_model.load_state_dict(cs)
        if "scale_factor" in sd:
            self.scale_factor = float(sd["scale_factor"])
        return self

    def load_recipe(self, seed: int = 0, encoder: bool = False):
        """``encoder``: also load the VAE encoder (``recipe.vae_encoder_state``), which the audio-in paths need."""
        self.unet.diffusion_model.load_state_dict(recipe.dit_state(seed))
        vae = dict(recipe.vae_state(seed))
        if encoder:
            vae.update(recipe.vae_encoder_state(seed))
        self.first_stage_model.load_state_dict(vae)
        if self.cond_stage_model is not None and hasattr(self.cond_stage_model, "load_state_dict"):
            self.cond_stage_model.load_state_dict(recipe.text_state(seed))
            if hasattr(self.cond_stage_model, "use_synthetic_tokenizer"):  # recipe weights: hash ids are as good
                self.cond_stage_model.use_synthetic_tokenizer()
        return self

    @property
    def betas(self):
        return None

    # -- reference methods -----------------------------------------------------------------------
    def get_learned_conditioning(self, c):
        if self.cond_stage_model is None:
            raise RuntimeError("no cond_stage_model configured")
        return self.cond_stage_model.encode(c) if hasattr(self.cond_stage_model, "encode") else self.cond_stage_model(c)

    def apply_model(self, x_noisy, t, cond, model=None, w_cond=None, return_ids=False):
        model = model or self.unet
        if not isinstance(cond, (list, tuple)):
            cond = [cond]
        return model(x_noisy, t, c_crossattn=cond, w_cond=w_cond)

    def decode_first_stage(self, z):
        return self.first_stage_model.decode(z, self.scale_factor)

    def encode_first_stage(self, x):
        """lcm_audio.py:425-427: mel (B, 80, M) -> DiagonalGaussianDistribution over the latent."""
        return self.first_stage_model.encode(x)

    def get_first_stage_encoding(self, encoder_posterior, generator=None):
        """lcm_audio.py:197-204: scale_factor * posterior.sample() (a tensor passes through)."""
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample(generator)
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    def eval(self):
        return self

    def cuda(self):
        return self

    def to(self, *a, **k):
        return self

    class _Null:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    def ema_scope(self, context=None):
        return LCM_audio._Null()


def _h2d(t: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device through the pinned caching allocator, asynchronously on the current stream (the pinned
    block stays reserved until the copy has run)."""
    return t.pin_memory().to(dev, non_blocking=True)


_weights_dev = {}


def window_weights_device(starts, W: int, L: int, overlap: int, ring: bool, device) -> torch.Tensor:
    """``windows.window_weights(...)`` on ``device``, uploaded once per argument tuple and device."""
    key = (tuple(int(s) for s in starts), int(W), int(L), int(overlap), bool(ring), torch.device(device))
    if key not in _weights_dev:
        _weights_dev[key] = torch.from_numpy(windows.window_weights(*key[:5]).copy()).to(device)
    return _weights_dev[key]


class LCMSampler:
    """LCM multistep sampler (scheduling_lcm.py) over the HIP DiT and the fused step kernel."""

    def __init__(self, model: LCM_audio, **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.original_inference_steps = 100
        self.num_inference_steps = None
        self.timesteps = torch.arange(self.ddpm_num_timesteps - 1, -1, -1, dtype=torch.long)
        self.timestep_scaling = 10.0
        self.prediction_type = "epsilon"
        self._gfreqs = {}

    def make_schedule(self, ddim_discretize="uniform", verbose=True):
        self.alphas_cumprod = self.model.alphas_cumprod

    def set_timesteps(self, num_inference_steps=None, device=None, original_inference_steps=None, timesteps=None,
                      strength=1.0):
        ts = schedule.lcm_timesteps(num_inference_steps, original_inference_steps or self.original_inference_steps,
                                    self.ddpm_num_timesteps, timesteps, strength)
        self.num_inference_steps = len(ts)
        self.timesteps = torch.tensor(ts, dtype=torch.long)
        self._step_index = None

    def retrieve_timesteps(self, num_inference_steps=None, device=None, timesteps=None, **kwargs):
        if timesteps is not None:
            self.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        else:
            self.set_timesteps(num_inference_steps, device=device, **kwargs)
        return self.timesteps, len(self.timesteps)

    def get_guidance_scale_embedding(self, w: torch.Tensor, embedding_dim: int = 512, dtype=torch.float32):
        """[sin | cos](1000 w f_i) on the device (scheduling_lcm.py:87-113)."""
        assert w.dim() == 1
        dev = torch.device("cuda")
        if embedding_dim not in self._gfreqs:
            self._gfreqs[embedding_dim] = schedule.guidance_freqs(embedding_dim).to(dev)
        f = self._gfreqs[embedding_dim]
        out = torch.empty((w.shape[0], 2 * f.numel()), device=dev, dtype=torch.float32)
        wv = w.to(device=dev, dtype=torch.float32).contiguous()
        check(lib().alcm_sincos_embedding(ptr(wv), 1000.0, ptr(f), w.shape[0], f.numel(), 0, ptr(out),
                                          stream_handle()), "guidance embedding")
        if embedding_dim % 2:
            out = torch.nn.functional.pad(out, (0, 1))
        return out

    @staticmethod
    def _cond(conditioning):
        """The conditioning tensor of a call: the reference passes it bare, or as the first entry of a dict of lists."""
        cond = conditioning
        if isinstance(cond, dict):
            cond = cond[list(cond.keys())[0]]
            while isinstance(cond, list):
                cond = cond[0]
        return cond

    def _set_plan(self, plan) -> int:
        """Takes the timesteps of ``plan`` (``schedule.sample_plan``); returns how many of its steps add noise."""
        self.num_inference_steps = len(plan)
        self.timesteps = torch.tensor([p["t"] for p in plan], dtype=torch.long)
        return sum(1 for p in plan if p["add_noise"])

    def _noise_start(self, plan, seeds, x_T, noise, B, Cc, T):
        """The start of ``sample`` and of ``sample_joint`` from pure noise: takes ``plan`` (``_set_plan``) and returns
        (x_T (B, C, T), the step noise or None), fp32 and contiguous on the device: per prompt from
        ``recipe.prompt_noise`` with ``seeds``, else from the global device RNG; ``x_T`` / ``noise`` replace the
        respective draw."""
        dev = torch.device("cuda")
        n_noise = self._set_plan(plan)
        if seeds is not None:
            # host draws (per-prompt generators), copied from pinned memory without blocking the host: a pageable
            # copy waits for everything already queued on the stream, so each call used to start only after the
            # previous call's vocoder had drained, with the GPU idle meanwhile (2.4 ms per bench step, rocprofv3
            # kernel trace of profiles/r4v6)
            xT_h, noise_h = recipe.prompt_noise(seeds, len(plan), Cc, T)
            img = _h2d(xT_h, dev) if x_T is None else x_T
            noise = _h2d(noise_h, dev) if noise is None else noise
        else:
            img = torch.randn((B, Cc, T), device=dev) if x_T is None else x_T
            if noise is None and n_noise:
                noise = torch.randn((n_noise, B, Cc, T), device=dev)
        img = img.to(dev).float().contiguous()
        noise = noise.to(dev).float().contiguous() if noise is not None else None
        return img, noise

    def _context(self, cond, guidance_scale, unconditional_conditioning, unconditional_guidance_scale):
        """(cfg, cemb, w_emb): whether the DiT runs batch-doubled on [uc; c], the embedded context of those rows and
        their guidance-scale embedding.  Step-invariant: once per call."""
        dev = torch.device("cuda")
        cfg = unconditional_conditioning is not None and unconditional_guidance_scale != 1.0
        c = cond.to(dev).float()
        if cfg:
            c = torch.cat([unconditional_conditioning.to(dev).float(), c], 0)
        cemb = self.model.unet.diffusion_model.embed_context(c)
        w = torch.full((c.shape[0],), float(guidance_scale - 1), device=dev, dtype=torch.float32)  # (no host copy)
        return cfg, cemb, self.get_guidance_scale_embedding(w, embedding_dim=256)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, verbose=True, x_T=None, guidance_scale=5., original_inference_steps=50,
               timesteps=None, seeds: Optional[Sequence[int]] = None, noise: Optional[torch.Tensor] = None,
               unconditional_conditioning: Optional[torch.Tensor] = None, unconditional_guidance_scale: float = 1.0,
               **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns (denoised, last sample) like the reference (scheduling_lcm.py:298-342)."""
        self.make_schedule(verbose=verbose)
        if len(shape) != 2:
            raise ValueError("audio latents are (C, T)")
        Cc, T = shape
        cond = self._cond(conditioning)
        if cond.shape[0] != batch_size:
            print(f"Warning: Got {cond.shape[0]} conditionings but batch-size is {batch_size}")
        plan = schedule.sample_plan(S, original_inference_steps, timesteps)
        img, noise = self._noise_start(plan, seeds, x_T, noise, batch_size, Cc, T)
        return self._run(plan, img, noise, cond, batch_size, guidance_scale, unconditional_conditioning,
                         unconditional_guidance_scale)

    def _run(self, plan, img, noise, cond, batch_size, guidance_scale, unconditional_conditioning,
             unconditional_guidance_scale, z0=None, mask=None):
        """The step loop of ``sample`` and ``sample_edit``: img (B, C, T), fp32 and contiguous, at plan[0]'s noise level,
        noise[i] the noise of step i.  With z0 / mask every step blends the denoised estimate with the known latent
        (alcm_lcm_step_edit)."""
        dev = img.device
        dit: ConcatDiT2MLP = self.model.unet.diffusion_model
        cfg, cemb, w_emb = self._context(cond, guidance_scale, unconditional_conditioning, unconditional_guidance_scale)
        B2 = cemb.shape[0]
        img = img.clone()  # never write into the caller's x_T
        n = img.numel()
        prev = torch.empty_like(img)
        denoised = torch.empty_like(img)
        for i, p in enumerate(plan):
            ts = torch.full((B2,), p["t"], device=dev, dtype=torch.long)
            xin = torch.cat([img, img], 0) if cfg else img
            eps = dit.forward_cached(xin, ts, cemb, w_emb)
            coeffs = (C.c_float * 6)(*p["coeffs"])
            nz = ptr(noise[i]) if p["add_noise"] else None
            eu, ec = (eps[:batch_size], eps[batch_size:]) if cfg else (None, eps)
            if mask is not None:
                check(lib().alcm_lcm_step_edit(ptr(img), ptr(ec), ptr(eu), float(unconditional_guidance_scale), nz,
                                               coeffs, ptr(z0), ptr(mask), ptr(prev), ptr(denoised), *img.shape,
                                               stream_handle()), "lcm_step_edit")
            elif cfg:
                check(lib().alcm_lcm_step_cfg(ptr(img), ptr(ec), ptr(eu), float(unconditional_guidance_scale), nz,
                                              coeffs, ptr(prev), ptr(denoised), n, stream_handle()), "lcm_step_cfg")
            else:
                check(lib().alcm_lcm_step(ptr(img), ptr(eps), nz, coeffs, ptr(prev), ptr(denoised), n,
                                          stream_handle()), "lcm_step")
            img, prev = prev, img
        return denoised, img

    JOINT_DIT_ROWS = 64  # sample_joint: rows per DiT call, the largest batch the suite runs the DiT at

    @torch.no_grad()
    def sample_joint(self, S, conditioning, length: int, starts: Sequence[int], window: int, overlap: int,
                     seeds: Optional[Sequence[int]] = None, x_T: Optional[torch.Tensor] = None,
                     noise: Optional[torch.Tensor] = None, guidance_scale=5., original_inference_steps=50,
                     unconditional_conditioning: Optional[torch.Tensor] = None,
                     unconditional_guidance_scale: float = 1.0,
                     clips_per_call: int = 1, ring: bool = False, init=None, mask=None, strength: float = 1.0,
                     init_noise: Optional[torch.Tensor] = None, posterior_noise: Optional[torch.Tensor] = None,
                     sample_posterior: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Joint long-form sampling: S LCM steps on one latent of ``length`` frames covered by the K windows of
        ``window`` frames at ``starts`` (``AudioLCMPipeline.long_windows``).  Every step runs the DiT on all windows of
        all clips (K * B rows, row k * B + b; [uc; c] doubled with guidance as in ``sample``) and then one
        alcm_lcm_step_joint: where windows overlap their denoised estimates are averaged with
        ``windows.window_weights(starts, window, length, overlap, ring)``, the long latent is re-noised once, and the windows
        of the next step are cut from it.  No window waits for another one, and every window sees both neighbours.

        The DiT is called on the windows of ``clips_per_call`` clips at a time (at most ``JOINT_DIT_ROWS`` rows).  The
        DiT picks its kernels by the rows of the call, so one and the same row differs by some 5e-6 between calls of
        different sizes; with the default of one clip per call (K rows, S calls per clip) a call's rows do not depend
        on the batch and neither does a clip, bit for bit.  A larger value makes fewer, larger calls (S at
        ``clips_per_call`` >= B) and gives that up: a clip then agrees across batch sizes to about 3e-6.  With one window
        the call is ``sample``'s own, the whole batch.

        RNG: with ``seeds`` ``recipe.prompt_noise(seeds, S, C, length)``, per prompt at the clip's whole length (a clip
        does not depend on its batch; with one window these are ``sample``'s draws and the result is ``sample``'s bit
        for bit); ``x_T`` / ``noise`` replace the respective draw; without seeds the global device RNG.

        ``ring``: the ``length`` frames are a ring (seamless loops): window k covers the frames (starts[k] + j) mod
        length, the plan is the ring's table (at least two windows: ``AudioLCMPipeline.loop_windows``) and the
        step alcm_lcm_step_ring.  Each window is still an ordinary DiT call on ``window`` frames, and everything else is
        as above; rotating ``x_T`` and ``noise`` by a multiple of the windows' spacing rotates the result.

        ``init``: joint denoising from a known latent, ``sample_edit`` on the long latent.  ``init`` (the encoder's
        ``DiagonalGaussianDistribution`` or a scaled (B, C, length) latent), ``mask`` (B, length) or None, ``strength``,
        ``init_noise``, ``posterior_noise`` and ``sample_posterior`` mean what they mean there: the plan is
        ``schedule.sample_plan(S, ..., strength=strength)``, the draws with ``seeds`` are ``recipe.edit_noise(seeds, S',
        C, length)`` at the clip's whole length, the start is one alcm_latent_init on the long latent, and every step is
        one alcm_lcm_step_joint_edit, which blends the joint estimate with z0 per frame: frames of mask 0 keep z0
        exactly.  Without a mask every frame is regenerated and the step is the open entry, as ``sample_edit``'s is the
        plain one.  With one window the result is ``sample_edit``'s bit for bit.  ``x_T`` is not used, and a ring
        cannot take ``init`` here (ValueError): joint editing on a ring is ``sample_ring_edit``.
        Returns (denoised, last sample) like ``sample``."""
        if ring and init is not None:
            raise ValueError("a ring cannot take `init` here: joint editing on a ring is `sample_ring_edit`")
        return self._sample_windows(S, conditioning, length, starts, window, overlap, seeds, x_T, noise, guidance_scale,
                                    original_inference_steps, unconditional_conditioning,
                                    unconditional_guidance_scale, clips_per_call, ring, init, mask, strength,
                                    init_noise, posterior_noise, sample_posterior)

    @torch.no_grad()
    def sample_ring_edit(self, S, conditioning, init, starts: Sequence[int], window: int, overlap: int, mask=None,
                         strength: float = 1.0, seeds: Optional[Sequence[int]] = None,
                         noise: Optional[torch.Tensor] = None, init_noise: Optional[torch.Tensor] = None,
                         posterior_noise: Optional[torch.Tensor] = None, sample_posterior: bool = True,
                         guidance_scale=5., original_inference_steps=50,
                         unconditional_conditioning: Optional[torch.Tensor] = None,
                         unconditional_guidance_scale: float = 1.0,
                         clips_per_call: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """Joint denoising from a known latent on a ring: ``sample_joint(init=...)`` with the frames of ``init`` (the
        encoder's ``DiagonalGaussianDistribution`` or a scaled (B, C, L) latent) closed into a ring of L frames, a loop
        made from a recording.  The plan is the ring's (``windows.loop_windows``; ``window_weights(..., ring=True)``),
        the start is ``sample_joint(init=...)``'s one alcm_latent_init on the long latent with the draws of
        ``recipe.edit_noise(seeds, S', C, L)``, the DiT calls are grouped as there, and every step is one
        alcm_lcm_step_ring_edit: the ring's weighted chain blended with z0 per frame, so frames of mask 0 keep z0
        exactly and the frames either side of the wrap are denoised as the neighbours they are.  Without a mask every
        frame is regenerated and the step is alcm_lcm_step_ring, as the line uses its open entry; at strength 1 that
        is ``sample_joint(ring=True)`` from ``init_noise``.  Returns (denoised, last sample) like ``sample``."""
        if isinstance(init, DiagonalGaussianDistribution):
            L = init.parameters.shape[2]
        else:
            L = init.shape[-1]
        return self._sample_windows(S, conditioning, L, starts, window, overlap, seeds, None, noise, guidance_scale,
                                    original_inference_steps, unconditional_conditioning,
                                    unconditional_guidance_scale, clips_per_call, True, init, mask, strength,
                                    init_noise, posterior_noise, sample_posterior)

    def _sample_windows(self, S, conditioning, length, starts, window, overlap, seeds, x_T, noise, guidance_scale,
                        original_inference_steps, unconditional_conditioning, unconditional_guidance_scale,
                        clips_per_call, ring, init, mask, strength, init_noise, posterior_noise, sample_posterior):
        """The body of ``sample_joint`` and ``sample_ring_edit``: a line or a ring, from noise or from ``init``."""
        self.make_schedule(verbose=False)
        dev = torch.device("cuda")
        dit: ConcatDiT2MLP = self.model.unet.diffusion_model
        W, L, K = int(window), int(length), len(starts)
        if W > dit.cfg.max_latent_len:
            raise ValueError(f"window {W} exceeds the DiT's {dit.cfg.max_latent_len} frames")
        wn = window_weights_device(starts, W, L, overlap, ring, dev)  # validates the plan
        cond = self._cond(conditioning)
        B, Cc = cond.shape[0], dit.cfg.in_channels
        z0 = None
        if init is not None:
            if x_T is not None:
                raise ValueError("`x_T` is not used with `init`: pass `init_noise`")
            plan, img, z0, noise, mask = self._edit_start(S, init, mask, strength, seeds, noise, init_noise,
                                                          posterior_noise, sample_posterior,
                                                          original_inference_steps, one_window=False)
            if mask is None:
                z0 = None       # every frame is regenerated: the open step
        else:
            plan = schedule.sample_plan(S, original_inference_steps)
            img, noise = self._noise_start(plan, seeds, x_T, noise, B, Cc, L)
        if tuple(img.shape) != (B, Cc, L):
            raise ValueError(f"x_T must be (B, C, length) = {(B, Cc, L)}, got {tuple(img.shape)}")

        cfg, cemb, w_emb = self._context(cond, guidance_scale, unconditional_conditioning, unconditional_guidance_scale)
        # DiT calls: the windows of g clips each, rows k * g + j ([uc; c] halves with guidance), so that the rows of a
        # call, and with them the DiT's kernel plan, do not depend on the batch; one window is ``sample``'s own call
        per_clip = K * (2 if cfg else 1)
        g = B if K == 1 else max(1, min(int(clips_per_call), B, self.JOINT_DIT_ROWS // per_clip))
        groups = []
        for b0 in range(0, B, g):
            b1 = min(b0 + g, B)
            ce = cemb[b0:b1].repeat(K, 1, 1)
            if cfg:
                ce = torch.cat([ce, cemb[B + b0:B + b1].repeat(K, 1, 1)], 0)
            groups.append((b0, b1, ce, w_emb[:1].repeat(ce.shape[0], 1)))
        KB = K * B
        xw = torch.empty((KB, Cc, W), device=dev, dtype=torch.float32)
        ec = torch.empty_like(xw)
        eu = torch.empty_like(xw) if cfg else None
        kernels.lcm_step_joint(img, None, None, plan[0]["coeffs"], starts, wn, xw=xw, ring=ring)   # the first windows
        if ring and z0 is not None:
            step = functools.partial(kernels.lcm_step_ring_edit, z0=z0, mask=mask)
        else:
            step = functools.partial(kernels.lcm_step_joint, ring=ring, z0=z0, mask=mask)
        outs = [torch.empty_like(img), torch.empty_like(img)]   # never write into the caller's x_T
        denoised = torch.empty_like(img)
        for i, p in enumerate(plan):
            for b0, b1, ce, we in groups:
                n = K * (b1 - b0)
                xg = xw.view(K, B, Cc, W)[:, b0:b1].reshape(n, Cc, W)
                ts = torch.full((ce.shape[0],), p["t"], device=dev, dtype=torch.long)
                whole = b1 - b0 == B
                if not cfg:
                    e = dit.forward_cached(xg, ts, ce, we, out=ec if whole else None)
                else:
                    e = dit.forward_cached(torch.cat([xg, xg], 0), ts, ce, we)
                    eu.view(K, B, Cc, W)[:, b0:b1] = e[:n].view(K, b1 - b0, Cc, W)
                if cfg or not whole:
                    ec.view(K, B, Cc, W)[:, b0:b1] = e[-n:].view(K, b1 - b0, Cc, W)
            last = i + 1 == len(plan)
            step(img, ec, noise[i] if p["add_noise"] else None, p["coeffs"], starts, wn, eps_uncond=eu,
                 cfg_scale=float(unconditional_guidance_scale), prev=outs[i % 2], den=denoised,
                 xw=None if last else xw, want_xw=not last)
            img = outs[i % 2]
        return denoised, img

    @torch.no_grad()
    def sample_edit(self, S, conditioning, init, mask=None, strength: float = 1.0,
                    seeds: Optional[Sequence[int]] = None, noise: Optional[torch.Tensor] = None,
                    init_noise: Optional[torch.Tensor] = None, posterior_noise: Optional[torch.Tensor] = None,
                    sample_posterior: bool = True, guidance_scale=5., original_inference_steps=50,
                    unconditional_conditioning: Optional[torch.Tensor] = None,
                    unconditional_guidance_scale: float = 1.0, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """Audio-conditioned sampling: S LCM steps from a known latent instead of pure noise.

        ``init``: the encoder's ``DiagonalGaussianDistribution`` (z0 = scale_factor * its sample with the noise e0, or
        its mode with ``sample_posterior=False``) or a (B, C, T) latent z0 already scaled.  ``mask`` (B, T) in [0, 1]
        or None (= 1 everywhere): frames of mask 1 are regenerated, frames of mask 0 keep z0 exactly (every step
        blends its denoised estimate with z0 per frame).  ``strength`` in (0, 1] places the first timestep t0
        (``schedule.sample_plan``).  Kept frames start from sqrt(ac[t0]) z0 + sqrt(1 - ac[t0]) n0; regenerated frames
        too when strength < 1 (the input is a hint), and from pure n0 at strength 1 (the reference's x_T).

        RNG: with ``seeds``, per prompt n0, the step noise and e0 from ``recipe.edit_noise``; ``init_noise``, ``noise``
        and ``posterior_noise`` replace the respective draw; without seeds the global device RNG.
        Returns (denoised, last sample) like ``sample``."""
        plan, img, z0, noise, mask = self._edit_start(S, init, mask, strength, seeds, noise, init_noise,
                                                      posterior_noise, sample_posterior, original_inference_steps)
        return self._run(plan, img, noise, self._cond(conditioning), img.shape[0], guidance_scale, unconditional_conditioning,
                         unconditional_guidance_scale, z0=z0 if mask is not None else None, mask=mask)

    def _edit_start(self, S, init, mask, strength, seeds, noise, init_noise, posterior_noise, sample_posterior,
                    original_inference_steps, one_window: bool = True):
        """The start of ``sample_edit`` and of ``sample_joint(init=...)``: (plan, x at plan[0]'s noise level, z0, the
        step noise, the mask on the device or None) from their arguments, with one alcm_latent_init on the whole
        latent.  ``one_window``: the latent must fit the DiT."""
        self.make_schedule(verbose=False)
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"`strength` must be in (0, 1], got {strength}")
        dev = torch.device("cuda")
        post = init if isinstance(init, DiagonalGaussianDistribution) else None
        if post is not None:
            moments = post.parameters.to(dev).float().contiguous()
            B, Cc, T = moments.shape[0], moments.shape[1] // 2, moments.shape[2]
            z_in = None
        else:
            z_in = init.to(dev).float().contiguous()
            if z_in.dim() != 3:
                raise ValueError("audio latents are (B, C, T)")
            B, Cc, T = z_in.shape
            moments = None
        dit: ConcatDiT2MLP = self.model.unet.diffusion_model
        if one_window and T > dit.cfg.max_latent_len:
            raise ValueError(f"latent length {T} exceeds the DiT's {dit.cfg.max_latent_len} frames")
        if mask is not None:
            mask = torch.as_tensor(mask, dtype=torch.float32)
            if mask.dim() == 0:
                mask = mask.expand(B, T)
            if tuple(mask.shape) != (B, T):
                raise ValueError(f"mask must be (B, T) = {(B, T)}, got {tuple(mask.shape)}")
            mask = mask.to(dev).contiguous()
        plan = schedule.sample_plan(S, original_inference_steps, strength=strength)
        n_noise = self._set_plan(plan)
        e0 = posterior_noise if post is not None and sample_posterior else None
        draw_e0 = post is not None and sample_posterior and posterior_noise is None
        if seeds is not None:
            n0_h, noise_h, e0_h = recipe.edit_noise(seeds, len(plan), Cc, T)
            n0 = _h2d(n0_h, dev) if init_noise is None else init_noise
            noise = _h2d(noise_h, dev) if noise is None else noise
            if draw_e0:
                e0 = _h2d(e0_h, dev)
        else:
            n0 = torch.randn((B, Cc, T), device=dev) if init_noise is None else init_noise
            if noise is None and n_noise:
                noise = torch.randn((n_noise, B, Cc, T), device=dev)
            if draw_e0:
                e0 = torch.randn((B, Cc, T), device=dev)
        n0 = n0.to(dev).float().contiguous()
        noise = noise.to(dev).float().contiguous() if noise is not None else None
        e0 = e0.to(dev).float().contiguous() if e0 is not None else None
        keep = tuple(plan[0]["coeffs"][:2])  # sqrt(ac[t0]), sqrt(1 - ac[t0])
        regen = keep if strength < 1.0 else (0.0, 1.0)
        z0 = torch.empty((B, Cc, T), device=dev, dtype=torch.float32)
        img = torch.empty_like(z0)
        sk = regen if mask is None else keep  # no mask: every frame is regenerated
        check(lib().alcm_latent_init(ptr(moments), ptr(z_in), ptr(e0), float(self.model.scale_factor), ptr(n0),
                                     ptr(mask), sk[0], sk[1], regen[0], regen[1], ptr(z0), ptr(img), B, Cc, T,
                                     stream_handle()), "latent_init")
        return plan, img, z0, noise, mask
