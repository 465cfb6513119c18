"""The band-limited rational resampler's filter: plan and tap table (host, float64, cached per rate pair).

No reference counterpart: the reference writes ``soundfile.write(..., opt.sample_rate)`` without resampling.  The
filter is a Kaiser-windowed sinc evaluated per output phase; the kernel (``alcm_resample``) only applies the table.

For ``rate_in -> rate_out`` with g = gcd: up = rate_out / g, down = rate_in / g,
  fcn   = rolloff * min(rate_in, rate_out) / (2 * rate_in)   cutoff in cycles per input sample
  Hw    = zeros / (2 * fcn)                                  half-width in input samples
  first = -floor(Hw),  ntaps = 2 * floor(Hw) + 2
  h(t)  = 2 fcn sinc(2 fcn t) I0(beta sqrt(1 - (t / Hw)^2)) / I0(beta) for |t| <= Hw, else 0
  taps[r][k] = fp32(h(k + first - r / up)),  r in [0, up), k in [0, ntaps)
  y[n]  = sum_k taps[(n * down) mod up][k] * x[floor(n * down / up) + first + k],  x = 0 outside [0, N_in)
  N_out = ceil(N_in * up / down)
The filter is zero-phase: output n sits at input position n * down / up.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

ZEROS, BETA, ROLLOFF = 32, 9.0, 0.92


@dataclass(frozen=True)
class ResamplePlan:
    rate_in: int
    rate_out: int
    up: int
    down: int
    fcn: float
    half_width: float
    first: int
    ntaps: int
    taps: np.ndarray  # (up, ntaps) float32, read-only

    def out_len(self, n_in: int) -> int:
        return -(-n_in * self.up // self.down)


def kaiser_sinc(t: np.ndarray, fcn: float, half_width: float, beta: float = BETA) -> np.ndarray:
    """h(t) in float64."""
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) <= half_width
    u = np.where(inside, t / half_width, 0.0)
    h = 2.0 * fcn * np.sinc(2.0 * fcn * t) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta)
    return np.where(inside, h, 0.0)


@lru_cache(maxsize=None)
def plan(rate_in: int, rate_out: int, zeros: int = ZEROS, beta: float = BETA, rolloff: float = ROLLOFF) -> ResamplePlan:
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError(f"sample rates must be positive, got {rate_in} -> {rate_out}")
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    fcn = rolloff * min(rate_in, rate_out) / (2.0 * rate_in)
    hw = zeros / (2.0 * fcn)
    first = -math.floor(hw)
    ntaps = 2 * math.floor(hw) + 2
    k = np.arange(ntaps, dtype=np.float64)[None, :]
    r = np.arange(up, dtype=np.float64)[:, None]
    taps = kaiser_sinc(k + first - r / up, fcn, hw, beta).astype(np.float32)
    taps.setflags(write=False)
    return ResamplePlan(rate_in, rate_out, up, down, fcn, hw, first, ntaps, taps)


def frame_samples_at(rate: int, base_rate: int = 16000, base_frame: int = 512):
    """Samples of one latent frame at ``rate`` (512 at 16 kHz), or None when that is not a whole number."""
    num = base_frame * int(rate)
    return num // base_rate if num % base_rate == 0 else None
