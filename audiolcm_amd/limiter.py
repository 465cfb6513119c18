"""The look-ahead peak limiter's host plan: look-ahead and release in samples, and the kernel's tiling (host).

No reference counterpart: the reference hands the vocoder's waveform to ``soundfile.write`` as it is.  Under a binding
ceiling a static gain scales the whole clip down and ends below the loudness target; the limiter turns down only what
passes the ceiling.  Per clip, with the pre-gain g, the linear ceiling c, the look-ahead La in samples and the release
coefficient a = exp(-1 / (release_s * rate)):
  u[n] = fl32(x[n] g);  e[n] = |u[n]|, or the larger of it and the oversampled copy's samples n os .. n os + os - 1;
  r[n] = c / e[n] where e[n] > c, else 1 (1 outside the clip);
  hold:    m[j] = min r[j .. j + La]
  attack:  s[n] = mean m[n - La .. n]         (<= r[n]: a linear ramp of La samples that arrives exactly at the peak)
  release: y[n] = min(s[n], a y[n-1] + (1 - a) s[n]),  y[-1] = 1
  out[n] = copysign(min(|fl32(u[n] fl32(y[n]))|, c), u[n])
with m, s and y in float64.  The kernel (``alcm_limiter`` in ``csrc/alcm_limiter.hip``) runs the release in parallel
over time: its steps y -> min(C, A y + D) are closed under composition, so a thread composes the CHUNK maps of its
samples, a workgroup scans its LANES chunk maps and the spans' maps are folded in rising order.

The defaults, 5 ms of look-ahead and 100 ms of release, are choices and not measurements: there are no trained weights
here to listen to.  ``release_ms`` must be positive: a release of 0 would be a = 0 (the gain follows the attack curve
with no memory), which ``alcm_limiter`` accepts as ``release_coef = 0`` but which is no release time, so ``plan``
refuses it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

CHUNK = 8          # samples one thread runs (alcm_limiter.hip: kLmChunk)
LANES = 256        # chunks per workgroup (kLmLanes); a workgroup owns a span of CHUNK * LANES samples
SPAN = CHUNK * LANES
SUM_CHUNK = 12     # hold values one thread sums in the attack's prefix sum (kLmSumChunk)
MAX_LOOKAHEAD = 1024   # samples: 5 ms at 192 kHz (kLmMaxLa); the halo a workgroup holds either side of its span

DEFAULT_LOOKAHEAD_MS, DEFAULT_RELEASE_MS = 5.0, 100.0
DEFAULT_PASSES = 3


@dataclass(frozen=True)
class LimiterPlan:
    rate: int
    n: int
    lookahead: int        # La in samples, round(lookahead_ms * rate / 1000)
    release_coef: float   # a = exp(-1000 / (release_ms * rate))


def check_times(lookahead_ms: float, release_ms: float) -> None:
    """ValueError for a look-ahead that is negative or not finite, or a release that is not a finite positive time."""
    if not (0.0 <= float(lookahead_ms) < math.inf):     # refuses NaN too
        raise ValueError(f"limiter_lookahead_ms (--limiter-lookahead-ms) must be a finite time of at least 0 ms, got "
                         f"{lookahead_ms!r}")
    if not (0.0 < float(release_ms) < math.inf):
        raise ValueError(f"limiter_release_ms (--limiter-release-ms) must be a finite time above 0 ms, got "
                         f"{release_ms!r}")


def plan(rate: int, n: int, lookahead_ms: float = DEFAULT_LOOKAHEAD_MS,
         release_ms: float = DEFAULT_RELEASE_MS) -> LimiterPlan:
    """The limiter of a clip of ``n`` samples at ``rate``; ValueError for a negative look-ahead, one over
    MAX_LOOKAHEAD samples at ``rate``, or a release of 0 or less."""
    rate, n = int(rate), int(n)
    if rate < 1:
        raise ValueError(f"sample rate must be positive, got {rate}")
    if n < 0:
        raise ValueError(f"sample count must not be negative, got {n}")
    check_times(lookahead_ms, release_ms)
    lookahead = int(round(float(lookahead_ms) * rate / 1000.0))
    if lookahead > MAX_LOOKAHEAD:
        raise ValueError(f"limiter_lookahead_ms (--limiter-lookahead-ms) {lookahead_ms!r} is {lookahead} samples at "
                         f"{rate} Hz: the limiter looks at most {MAX_LOOKAHEAD} samples ahead "
                         f"({1000.0 * MAX_LOOKAHEAD / rate:.3g} ms)")
    coef = math.exp(-1000.0 / (float(release_ms) * rate))
    if not coef < 1.0:
        raise ValueError(f"limiter_release_ms (--limiter-release-ms) {release_ms!r} at {rate} Hz never releases: its "
                         f"coefficient rounds to 1")
    return LimiterPlan(rate, n, lookahead, coef)
