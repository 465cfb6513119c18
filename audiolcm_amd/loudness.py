"""The loudness meter's host plan: K-weighting coefficients, block geometry and the kernel's tables (host, float64).

No reference counterpart: the reference hands the vocoder's waveform to ``soundfile.write`` as it is.  The measure is
ITU-R BS.1770-4 / EBU R 128 integrated loudness of a mono clip: K-weighting (a high shelf and a high pass, two biquads
in cascade), mean squares over 400 ms blocks every 100 ms, an absolute gate at -70 LUFS and a relative gate 10 LU
under the mean of what the absolute gate kept.  The kernels (``alcm_loudness_hops`` / ``alcm_loudness_gain`` in
``csrc/alcm_loudness.hip``) apply what is planned here.

The biquads come from their analog prototypes by the bilinear transform with prewarping, K = tan(pi f0 / rate):
  shelf:     Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2,
             b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0,  a1 = 2 (K^2 - 1) / a0,
             a2 = (1 - K/Q + K^2) / a0
  high pass: b = [1, -2, 1], a1, a2 as above with its own f0 and Q
with the constants that reproduce the standard's 48 kHz table (to 9e-16).

The cascade in transposed direct form II has the state s = (s1, s2, t1, t2):
  y1 = b0 x + s1,  s1' = b1 x - a1 y1 + s2,  s2' = b2 x - a2 y1          (shelf)
  y  = y1 + t1,    t1' = -2 y1 - c1 y + t2,  t2' = y1 - c2 y             (high pass)
so that s' = M s + u x with a constant 4 x 4 matrix M: the state after a chunk of L samples is M^L s + z, z the state
the chunk reaches from zero.  ``tables`` gives the kernel the powers of M it scans these maps with.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Tuple

import numpy as np

SHELF_F0, SHELF_GAIN_DB, SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
SHELF_VB_EXP = 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773

CHUNK = 32        # samples one thread runs (alcm_loudness.hip: kLdChunk)
LANES = 256       # chunks per workgroup (kLdLanes); a workgroup owns a span of CHUNK * LANES samples
SPAN = CHUNK * LANES
SCAN_STEPS = 8    # log2(LANES)
COEF_DOUBLES = 10 + 16 * (SCAN_STEPS + 1)

ABS_GATE, REL_GATE, OFFSET = -70.0, -10.0, -0.691
DEFAULT_CEILING_DBFS = -1.0


def k_weighting(rate: int) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """The two biquads at ``rate`` as (b0, b1, b2, a1, a2) in float64: (high shelf, high pass)."""
    rate = int(rate)
    if rate < 1:
        raise ValueError(f"sample rate must be positive, got {rate}")
    K = math.tan(math.pi * SHELF_F0 / rate)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = ((Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0)
    K = math.tan(math.pi * HIGHPASS_F0 / rate)
    a0 = 1.0 + K / HIGHPASS_Q + K * K
    highpass = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HIGHPASS_Q + K * K) / a0)
    return shelf, highpass


def transition(rate: int) -> np.ndarray:
    """M (4, 4) float64: the cascade's state after one sample of zero input, s' = M s."""
    (b0, b1, b2, a1, a2), (c0, c1, c2, d1, d2) = k_weighting(rate)
    return np.array([[-a1, 1.0, 0.0, 0.0],
                     [-a2, 0.0, 0.0, 0.0],
                     [c1 - d1 * c0, 0.0, -d1, 1.0],
                     [c2 - d2 * c0, 0.0, -d2, 0.0]], dtype=np.float64)


@lru_cache(maxsize=None)
def tables(rate: int) -> np.ndarray:
    """The ``coef`` array of ``alcm_loudness_hops`` (COEF_DOUBLES float64, read-only): the shelf's and the high pass's
    (b0, b1, b2, a1, a2), then M^(CHUNK * 2^j) for j = 0 .. SCAN_STEPS - 1 and M^SPAN, each 4 x 4 row-major.  The powers
    are repeated squarings of M^CHUNK in float64."""
    shelf, highpass = k_weighting(rate)
    P = np.linalg.matrix_power(transition(rate), CHUNK)
    mats = []
    for _ in range(SCAN_STEPS + 1):
        mats.append(P)
        P = P @ P
    out = np.concatenate([np.array(shelf + highpass, dtype=np.float64)] + [m.reshape(-1) for m in mats])
    assert out.size == COEF_DOUBLES
    out.setflags(write=False)
    return out


@dataclass(frozen=True)
class LoudnessPlan:
    rate: int
    n: int
    hop: int           # 100 ms in samples, rounded to nearest
    block: int         # 400 ms = 4 hops
    nh: int            # whole hops in n
    nb: int            # gating blocks
    coef: np.ndarray   # ``tables(rate)``


def hop_of(rate: int) -> int:
    return (int(rate) + 5) // 10


def plan(rate: int, n: int) -> LoudnessPlan:
    """The geometry of a clip of ``n`` samples at ``rate``; ValueError under one block (400 ms), where the integrated
    loudness is undefined."""
    rate, n = int(rate), int(n)
    if rate < 10:
        raise ValueError(f"sample rate {rate}: a 100 ms hop needs at least 10 Hz")
    hop = hop_of(rate)
    block = 4 * hop
    if n < block:
        raise ValueError(f"{n} samples at {rate} Hz: integrated loudness needs one 400 ms block ({block} samples)")
    return LoudnessPlan(rate, n, hop, block, n // hop, (n - block) // hop + 1, tables(rate))
