"""The audio-input half of the front end: reading ``--init-audio`` / ``init_audio`` and planning the request.

``plan_edit`` is the one place that decides what an audio-conditioned request is (a variation, an inpainting of the
cropped clip or, jointly denoised, of the whole one, a keep-original inpainting at 16 kHz or at the recording's own
rate, an extension of the recording, or a loop made from it) and the one place that refuses one; ``AudioLCMPipeline.run_edit`` turns its ``EditPlan`` into audio.  The command line and ``AudioLCMEditInfer`` are
callers of the two.  Importing this module does not touch the GPU (``kernels`` is imported where a file has to be
resampled).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .resample import frame_samples_at
from .wavio import read_audio, read_wav

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


def frame_samples_of(rate: int) -> int:
    """The samples of one latent frame at ``rate``; ValueError for a rate at which that is not a whole number."""
    F = frame_samples_at(rate, SAMPLE_RATE, FRAME_SAMPLES)
    if F is None:
        raise ValueError(f"sample rate {rate}: keep_original pastes whole latent frames of {FRAME_SAMPLES} * rate / "
                         f"{SAMPLE_RATE} samples, so it takes multiples of 125 Hz: 8000, 16000, 32000, 48000, 96000")
    return F


def loop_multiple(rate: int) -> int:
    """The latent frames a loop's period and halo are a multiple of at ``rate``, so that both are whole numbers of
    output samples: a frame is 512 * rate / 16000 = 4 * rate / 125 samples, hence 125 / gcd(125, rate) frames (1 at
    16, 32, 48 and 96 kHz, 5 at 44.1 and 22.05 kHz)."""
    return 125 // math.gcd(125, int(rate))


def loop_frames(duration_s: float, out_sample_rate: Optional[int] = None) -> int:
    """The period of a loop of ``duration_s`` seconds in latent frames: the smallest L >= ceil(duration_s * 16000 /
    512) (at least 2: a ring has two windows) that is a multiple of ``loop_multiple(out_sample_rate or 16000)``.  The
    period is never cropped to ``duration_s``: a crop would cut the seam."""
    if not duration_s > 0:
        raise ValueError("duration_s must be positive")
    m = loop_multiple(SAMPLE_RATE if out_sample_rate is None else out_sample_rate)
    need = max(2, math.ceil(duration_s * SAMPLE_RATE / FRAME_SAMPLES))
    return -(-need // m) * m


def check_native_keep_original(path: str, rate: int, channels: int, out_sample_rate: Optional[int]) -> int:
    """What a keep-original edit of a file needs; returns the samples F of one latent frame at the file's rate."""
    if channels != 1:
        raise ValueError(f"{path}: {channels} channels; keep_original keeps the input's samples bit for bit, which a "
                         "downmix cannot: pass a mono file")
    F = frame_samples_of(rate)
    if out_sample_rate is not None and out_sample_rate != rate:
        raise ValueError(f"{path}: keep_original writes the input's own sample rate {rate}, not out_sample_rate "
                         f"{out_sample_rate}")
    return F


def _read_mono(path: str, resample: bool, own_rate: bool = False,
               out_sample_rate: Optional[int] = None) -> Tuple[np.ndarray, int, int]:
    """One read of ``path`` -> (mono float32 samples, their rate, the samples of one latent frame at that rate).
    Without ``resample`` only 16 kHz mono PCM16 is read (``read_wav``); with it any rate, 1 to 8 channels and PCM16 /
    PCM24 / float32 (``read_audio``).  The samples are downmixed and resampled to 16 kHz on the GPU, unless
    ``own_rate``: then they are the file's own, which ``check_native_keep_original`` has to allow."""
    if resample:
        x, rate = read_audio(path)
    else:
        x, rate = read_wav(path)
        x = x[:, None]
        if rate != SAMPLE_RATE:
            raise ValueError(f"{path}: sample rate {rate}, need {SAMPLE_RATE} (resampling is not done here; pass "
                             "resample=True, --resample on the command line, to resample on the GPU)")
    F = check_native_keep_original(path, rate, x.shape[1], out_sample_rate) if own_rate else FRAME_SAMPLES
    if x.shape[0] == 0:
        raise ValueError(f"{path}: no samples")
    if own_rate:
        return np.ascontiguousarray(x[:, 0]), rate, F
    return _to_16k_mono(x, rate), SAMPLE_RATE, F


def _to_16k_mono(x: np.ndarray, rate: int) -> np.ndarray:
    """(N, channels) at ``rate`` -> (N16,) at 16 kHz: the channel mean and the resampling in one ``kernels.resample``."""
    if rate == SAMPLE_RATE and x.shape[1] == 1:
        return np.ascontiguousarray(x[:, 0])
    from . import kernels
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()[None]
    return kernels.resample(xd, rate, SAMPLE_RATE, channels=x.shape[1])[0].cpu().numpy()


def _pad_to_frames(x: np.ndarray, frame_samples: int = FRAME_SAMPLES) -> np.ndarray:
    return np.pad(x, (0, -x.size % frame_samples))


def load_init_audio(path: str, max_frames: Optional[int] = None, resample: bool = False) -> np.ndarray:
    """16 kHz mono PCM16 WAV -> float32 samples, zero-padded up to a whole number of latent frames (512 samples) and
    cropped to ``max_frames`` of them (the DiT's length limit) when given.  Another sample rate raises ValueError,
    unless ``resample``: then the file is read by ``read_audio`` (any rate, 1 to 8 channels, PCM16 / PCM24 / float32)
    and downmixed and resampled to 16 kHz on the GPU first."""
    x = load_init_audio_whole(path, resample)[0]
    return x if max_frames is None else x[:max_frames * FRAME_SAMPLES]


def load_init_audio_whole(path: str, resample: bool = False) -> Tuple[np.ndarray, int]:
    """``load_init_audio`` without a crop, and the sample count before padding (a keep-original edit writes that
    many)."""
    x = _read_mono(path, resample)[0]
    return _pad_to_frames(x), x.size


def load_native_audio(path: str, out_sample_rate: Optional[int] = None) -> Tuple[np.ndarray, int, int, int]:
    """The input of a keep-original edit at the recording's own rate: (mono float32 samples zero-padded to whole latent
    frames, the file's sample count, its rate, the samples F of one latent frame at that rate).  ValueError for more
    than one channel, a rate at which F is not whole, or an ``out_sample_rate`` that is not the file's."""
    x, rate, F = _read_mono(path, True, True, out_sample_rate)
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


@dataclass(frozen=True)
class Level:
    """What ``check_level`` decided about the level of the output; ``finish_output`` applies it."""
    loudness: Optional[float]   # target integrated loudness in LUFS, None: none
    peak_dbfs: Optional[float]  # peak ceiling in dBFS, None: none
    true_peak: bool             # the ceiling acts on the 4x oversampled peak estimate
    limiter: bool = False       # the ceiling is kept by the look-ahead limiter, not by a smaller static gain
    lookahead_ms: float = 5.0   # the limiter's look-ahead
    release_ms: float = 100.0   # the limiter's release time


def check_level(loudness: Optional[float] = None, peak_dbfs: Optional[float] = None,
                true_peak: bool = False, limiter: bool = False, limiter_lookahead_ms: float = 5.0,
                limiter_release_ms: float = 100.0) -> Optional[Level]:
    """Validates the level options; None when none is given (the output is then written as it is).  A target is
    within -70 .. 0 LUFS, a ceiling is at most 0 dBFS, ``true_peak`` needs one of them, and a target alone implies a
    ceiling of -1 dBFS, so that a normalised file never clips.  ``limiter`` needs one of them too: the ceiling is then
    kept by the look-ahead limiter (``audiolcm_amd/limiter.py``), whose times must be a look-ahead of at least 0 ms
    and a release above 0 ms; whether the look-ahead fits the kernel's 1024 samples is known at the rate that is
    written (``finish_output``)."""
    from .loudness import ABS_GATE, DEFAULT_CEILING_DBFS
    if loudness is None and peak_dbfs is None:
        if true_peak:
            raise ValueError("true_peak says how the peak is measured: give it with loudness or peak_dbfs")
        if limiter:
            raise ValueError("limiter (--limiter) keeps a ceiling: give it with loudness or peak_dbfs (--loudness, "
                             "--peak)")
        return None
    if limiter:
        from .limiter import check_times
        check_times(limiter_lookahead_ms, limiter_release_ms)
    if loudness is not None and not (ABS_GATE <= float(loudness) <= 0.0):   # refuses NaN too
        raise ValueError(f"loudness must lie within {ABS_GATE:g} .. 0 LUFS, got {loudness!r}")
    if peak_dbfs is not None and not (-math.inf < float(peak_dbfs) <= 0.0):
        raise ValueError(f"peak_dbfs must be a finite ceiling of at most 0 dBFS, got {peak_dbfs!r}")
    return Level(None if loudness is None else float(loudness),
                 DEFAULT_CEILING_DBFS if peak_dbfs is None else float(peak_dbfs), bool(true_peak), bool(limiter),
                 float(limiter_lookahead_ms), float(limiter_release_ms))


def finish_output(wav16: torch.Tensor, out_sample_rate: Optional[int], level: Optional[Level] = None,
                  n_out: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """The output stage: (B, L) at 16 kHz on the device -> (what is written, its rate).  ``to_out_rate``, then a crop
    to ``n_out`` samples when given, then with ``level`` the normalisation of exactly those samples at that rate
    (``kernels.normalize_loudness``), with ``level.limiter`` through the limiter planned for them
    (``limiter.plan``).  ``level`` None launches nothing more than ``to_out_rate``."""
    wav, rate = to_out_rate(wav16, out_sample_rate)
    if n_out is not None:
        wav = wav[:, :n_out]
    if level is not None:
        from . import kernels
        lim = None
        if level.limiter:
            from . import limiter as _lm
            lim = _lm.plan(rate, wav.shape[1], level.lookahead_ms, level.release_ms)
        wav = kernels.normalize_loudness(wav, rate, level.loudness, level.peak_dbfs, level.true_peak,
                                         limiter=lim)["wav"]
    return wav, rate


# ---------------------------------------------------------------------------- the request plan
@dataclass(frozen=True, eq=False)
class EditPlan:
    """What ``plan_edit`` decided about one audio-conditioned request; ``AudioLCMPipeline.run_edit`` runs it."""
    mode: str                                           # "variation", "inpaint", "keep_original", "extend",
    #                                                     "loop_from" or "loop_vary"
    samples: np.ndarray                                 # mono float32 at `rate`, zero-padded to whole latent frames
    n_samples: int                                      # the sample count before padding
    rate: int                                           # the rate the edit runs at
    frame_samples: int                                  # the samples of one latent frame at `rate`
    spans: Optional[Tuple[Tuple[float, float], ...]]    # inpaint: the spans to regenerate, in seconds
    mask: Optional[np.ndarray]                          # keep_original: (frames,) 1 = regenerate
    fade: int                                           # `fade_ms` in samples at `rate`
    out_rate: int                                       # the rate to write into the header
    resample_out: bool                                  # the output is resampled from 16 kHz to `out_rate`
    pcm_scale: float                                    # PCM16 scale: 32768 gives kept samples back bit for bit
    native: bool                                        # keep_original with resample: the file's own rate was read,
    #                                                     so the header rate is no label on 16 kHz samples
    level: Optional[Level] = None                       # the level of the output (`check_level`), None: as generated
    joint: bool = False                                 # denoise jointly (`edit_long(joint=True)`), the whole recording
    extend_frames: int = 0                              # extend: the latent frames generated after `samples`
    n_out: int = 0                                      # extend: the samples written
    seam_frames: int = 0                                # loop_from: the frames made anew either side of the wrap
    loop_fade: int = 0                                  # loop_vary: the seam fade of the decode, in output samples
    dropped: int = 0                                    # loop_from, loop_vary: the samples trimmed at the recording's end
    fade_law: str = "linear"                            # the paste's fade law: "linear", "equal-power" or "matched"
    match_gain: bool = False                            # the paste scales each regenerated run to the recording's level


FADE_LAWS = ("linear", "equal-power", "matched")


def check_fade_law(fade_law: str, match_gain: bool, pastes: bool, why: str = "") -> None:
    """ValueError unless ``fade_law`` is one of ``FADE_LAWS`` and, where the request pastes nothing into a recording
    (``pastes`` false; ``why`` says so in the message), both options are at their defaults."""
    if fade_law not in FADE_LAWS:
        raise ValueError(f"fade_law (--fade-law) must be one of {', '.join(FADE_LAWS)}, got {fade_law!r}")
    if not pastes and (fade_law != "linear" or match_gain):
        raise ValueError("fade_law and match_gain (--fade-law, --match-gain) act where regenerated audio is pasted into "
                         "a recording: with keep_original, extend_s or loop_from (--keep-original, --extend, "
                         "--loop-from)" + why)


def ring_spans_mask(spans: Sequence[Tuple[float, float]], n_frames: int) -> np.ndarray:
    """(n_frames,) float32 mask of time spans on a loop's period of ``n_frames`` latent frames at 16 kHz: the whole
    frames inside each span, as ``keep_original_mask`` takes them.  A span whose end is not after its start goes
    across the wrap: (t0, t1) with t1 <= t0 is [t0, the period's end) and [0, t1)."""
    end = (n_frames + 1) * FRAME_SAMPLES / SAMPLE_RATE      # past the period's end: ``spans_to_mask`` clips to it
    parts = []
    for t0, t1 in spans:
        parts += [(t0, t1)] if t1 > t0 else [(t0, end), (0.0, t1)]
    return spans_to_mask(parts, n_frames, inward=True)


def plan_loop(init_audio: str, seam_s: float = 1.0, vary: bool = False,
              mask_spans: Optional[Sequence[Tuple[float, float]]] = None, fade_ms: float = 32.0, resample: bool = False,
              out_sample_rate: Optional[int] = None, loudness: Optional[float] = None, peak_dbfs: Optional[float] = None,
              true_peak: bool = False, loop_fade_ms: float = 32.0, limiter: bool = False, fade_law: str = "linear",
              match_gain: bool = False) -> EditPlan:
    """Reads the recording ``init_audio`` once and plans a loop made from it, or refuses with ValueError (the messages
    name the arguments and the command line's flags).  The recording is trimmed at its end to L whole latent frames,
    one period; ``dropped`` counts the samples that leaves out.  ``resample`` brings any input to 16 kHz first.

    Mode "loop_from" (``vary`` false): ``AudioLCMPipeline.loop_from``.  Only the m = ceil(``seam_s`` * 16000 / 512)
    frames either side of the wrap are made anew, and the whole frames inside ``mask_spans`` (``ring_spans_mask``: a
    span may go across the wrap) besides; ``fade_ms`` is the paste's fade.  The file holds L * 512 samples at 16 kHz,
    the recording's own outside the fades, so a level and an output rate are refused.  Needs L >= 2 and 2 m <= L.

    Mode "loop_vary": ``AudioLCMPipeline.edit_loop`` without a mask, the whole ring regenerated from the recording as a
    hint.  ``out_sample_rate``, the level and ``loop_fade_ms`` apply as for a loop from text, and L is trimmed further
    to a multiple of ``loop_multiple(out_sample_rate)``.  ``limiter`` is refused in both modes: its gain varies in
    time and starts from 1 at the first sample, which would break the period that a static gain keeps.
    ``fade_law`` and ``match_gain`` are the paste's (``check_fade_law``): refused with ``vary``, which pastes nothing."""
    check_fade_law(fade_law, match_gain, not vary, "; loop_vary (--loop-vary) decodes the whole ring and pastes nothing")
    if limiter:
        raise ValueError("limiter (--limiter) does not combine with loop_from (--loop-from), with or without loop_vary "
                         "(--loop-vary): a gain that varies in time and starts from 1 at the first sample would break "
                         "the period")
    level = check_level(loudness, peak_dbfs, true_peak)
    out_sample_rate = check_out_rate(out_sample_rate)
    if not vary and (level is not None or out_sample_rate is not None):
        raise ValueError("loop_from (--loop-from) keeps the recording's samples bit for bit at 16 kHz: loudness, "
                         "peak_dbfs, true_peak and out_sample_rate (--loudness, --peak, --true-peak, "
                         "--out-sample-rate) are used with loop_vary (--loop-vary)")
    if vary and mask_spans:
        raise ValueError("loop_vary (--loop-vary) regenerates the whole ring: it does not take mask_spans (--mask-spans)")
    if loop_fade_ms < 0:
        raise ValueError("loop_fade_ms (--loop-fade-ms) must not be negative")
    x, rate, F = _read_mono(init_audio, resample)
    out_rate = out_sample_rate or SAMPLE_RATE
    L = x.size // F
    if vary:
        L -= L % loop_multiple(out_rate)
    if L < 2:
        raise ValueError(f"{init_audio}: loop_from (--loop-from) needs a recording of at least two latent frames "
                         f"({2 * F} samples at {SAMPLE_RATE} Hz"
                         + (f", a multiple of {loop_multiple(out_rate)} frames at {out_rate} Hz" if vary else "")
                         + f"), got {x.size} samples")
    samples = np.ascontiguousarray(x[:L * F])
    if vary:
        return EditPlan(mode="loop_vary", samples=samples, n_samples=samples.size, rate=rate, frame_samples=F,
                        spans=None, mask=None, fade=0, out_rate=out_rate, resample_out=out_rate != rate,
                        pcm_scale=32767.0, native=False, level=level,
                        loop_fade=fade_samples_of(loop_fade_ms, out_rate), dropped=x.size - samples.size)
    m = math.ceil(seam_s * SAMPLE_RATE / FRAME_SAMPLES) if seam_s == seam_s else 0     # NaN: refused below
    if m < 1 or 2 * m > L:
        raise ValueError(f"loop_seam_s (--loop-seam) {seam_s!r} is {m} latent frames either side of the wrap: a loop "
                         f"from (--loop-from) a recording of {L} frames takes 1 <= frames and 2 * frames <= {L}")
    mask = ring_spans_mask(mask_spans, L) if mask_spans else None
    return EditPlan(mode="loop_from", samples=samples, n_samples=samples.size, rate=rate, frame_samples=F, spans=None,
                    mask=mask, fade=fade_samples_of(fade_ms, rate), out_rate=rate, resample_out=False,
                    pcm_scale=32768.0, native=False, seam_frames=m, dropped=x.size - samples.size, fade_law=fade_law,
                    match_gain=bool(match_gain))


def extend_counts(n_samples: int, extend_s: float) -> Tuple[int, int, int]:
    """The arithmetic of an extension of a recording of ``n_samples`` samples at 16 kHz by ``extend_s`` seconds:
    (J, the new latent frames, the samples written).  The junction is frame J = n_samples // 512: the samples of a last
    partial frame are regenerated, so nothing of a zero padding is ever kept as audio.  n_samples +
    round(extend_s * 16000) samples are written, which takes ceil of that / 512 frames in all.  ValueError for a
    recording shorter than one frame or an extension of less than one sample."""
    J = n_samples // FRAME_SAMPLES
    if J < 1:
        raise ValueError(f"the recording has {n_samples} samples at {SAMPLE_RATE} Hz: an extension needs at least one "
                         f"latent frame of {FRAME_SAMPLES} to continue")
    extra = int(round(extend_s * SAMPLE_RATE)) if extend_s == extend_s else 0   # NaN: refused below
    if extra < 1:
        raise ValueError(f"extend_s must add at least one sample, got {extend_s!r}")
    n_out = n_samples + extra
    return J, -(-n_out // FRAME_SAMPLES) - J, n_out


def plan_edit(init_audio: str, mask_spans: Optional[Sequence[Tuple[float, float]]] = None, keep_original: bool = False,
              fade_ms: float = 32.0, resample: bool = False, out_sample_rate: Optional[int] = None,
              max_frames: Optional[int] = None, loudness: Optional[float] = None, peak_dbfs: Optional[float] = None,
              true_peak: bool = False, joint: bool = False, extend_s: Optional[float] = None, loop_from: bool = False,
              loop_seam_s: float = 1.0, loop_vary: bool = False, loop_fade_ms: float = 32.0, limiter: bool = False,
              limiter_lookahead_ms: float = 5.0, limiter_release_ms: float = 100.0, fade_law: str = "linear",
              match_gain: bool = False) -> EditPlan:
    """Reads ``init_audio`` once and decides the request, or refuses it with ValueError.  No ``mask_spans``: a
    variation; with them: an inpainting of the clip (both crop to ``max_frames`` latent frames here when given;
    ``run_edit`` crops to the DiT's limit in any case); ``keep_original``: the whole frames inside the spans are
    regenerated in a clip of any length, at 16 kHz or, with ``resample``, at the recording's own rate.  ``loudness``,
    ``peak_dbfs``, ``true_peak``, ``limiter``, ``limiter_lookahead_ms``, ``limiter_release_ms``: the level of the output
    (``check_level``); refused with ``keep_original``, and the limiter wherever a level is and with every loop.
    ``joint``: the frames to regenerate are denoised jointly (``edit_long(joint=True)``); a variation or an inpainting
    is then made from the whole recording instead of a crop to the DiT's limit.  ``extend_s``: the recording is
    continued by that many seconds (``AudioLCMPipeline.extend``, ``extend_counts``) at 16 kHz; with ``resample`` any
    input is brought to 16 kHz first and the kept part is the resampled recording.  Refused with ``mask_spans`` and
    ``keep_original``, with a level (it would scale the kept samples) and with ``out_sample_rate``.
    ``loop_from``: the recording is made to loop (``plan_loop``: modes "loop_from" and, with ``loop_vary``,
    "loop_vary"; ``loop_seam_s`` and ``loop_fade_ms`` are its ``seam_s`` and ``loop_fade_ms``).  Refused with
    ``keep_original`` and ``extend_s``; ``loop_vary`` alone is refused too.
    ``fade_law`` ("linear", "equal-power", "matched") and ``match_gain``: the fade law and the gain alignment of the
    paste (``kernels.paste``); refused (``check_fade_law``) wherever nothing is pasted: without ``keep_original``,
    ``extend_s`` or ``loop_from``, and with ``loop_vary``."""
    check_fade_law(fade_law, match_gain, bool(keep_original or extend_s is not None or loop_from))
    if loop_vary and not loop_from:
        raise ValueError("loop_vary (--loop-vary) is used with loop_from (--loop-from)")
    if loop_from:
        if keep_original or extend_s is not None:
            raise ValueError("loop_from (--loop-from) does not combine with keep_original (--keep-original) or extend_s "
                             "(--extend): it keeps the recording by itself, and a continued recording does not loop")
        return plan_loop(init_audio, loop_seam_s, loop_vary, mask_spans, fade_ms, resample, out_sample_rate, loudness,
                         peak_dbfs, true_peak, loop_fade_ms, limiter, fade_law, match_gain)
    if extend_s is not None:
        if mask_spans or keep_original:
            raise ValueError("extend_s continues the recording: it does not combine with mask_spans or keep_original")
        if loudness is not None or peak_dbfs is not None or true_peak:
            raise ValueError("extend_s keeps the recording's samples bit for bit; loudness, peak_dbfs and true_peak "
                             "would scale them")
        if limiter:
            raise ValueError("extend_s (--extend) keeps the recording's samples bit for bit; limiter (--limiter) would "
                             "scale them")
        if out_sample_rate is not None:
            raise ValueError(f"extend_s writes {SAMPLE_RATE} Hz, the rate it keeps the recording at, not "
                             f"out_sample_rate {out_sample_rate}")
        x, rate, F = _read_mono(init_audio, resample)
        J, frames, n_out = extend_counts(x.size, extend_s)
        return EditPlan("extend", np.ascontiguousarray(x[:J * F]), x.size, rate, F, None, None,
                        fade_samples_of(fade_ms, rate), rate, False, 32768.0, False, None, True, frames, n_out,
                        fade_law=fade_law, match_gain=bool(match_gain))
    if keep_original and not mask_spans:
        raise ValueError("keep_original needs mask_spans: the time spans to regenerate")
    if keep_original and limiter:
        raise ValueError("keep_original (--keep-original) keeps the input's samples bit for bit outside the spans; "
                         "limiter (--limiter) would scale them")
    level = check_level(loudness, peak_dbfs, true_peak, limiter, limiter_lookahead_ms, limiter_release_ms)
    if keep_original and level is not None:
        raise ValueError("keep_original keeps the input's samples bit for bit outside the spans; loudness, peak_dbfs and "
                         "true_peak would scale them")
    out_sample_rate = check_out_rate(out_sample_rate)
    x, rate, F = _read_mono(init_audio, resample, keep_original, out_sample_rate)
    samples = _pad_to_frames(x, F)
    spans = mask = None
    if keep_original:
        mode, mask = "keep_original", keep_original_mask(mask_spans, samples.size // F)
    else:
        mode = "variation" if mask_spans is None else "inpaint"
        spans = None if mask_spans is None else tuple((float(a), float(b)) for a, b in mask_spans)
        samples = samples if max_frames is None else samples[:max_frames * F]
    out_rate = rate if keep_original else out_sample_rate or SAMPLE_RATE
    return EditPlan(mode, samples, x.size, rate, F, spans, mask, fade_samples_of(fade_ms, rate), out_rate,
                    out_rate != rate, 32768.0 if keep_original else 32767.0, keep_original and resample, level,
                    bool(joint), fade_law=fade_law, match_gain=bool(match_gain))
