"""The host plan of windowed denoising: where the windows of a long, looped or edited clip lie and the weights their
overlaps are averaged with.  Pure functions of lengths and masks (numpy only): the sampler and the pipeline call them,
and the host tests reach them without a model."""
from __future__ import annotations

import functools
from typing import Optional

import numpy as np

JOINT_MAX_WINDOWS = 32  # alcm_lcm_step_joint: the window starts travel in the kernel's arguments


def edit_windows(union, window: int, overlap: Optional[int] = None):
    """(window starts, window length W) of ``edit_long`` for a clip of L = len(union) latent frames: ``union[t]`` is
    true where any clip of the batch regenerates frame t.  W = min(window, L); ``overlap`` defaults to W // 2.  Each
    window starts ``overlap`` frames before the first frame still to do (clamped to the clip) and clears its W frames; a
    span longer than a window is continued by the next one, which sees the frames already produced as known context."""
    todo = [bool(v) for v in union]
    L = len(todo)
    W = min(window, L)
    overlap = W // 2 if overlap is None else overlap
    if not 0 < overlap < W:
        raise ValueError("need 0 < overlap < window")
    starts = []
    while any(todo):
        s = min(max(todo.index(True) - overlap, 0), L - W)
        starts.append(s)
        todo[s:s + W] = [False] * W
    return starts, W


def paste_regions(union, halo: int):
    """The latent-frame ranges [a, b) ``edit_long(keep_original=True)`` decodes: every maximal run [lo, hi) of
    regenerated frames widened by ``halo`` frames either side, clamped to the clip; overlapping or touching ranges are
    merged."""
    todo = [bool(v) for v in union]
    L = len(todo)
    regions, t = [], 0
    while t < L:
        if not todo[t]:
            t += 1
            continue
        hi = t
        while hi < L and todo[hi]:
            hi += 1
        a, b = max(t - halo, 0), min(hi + halo, L)
        if regions and a <= regions[-1][1]:
            regions[-1] = (regions[-1][0], b)
        else:
            regions.append((a, b))
        t = hi
    return regions


def long_windows(latent_len: int, window: int, overlap: Optional[int] = None):
    """([(start, known)], window length) of ``generate_long``: window k covers frames start .. start + window, of
    which the first ``known`` are already generated.  The stride is window - overlap (``overlap`` defaults to
    window // 2); the last window is shifted back to end at latent_len when the stride does not divide; a clip no
    longer than one window is that one window."""
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


def loop_windows(latent_len: int, window: int, overlap: Optional[int] = None):
    """(window starts, window length W, overlap) of ``generate_loop``: the plan of a ring of L = ``latent_len``
    frames.  W = min(window, L); ``overlap`` defaults to W // 2, 0 < overlap < W.  K = max(2, ceil(L / (W - overlap)))
    windows start at floor(k * L / K): every gap between cyclic neighbours is at most W - overlap, so they share at
    least ``overlap`` frames.  One window cannot close a ring, so K is never 1: a ring of one window's length is covered
    by two windows with different cut points.  When L and W are multiples of 4 the starts are rounded down to
    multiples of 4 (the step kernel's 16-byte path), provided they stay strictly ascending and no cyclic gap exceeds
    W - overlap.  ValueError for more than 32 windows."""
    L = int(latent_len)
    W = min(int(window), L)
    overlap = W // 2 if overlap is None else int(overlap)
    if not 0 < overlap < W:
        raise ValueError("need 0 < overlap < window")
    stride = W - overlap
    K = max(2, -(-L // stride))
    if K > JOINT_MAX_WINDOWS:
        raise ValueError(f"{K} windows of {W} frames for a ring of {L}: at most {JOINT_MAX_WINDOWS}")
    starts = [k * L // K for k in range(K)]
    if L % 4 == 0 and W % 4 == 0:
        r = [s - s % 4 for s in starts]
        gaps = [b - a for a, b in zip(r, r[1:] + [L])]
        if min(gaps) > 0 and max(gaps) <= stride:
            starts = r
    return starts, W, overlap


def check_region_windows(a: int, b: int, n_windows: int, W: int) -> None:
    """ValueError when the region [a, b) of a joint edit needs more windows than one step kernel takes."""
    if n_windows > JOINT_MAX_WINDOWS:
        raise ValueError(f"the region of frames {a} .. {b} needs {n_windows} windows of {W} frames: at most "
                         f"{JOINT_MAX_WINDOWS} are denoised jointly")


def joint_edit_regions(union, window: int, overlap: Optional[int] = None):
    """The host plan of ``edit_long(joint=True)`` for a clip of L = len(union) latent frames, ``union[t]`` true where
    any clip of the batch regenerates frame t: a list of (a, b, starts, W).  Every maximal run of regenerated frames
    is widened by ``overlap`` frames of known context either side and clamped to the clip, and touching or overlapping
    ranges are merged (``paste_regions(union, overlap)``); region [a, b) of R = b - a frames is denoised jointly on
    ``long_windows(R, window, overlap)``'s plan: K windows of W = min(window, R) frames at ``starts``, relative to a.
    ``overlap`` defaults to min(window, L) // 2.  ValueError for a region of more than ``JOINT_MAX_WINDOWS``
    windows."""
    L = len(union)
    overlap = min(window, L) // 2 if overlap is None else overlap
    if not 0 < overlap < window:
        raise ValueError("need 0 < overlap < window")
    plan = []
    for a, b in paste_regions(union, overlap):
        spans, W = long_windows(b - a, window, overlap)
        check_region_windows(a, b, len(spans), W)
        plan.append((a, b, [s for s, _ in spans], W))
    return plan


def _ring_runs(union, widen: int):
    """The maximal runs of true frames of the circular ``union``, each widened by ``widen`` frames either side, with
    touching or overlapping runs merged round the ring: a list of (a, n), the frames (a + j) mod L for j < n, in
    ascending a; or None when they cover the whole ring."""
    todo = [bool(v) for v in union]
    L = len(todo)
    if not any(todo):
        return []
    if all(todo):
        return None
    p = todo.index(False)       # no run crosses a kept frame: the ring is walked from p + 1 to p + L, unwrapped
    runs, t = [], p + 1
    while t < p + L:
        if not todo[t % L]:
            t += 1
            continue
        hi = t
        while todo[hi % L]:
            hi += 1
        a, b = t - widen, hi + widen
        if runs and a <= runs[-1][1]:
            runs[-1][1] = b
        else:
            runs.append([a, b])
        t = hi
    while len(runs) > 1 and runs[-1][1] >= runs[0][0] + L:      # the last run reaches the first across the wrap
        runs[-1][1] = max(runs[-1][1], runs[0][1] + L)
        runs.pop(0)
    if sum(b - a for a, b in runs) >= L:
        return None
    return sorted((a % L, b - a) for a, b in runs)


def ring_edit_regions(union, window: int, overlap: Optional[int] = None):
    """The host plan of ``edit_loop`` for a ring of L = len(union) latent frames, ``union[t]`` true where any clip of
    the batch regenerates frame t.  The maximal runs of regenerated frames are found circularly (a run may cross the
    wrap), widened by ``overlap`` frames of known context either side and merged where they touch or overlap, also
    across the wrap.  If what is left covers the whole ring the plan is one entry ("ring", starts, W, overlap) =
    ("ring", *loop_windows(L, window, overlap)): the ring is denoised as a ring.  Otherwise every region is
    ("line", a, R, starts, W): the frames (a + j) mod L, j < R, gathered into a line that is denoised jointly on
    ``long_windows(R, window, overlap)``'s plan, in ascending a.  ``overlap`` defaults to min(window, L) // 2.  An
    empty union gives [].  ValueError for a region of more than ``JOINT_MAX_WINDOWS`` windows."""
    L = len(union)
    overlap = min(window, L) // 2 if overlap is None else overlap
    if not 0 < overlap < window:
        raise ValueError("need 0 < overlap < window")
    runs = _ring_runs(union, overlap)
    if runs is None:
        return [("ring", *loop_windows(L, window, overlap))]
    plan = []
    for a, R in runs:
        spans, W = long_windows(R, window, overlap)
        check_region_windows(a, a + R, len(spans), W)
        plan.append(("line", a, R, [s for s, _ in spans], W))
    return plan


def ring_paste_regions(union, halo: int):
    """The latent-frame regions ``edit_loop(keep_original=True)`` decodes: the circular runs of regenerated frames
    widened by ``halo`` frames either side and merged round the ring, a list of (a, n), the frames (a + j) mod L for
    j < n, in ascending a; [("ring",)] when they cover the whole ring."""
    runs = _ring_runs(union, halo)
    return [("ring",)] if runs is None else runs


def ring_paste_cut(union, fade_frames: int) -> int:
    """Where ``edit_loop(keep_original=True)`` cuts the ring open when its paste regions cover it: the frame a at which
    the decoded ring starts and, L frames on, ends.  The two ends are two renderings of neighbouring frames, so the cut
    belongs where the paste does not use the decode: a is the middle of the longest circular run of kept frames of
    ``union`` (the first such run among equals), provided both sides of the cut are then at least ``fade_frames`` kept
    frames away from a regenerated one (n // 2 >= fade_frames for a run of n, and n >= 2), so that g = 0 either side of
    it.  Without such a run (every frame regenerated, or only short gaps) a = 0: the cut is the wrap itself, the
    period's own first and last sample."""
    todo = [bool(v) for v in union]
    L = len(todo)
    if all(todo) or not any(todo):
        return 0
    p = todo.index(True)
    best, t = (0, 0), p + 1
    while t < p + L:
        if todo[t % L]:
            t += 1
            continue
        hi = t
        while not todo[hi % L]:
            hi += 1
        if hi - t > best[1]:
            best = (t, hi - t)
        t = hi
    s, n = best
    return (s + n // 2) % L if n >= 2 and n // 2 >= fade_frames else 0


def seam_mask(L: int, seam_frames: int) -> np.ndarray:
    """The mask of ``loop_from``: a bool array of L frames, true on the m = ``seam_frames`` frames either side of the
    wrap, [L - m, L) and [0, m).  ValueError unless 1 <= m and 2 * m <= L."""
    L, m = int(L), int(seam_frames)
    if m < 1 or 2 * m > L:
        raise ValueError(f"the seam takes 1 <= seam_frames and 2 * seam_frames <= the ring's {L} frames, got {m}")
    mask = np.zeros(L, dtype=bool)
    mask[:m] = mask[L - m:] = True
    return mask


@functools.lru_cache(maxsize=None)
def _window_weights(starts: tuple, W: int, L: int, overlap: int, ring: bool) -> np.ndarray:
    K, least = len(starts), 2 if ring else 1
    if not least <= K <= JOINT_MAX_WINDOWS:
        raise ValueError(f"{'a ring' if ring else 'a clip'} needs {least} to {JOINT_MAX_WINDOWS} windows, got {K}")
    if not 1 <= W <= L or overlap < 0:
        raise ValueError(f"need 1 <= window <= the clip's {L} frames and overlap >= 0")
    if starts[0] != 0:
        raise ValueError("the first window must start at frame 0")
    for a, b in zip(starts, starts[1:]):
        if b <= a:
            raise ValueError(f"window starts must ascend strictly, got {list(starts)}")
        if b > a + W:
            raise ValueError(f"frames {a + W} .. {b - 1} are under no window")
    end = starts[-1] + W
    if ring and not starts[-1] < L <= end:
        raise ValueError(f"the last window covers frames {starts[-1]} .. {end - 1}: it must start inside the ring's {L} "
                         "frames and reach its end")
    if not ring and end != L:
        raise ValueError(f"the last window must end at the clip's {L} frames, it ends at {end}")
    j = np.arange(W, dtype=np.float64)
    w = np.minimum(1.0, (np.minimum(j, W - 1 - j) + 1.0) / (overlap + 1.0))
    frames = [(s + np.arange(W)) % L for s in starts]     # on a line no window wraps: s + W <= L
    total = np.zeros(L, dtype=np.float64)
    for f in frames:
        total[f] += w     # W <= L: a window covers a frame at most once
    wn = np.stack([w / total[f] for f in frames], 0).astype(np.float32)
    wn.setflags(write=False)
    return wn


def window_weights(starts, W: int, L: int, overlap: int, ring: bool = False) -> np.ndarray:
    """The host plan of joint denoising (``LCMSampler.sample_joint``; alcm_lcm_step_joint, _ring and _joint_edit): the
    normalised weights wn (K, W), fp32, of K windows of W frames at the frames ``starts`` of a clip of L frames.  On a
    line window k covers the frames starts[k] + j, on a ring (starts[k] + j) mod L, j = 0 .. W - 1.  The raw profile of
    a window is a linear ramp over ``overlap`` frames at each end, w[j] = min(1, (min(j, W - 1 - j) + 1) /
    (overlap + 1)), strictly positive; wn[k][j] = w[j] over the sum of w over the windows that cover that frame,
    evaluated in float64 and rounded to fp32 once: per frame the covering weights sum to 1, and a frame under one window
    has exactly 1.0.  A line plan has the same table in both forms.

    ValueError unless 1 <= W <= L, ``overlap`` >= 0, the starts begin at 0, ascend strictly, leave no frame uncovered
    (starts[k] <= starts[k - 1] + W) and are at most 32; and on a line there is at least one window and the last ends
    at L (starts[-1] + W == L), on a ring there are at least two, the last starts below L and closes the gap across
    the wrap (starts[-1] < L <= starts[-1] + W).  Built once per argument tuple; the array is read-only."""
    return _window_weights(tuple(int(s) for s in starts), int(W), int(L), int(overlap), bool(ring))
