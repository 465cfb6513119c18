"""Windowed float64 parity: the yardstick of tests/test_gpu_voc_windows.py, test_gpu_vae_windows.py and their host twin.

A whole-clip relative L2 cannot see a fault confined to a few positions (a clip end, a tile seam, a batch boundary):
window_errors cuts every clip into windows of W positions and measures each against the clip's own level.

The bar comes from the reference alone.  The oracle (oracle/alcm_oracle.py) runs twice in float64: as it is, and with
the matrix-core operand roundings of the precision policy emulated by patching conv1d / conv_transpose1d
(groups == 1 only: the depthwise Activation1d FIRs stay fp32 on the device) and, for the VAE, torch.bmm, as the oracle
module sees them.  E = the largest window error of the emulated run against the exact one; every window of the device
output must stay at or below MARGIN * E.  The emulation leaves out the fp32 accumulation order, the fp16 FIR inputs of
the matrix-core Activation1d and the fp16 conv1 hand-off (+2e-5 on 6e-4), and two realisations of
rounding noise differ window to window (emulated max / median window ratio 1.1-2.4): hence 4, fixed.
"""
import contextlib
import functools
import os
import re
import types

import numpy as np
import torch
import torch.nn.functional as F

from audiolcm_amd import _hip, recipe
from audiolcm_amd import kernels as K
from oracle import alcm_oracle as O

MARGIN = 4.0
GAINS = (0.5, 1.0, 2.0)
NCU = 256  # compute units of an MI355X: what the case tables were planned for


# ---------------------------------------------------------------------------------------------- windows
def window_errors(y, ref, W):
    """y, ref (B, C, T): per clip, rms(y - ref over a window, all channels) / rms(ref over the whole clip) in float64
    for the consecutive windows of W positions of the time axis plus one window over the last W positions (a clip
    shorter than W: the one window that covers it).  -> list of B float64 arrays."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    assert y.shape == ref.shape and y.ndim == 3 and W > 0, (y.shape, ref.shape, W)
    T = y.shape[-1]
    if T <= W:
        spans = [(0, T)]
    else:
        spans = [(t, min(t + W, T)) for t in range(0, T, W)] + [(T - W, T)]
    out = []
    for b in range(y.shape[0]):
        level = np.sqrt(np.mean(ref[b] ** 2))
        d2 = (y[b] - ref[b]) ** 2
        out.append(np.array([np.sqrt(np.mean(d2[:, a:e])) for a, e in spans]) / level)
    return out


def clip_l2(y, ref):
    """Whole-clip relative L2 per clip (float64)."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    return [float(np.linalg.norm(y[b] - ref[b]) / np.linalg.norm(ref[b])) for b in range(y.shape[0])]


def check_windows(tag, got, exact, emulated, W, l2_bar):
    """The assertion (every window of every clip, and the whole-clip bar); prints the measured row first.
    -> (E, largest device window, ratio, largest whole-clip L2) over the clips."""
    we, wg, l2 = window_errors(emulated, exact, W), window_errors(got, exact, W), clip_l2(got, exact)
    rows = [(float(e.max()), float(g.max()), int(g.argmax()), len(g)) for e, g in zip(we, wg)]
    worst = max(range(len(rows)), key=lambda b: rows[b][1] / rows[b][0])
    E, G = rows[worst][0], rows[worst][1]
    print(f"{tag}: E {E:.2e} gpu {G:.2e} ratio {G / E:.2f} l2 {max(l2):.2e}")
    for b, ((e, g, at, n), l) in enumerate(zip(rows, l2)):
        assert e > 0 and np.isfinite(wg[b]).all(), (tag, b)
        assert g <= MARGIN * e, f"{tag} clip {b}: window {at} of {n} (W = {W}) at {g:.3e} > {MARGIN} x E = {e:.3e}"
        assert l < l2_bar, f"{tag} clip {b}: whole-clip rel-L2 {l:.3e} >= {l2_bar}"
    return E, G, G / E, max(l2)


# ---------------------------------------------------------------------------------------------- operand roundings
def _hi_lo(v, dt):
    h = v.to(dt).to(v.dtype)
    return h, (v - h).to(dt).to(v.dtype)


def product(op, x, w, bias, prec):
    """op(x, w, bias), bilinear in (x, w), as a matrix core computes it at `prec` (None: as it is)."""
    if prec is None:
        return op(x, w, bias)
    if prec == "bf16x3":  # (hi + lo) x (hi + lo) without lo x lo
        xh, xl = _hi_lo(x, torch.bfloat16)
        wh, wl = _hi_lo(w, torch.bfloat16)
        return op(xh, wh, bias) + op(xh, wl, None) + op(xl, wh, None)
    x16 = x.to(torch.float16).to(x.dtype)
    if prec == "f16":
        return op(x16, w.to(torch.float16).to(w.dtype), bias)
    if prec == "f16w2":  # fp16 activations x fp16 hi + lo weights
        wh, wl = _hi_lo(w, torch.float16)
        return op(x16, wh, bias) + op(x16, wl, None)
    raise ValueError(prec)


@contextlib.contextmanager
def roundings(choose):
    """Within the block the oracle's conv1d / conv_transpose1d (groups == 1) and torch.bmm round their operands as
    choose(kind, w) says: kind in ("conv", "convt", "bmm"), w the weight (None for bmm) -> a `product` precision."""
    def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        op = lambda a, c, bias: F.conv1d(a, c, bias, stride, padding, dilation, groups)
        return product(op, x, w, b, choose("conv", w) if groups == 1 else None)

    def convt(x, w, b=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
        op = lambda a, c, bias: F.conv_transpose1d(a, c, bias, stride, padding, output_padding, groups, dilation)
        return product(op, x, w, b, choose("convt", w) if groups == 1 else None)

    def bmm(a, b):
        return product(lambda p, q, _: torch.bmm(p, q), a, b, None, choose("bmm", None))

    fns = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("_")})
    fns.conv1d, fns.conv_transpose1d = conv1d, convt
    tns = types.SimpleNamespace(**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})
    tns.bmm = bmm
    old = O.F, O.torch
    O.F, O.torch = fns, tns
    try:
        yield
    finally:
        O.F, O.torch = old


PREC_NAME = {_hip.PREC_SPLIT: "bf16x3", _hip.PREC_F16: "f16", _hip.PREC_F16W2: "f16w2"}


# ---------------------------------------------------------------------------------------------- vocoder
def voc_config(c0=1536, rates=(4, 4, 2, 2, 2, 2), kernels=(8, 8, 4, 4, 4, 4)):
    return recipe.BigVGANConfig(upsample_initial_channel=c0, upsample_rates=tuple(rates),
                                upsample_kernel_sizes=tuple(kernels))


# name -> (config, input scale: seeded randn * scale * GAINS keeps every reference sample inside |ref| <= 0.95)
VOC_CONFIGS = {
    "tail": (voc_config(96, (2, 2), (4, 4)), 0.2),
    "mid": (voc_config(384, (2, 2), (4, 4)), 0.2),
    "head": (voc_config(1536, (4,), (8,)), 0.2),
    "full": (voc_config(), 1.0),
}


def voc_layer_precisions(cfg, policy, B, M):
    """Per layer of the vocoder forward, the operand rounding the executor applies (alcm_models.cpp bigvgan_forward,
    DESIGN.md §3): conv_pre bf16x3 under both policies; an upsampler on operand planes at its stage's precision, else
    bf16x3 (ups2 and the phase convs); the AMPBlock convs at the stage plan's precision; conv_post exact fp32 in the
    fused 24-channel head, else bf16x3."""
    plans = K.voc_plan(cfg, policy, True, B, M, NCU)
    n = len(cfg.upsample_rates)
    return dict(pre="bf16x3",
                ups=[PREC_NAME[p["prec"]] if p["ups"] == "planes" else "bf16x3" for p in plans],
                amp=[PREC_NAME[p["prec"]] for p in plans],
                post=None if cfg.stage_channels(n - 1) == 24 else "bf16x3")


def voc_oracle(W, mel, cfg, precs=None):
    """oracle.bigvgan_forward of cfg in the dtype of W / mel; precs (voc_layer_precisions) rounds the operands of
    each layer, None runs the oracle untouched."""
    kw = dict(upsample_rates=cfg.upsample_rates, upsample_kernel_sizes=cfg.upsample_kernel_sizes,
              resblock_kernel_sizes=cfg.resblock_kernel_sizes, resblock_dilation_sizes=cfg.resblock_dilation_sizes)
    with torch.no_grad():
        if precs is None:
            return O.bigvgan_forward(W, mel, **kw)
        state = dict(where="pre", ups=0)
        nk = len(cfg.resblock_kernel_sizes)

        def choose(kind, w):
            if kind == "convt":
                state["ups"] += 1
                state["where"] = "post"  # what follows the last stage
                return precs["ups"][state["ups"] - 1]
            if state["where"] in ("pre", "post"):
                return precs[state["where"]]
            return precs["amp"][state["where"]]

        real_amp = O.amp_block1

        def amp(Wd, p, x, k, d):
            state["where"] = int(p.split(".")[1]) // nk
            try:
                return real_amp(Wd, p, x, k, d)
            finally:
                state["where"] = "post"

        O.amp_block1 = amp
        try:
            with roundings(choose):
                return O.bigvgan_forward(W, mel, **kw)
        finally:
            O.amp_block1 = real_amp


def voc_input(cfg, scale, B, M, seed=0):
    """(B, num_mels, M) fp32: the clips are different draws at gains x0.5, x1, x2 (cycling)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + M)
    mel = torch.randn((B, cfg.num_mels, M), generator=g) * scale
    return mel * torch.tensor([GAINS[b % 3] for b in range(B)]).view(B, 1, 1)


_states = {}


def voc_state64(name):
    if name not in _states:
        _states[name] = {k: v.double() for k, v in recipe.bigvgan_state(0, VOC_CONFIGS[name][0]).items()}
    return _states[name]


def _threads():
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


@functools.lru_cache(maxsize=None)
def voc_exact(name, B, M):
    """-> (mel fp32, exact float64 waveform (B, 1, T)); computed once per process, read-only."""
    _threads()
    cfg, scale = VOC_CONFIGS[name]
    mel = voc_input(cfg, scale, B, M)
    out = voc_oracle(voc_state64(name), mel.double(), cfg).numpy()
    out.setflags(write=False)
    return mel, out


@functools.lru_cache(maxsize=None)
def _voc_emulated(name, B, M, key):
    _threads()
    cfg, _ = VOC_CONFIGS[name]
    precs = dict(pre=key[0], ups=list(key[1]), amp=list(key[2]), post=key[3])
    out = voc_oracle(voc_state64(name), voc_exact(name, B, M)[0].double(), cfg, precs).numpy()
    out.setflags(write=False)
    return out


def voc_references(name, policy, B, M):
    """-> (mel fp32, exact float64 waveform, emulated float64 waveform) as (B, 1, T) arrays."""
    mel, exact = voc_exact(name, B, M)
    p = voc_layer_precisions(VOC_CONFIGS[name][0], policy, B, M)
    return mel, exact, _voc_emulated(name, B, M, (p["pre"], tuple(p["ups"]), tuple(p["amp"]), p["post"]))


# ---------------------------------------------------------------------------------------------- VAE decoder
_K3 = re.compile(r"\.(block_\d|block\.\d+)\.conv[12]\.weight$|\.upsample\.conv\.weight$")


def vae_chooser(W, policy):
    """The decoder's roundings (alcm_models.cpp vae_decode): bf16x3 everywhere under the split policy; under mixed the
    ResnetBlock1D and Upsample1D convs on fp16 planes, everything else (post_quant_conv, conv_in, the 1x1 convs, both
    attention products, conv_out) bf16x3."""
    f16 = {id(v) for k, v in W.items() if _K3.search(k)} if policy == "mixed" else set()
    return lambda kind, w: "f16" if id(w) in f16 else "bf16x3"


def vae_input(B, T, seed=0):
    g = torch.Generator().manual_seed(2000 * seed + 31 * B + T)
    z = torch.randn((B, 20, T), generator=g)
    return z * torch.tensor([GAINS[b % 3] for b in range(B)]).view(B, 1, 1)


@functools.lru_cache(maxsize=None)
def vae_exact(B, T):
    _threads()
    if "vae" not in _states:
        _states["vae"] = {k: v.double() for k, v in recipe.vae_state(0).items()}
    z = vae_input(B, T)
    with torch.no_grad():
        out = O.vae_decode(_states["vae"], z.double()).numpy()
    out.setflags(write=False)
    return z, out


@functools.lru_cache(maxsize=None)
def vae_references(policy, B, T):
    """-> (z fp32, exact float64 mel, emulated float64 mel) as (B, 80, 2 T) arrays."""
    z, exact = vae_exact(B, T)
    W = _states["vae"]
    with torch.no_grad(), roundings(vae_chooser(W, policy)):
        emu = O.vae_decode(W, z.double()).numpy()
    emu.setflags(write=False)
    return z, exact, emu


# ---------------------------------------------------------------------------------------------- the case tables
# (shared by the device tests and their host twin, tests/test_voc_windows_host.py)
def _voc_cases():
    c = []
    for pol in ("split", "mixed"):
        c += [("tail", pol, B, M) for B in (1, 3) for M in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
        c += [("mid", pol, B, M) for B in (1, 3) for M in (1, 5, 31, 33, 64, 129)]
        c += [("head", pol, 1, 5), ("head", pol, 2, 129)]
        c += [("full", pol, 1, 1), ("full", pol, 2, 5), ("full", pol, 1, 33)]
    c.append(("mid", "mixed", 4, 256))  # the fp16 conv1 hand-off of the wide stage (h16) is on from 1024 rows
    return c


VOC_CASES = _voc_cases()
VOC_W = 32  # waveform samples per window
# ups2's persistent walk (ALCM_UPS2_GRID): one to three workgroups over every tile of the batch, across the clip
# boundaries, with a ragged last tile per clip (129 = 128 + 1 input rows at stage 0)
UPS2_GRID_CASES = [("tail", "split", B, M, cap) for B, M in ((3, 129), (2, 257)) for cap in (1, 2, 3)]
# the plane hand-off between wide stages (writes_next / planes_from_prev): planned by shape only from about 2000 mel
# frames (30 s of float64 oracle per run), and at any size with ALCM_WCONV3=1
HANDOFF_CASES = [("mid", "mixed", 1, 5), ("mid", "mixed", 3, 129), ("full", "mixed", 2, 5)]

VAE_W = 4  # mel frames per window (x 80 bins)
VAE_CASES = ([("split", B, T) for B in (1, 2) for T in (1, 2, 3, 31, 32, 33, 129)]
             # either side of the 1024-row switch to the wide-layer kernel (3 x 341 = 1023, 4 x 256 = 1024)
             + [(pol, B, T) for pol in ("split", "mixed") for B, T in ((3, 341), (4, 256))])


def case_id(c):
    return "-".join(str(v) for v in c)
