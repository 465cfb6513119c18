"""Thin torch-facing wrappers over the op-level C-ABI entry points.

Each function takes CUDA (HIP) fp32 tensors, allocates its output with torch,
and enqueues one or more libaudiolcm_hip kernels on the current stream.  They
are the per-op drop-ins for the ATen ops the reference path runs
(F.conv1d / conv_transpose1d / linear / group_norm / layer_norm / softmax,
Activation1d, LCMSampler.step) and are what the op-level parity tests call.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip
from ._hip import check, lib, ptr, stream_handle

BK = 32


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _prec(split: bool, prec: Optional[int]) -> int:
    """MFMA operand precision code: explicit `prec` (_hip.PREC_*) or split -> PREC_SPLIT / PREC_BF16."""
    if prec is not None:
        assert prec in (_hip.PREC_BF16, _hip.PREC_SPLIT, _hip.PREC_F16, _hip.PREC_F16W2), prec
        return int(prec)
    return _hip.PREC_SPLIT if split else _hip.PREC_BF16


@dataclass
class PackedWeight:
    """[rows][Kpad] GEMM operand planes bf16 hi, bf16 lo, fp16 hi, fp16 lo (K index = tap*cpad + ci)."""
    data: torch.Tensor  # int16 (4, rows, kpad) on device
    rows: int
    cin: int
    cpad: int
    taps: int
    kpad: int

    @property
    def lo_off(self) -> int:
        return self.rows * self.kpad


def pack_conv_weight(w: torch.Tensor, transposed: bool = False, stride: int = 1, phase: int = 0) -> PackedWeight:
    """Pack Conv1d weight (Cout,Cin,K) — or ConvTranspose1d weight (Cin,Cout,K) for one phase."""
    assert w.is_cuda and w.dtype == torch.float32
    w = w.contiguous()
    if w.dim() == 2:
        w = w.unsqueeze(-1)
    if transposed:
        cin, cout, k = w.shape
        taps = k // stride
    else:
        cout, cin, k = w.shape
        taps = k
    cpad = _round_up(cin, 8)
    kpad = _round_up(taps * cpad, BK)
    out = torch.empty((4, cout, kpad), dtype=torch.int16, device=w.device)
    check(lib().alcm_pack_conv_weight(ptr(w), cout, cin, k, cpad, kpad, int(transposed), stride, phase, ptr(out),
                                      stream_handle()), "pack_conv_weight")
    return PackedWeight(out, cout, cin, cpad, taps, kpad)


def _act_operand(x: torch.Tensor, sb: int, st: int, sc: int, T_in: int, C_in: int, cpad: int, ksize: int, dil: int,
                 pad: int, up: int, rows_per_batch: int) -> _hip.Operand:
    o = _hip.Operand()
    o.kind = _hip.ALCM_OPND_ACT
    o.ptr = ptr(x)
    o.sb, o.st, o.sc = sb, st, sc
    o.T_in, o.C_in, o.Cpad, o.ksize, o.dil, o.pad, o.up = T_in, C_in, cpad, ksize, dil, pad, up
    o.rows_per_batch = rows_per_batch
    return o


def gemm(args: _hip.GemmArgs) -> None:
    check(lib().alcm_gemm(C.byref(args), stream_handle()), "alcm_gemm")


def conv1d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, padding: int = 0,
           dilation: int = 1, upsample: int = 1, split: bool = True, channels_last: bool = False,
           act: int = 0, residual: Optional[torch.Tensor] = None, packed: Optional[PackedWeight] = None,
           prologue: Optional[dict] = None, window: bool = True, tile_n: int = 0,
           prec: Optional[int] = None) -> torch.Tensor:
    """F.conv1d(x, w, bias, padding=padding, dilation=dilation) on the MFMA implicit GEMM.

    x is (B, Cin, T) (reference NCT layout) or, with channels_last, (B, T, Cin); the result
    uses the same layout.  ``upsample=2`` applies nearest x2 to the input first
    (F.interpolate(scale_factor=2, mode='nearest'))."""
    pw = packed or pack_conv_weight(w)
    if channels_last:
        B, T, Cin = x.shape
        sb, st, sc = x.stride()
    else:
        B, Cin, T = x.shape
        sb, sc, st = x.stride()
    K = pw.taps
    Tu = T * upsample
    Tout = Tu + 2 * padding - dilation * (K - 1)
    assert Tout > 0
    g = _hip.GemmArgs()
    g.M, g.N, g.Kpad, g.batch, g.zdiv = B * Tout, pw.rows, pw.kpad, 1, 1
    g.a = _act_operand(x, sb, st, sc, T, Cin, pw.cpad, K, dilation, padding, upsample, Tout)
    if prologue:
        g.a.pro_scale = ptr(prologue.get("scale"))
        g.a.pro_shift = ptr(prologue.get("shift"))
        g.a.pro_sb = prologue.get("sb", 0)
        g.a.pro_mean = ptr(prologue.get("mean"))
        g.a.pro_rstd = ptr(prologue.get("rstd"))
        g.a.pro_act = prologue.get("act", 0)
    b = _hip.Operand()
    b.kind, b.ptr, b.rows, b.w_lo_off = _hip.ALCM_OPND_WEIGHT, ptr(pw.data), pw.rows, pw.lo_off
    g.b = b
    g.bias = ptr(bias)
    g.acc_scale, g.out_scale, g.act = 1.0, 1.0, act
    if channels_last:
        out = torch.empty((B, Tout, pw.rows), device=x.device, dtype=torch.float32)
        g.o_sb, g.o_st, g.o_sc = Tout * pw.rows, pw.rows, 1
    else:
        out = torch.empty((B, pw.rows, Tout), device=x.device, dtype=torch.float32)
        g.o_sb, g.o_st, g.o_sc = pw.rows * Tout, 1, Tout
    if residual is not None:
        assert residual.shape == out.shape
        r = residual
        g.res = ptr(r)
        if channels_last:
            g.r_sb, g.r_st, g.r_sc = r.stride()
        else:
            g.r_sb, g.r_sc, g.r_st = r.stride()
    g.out = ptr(out)
    g.out_rows_per_batch, g.out_step, g.out_off = Tout, 1, 0
    g.prec = _prec(split, prec)
    g.disable_window = int(not window)
    g.tile_n = tile_n
    gemm(g)
    return out


def conv_transpose1d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, padding: int,
                     split: bool = True, prec: Optional[int] = None) -> torch.Tensor:
    """F.conv_transpose1d on NCT input as ``stride`` phase convolutions."""
    B, Cin, T = x.shape
    _, Cout, K = w.shape
    assert K % stride == 0 and (K - stride) == 2 * padding, "polyphase form needs k = s*Q and pad = (k-s)/2"
    Q = K // stride
    Tout = T * stride
    out = torch.empty((B, Cout, Tout), device=x.device, dtype=torch.float32)
    sb, sc, st = x.stride()
    for r in range(stride):
        o = (r - padding) % stride
        c = (o + padding - r) // stride
        pw = pack_conv_weight(w, transposed=True, stride=stride, phase=r)
        g = _hip.GemmArgs()
        g.M, g.N, g.Kpad, g.batch, g.zdiv = B * T, Cout, pw.kpad, 1, 1
        g.a = _act_operand(x, sb, st, sc, T, Cin, pw.cpad, Q, 1, Q - 1 - c, 1, T)
        b = _hip.Operand()
        b.kind, b.ptr, b.rows, b.w_lo_off = _hip.ALCM_OPND_WEIGHT, ptr(pw.data), pw.rows, pw.lo_off
        g.b = b
        g.bias = ptr(bias)
        g.acc_scale, g.out_scale = 1.0, 1.0
        g.out = ptr(out)
        g.o_sb, g.o_st, g.o_sc = Cout * Tout, 1, Tout
        g.out_rows_per_batch, g.out_step, g.out_off = T, stride, o
        g.prec = _prec(split, prec)
        gemm(g)
    return out


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, split: bool = True,
           act: int = 0, prec: Optional[int] = None) -> torch.Tensor:
    """F.linear on (..., K) rows."""
    shp = x.shape
    x2 = x.reshape(-1, shp[-1]).contiguous()
    y = conv1d(x2.unsqueeze(0), w.unsqueeze(-1), bias, split=split, channels_last=True, act=act, prec=prec)
    return y.reshape(*shp[:-1], w.shape[0])


def bmm_nt(a: torch.Tensor, b: torch.Tensor, scale: float = 1.0, split: bool = True,
           prec: Optional[int] = None) -> torch.Tensor:
    """(Z, M, K) x (Z, N, K)^T -> (Z, M, N): the Q K^T product of attention."""
    Z, M, K = a.shape
    N = b.shape[1]
    assert K % 8 == 0 and a.is_contiguous() and b.is_contiguous()
    out = torch.empty((Z, M, N), device=a.device, dtype=torch.float32)
    g = _hip.GemmArgs()
    g.M, g.N, g.Kpad, g.batch, g.zdiv = M, N, _round_up(K, BK), Z, 1
    g.a = _act_operand(a, 0, K, 1, M, K, K, 1, 1, 0, 1, M)
    g.a.zs1 = M * K
    g.b = _act_operand(b, 0, K, 1, N, K, K, 1, 1, 0, 1, N)
    g.b.zs1 = N * K
    g.acc_scale, g.out_scale = scale, 1.0
    g.out = ptr(out)
    g.o_st, g.o_sc, g.o_zs1 = N, 1, M * N
    g.out_rows_per_batch, g.out_step = M, 1
    g.prec = _prec(split, prec)
    gemm(g)
    return out


def bmm_nn(p: torch.Tensor, v: torch.Tensor, split: bool = True, prec: Optional[int] = None) -> torch.Tensor:
    """(Z, M, K) x (Z, K, N) -> (Z, M, N): the P V product (V read N-contiguous)."""
    Z, M, K = p.shape
    N = v.shape[2]
    Kp = _round_up(K, 8)
    if Kp != K:
        p = torch.nn.functional.pad(p, (0, Kp - K))
    p = p.contiguous()
    v = v.contiguous()
    out = torch.empty((Z, M, N), device=p.device, dtype=torch.float32)
    g = _hip.GemmArgs()
    g.M, g.N, g.Kpad, g.batch, g.zdiv = M, N, _round_up(Kp, BK), Z, 1
    g.a = _act_operand(p, 0, Kp, 1, M, Kp, Kp, 1, 1, 0, 1, M)
    g.a.zs1 = M * Kp
    b = _hip.Operand()
    b.kind, b.ptr, b.st, b.sc, b.T_in, b.rows, b.zs1 = _hip.ALCM_OPND_ACT_T, ptr(v), N, 1, K, N, K * N
    g.b = b
    g.acc_scale, g.out_scale = 1.0, 1.0
    g.out = ptr(out)
    g.o_st, g.o_sc, g.o_zs1 = N, 1, M * N
    g.out_rows_per_batch, g.out_step = M, 1
    g.prec = _prec(split, prec)
    gemm(g)
    return out


def group_norm_affine(x_cl: torch.Tensor, groups: int, gamma: torch.Tensor, beta: torch.Tensor,
                      eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-(b, c) scale/shift equal to nn.GroupNorm on a channels-last (B, T, C) tensor."""
    B, T, Cc = x_cl.shape
    sb, st, sc = x_cl.stride()
    assert sc == 1
    scale = torch.empty((B, Cc), device=x_cl.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    check(lib().alcm_group_norm_affine(ptr(x_cl), B, T, Cc, sb, st, groups, eps, ptr(gamma), ptr(beta), ptr(scale),
                                       ptr(shift), stream_handle()), "group_norm_affine")
    return scale, shift


def row_stats(x: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    rows = x.numel() // x.shape[-1]
    Cc = x.shape[-1]
    x = x.contiguous()
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    check(lib().alcm_row_stats(ptr(x), rows, Cc, Cc, eps, ptr(mean), ptr(rstd), stream_handle()), "row_stats")
    return mean, rstd


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    x = x.contiguous()
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    check(lib().alcm_layer_norm(ptr(x), rows, Cc, Cc, eps, ptr(gamma), ptr(beta), None, 0, ptr(y), Cc,
                                stream_handle()), "layer_norm")
    return y


def _score_rows(x: torch.Tensor, ld: Optional[int]) -> Tuple[int, int, int]:
    """(rows, n, ld) of a score tensor: contiguous (ld None), or the first n columns ``buf[:, :n]`` of a contiguous
    (rows, ld) buffer."""
    n = x.shape[-1]
    if ld is None:
        assert x.is_contiguous()    # the kernel walks rows of pitch n: a strided view was silently misread before
        return x.numel() // n, n, n
    assert x.dim() == 2 and ld >= n and x.stride(1) == 1 and (x.shape[0] == 1 or x.stride(0) == ld)
    return x.shape[0], n, int(ld)


def softmax_(x: torch.Tensor, ld: Optional[int] = None) -> torch.Tensor:
    """In-place softmax over the last dim of a contiguous tensor.  With ``ld``, x is the first n columns
    ``buf[:, :n]`` of a contiguous (rows, ld) buffer, whose columns [n, ld) are zeroed."""
    rows, n, ld = _score_rows(x, ld)
    check(lib().alcm_softmax_rows(ptr(x), rows, n, ld, stream_handle()), "softmax_rows")
    return x


def softmax_bias_(x: torch.Tensor, bias: torch.Tensor, L: int, ld: Optional[int] = None) -> torch.Tensor:
    """In-place softmax(x + bias[h, i, :n]) of T5's scores: rows (z, i) with i < L and head h = z % heads, bias
    (heads, bld, bld) fp32.  ``ld`` as in softmax_."""
    rows, n, ld = _score_rows(x, ld)
    heads, bld = bias.shape[0], bias.shape[-1]
    assert bias.dtype == torch.float32 and tuple(bias.shape) == (heads, bld, bld) and bias.is_contiguous()
    assert rows % L == 0
    check(lib().alcm_softmax_rows_bias(ptr(x), rows, n, ld, int(L), heads, ptr(bias), bld, stream_handle()),
          "softmax_rows_bias")
    return x


def snake_params(alpha: torch.Tensor, beta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """SnakeBeta logscale parameters -> (exp(alpha), 1/(exp(beta)+1e-9)) (activations.py:111-119)."""
    return torch.exp(alpha), 1.0 / (torch.exp(beta) + 0.000000001)


def activation1d(x_cl: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, up_filter: torch.Tensor,
                 down_filter: torch.Tensor) -> torch.Tensor:
    """Fused Activation1d(SnakeBeta) on a channels-last (B, T, C) tensor."""
    B, T, Cc = x_cl.shape
    x_cl = x_cl.contiguous()
    ae, ib = snake_params(alpha, beta)
    y = torch.empty_like(x_cl)
    fu = up_filter.detach().reshape(-1).float().cpu().contiguous()
    fd = down_filter.detach().reshape(-1).float().cpu().contiguous()
    check(lib().alcm_activation1d(ptr(x_cl), ptr(y), B, T, Cc, T * Cc, Cc, ptr(ae.contiguous()),
                                  ptr(ib.contiguous()), fu.data_ptr(), fd.data_ptr(), stream_handle()),
          "activation1d")
    return y


def lcm_step(x: torch.Tensor, eps: torch.Tensor, noise: Optional[torch.Tensor], coeffs) -> Tuple[torch.Tensor,
                                                                                                 torch.Tensor]:
    """LCMSampler.step (eps prediction).  coeffs = (sqrt_a, sqrt_b, c_out, c_skip, sqrt_a_prev, sqrt_b_prev)."""
    prev = torch.empty_like(x)
    den = torch.empty_like(x)
    arr = (C.c_float * 6)(*[float(c) for c in coeffs])
    check(lib().alcm_lcm_step(ptr(x), ptr(eps), ptr(noise), arr, ptr(prev), ptr(den), x.numel(), stream_handle()),
          "lcm_step")
    return prev, den


def lcm_step_edit(x: torch.Tensor, eps: torch.Tensor, noise: Optional[torch.Tensor], coeffs, z0: torch.Tensor,
                  mask: torch.Tensor, eps_uncond: Optional[torch.Tensor] = None,
                  cfg_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``lcm_step`` (with the guidance combine when ``eps_uncond`` is given) on (B, C, T) latents, blended per frame with
    the known latent ``z0``: mask (B, T) in [0, 1], 1 = take the step's value, 0 = keep z0.  Returns (prev, denoised)."""
    B, Cc, T = x.shape
    assert eps.shape == x.shape and z0.shape == x.shape and tuple(mask.shape) == (B, T)
    prev = torch.empty_like(x)
    den = torch.empty_like(x)
    arr = (C.c_float * 6)(*[float(c) for c in coeffs])
    check(lib().alcm_lcm_step_edit(ptr(x), ptr(eps), ptr(eps_uncond), float(cfg_scale), ptr(noise), arr, ptr(z0),
                                   ptr(mask), ptr(prev), ptr(den), B, Cc, T, stream_handle()), "lcm_step_edit")
    return prev, den


def lcm_step_joint(x: torch.Tensor, eps: Optional[torch.Tensor], noise: Optional[torch.Tensor], coeffs, starts,
                   wn: torch.Tensor, eps_uncond: Optional[torch.Tensor] = None, cfg_scale: float = 1.0,
                   want_prev: bool = True, want_den: bool = True, want_xw: bool = True,
                   prev: Optional[torch.Tensor] = None, den: Optional[torch.Tensor] = None,
                   xw: Optional[torch.Tensor] = None, ring: bool = False, z0: Optional[torch.Tensor] = None,
                   mask: Optional[torch.Tensor] = None):
    """``lcm_step`` on one long latent ``x`` (B, C, L) whose K overlapping windows of W frames at ``starts`` went through
    the DiT as one batch: ``eps`` (K * B, C, W), row k * B + b.  Where windows overlap their denoised estimates are
    averaged with the normalised weights ``wn`` (K, W) (``windows.window_weights``); a frame under one window is the
    plain step bit for bit (alcm_lcm_step_joint).  Returns (prev, denoised, xw): the two (B, C, L) results and prev
    gathered back into window layout (K * B, C, W), the next DiT input; a result not wanted is None, ``prev`` / ``den``
    / ``xw`` give the tensors to write.  ``eps`` None: only x itself is gathered into xw.  One launch.
    ``ring``: the L frames are a ring (alcm_lcm_step_ring): window k covers frame t at the offset (t - starts[k]) mod L
    when that is below W, and ``wn`` is the ring's table.
    ``z0`` and ``mask``: the known latent ``z0`` (B, C, L) is blended into the joint estimate per frame, as
    ``lcm_step_edit`` does for one window: ``mask`` (B, L) in [0, 1], 1 = take the joint step's value, 0 = keep z0
    (alcm_lcm_step_joint_edit).  ``eps`` is required then, and a ring cannot take them here (ValueError): the ring's edit
    form is ``lcm_step_ring_edit``."""
    if ring and z0 is not None:
        raise ValueError("a ring cannot take `z0`: joint editing exists on a line only (the ring's form is "
                         "lcm_step_ring_edit)")
    return _step_windows(x, eps, noise, coeffs, starts, wn, eps_uncond, cfg_scale, want_prev, want_den, want_xw, prev,
                         den, xw, ring, z0, mask)


def _step_windows(x, eps, noise, coeffs, starts, wn, eps_uncond=None, cfg_scale=1.0, want_prev=True, want_den=True,
                  want_xw=True, prev=None, den=None, xw=None, ring=False, z0=None, mask=None):
    """The one launch behind ``lcm_step_joint`` and ``lcm_step_ring_edit``: the entry follows from ``ring`` and from
    whether ``z0`` is given."""
    B, Cc, L = x.shape
    K, W = wn.shape
    edit = z0 is not None
    assert len(starts) == K and x.is_contiguous() and wn.is_contiguous()
    assert edit == (mask is not None) and not (edit and eps is None)
    if eps is None:
        want_prev = want_den = False
    else:
        assert tuple(eps.shape) == (K * B, Cc, W) and eps.is_contiguous()
        assert eps_uncond is None or (eps_uncond.shape == eps.shape and eps_uncond.is_contiguous())
        assert noise is None or (noise.shape == x.shape and noise.is_contiguous())
    if edit:
        assert z0.shape == x.shape and z0.is_contiguous() and tuple(mask.shape) == (B, L) and mask.is_contiguous()
    if want_prev and prev is None:
        prev = torch.empty_like(x)
    if want_den and den is None:
        den = torch.empty_like(x)
    if want_xw and xw is None:
        xw = torch.empty((K * B, Cc, W), device=x.device, dtype=torch.float32)
    arr = (C.c_float * 6)(*[float(c) for c in coeffs])
    st = (C.c_int * K)(*[int(s) for s in starts])
    name = ("lcm_step_ring_edit" if ring else "lcm_step_joint_edit") if edit else \
        "lcm_step_ring" if ring else "lcm_step_joint"
    known = (ptr(z0), ptr(mask)) if edit else ()
    check(getattr(lib(), "alcm_" + name)(ptr(x), ptr(eps), ptr(eps_uncond), float(cfg_scale), ptr(noise), arr, st, K,
                                         ptr(wn), *known, ptr(prev), ptr(den), ptr(xw), B, Cc, L, W, stream_handle()),
          name)
    return prev, den, xw


def lcm_step_joint_edit(x, eps, noise, coeffs, starts, wn, z0: torch.Tensor, mask: torch.Tensor, **kw):
    """``lcm_step_joint`` in its edit form, ``z0`` and ``mask`` required."""
    return lcm_step_joint(x, eps, noise, coeffs, starts, wn, z0=z0, mask=mask, **kw)


def lcm_step_ring_edit(x, eps, noise, coeffs, starts, wn, z0: torch.Tensor, mask: torch.Tensor, **kw):
    """``lcm_step_joint_edit`` on a ring of L frames (alcm_lcm_step_ring_edit): the ring's offsets, chain and table
    ``wn``, then the blend with ``z0`` under ``mask`` per frame; xw is prev gathered with the wrap.  ``kw`` are
    ``lcm_step_joint``'s further arguments (not ``ring``)."""
    assert z0 is not None and mask is not None and "ring" not in kw
    return _step_windows(x, eps, noise, coeffs, starts, wn, ring=True, z0=z0, mask=mask, **kw)


def latent_init(noise: Optional[torch.Tensor], keep=(1.0, 0.0), regen=(0.0, 1.0), moments: Optional[torch.Tensor] = None,
                z0: Optional[torch.Tensor] = None, e0: Optional[torch.Tensor] = None, scale: float = 1.0,
                mask: Optional[torch.Tensor] = None, want_z0: bool = True,
                want_x: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Encoder moments (B, 2C, T) (with posterior noise ``e0``, None = the mode) or a given latent ``z0`` (B, C, T) ->
    (z0, x): z0 = scale * posterior sample, x = the sampler's start sa * z0 + sb * noise with (sa, sb) = ``keep`` on
    frames of mask 0 and ``regen`` on frames of mask 1 (mask None: ``keep`` everywhere).  One launch."""
    src = moments if moments is not None else z0
    B, T = src.shape[0], src.shape[2]
    Cc = src.shape[1] // 2 if moments is not None else src.shape[1]
    z0_out = torch.empty((B, Cc, T), device=src.device, dtype=torch.float32) if want_z0 else None
    x_out = torch.empty((B, Cc, T), device=src.device, dtype=torch.float32) if want_x else None
    check(lib().alcm_latent_init(ptr(moments), ptr(z0), ptr(e0), float(scale), ptr(noise), ptr(mask), float(keep[0]),
                                 float(keep[1]), float(regen[0]), float(regen[1]), ptr(z0_out), ptr(x_out), B, Cc, T,
                                 stream_handle()), "latent_init")
    return z0_out, x_out


PASTE_MAX_FADE_FRAMES = 16  # alcm_wave_paste: the ramp reaches at most 16 frames past a regenerated frame
_ramps = {}


def paste_ramp_host(R: int) -> torch.Tensor:
    """The fade weights of ``wave_paste``: ramp[d] = 0.5 * (1 + cos(pi * d / R)) for d = 0 .. R - 1, evaluated in
    float64 and rounded to fp32 (ramp[0] = 1, strictly decreasing, never 0).  R = 0: an empty table."""
    d = torch.arange(R, dtype=torch.float64)
    return (0.5 * (1.0 + torch.cos(math.pi * d / max(R, 1)))).float()


def paste_ramp(R: int, device) -> torch.Tensor:
    """``paste_ramp_host(R)`` on ``device``, built once per (R, device)."""
    key = (int(R), torch.device(device))
    if key not in _ramps:
        _ramps[key] = paste_ramp_host(R).to(device)
    return _ramps[key]


def wave_paste(orig: torch.Tensor, gen: torch.Tensor, mask: torch.Tensor, gen_start: int = 0, fade_samples: int = 512,
               frame_samples: int = 512, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Blend the decoded region ``gen`` (B, Ng), samples gen_start .. gen_start + Ng of each clip, into ``orig`` (B, N)
    around the regenerated frames of ``mask`` (B, T; > 0 = regenerated, ``frame_samples`` samples per frame): gen
    inside a regenerated frame, a raised-cosine fade over the ``fade_samples`` samples either side of one, orig bit for
    bit further away and outside gen (alcm_wave_paste).  ``out`` None: a new tensor; ``out=orig`` pastes in place and
    touches only what changes.  One launch."""
    return _paste("wave_paste", orig, gen, mask, gen_start, fade_samples, frame_samples, out)


def wave_paste_ring(orig: torch.Tensor, gen: torch.Tensor, mask: torch.Tensor, gen_start: int, fade_samples: int,
                    frame_samples: int = 512, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``wave_paste`` on one period of a loop (alcm_wave_paste_ring): ``orig`` (B, N) with N = T * ``frame_samples``
    exactly, ``mask`` (B, T) circular, and ``gen`` (B, Ng), 0 < Ng <= N, the ring's samples (gen_start + i) mod N with
    0 <= gen_start < N, so gen may go on across the wrap.  Distances are measured round the ring: a regenerated last
    frame fades into the first samples of frame 0, and a regenerated frame 0 into the end of the last frame.  In place
    only the frames gen covers are visited.  One launch."""
    return _paste("wave_paste_ring", orig, gen, mask, gen_start, fade_samples, frame_samples, out)


def _paste(name, orig, gen, mask, gen_start, fade_samples, frame_samples, out):
    B, N = orig.shape
    assert orig.is_contiguous() and gen.is_contiguous() and mask.is_contiguous()
    assert gen.shape[0] == B and mask.shape[0] == B and gen.dim() == 2 and mask.dim() == 2
    if out is None:
        out = torch.empty_like(orig)
    assert out.shape == orig.shape and out.is_contiguous()
    ramp = paste_ramp(fade_samples, orig.device) if 0 < fade_samples <= PASTE_MAX_FADE_FRAMES * frame_samples else None
    check(getattr(lib(), "alcm_" + name)(ptr(orig), ptr(gen), ptr(mask), ptr(ramp), ptr(out), B, N, int(gen_start),
                                         gen.shape[1], mask.shape[1], int(frame_samples), int(fade_samples),
                                         stream_handle()), name)
    return out


def seam_stats(orig: torch.Tensor, gen: torch.Tensor, mask: torch.Tensor, gen_start: int, fade_samples: int,
               frame_samples: int = 512, ring: bool = False):
    """What ``wave_paste_law`` blends by, measured on the samples it is about to blend (alcm_seam_stats; the arguments
    are ``wave_paste``'s, or ``wave_paste_ring``'s with ``ring``): per junction, an edge of a run of regenerated
    frames, the sums Sxx, Syy and Sxy of orig and gen over the junction's fade zone in float64.  Returns
    (rho (B, T + 1) fp32 per frame edge: the correlation clamped to [0, 1], 1 where there is nothing to measure;
    gam (B, T) fp32 per frame: sqrt(Sxx / Syy) pooled over the run's junctions and clamped to [0.5, 2], 1 in kept
    frames and where there is nothing to measure; sums (B, T + 1, 3) float64).  Two launches, no host round trip."""
    B, N = orig.shape
    assert orig.is_contiguous() and gen.is_contiguous() and mask.is_contiguous()
    assert gen.shape[0] == B and mask.shape[0] == B and gen.dim() == 2 and mask.dim() == 2
    T = mask.shape[1]
    rho = torch.empty((B, T + 1), device=orig.device, dtype=torch.float32)
    gam = torch.empty((B, T), device=orig.device, dtype=torch.float32)
    sums = torch.empty((B, T + 1, 3), device=orig.device, dtype=torch.float64)
    check(lib().alcm_seam_stats(ptr(orig), ptr(gen), ptr(mask), B, N, int(gen_start), gen.shape[1], T,
                                int(frame_samples), int(fade_samples), int(bool(ring)), ptr(rho), ptr(gam), ptr(sums),
                                stream_handle()), "seam_stats")
    return rho, gam, sums


def wave_paste_law(orig: torch.Tensor, gen: torch.Tensor, mask: torch.Tensor, gen_start: int, fade_samples: int,
                   frame_samples: int = 512, out: Optional[torch.Tensor] = None, ring: bool = False,
                   rho: Optional[torch.Tensor] = None, gam: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``wave_paste`` (``ring``: ``wave_paste_ring``) with the fade out = n * ((1 - g) * orig + g * gam * gen), n =
    1 / sqrt((1 - g)^2 + g^2 + 2 (1 - g) g rho), in place of orig + g * (gen - orig) (alcm_wave_paste_law, which states
    the fp32 operation order).  ``rho`` (B, T + 1) and ``gam`` (B, T) are ``seam_stats``' tables; ``rho`` None is 0
    everywhere, the equal-power law, and ``gam`` None is 1.  g = 0 keeps orig's bits and g = 1 with ``gam`` None takes
    gen's.  One launch."""
    B, N = orig.shape
    T = mask.shape[1]
    assert orig.is_contiguous() and gen.is_contiguous() and mask.is_contiguous()
    assert gen.shape[0] == B and mask.shape[0] == B and gen.dim() == 2 and mask.dim() == 2
    assert rho is None or (rho.shape == (B, T + 1) and rho.is_contiguous() and rho.dtype == torch.float32)
    assert gam is None or (gam.shape == (B, T) and gam.is_contiguous() and gam.dtype == torch.float32)
    if out is None:
        out = torch.empty_like(orig)
    assert out.shape == orig.shape and out.is_contiguous()
    ramp = paste_ramp(fade_samples, orig.device) if 0 < fade_samples <= PASTE_MAX_FADE_FRAMES * frame_samples else None
    check(lib().alcm_wave_paste_law(ptr(orig), ptr(gen), ptr(mask), ptr(ramp), ptr(rho), ptr(gam), ptr(out), B, N,
                                    int(gen_start), gen.shape[1], T, int(frame_samples), int(fade_samples),
                                    int(bool(ring)), stream_handle()), "wave_paste_law")
    return out


def paste(orig: torch.Tensor, gen: torch.Tensor, mask: torch.Tensor, gen_start: int, fade_samples: int,
          frame_samples: int = 512, out: Optional[torch.Tensor] = None, ring: bool = False, fade_law: str = "linear",
          match_gain: bool = False) -> torch.Tensor:
    """The paste of every edit that keeps a recording.  ``fade_law`` "linear" without ``match_gain`` is ``wave_paste``
    (``ring``: ``wave_paste_ring``) itself, one launch.  Otherwise ``seam_stats`` measures on this ``orig`` and ``gen``
    and ``wave_paste_law`` blends: "equal-power" with rho = 0, "matched" with the measured rho, "linear" (with
    ``match_gain``) with rho = 1; ``match_gain`` passes the measured gam.  "equal-power" alone measures nothing."""
    from .audio_in import check_fade_law
    check_fade_law(fade_law, match_gain, True)
    if fade_law == "linear" and not match_gain:
        return (wave_paste_ring if ring else wave_paste)(orig, gen, mask, gen_start, fade_samples, frame_samples, out)
    rho = gam = None
    if fade_law == "matched" or match_gain:
        rho, gam, _ = seam_stats(orig, gen, mask, gen_start, fade_samples, frame_samples, ring)
    if fade_law == "linear":
        rho = torch.ones_like(rho)
    elif fade_law == "equal-power":
        rho = None
    return wave_paste_law(orig, gen, mask, gen_start, fade_samples, frame_samples, out, ring, rho,
                          gam if match_gain else None)


def wave_loop(ext: torch.Tensor, start: int, N: int, fade_samples: int = 0) -> torch.Tensor:
    """One period of a looping clip from ``ext`` (B, Next), the decode of the ring's latent padded circularly: the N
    samples from ``start`` on, with the seam closed over the first R = ``fade_samples`` of them (alcm_wave_loop).
    out[n] = ext[start + n] bit for bit from n = R on; out[0] = ext[start + N] bit for bit, the sample that follows the
    period's last one in ``ext``; for 0 < n < R a fade from that continuation to the period's own start,
    fmaf(ramp[n], ext[start + N + n] - ext[start + n], ext[start + n]) with ``paste_ramp(R)``.  R = 0 is a plain crop.
    ValueError unless start >= 0, R <= N and start + N + R <= Next.  One launch."""
    start, N, R = int(start), int(N), int(fade_samples)
    assert ext.dim() == 2 and ext.is_cuda and ext.dtype == torch.float32 and ext.is_contiguous()
    B, Next = ext.shape
    if start < 0 or N < 0 or not 0 <= R <= N or start + N + R > Next:
        raise ValueError(f"wave_loop: need start >= 0, 0 <= fade_samples <= N and start + N + fade_samples <= {Next}, "
                         f"got start {start}, N {N}, fade_samples {R}")
    out = torch.empty((B, N), device=ext.device, dtype=torch.float32)
    ramp = paste_ramp(R, ext.device) if R > 0 else None
    check(lib().alcm_wave_loop(ptr(ext), ptr(ramp), ptr(out), B, Next, start, N, R, stream_handle()), "wave_loop")
    return out


_resample_taps = {}


def resample_taps(rate_in: int, rate_out: int, device):
    """(plan, device tap table (up, ntaps)) of ``resample.plan(rate_in, rate_out)``, uploaded once per rate pair and
    device."""
    from . import resample as _rs
    key = (int(rate_in), int(rate_out), torch.device(device))
    if key not in _resample_taps:
        pl = _rs.plan(int(rate_in), int(rate_out))
        _resample_taps[key] = (pl, torch.from_numpy(pl.taps.copy()).to(device))
    return _resample_taps[key]


def resample(x: torch.Tensor, rate_in: int, rate_out: int, channels: int = 1) -> torch.Tensor:
    """Band-limited resampling ``rate_in -> rate_out`` of x (B, N_in), or (B, N_in, channels) interleaved as a WAV file
    stores it and downmixed to the channel mean in the same launch -> (B, ceil(N_in * up / down)) (alcm_resample; the
    filter: ``audiolcm_amd/resample.py``).  ``rate_in == rate_out`` with one channel returns ``x`` and launches nothing."""
    if x.dim() == 2 and channels == 1:
        x3 = x
    elif x.dim() == 3 and x.shape[2] == channels:
        x3 = x
    else:
        raise ValueError(f"x must be (B, N_in) or (B, N_in, channels = {channels}), got {tuple(x.shape)}")
    if int(rate_in) == int(rate_out) and channels == 1:
        return x if x.dim() == 2 else x[:, :, 0]
    assert x3.is_cuda and x3.dtype == torch.float32 and x3.is_contiguous()
    pl, taps = resample_taps(rate_in, rate_out, x3.device)
    B, n_in = x3.shape[0], x3.shape[1]
    n_out = pl.out_len(n_in)
    y = torch.empty((B, n_out), device=x3.device, dtype=torch.float32)
    if B == 0 or n_in == 0:
        return y
    check(lib().alcm_resample(ptr(x3), ptr(y), B, n_in, int(channels), n_out, pl.up, pl.down, ptr(taps), pl.ntaps,
                              pl.first, stream_handle()), "resample")
    return y


_loudness_coef = {}


def loudness_coef(rate: int, device) -> torch.Tensor:
    """``loudness.tables(rate)`` on ``device`` (float64), uploaded once per rate and device."""
    from . import loudness as _ld
    key = (int(rate), torch.device(device))
    if key not in _loudness_coef:
        _loudness_coef[key] = torch.from_numpy(_ld.tables(int(rate)).copy()).to(device)
    return _loudness_coef[key]


def _row_stride(wav: torch.Tensor) -> int:
    """The row stride of a (B, N) fp32 device tensor with unit column stride."""
    assert wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2
    assert wav.shape[1] <= 1 or wav.stride(1) == 1, "samples must be contiguous within a clip"
    ld = wav.stride(0) if wav.shape[0] > 1 else max(wav.stride(0), wav.shape[1])
    assert ld >= wav.shape[1], "rows overlap"
    return int(ld)


def _loudness_pass(wav: torch.Tensor, coef: Optional[torch.Tensor], hop: int, want_sums: bool, want_peak: bool):
    """One ``alcm_loudness_hops``: (hop sums (B, N // hop) float64 or None, peak (B,) or None)."""
    B, N = wav.shape
    sums = torch.empty((B, N // hop), device=wav.device, dtype=torch.float64) if want_sums else None
    peak = torch.empty((B,), device=wav.device, dtype=torch.float32) if want_peak else None
    if B == 0:
        return sums, peak
    nbytes = lib().alcm_loudness_workspace_bytes(B, N, hop)
    ws = torch.empty((max(nbytes, 8) + 7) // 8, device=wav.device, dtype=torch.float64)
    check(lib().alcm_loudness_hops(ptr(wav), B, N, _row_stride(wav), ptr(coef) if want_sums else None, hop, ptr(sums),
                                   ptr(peak), ptr(ws), ws.numel() * 8, stream_handle()), "loudness_hops")
    return sums, peak


def _measure(wav: torch.Tensor, rate: int, true_peak: bool):
    """(plan, hop sums, peak, the 4x oversampled copy the peak was taken from or None)."""
    from . import loudness as _ld
    pl = _ld.plan(rate, wav.shape[1])
    sums, peak = _loudness_pass(wav, loudness_coef(rate, wav.device), pl.hop, True, not true_peak)
    over = None
    if true_peak:
        over = resample(wav.contiguous(), rate, 4 * int(rate))
        peak = _loudness_pass(over, None, pl.hop, False, True)[1]
    return pl, sums, peak, over


def _loudness_gain(pl, sums, peak, target: float, ceiling: float, want_lufs: bool, want_gain: bool):
    B = sums.shape[0]
    lufs = torch.empty((B,), device=sums.device, dtype=torch.float32) if want_lufs else None
    gain = torch.empty((B,), device=sums.device, dtype=torch.float32) if want_gain else None
    check(lib().alcm_loudness_gain(ptr(sums), ptr(peak), B, pl.nh, pl.hop, float(target), float(ceiling), ptr(lufs),
                                   ptr(gain), stream_handle()), "loudness_gain")
    return lufs, gain


def loudness(wav: torch.Tensor, rate: int, true_peak: bool = False):
    """ITU-R BS.1770 integrated loudness of the mono clips wav (B, N) at ``rate`` -> (lufs (B,) fp32, -inf for a clip
    no block of which passes the absolute gate; peak (B,) fp32: max |wav|, or with ``true_peak`` the same maximum over
    ``resample(wav, rate, 4 * rate)``; hop_sums (B, N // hop) float64), all on the device and without a host
    synchronisation (alcm_loudness_hops, alcm_loudness_gain; the plan: ``audiolcm_amd/loudness.py``).  ValueError for a
    clip under 400 ms."""
    pl, sums, peak, _ = _measure(wav, rate, true_peak)
    lufs, _ = _loudness_gain(pl, sums, peak, float("nan"), 0.0, True, False)
    return lufs, peak, sums


def limit(wav: torch.Tensor, gain: torch.Tensor, ceiling: float, lookahead: int, release_coef: float,
          env: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The look-ahead peak limiter (alcm_limiter; the definition and the plan: ``audiolcm_amd/limiter.py``): each clip
    of wav (B, N) times its ``gain`` (B,) device fp32, turned down around the samples that would pass the linear
    ``ceiling`` so that no |out| exceeds fp32(ceiling).  ``lookahead`` in samples (0 .. 1024), ``release_coef`` =
    exp(-1 / (release_s * rate)) in [0, 1).  ``env`` (B, N) or (B, 4 N): an oversampled copy of the clip whose peaks
    count too.  ``out`` None: a new tensor; ``out=wav`` limits in place, same bits.  No host synchronisation."""
    B, N = wav.shape
    assert gain.is_cuda and gain.dtype == torch.float32 and gain.is_contiguous() and gain.numel() == B
    if out is None:
        out = torch.empty(wav.shape, device=wav.device, dtype=torch.float32)
    assert out.shape == wav.shape
    os_, ld_env = 1, 0
    if env is not None:
        if env.shape[0] != B or env.shape[1] not in (N, 4 * N) or (N == 0 and env.shape[1] != 0):
            raise ValueError(f"env must be (B, N) or (B, 4 N) = ({B}, {N}) or ({B}, {4 * N}), got {tuple(env.shape)}")
        os_, ld_env = (4 if env.shape[1] == 4 * N and N > 0 else 1), _row_stride(env)
    nbytes = lib().alcm_limiter_workspace_bytes(B, N, int(lookahead))
    ws = torch.empty((max(nbytes, 8) + 7) // 8, device=wav.device, dtype=torch.float64)
    check(lib().alcm_limiter(ptr(wav), ptr(env), os_, ptr(gain), ptr(out), B, N, _row_stride(wav), ld_env,
                             _row_stride(out), float(ceiling), int(lookahead), float(release_coef), ptr(ws),
                             ws.numel() * 8, stream_handle()), "limiter")
    return out


def normalize_loudness(wav: torch.Tensor, rate: int, target: Optional[float] = None,
                       peak_dbfs: Optional[float] = None, true_peak: bool = False,
                       out: Optional[torch.Tensor] = None, limiter=None, passes: int = 3,
                       report: bool = False) -> dict:
    """Scale each clip of wav (B, N) to ``target`` LUFS, and by less where its peak would pass ``peak_dbfs``: ->
    dict(wav, lufs (the input's), gain, peak (the input's)), device tensors.  ``target`` None: only the ceiling acts;
    ``peak_dbfs`` None: no ceiling.  The ceiling holds exactly for the sample peak: no |out| exceeds
    fp32(10^(peak_dbfs / 20)); with ``true_peak`` the peak is the 4x oversampled estimate and the ceiling holds for
    it up to rounding.  ``out`` None: a new tensor; ``out=wav`` scales in place.  A gain of 1 returns the input's bits.

    ``limiter`` (a ``limiter.LimiterPlan``; needs ``peak_dbfs``): the ceiling is kept by ``limit`` instead of a smaller
    static gain, so a clip with a binding ceiling still reaches the target.  The pre-gain is the gain to the target
    with no ceiling (1 without a target).  Limiting lowers the loudness a little, so with a target and ``passes`` > 1
    the limited clip is measured again and the pre-gain of the clips whose peak passes the ceiling (fl(peak g0) >
    ceiling) is multiplied by the gain that measurement asks for, and the original is limited again: ``passes`` runs of
    the limiter in all.  A clip whose peak never passes the ceiling is limited once with y = 1 and gets the bytes it
    gets without a limiter.  With ``true_peak`` the limiter also sees ``resample(wav, rate, 4 * rate)``, the copy the peak
    was measured on.  ``gain`` is
    then the last pre-gain.  ``report``: the dict gains ``lufs_out``, the loudness of what is returned (one more
    measurement).  Nothing synchronises with the host."""
    pl, sums, peak, env = _measure(wav, rate, true_peak)
    ceiling = 0.0 if peak_dbfs is None else 10.0 ** (float(peak_dbfs) / 20.0)
    tgt = float("nan") if target is None else float(target)
    if limiter is None:
        lufs, gain = _loudness_gain(pl, sums, peak, tgt, ceiling, True, True)
        if out is None:
            out = torch.empty(wav.shape, device=wav.device, dtype=torch.float32)
        assert out.shape == wav.shape
        B, N = wav.shape
        check(lib().alcm_wave_gain(ptr(wav), ptr(gain), ptr(out), B, N, _row_stride(wav), _row_stride(out),
                                   stream_handle()), "wave_gain")
    else:
        if peak_dbfs is None:
            raise ValueError("a limiter needs a ceiling: give peak_dbfs")
        if int(passes) < 1:
            raise ValueError(f"passes must be at least 1, got {passes!r}")
        assert (limiter.rate, limiter.n) == (int(rate), wav.shape[1]), "the limiter's plan is for another clip"
        if out is not None and out.data_ptr() == wav.data_ptr() and target is not None and int(passes) > 1:
            raise ValueError("with a limiter and more than one pass the original is read again: out must not be wav")
        lufs, gain = _loudness_gain(pl, sums, peak, tgt, 0.0, True, True)
        binds = peak * gain > ceiling_f32(ceiling)
        out = limit(wav, gain, ceiling, limiter.lookahead, limiter.release_coef, env, out)
        for _ in range(int(passes) - 1 if target is not None else 0):
            sums_k = _loudness_pass(out, loudness_coef(rate, wav.device), pl.hop, True, False)[0]
            step = _loudness_gain(pl, sums_k, None, tgt, 0.0, False, True)[1]
            gain = torch.where(binds, gain * step, gain)
            out = limit(wav, gain, ceiling, limiter.lookahead, limiter.release_coef, env, out)
    res = dict(wav=out, lufs=lufs, gain=gain, peak=peak)
    if report:
        sums_o = _loudness_pass(out, loudness_coef(rate, wav.device), pl.hop, True, False)[0]
        res["lufs_out"] = _loudness_gain(pl, sums_o, None, float("nan"), 0.0, True, False)[0]
    return res


def ceiling_f32(ceiling: float) -> float:
    """The linear ceiling as the kernels compare against it: rounded to fp32."""
    return float(torch.tensor(float(ceiling), dtype=torch.float32))


def sincos_embedding(v: torch.Tensor, freqs: torch.Tensor, scale: float, cos_first: bool) -> torch.Tensor:
    B = v.shape[0]
    half = freqs.numel()
    out = torch.empty((B, 2 * half), device=v.device, dtype=torch.float32)
    check(lib().alcm_sincos_embedding(ptr(v.float().contiguous()), scale, ptr(freqs), B, half, int(cos_first),
                                      ptr(out), stream_handle()), "sincos_embedding")
    return out


def operand_planes(x_cl: torch.Tensor, prec: int, Cp: Optional[int] = None) -> torch.Tensor:
    """(B, T, C) fp32 -> MFMA operand planes int16 (NP, B, T, Cp) as alcm_activation1d_op writes them
    (without the activation): fp16 for PREC_F16/F16W2, bf16 for PREC_BF16, bf16 hi/lo for PREC_SPLIT."""
    B, T, Cc = x_cl.shape
    Cp = Cp or _round_up(Cc, 32)
    x = torch.nn.functional.pad(x_cl.float(), (0, Cp - Cc))
    if prec in (_hip.PREC_F16, _hip.PREC_F16W2):
        return x.half().view(torch.int16).unsqueeze(0).contiguous()
    hi = x.bfloat16()
    if prec == _hip.PREC_BF16:
        return hi.view(torch.int16).unsqueeze(0).contiguous()
    lo = (x - hi.float()).bfloat16()
    return torch.stack([hi.view(torch.int16), lo.view(torch.int16)]).contiguous()


def activation1d_op(x_cl: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, up_filter: torch.Tensor,
                    down_filter: torch.Tensor, prec: int, Cp: Optional[int] = None) -> torch.Tensor:
    """Activation1d of channels-last (B, T, C) into operand planes int16 (NP, B, T, Cp)."""
    B, T, Cc = x_cl.shape
    Cp = Cp or _round_up(Cc, 32)
    x_cl = x_cl.contiguous()
    ae, ib = snake_params(alpha, beta)
    ae, ib = ae.contiguous(), ib.contiguous()
    fu = up_filter.detach().reshape(-1).float().cpu().contiguous()
    fd = down_filter.detach().reshape(-1).float().cpu().contiguous()
    npl = 2 if prec == _hip.PREC_SPLIT else 1
    y = torch.empty((npl, B, T, Cp), dtype=torch.int16, device=x_cl.device)
    check(lib().alcm_activation1d_op(ptr(x_cl), ptr(y), B, T, Cc, Cp, ptr(ae), ptr(ib), fu.data_ptr(), fd.data_ptr(),
                                     int(prec), stream_handle()), "activation1d_op")
    return y


def activation1d_op_f16in(x16: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, up_filter: torch.Tensor,
                          down_filter: torch.Tensor, prec: int) -> torch.Tensor:
    """Activation1d of an fp16 operand plane (1, B, T, C) int16 (an `opconv(..., out_plane=True)` result) into
    operand planes (1, B, T, C): alcm_activation1d_op_f16in (the wide-stage conv1 -> Activation1d hand-off)."""
    _, B, T, Cc = x16.shape
    assert x16.dtype == torch.int16 and x16.is_contiguous()
    ae, ib = snake_params(alpha, beta)
    ae, ib = ae.contiguous(), ib.contiguous()
    fu = up_filter.detach().reshape(-1).float().cpu().contiguous()
    fd = down_filter.detach().reshape(-1).float().cpu().contiguous()
    y = torch.empty((1, B, T, Cc), dtype=torch.int16, device=x16.device)
    check(lib().alcm_activation1d_op_f16in(ptr(x16), ptr(y), B, T, Cc, Cc, ptr(ae), ptr(ib), fu.data_ptr(),
                                           fd.data_ptr(), int(prec), stream_handle()), "activation1d_op_f16in")
    return y


def activation1d_op_x3(x_cl: torch.Tensor, alphas, betas, up_filter: torch.Tensor, down_filter: torch.Tensor,
                       prec: int) -> list:
    """Three Activation1d of one channels-last (B, T, C) input, with their own SnakeBeta parameters and the same FIR
    taps, in one launch (alcm_activation1d_planes, nset = 3) -> three operand planes int16 (NP, B, T, Cp)."""
    B, T, Cc = x_cl.shape
    Cp = _round_up(Cc, 32)
    x_cl = x_cl.contiguous()
    params = [tuple(t.contiguous() for t in snake_params(a, b)) for a, b in zip(alphas, betas)]
    fu = up_filter.detach().reshape(-1).float().cpu().contiguous()
    fd = down_filter.detach().reshape(-1).float().cpu().contiguous()
    ys = [torch.empty((2 if prec == _hip.PREC_SPLIT else 1, B, T, Cp), dtype=torch.int16, device=x_cl.device)
          for _ in range(3)]
    a = _hip.ActArgs()
    a.x, a.nset, a.B, a.T, a.C, a.Cp, a.prec = ptr(x_cl), 3, B, T, Cc, Cp, int(prec)
    for i in range(3):
        a.y[i], a.alpha_exp[i], a.inv_beta[i] = ptr(ys[i]), ptr(params[i][0]), ptr(params[i][1])
    a.up_filter, a.down_filter = fu.data_ptr(), fd.data_ptr()
    check(lib().alcm_activation1d_planes(C.byref(a), stream_handle()), "activation1d_planes")
    return ys


def act_plan(args: _hip.ActArgs) -> dict:
    """Which kernel an Activation1d-into-planes call would launch: name = its profile row, kernel ("coop", "mfma",
    "mfma3"), its template parameters prec, np, nset, defer, in16, grid, the kernel scalars tiles_t, tiles_c, strips_t,
    y_lo, flops, bytes.  Launches nothing and needs no GPU."""
    return _hip.debug_act_plan(args)


def attn_plan(args: _hip.AttnArgs) -> dict:
    """Which kernel a fused-attention call would launch: name = its profile row, form ("resident_plane",
    "resident_f32", "tiled"), prec, bias, lp, dh, scale, grid, block, flops, bytes.  Launches nothing and needs no GPU."""
    return _hip.debug_attn_plan(args)


def conv_plan(args, ncu: int = 0, dense: bool = False) -> list:
    """Which kernel(s) an operand-plane conv call would launch: args is one _hip.OpConvArgs (alcm_opconv, or
    alcm_opconv_dense with dense = True) or a sequence of up to three (alcm_opconv_sum).  -> one dict per launch (name =
    its profile row, kernel, bm, bn, grid, ksplit, n_major, ncu, tiles_per_batch, tiles, flops, bytes; for the tail
    convs also inst = the template-id, block, ncg, wslots); needs no GPU when ncu is given."""
    if isinstance(args, _hip.OpConvArgs):
        return _hip.debug_conv_plan(args, 1, _hip.PLAN_DENSE if dense else _hip.PLAN_OPCONV, ncu)
    arr = (_hip.OpConvArgs * len(args))(*args)
    return _hip.debug_conv_plan(arr, len(args), _hip.PLAN_SUM, ncu)


def gemm_plan(args: _hip.GemmArgs) -> dict:
    """Which kernel an alcm_gemm call would launch: name = its profile row, family ("none" for M or N <= 0,
    "window_conv", "skinny", "gemm"), bm, bn, wm, wn, grid, flops, bytes.  Launches nothing and needs no GPU."""
    return _hip.debug_gemm_plan(args)


def voc_stage_shapes(cfg) -> list:
    """The BigVGAN stages of a recipe.BigVGANConfig as the stage planner reads them (_hip.VocStageShape), as the
    library's loader derives them from the packed weights: phase weights of one shape, the tail convs' dense packing
    for cout <= 96 with cout % 8 == 0, and the resblocks' Activation1d filters equal (one kaiser-sinc design)."""
    shapes = []
    for i, (rate, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        h = _hip.VocStageShape()
        h.cin, h.cout, h.rate, h.taps = cfg.upsample_initial_channel >> i, cfg.stage_channels(i), rate, k // rate
        h.cpad = (h.cin + 7) // 8 * 8
        h.phases_share = h.act0_equal = 1
        h.dense_weights = int(h.cout <= 96 and h.cout % 8 == 0)
        h.nrb, h.ndil = len(cfg.resblock_kernel_sizes), len(cfg.resblock_dilation_sizes[0])
        h.rb_k[:h.nrb] = cfg.resblock_kernel_sizes
        h.dil[:h.ndil] = cfg.resblock_dilation_sizes[0]
        shapes.append(h)
    return shapes


def voc_plan(cfg, policy, streams: bool, B: int, M: int, ncu: int = 0) -> list:
    """What every BigVGAN stage of `cfg` runs at batch B and M mel frames under the policy (a name in _hip.POLICIES or
    its code) and the current ALCM_* switches: one dict of the alcm_voc_stage_plan fields per stage."""
    return _hip.debug_voc_plan(voc_stage_shapes(cfg), _hip.POLICIES.get(policy, policy), streams, B, M, ncu)


def opconv_sum(terms, prec: int, out_scale: float = 1.0, accumulate_into: Optional[torch.Tensor] = None,
               out_plane: bool = False):
    """alcm_opconv_sum: out (B, T, N) = (sum over terms of conv_k(planes) + bias + residual) * out_scale (+ out) — the
    mean over a BigVGAN stage's resblocks at their last conv2 + residual (vocoder/bigvgan/models.py:190-199).
    terms: up to three (planes (1, B, T, Cp), w (N, C, k), bias or None, residual (B, T, N) or None, packed or None),
    same-length dilation-1 convs sharing B, T and N.  out_plane = True: the result as one PREC operand plane
    (1, B, T, N) instead (the one-launch form only, no accumulate)."""
    n = len(terms)
    assert 1 <= n <= 3
    args = (_hip.OpConvArgs * n)()
    keep = []
    out = None
    for i, (planes, w, bias, res, packed) in enumerate(terms):
        npl, B, T, Cp = planes.shape
        assert planes.dtype == torch.int16 and planes.is_contiguous()
        N, cin, k = w.shape
        if packed is None:
            wp = torch.nn.functional.pad(w, (0, 0, 0, Cp - cin)).contiguous() if Cp != cin else w
            packed = pack_conv_weight(wp)
        keep.append(packed)
        if out is None:
            out = accumulate_into if accumulate_into is not None else torch.empty((B, T, N), device=planes.device)
        a = args[i]
        a.a, a.a_lo_off, a.B, a.T, a.C, a.Cp = ptr(planes), B * T * Cp, B, T, cin, Cp
        a.ksize, a.dil, a.pad = k, 1, (k - 1) // 2
        a.w, a.w_lo_off, a.kpad, a.N = ptr(packed.data), packed.lo_off, packed.kpad, N
        a.bias = ptr(bias)
        if res is not None:
            res = res.contiguous()
            keep.append(res)
        a.res = ptr(res)
        a.prec = int(prec)
        if i == 0:
            a.out, a.out_scale, a.accumulate = ptr(out), out_scale, int(accumulate_into is not None)
            if out_plane:
                assert accumulate_into is None
                out = torch.empty((1, B, T, N), dtype=torch.int16, device=planes.device)
                a.out, a.out_plane = None, ptr(out)
    check(lib().alcm_opconv_sum(args, n, stream_handle()), "opconv_sum")
    return out


def opconv(planes: torch.Tensor, C_real: int, w: torch.Tensor, bias: Optional[torch.Tensor], dilation: int,
           prec: int, residual: Optional[torch.Tensor] = None, out_act: int = 0, out_scale: float = 1.0,
           accumulate_into: Optional[torch.Tensor] = None, packed: Optional["PackedWeight"] = None,
           act: Optional[tuple] = None, fp32_out: bool = True, geglu: bool = False,
           strided: Optional[tuple] = None, dense: bool = False, out_plane: bool = False,
           ksplit_ws: Optional[torch.Tensor] = None):
    """Same-length conv1d (B, T, N) = conv_{k,dilation}(operand planes (NP, B, T, Cp)) + bias (+res ...).

    act = (alpha, beta, up_filter, down_filter): also return Activation1d(conv + bias (+res)) as operand
    planes (NP, B, T, round_up(N, 32)) from the fused epilogue -> (out or None, planes).
    strided = (out, stride, offset, pad): one ConvTranspose1d phase, row t -> row t*stride + offset of the
    fp32 (B, R, N) tensor `out` (written in place and returned), input rows t - pad + tap*dilation.
    dense = True: the narrow-stage resident-weight kernel (alcm_opconv_dense): weights packed with cpad = C_real
    (pack_conv_weight(w)), planes channels >= C_real ignored, the fused Activation1d writes channels < N only.
    out_plane = True: conv + bias as one PREC operand plane (1, B, T, N) instead of the fp32 output (no residual /
    activation / accumulate; the DiT q,k,v projection).
    ksplit_ws: fp32 device workspace the library may use for K-split partial sums (alcm_opconv_args.ksplit_ws)."""
    npl, B, T, Cp = planes.shape
    assert planes.dtype == torch.int16 and planes.is_contiguous()
    N, cin, k = w.shape
    assert cin == C_real <= Cp
    if dense and packed is None:
        packed = pack_conv_weight(w)
    if packed is None:
        wp = torch.nn.functional.pad(w, (0, 0, 0, Cp - cin)).contiguous() if Cp != cin else w
        packed = pack_conv_weight(wp)
    a = _hip.OpConvArgs()
    a.a, a.a_lo_off, a.B, a.T, a.C, a.Cp = ptr(planes), B * T * Cp, B, T, C_real, Cp
    a.ksize, a.dil, a.pad = k, dilation, (k - 1) * dilation // 2
    a.w, a.w_lo_off, a.kpad, a.N = ptr(packed.data), packed.lo_off, packed.kpad, N
    a.bias = ptr(bias)
    if ksplit_ws is not None:
        assert ksplit_ws.dtype == torch.float32 and ksplit_ws.is_contiguous()
        a.ksplit_ws, a.ksplit_ws_floats = ptr(ksplit_ws), ksplit_ws.numel()
    if strided is not None:
        out, a.out_stride, a.out_offset, a.pad = strided
        assert out.is_contiguous() and out.shape[0] == B and out.shape[2] == N
        a.out, a.out_rows, a.out_scale, a.prec = ptr(out), out.shape[1], 1.0, int(prec)
        check(lib().alcm_opconv(C.byref(a), stream_handle()), "opconv")
        return out
    a.res = ptr(residual.contiguous()) if residual is not None else None
    if accumulate_into is not None:
        out = accumulate_into
    else:
        out = torch.empty((B, T, N), device=planes.device) if (fp32_out or act is None) else None
    a.out, a.out_act, a.accumulate, a.out_scale, a.prec = ptr(out), out_act, int(accumulate_into is not None), \
        out_scale, int(prec)
    keep = []
    if out_plane:
        op = torch.empty((1, B, T, N), dtype=torch.int16, device=planes.device)
        a.out, a.out_plane = None, ptr(op)
        check(lib().alcm_opconv(C.byref(a), stream_handle()), "opconv")
        return op
    if geglu:  # GEGLU epilogue (interleaved value/gate output columns) -> operand plane (1, B, T, N/2)
        gp = torch.empty((1, B, T, N // 2), dtype=torch.int16, device=planes.device)
        a.out, a.geglu_plane = None, ptr(gp)
        check(lib().alcm_opconv(C.byref(a), stream_handle()), "opconv")
        return gp
    if act is not None:
        alpha, beta, fu, fd = act
        ae, ib = snake_params(alpha, beta)
        ae, ib = ae.contiguous(), ib.contiguous()
        fu = fu.detach().reshape(-1).float().cpu().contiguous()
        fd = fd.detach().reshape(-1).float().cpu().contiguous()
        cpo = _round_up(N, 32)
        nplo = 2 if prec == _hip.PREC_SPLIT else 1
        # (dense=True writes channels < N only: zero planes keep the operand padding safe for any consumer)
        y = (torch.zeros if dense else torch.empty)((nplo, B, T, cpo), dtype=torch.int16, device=planes.device)
        keep = [ae, ib, fu, fd]
        a.act_plane, a.act_plane_lo_off = ptr(y), B * T * cpo
        a.act_alpha_exp, a.act_inv_beta = ptr(ae), ptr(ib)
        a.act_up_filter = fu.data_ptr()
        a.act_down_filter = fd.data_ptr()
    if dense:
        check(lib().alcm_opconv_dense(C.byref(a), stream_handle()), "opconv_dense")
    else:
        check(lib().alcm_opconv(C.byref(a), stream_handle()), "opconv")
    del keep
    if act is not None:
        return out, y
    return out


def flash_attention(qkv: Optional[torch.Tensor], heads: int, prec: int, *, bias: Optional[torch.Tensor] = None,
                    scale: float = 0.0, qkv_plane: Optional[torch.Tensor] = None,
                    out_plane: bool = False) -> torch.Tensor:
    """(B, L, 3H) fp32 [q | k | v] rows -> (B, L, H) multi-head softmax(q k^T / sqrt(dh)) v (fused kernel).

    The keywords reach the forms the models launch (alcm_flash_attention_ex): ``bias`` (heads, bld, bld) fp32 added
    to the scores, ``scale`` > 0 instead of dh^-1/2, ``qkv_plane`` (B, L, 3H) int16 operand rows (fp16 / bf16 bits of
    ``prec``) instead of ``qkv``, ``out_plane``: the result as an int16 (B, L, H) operand plane instead of fp32."""
    if bias is None and scale == 0.0 and qkv_plane is None and not out_plane:
        # the plain call stays on alcm_flash_attention, so that the older entry keeps being exercised by the tests
        B, L, H3 = qkv.shape
        H = H3 // 3
        qkv = qkv.contiguous()
        out = torch.empty((B, L, H), device=qkv.device)
        check(lib().alcm_flash_attention(ptr(qkv), ptr(out), B, L, H, heads, int(prec), stream_handle()),
              "flash_attention")
        return out
    src = qkv_plane if qkv_plane is not None else qkv
    B, L, H3 = src.shape
    H = H3 // 3
    if qkv is not None:
        assert qkv.dtype == torch.float32 and tuple(qkv.shape) == (B, L, H3)
        qkv = qkv.contiguous()
    if qkv_plane is not None:
        assert qkv_plane.dtype == torch.int16 and qkv_plane.is_contiguous()
    bld = 0
    if bias is not None:
        bld = bias.shape[-1]
        assert bias.dtype == torch.float32 and tuple(bias.shape) == (heads, bld, bld) and bias.is_contiguous()
    out = torch.empty((B, L, H), device=src.device, dtype=torch.int16 if out_plane else torch.float32)
    check(lib().alcm_flash_attention_ex(ptr(qkv), ptr(qkv_plane), None if out_plane else ptr(out),
                                        ptr(out) if out_plane else None, B, L, H, heads, int(prec), ptr(bias), bld,
                                        float(scale), stream_handle()), "flash_attention_ex")
    return out


def layer_norm_plane(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, prec: int, eps: float = 1e-5):
    """LayerNorm over the last dim of (B, T, C) fp32 -> operand plane int16 (1, B, T, C) (fp16 or bf16 bits)."""
    B, T, Cc = x.shape
    x = x.contiguous()
    y = torch.empty((1, B, T, Cc), dtype=torch.int16, device=x.device)
    check(lib().alcm_layer_norm_plane(ptr(x), B * T, Cc, Cc, eps, ptr(gamma.contiguous()), ptr(beta.contiguous()),
                                      ptr(y), int(prec), stream_handle()), "layer_norm_plane")
    return y
