"""A float64 restatement of alcm_gemm, written from its definition in include/audiolcm_hip.h (the comments of
alcm_operand and alcm_gemm_args), not from the kernels, and the table of calls that tests/test_gemm_forms_host.py and
tests/test_gpu_gemm_forms.py run it on.

A call is a description ``d`` (the fields of alcm_gemm_args by name, the operands as the nested dicts ``a`` and ``b``,
in the style of test_gemmplan.py's conv_form / qk_form; a pointer is the key ``buf`` of a host buffer plus an element
offset ``off``) and a dict ``t`` of flat float32 host buffers: the operand buffers, ``w`` (the fp32 weight [N][C_in][k]
of a WEIGHT operand), ``bias``, ``res``, ``out`` (the prior contents of the output) and the prologue vectors.  The same
description gives the reference (evaluate) and the device call (gemm_args, run_device), so a case is written once.

evaluate() gathers A[z][m][k] and B[z][n][k] element by element as the header defines them (loops over z and tap, NumPy
index arithmetic over rows and channels), multiplies in float64 and applies the epilogue in the documented order.  A
``mutant`` makes it wrong in one named way (MUTANTS): the host tests use those to show that each case's data would
expose that mistake at the tolerance the GPU test applies.
"""
import functools

import numpy as np
import torch

GUARD = 64            # elements before and after every output / residual buffer
SENTINEL = -777.25    # what an output buffer holds where no prior value is read
ACT, ACT_T, WEIGHT = 0, 1, 2
SPLIT_TOL, BF16_TOL, F16_TOL = 2e-5, 1.5e-2, 2e-3    # the bounds of test_gpu_ops.py
TOL = {1: SPLIT_TOL, 0: BF16_TOL, 2: F16_TOL}
ROUND = {1: None, 0: "bf16", 2: "f16"}
PRECS = (1, 0, 2)

MUTANTS = (
    "pro_pad_rows",          # the prologue applied to padding rows
    "pro_pad_lanes",         # the prologue applied to channels >= C_in, with a non-zero weight pad
    "up_round",              # up = 2 indexed as (t_up + 1) / 2
    "drop_last_chunk",       # the last K chunk dropped
    "dil_last_tap",          # the dilation ignored on the last tap
    "geglu_swap",            # the GEGLU pair swapped
    "geglu_store_n",         # the GEGLU output stored at n instead of n / 2
    "geglu_erf_tanh",        # erf and tanh GELU exchanged
    "res_before_act",        # res added before the activation
    "out_scale_after_acc",   # out_scale applied after accumulate
    "acc_scale_after_bias",  # acc_scale applied after the bias
    "swap_zs_a", "swap_zs_b", "swap_zs_out", "swap_zs_res",  # zs1 and zs2 swapped
    "no_out_off",            # out_off ignored
    "res_swap_sc_st",        # r_sc and r_st swapped for an NCT residual
)


def _rup(x, m):
    return (x + m - 1) // m * m


def _round(x, fmt):
    """float64 -> fp32 -> bf16 / fp16 (round to nearest even, torch's casts) -> float64."""
    if fmt is None:
        return x
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]
    return torch.tensor(x).float().to(dt).double().numpy()


def _zoff(z, zdiv, s1, s2, swap=False):
    if swap:
        s1, s2 = s2, s1
    return (z // zdiv) * s1 + (z % zdiv) * s2


def _take(buf, idx, wrap):
    """buf[idx]; a mutant may index outside the buffer, and then wraps round."""
    if not wrap:
        assert idx.min() >= 0 and idx.max() < buf.size, (int(idx.min()), int(idx.max()), buf.size)
    return np.take(buf, idx, mode="wrap" if wrap else "raise")


def _silu(v):
    return v / (1.0 + np.exp(-v))


def _gelu_erf(v):
    return 0.5 * v * (1.0 + torch.erf(torch.tensor(v) * 2.0 ** -0.5).numpy())


def _gelu_tanh(v):
    return 0.5 * v * (1.0 + np.tanh((2.0 / np.pi) ** 0.5 * (v + 0.044715 * v ** 3)))


ACTS = {0: lambda v: v, 1: _silu, 2: _gelu_erf, 3: _gelu_tanh, 4: np.tanh}


def edge_rows(o, rows):
    """Rows of an ACT operand whose receptive field touches the zero padding in time."""
    t = np.arange(rows) % o["rows_per_batch"]
    T = o["T_in"] * (2 if o.get("up", 1) == 2 else 1)
    return (t - o["pad"] < 0) | (t + (o["ksize"] - 1) * o["dil"] - o["pad"] >= T)


def act_matrix(o, t, rows, nz, zdiv, Kpad, mutant=None, which="a"):
    """The ACT operand as [nz][rows][Kpad] float64: element (b, t, c) at off + zoff + b*sb + t*st + c*sc, K index
    k = tap*Cpad + ci, t_src = t + tap*dil - pad (up == 2: t_up = t + tap*dil - pad on the x2 upsampled input, t_src =
    t_up / 2), zero for t_up outside the (upsampled) input, ci >= C_in and k >= ksize*Cpad; the prologue on the valid
    elements only."""
    buf = t[o["buf"]].astype(np.float64)
    up = 2 if o.get("up", 1) == 2 else 1
    T_in, C_in, Cpad, ks = o["T_in"], o["C_in"], o["Cpad"], o["ksize"]
    m = np.arange(rows)
    b, tt = m // o["rows_per_batch"], m % o["rows_per_batch"]
    c = np.arange(Cpad)
    lane_ok = c < C_in
    cc = np.minimum(c, C_in - 1)
    mean = t.get(o.get("pro_mean"))
    rstd = t.get(o.get("pro_rstd"))
    scale = t.get(o.get("pro_scale"))
    shift = t.get(o.get("pro_shift"))
    wrap = mutant is not None
    A = np.zeros((nz, rows, Kpad))
    for z in range(nz):
        zo = _zoff(z, zdiv, o.get("zs1", 0), o.get("zs2", 0), mutant == "swap_zs_" + which)
        for tap in range(ks):
            step = 1 if (mutant == "dil_last_tap" and tap == ks - 1) else o["dil"]
            tu = tt + tap * step - o["pad"]
            row_ok = (tu >= 0) & (tu < up * T_in)
            ts = tu
            if up == 2:
                ts = (tu + 1) // 2 if mutant == "up_round" else tu // 2
            ts = np.clip(ts, 0, T_in - 1)
            valid = row_ok[:, None] & lane_ok[None, :]
            idx = o.get("off", 0) + zo + b[:, None] * o["sb"] + ts[:, None] * o["st"] + cc[None, :] * o["sc"]
            v = np.where(valid, _take(buf, np.where(valid, idx, 0), wrap), 0.0)
            apply = valid
            if mutant == "pro_pad_rows":
                apply = np.broadcast_to(lane_ok[None, :], valid.shape)
            if mean is not None:
                ri = b * T_in + ts
                norm_on = np.broadcast_to(row_ok[:, None], valid.shape) if mutant == "pro_pad_lanes" else apply
                v = np.where(norm_on, (v - mean[ri].astype(np.float64)[:, None]) * rstd[ri].astype(np.float64)[:, None], v)
            if scale is not None:
                pi = b[:, None] * o.get("pro_sb", 0) + cc[None, :]
                v = np.where(apply, v * scale.astype(np.float64)[pi] + shift.astype(np.float64)[pi], v)
            if o.get("pro_act", 0):
                assert o["pro_act"] == 1
                v = np.where(apply, _silu(v), v)
            A[z, :, tap * Cpad:(tap + 1) * Cpad] = v
    if mutant == "drop_last_chunk":
        A[:, :, Kpad - 32:] = 0.0
    return A


def b_matrix(d, t, nz, mutant=None):
    """The B operand as [nz][N][Kpad] float64."""
    o, N, Kpad = d["b"], d["N"], d["Kpad"]
    if o["kind"] == WEIGHT:   # the original fp32 weight [N][C_in][k] at K index tap*Cpad + ci, zero elsewhere
        w = t["w"].astype(np.float64)
        n, cin, ks = w.shape
        Cpad = d["a"]["Cpad"]
        assert n == N and cin == d["a"]["C_in"] and ks == d["a"]["ksize"]
        Bm = np.zeros((1, N, Kpad))
        for tap in range(ks):
            Bm[0, :, tap * Cpad:tap * Cpad + cin] = w[:, :, tap]
            if mutant == "pro_pad_lanes":
                Bm[0, :, tap * Cpad + cin:(tap + 1) * Cpad] = 1.0
        return np.broadcast_to(Bm, (nz, N, Kpad))
    if o["kind"] == ACT:
        return act_matrix(o, t, N, nz, d["zdiv"], Kpad, mutant, "b")
    assert o["kind"] == ACT_T   # element (n, k) at k*st + n*sc, valid k < T_in, n < rows
    buf = t[o["buf"]].astype(np.float64)
    Bm = np.zeros((nz, N, Kpad))
    n, k = np.arange(min(N, o["rows"])), np.arange(min(Kpad, o["T_in"]))
    for z in range(nz):
        zo = _zoff(z, d["zdiv"], o.get("zs1", 0), o.get("zs2", 0), mutant == "swap_zs_b")
        idx = o.get("off", 0) + zo + k[None, :] * o["st"] + n[:, None] * o["sc"]
        Bm[z, :n.size, :k.size] = _take(buf, idx, mutant is not None)
    return Bm


def _epi_index(d, base, zs1, zs2, sb, st, sc, cols, swap=False, no_off=False):
    """[nz][M][cols]: zoff + b*sb + (t*out_step + out_off)*st + n*sc for output row m -> (b, t)."""
    nz = max(d.get("batch", 1), 1)
    z = np.arange(nz)
    zo = _zoff(z, max(d.get("zdiv", 1), 1), zs1, zs2, swap)
    m = np.arange(d["M"])
    b, tt = m // d["out_rows_per_batch"], m % d["out_rows_per_batch"]
    to = tt * (d.get("out_step", 1) or 1) + (0 if no_off else d.get("out_off", 0))
    return base + zo[:, None, None] + (b * sb + to * st)[None, :, None] + (cols * sc)[None, None, :]


def out_index(d, **kw):
    ncol = d["N"] // 2 if d.get("geglu") else d["N"]
    return _epi_index(d, d.get("out_base", 0), d.get("o_zs1", 0), d.get("o_zs2", 0), d.get("o_sb", 0), d["o_st"],
                      d["o_sc"], np.arange(ncol), **kw)


def res_index(d, cols=None, **kw):
    ncol = d["N"] // 2 if d.get("geglu") else d["N"]
    return _epi_index(d, d.get("res_base", 0), d.get("r_zs1", 0), d.get("r_zs2", 0), d.get("r_sb", 0), d["r_st"],
                      d["r_sc"], np.arange(ncol) if cols is None else cols, **kw)


class Result:
    """out: the output buffer after the call (float64); written: the elements the call stores; edge: those of rows
    whose receptive field touches the padding."""

    def __init__(self, out, written, edge):
        self.out, self.written, self.edge = out, written, edge


def evaluate(d, t, round_operands=None, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    assert d["a"]["kind"] == ACT
    M, N, Kpad = d["M"], d["N"], d["Kpad"]
    nz, zdiv = max(d.get("batch", 1), 1), max(d.get("zdiv", 1), 1)
    wrap = mutant is not None
    A = _round(act_matrix(d["a"], t, M, nz, zdiv, Kpad, mutant, "a"), round_operands)
    Bm = _round(b_matrix(d, t, nz, mutant), round_operands)
    acc = np.einsum("zmk,znk->zmn", A, Bm)

    # v = acc*acc_scale + bias[n]; v = act(v) | geglu; v += res; v *= out_scale; if accumulate v += out; out = v
    bias = t["bias"].astype(np.float64) if d.get("bias") else np.zeros(N)
    v = (acc + bias) * d["acc_scale"] if mutant == "acc_scale_after_bias" else acc * d["acc_scale"] + bias
    res = t["res"].astype(np.float64) if d.get("res") else None
    geglu = d.get("geglu", 0)
    cols = np.arange(N // 2 if geglu else N)
    if mutant == "res_before_act":
        v = v + _take(res, res_index(d), wrap)
    if geglu:       # pairs (even, odd): v_even * gelu(v_odd) -> column n / 2; act is ignored
        val, gate = v[..., 0::2], v[..., 1::2]
        if mutant == "geglu_swap":
            val, gate = gate, val
        erf = (geglu == 1) != (mutant == "geglu_erf_tanh")
        v = val * (_gelu_erf(gate) if erf else _gelu_tanh(gate))
    else:
        v = ACTS[d.get("act", 0)](v)
    if res is not None and mutant != "res_before_act":
        if mutant == "res_swap_sc_st":
            dd = dict(d, r_sc=d["r_st"], r_st=d["r_sc"])
            v = v + _take(res, res_index(dd), wrap)
        else:
            v = v + _take(res, res_index(d, swap=mutant == "swap_zs_res"), wrap)
    oi = out_index(d)
    oi_m = oi
    if mutant == "geglu_store_n":
        oi_m = _epi_index(d, d.get("out_base", 0), d.get("o_zs1", 0), d.get("o_zs2", 0), d.get("o_sb", 0), d["o_st"],
                          d["o_sc"], 2 * cols)
    if mutant in ("swap_zs_out", "no_out_off"):
        oi_m = out_index(d, swap=mutant == "swap_zs_out", no_off=mutant == "no_out_off")
    prior = t["out"].astype(np.float64)
    if wrap:
        oi_m = oi_m % prior.size
    else:
        assert oi.min() >= 0 and oi.max() < prior.size and np.unique(oi).size == oi.size, "stores overlap or leave out"
    if d.get("accumulate"):
        v = (v + prior[oi_m]) * d["out_scale"] if mutant == "out_scale_after_acc" else v * d["out_scale"] + prior[oi_m]
    else:
        v = v * d["out_scale"]
    out = prior.copy()
    out[oi_m] = v
    written = np.zeros(prior.size, bool)
    written[oi] = True
    edge = np.zeros(prior.size, bool)
    edge[oi[:, edge_rows(d["a"], M), :]] = True
    return Result(out, written, edge)


def mutants_for(d, t):
    """The mutations that are meaningful for a call."""
    a, m = d["a"], ["drop_last_chunk"]
    pro = bool(a.get("pro_mean") or a.get("pro_scale") or a.get("pro_act"))
    if pro and edge_rows(a, d["M"]).any():
        m.append("pro_pad_rows")
    if a.get("pro_mean") and a["C_in"] < a["Cpad"] and d["b"]["kind"] == WEIGHT:
        m.append("pro_pad_lanes")
    if a.get("up", 1) == 2:
        m.append("up_round")
    if a["ksize"] > 1 and a["dil"] > 1:
        m.append("dil_last_tap")
    if d.get("geglu"):
        m += ["geglu_swap", "geglu_store_n", "geglu_erf_tanh"]
    if d.get("res") and d.get("act") and not d.get("geglu"):
        m.append("res_before_act")
    if d.get("accumulate") and d["out_scale"] != 1.0:
        m.append("out_scale_after_acc")
    if d.get("bias") and d["acc_scale"] != 1.0:
        m.append("acc_scale_after_bias")
    if max(d.get("zdiv", 1), 1) > 1:
        m += ["swap_zs_a", "swap_zs_b", "swap_zs_out"] + (["swap_zs_res"] if d.get("res") else [])
    if d.get("out_off"):
        m.append("no_out_off")
    if d.get("res") and d["r_st"] == 1 and d["r_sc"] != 1:
        m.append("res_swap_sc_st")
    return m


def has_prologue(d):
    a = d["a"]
    return bool(a.get("pro_mean") or a.get("pro_scale") or a.get("pro_act"))


# ------------------------------------------------------------------ the description as _hip.GemmArgs
A_PTRS = ("pro_scale", "pro_shift", "pro_mean", "pro_rstd")


def fake_addresses(t):
    """A 16-byte aligned made-up address per buffer: enough for the planner, which never dereferences."""
    return {k: (i + 1) << 32 for i, k in enumerate(sorted(set(t) | {"wpack"}))}


def gemm_args(d, addr, prec):
    """_hip.GemmArgs of a description; addr: the address of every buffer of t (and "wpack", the packed weight)."""
    from audiolcm_amd import _hip
    g = _hip.GemmArgs()
    for f, _ in _hip.GemmArgs._fields_:
        if f in ("a", "b"):
            o, od = getattr(g, f), d[f]
            if od["kind"] == WEIGHT:
                o.kind, o.ptr, o.rows, o.w_lo_off = WEIGHT, addr["wpack"], d["N"], d["N"] * d["Kpad"]
                continue
            for of, _ in _hip.Operand._fields_:
                if of == "ptr":
                    o.ptr = addr[od["buf"]] + 4 * od.get("off", 0)
                elif of in A_PTRS:
                    setattr(o, of, addr[od[of]] if od.get(of) else None)
                else:
                    setattr(o, of, od.get(of, 0))
        elif f == "bias":
            g.bias = addr["bias"] if d.get("bias") else None
        elif f == "res":
            g.res = addr["res"] + 4 * d.get("res_base", 0) if d.get("res") else None
        elif f == "out":
            g.out = addr["out"] + 4 * d.get("out_base", 0)
        elif f == "prec":
            g.prec = prec
        else:
            setattr(g, f, d.get(f, 0))
    return g


def run_device(K, _hip, d, t, prec):
    """The call on the device: the output buffer after it (host, float32), the plan of the call and the profile rows it
    recorded; every input buffer is checked unchanged."""
    dev = {k: torch.tensor(v).cuda() for k, v in t.items() if k != "w"}
    keep = {}
    if d["b"]["kind"] == WEIGHT:
        if "w_transposed" in d:   # a ConvTranspose1d phase: packed from the [C_in][N][k] weight as the models do
            s, r = d["w_transposed"]
            pw = K.pack_conv_weight(dev["wT"].reshape(d["wT_shape"]), transposed=True, stride=s, phase=r)
        else:
            pw = K.pack_conv_weight(torch.tensor(t["w"]).cuda())
        assert (pw.rows, pw.cpad, pw.kpad) == (d["N"], d["a"]["Cpad"], d["Kpad"]), (pw.rows, pw.cpad, pw.kpad)
        keep["wpack"] = pw.data
    addr = {k: v.data_ptr() for k, v in {**dev, **keep}.items()}
    args = gemm_args(d, addr, prec)
    plan = K.gemm_plan(args)
    torch.cuda.synchronize()
    _hip.profile_begin()
    try:
        K.gemm(args)
        torch.cuda.synchronize()
    finally:
        rows = _hip.profile_end()
    for k, v in dev.items():
        if k != "out":
            assert np.array_equal(v.cpu().numpy().view(np.int32), t[k].view(np.int32)), f"input {k} changed"
    return dev["out"].cpu().numpy(), plan, rows


# ------------------------------------------------------------------ the cases
def _randn(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).numpy().astype(np.float32)


def finish(d, t, seed, res_scale=1.0, prior_scale=1.0):
    """The output and residual buffers of a description: guard margins at both ends, sized by the strides so that every
    gap they leave is inside; sentinel-filled, or known random values where accumulate reads them."""
    last = dict(d, out_base=0, res_base=0, out_off=(d.get("out_step", 1) or 1) - 1)   # (one size for every phase)
    hi = int(out_index(last).max())
    d["out_base"] = GUARD
    n = GUARD + hi + 1 + GUARD
    t["out"] = _randn((n,), seed + 90, prior_scale) if d.get("accumulate") else np.full(n, SENTINEL, np.float32)
    if d.get("res"):
        hi = int(res_index(last).max())
        d["res_base"] = GUARD
        t["res"] = _randn((GUARD + hi + 1 + GUARD,), seed + 91, res_scale)
    return d, t


def conv_case(B, T, C, N, k=1, *, dil=1, pad=None, up=1, nct=False, a_pitch=0, rpb_gap=0, pro=None, shift=0.0,
              x_offset=0.0, bias=0.1, act=0, geglu=0, acc_scale=1.0, out_scale=1.0, accumulate=False, res=None,
              out_nct=False, out_step=1, out_off=0, tile_n=0, disable_window=0, seed=0, res_scale=1.0, w=None,
              w_scale=None, extra=None):
    """A conv / linear call in the argument form of kernels.conv1d: B clips of T output rows, C input channels (Cpad =
    round_up(C, 8)), packed weight [N][C][k]; channels-last input of row pitch C + a_pitch, or NCT.  pro: None, "affine"
    (per-clip scale / shift, pro_sb = C, + SiLU) or "ln" (row mean / rstd + one scale / shift).  res / out: channels-last
    with a pitch gap, or NCT (res="nct", out_nct)."""
    cpad = _rup(C, 8)
    T_in = T // 2 if up == 2 else T
    pad = (k - 1) * dil // 2 if pad is None else pad
    a = dict(kind=ACT, buf="a", off=0, T_in=T_in, C_in=C, Cpad=cpad, ksize=k, dil=dil, pad=pad, up=up, rows_per_batch=T)
    if nct:
        a.update(sb=C * T_in + rpb_gap, st=1, sc=T_in)
    else:
        a.update(sb=T_in * (C + a_pitch) + rpb_gap, st=C + a_pitch, sc=1)
    t = {"a": _randn((B * a["sb"],), seed + 1, 1.0, x_offset)}
    if pro == "affine":
        a.update(pro_scale="pro_scale", pro_shift="pro_shift", pro_sb=C, pro_act=1)
        t["pro_scale"] = _randn((B * C,), seed + 2, 0.2, 1.0)
        t["pro_shift"] = (np.sign(_randn((B * C,), seed + 3)) * shift + _randn((B * C,), seed + 4, 0.2)).astype(np.float32)
    if pro == "ln":
        a.update(pro_mean="pro_mean", pro_rstd="pro_rstd", pro_scale="pro_scale", pro_shift="pro_shift", pro_sb=0)
        x = t["a"].astype(np.float64).reshape(B, T_in, C + a_pitch)[:, :, :C]
        t["pro_mean"] = x.mean(-1).reshape(-1).astype(np.float32)
        t["pro_rstd"] = (1.0 / np.sqrt(x.var(-1) + 1e-5)).reshape(-1).astype(np.float32)
        t["pro_scale"] = _randn((C,), seed + 2, 0.2, 1.0)
        t["pro_shift"] = _randn((C,), seed + 3, 0.2)
    kpad = _rup(k * cpad, 32)
    t["w"] = _randn((N, C, k), seed + 5, w_scale or 1.0 / np.sqrt(C * k)) if w is None else w
    No = N // 2 if geglu else N
    To = T * out_step
    d = dict(M=B * T, N=N, Kpad=kpad, batch=1, zdiv=1, a=a, b=dict(kind=WEIGHT), acc_scale=acc_scale,
             out_scale=out_scale, act=act, geglu=geglu, accumulate=int(accumulate), out_rows_per_batch=T,
             out_step=out_step, out_off=out_off, tile_n=tile_n, disable_window=disable_window)
    if bias:
        d["bias"] = True
        t["bias"] = _randn((N,), seed + 6, bias)
    d.update(dict(o_sc=To + 2, o_st=1, o_sb=No * (To + 2) + 7) if out_nct else
             dict(o_st=No + 3, o_sc=1, o_sb=To * (No + 3) + 11))
    if res:
        d["res"] = True
        d.update(dict(r_sc=To + 6, r_st=1, r_sb=No * (To + 6) + 3) if res == "nct" else
                 dict(r_st=No + 5, r_sc=1, r_sb=To * (No + 5) + 13))
    if extra:
        d.update(extra)
    return finish(d, t, seed, res_scale)


def transpose_phase_case(B, T, Cin, N, k, s, r, seed):
    """One phase of F.conv_transpose1d(x, w, bias, stride=s, padding=(k - s)/2) on NCT input, as
    kernels.conv_transpose1d launches it: taps j = r + s*(Q - 1 - tap), output samples o + s*t."""
    Q, padding = k // s, (k - s) // 2
    wT = _randn((Cin, N, k), seed + 7, 1.0 / np.sqrt(Cin * Q))
    o = (r - padding) % s
    c = (o + padding - r) // s
    w = np.ascontiguousarray(np.stack([wT[:, :, r + s * (Q - 1 - tap)].T for tap in range(Q)], axis=-1))
    d, t = conv_case(B, T, Cin, N, Q, pad=Q - 1 - c, nct=True, out_nct=True, out_step=s, out_off=o, seed=seed, w=w,
                     extra=dict(w_transposed=(s, r), wT_shape=wT.shape))
    t["wT"] = wT.reshape(-1)
    return d, t


def qk_case(B, L, nh, dh, seed):
    """Q K^T per (clip, head) on a packed (B, L, 3*nh*dh) qkv buffer (B operand ACT, zdiv = nh), scaled by dh^-0.5,
    plus a residual laid out (nh, B, L, L + 5); output (B, nh, L, round_up(L, 8))."""
    I, Lp = nh * dh, _rup(L, 8)
    a = dict(kind=ACT, buf="a", off=0, sb=0, st=3 * I, sc=1, T_in=L, C_in=dh, Cpad=dh, ksize=1, dil=1, pad=0, up=1,
             rows_per_batch=L, zs1=L * 3 * I, zs2=dh)
    t = {"a": _randn((B * L * 3 * I,), seed + 1)}
    d = dict(M=L, N=L, Kpad=_rup(dh, 32), batch=B * nh, zdiv=nh, a=a, b=dict(a, off=I), acc_scale=dh ** -0.5,
             out_scale=1.0, o_sb=0, o_st=Lp, o_sc=1, o_zs1=nh * L * Lp + 16, o_zs2=L * Lp, out_rows_per_batch=L,
             out_step=1, res=True, r_sb=0, r_st=L + 5, r_sc=1, r_zs1=L * (L + 5), r_zs2=B * L * (L + 5))
    return finish(d, t, seed)


def pv_case(B, L, nh, dh, seed):
    """P V per (clip, head): P (B, nh, L, round_up(L, 8)) with zero pad columns, V read from the packed qkv buffer
    (B operand ACT_T, st = 3*I, zs2 = dh), accumulated into a head-interleaved (B, L, nh*dh) output (with a gap between the clips)."""
    I, Lp = nh * dh, _rup(L, 8)
    p = np.abs(_randn((B * nh, L, Lp), seed + 1, 0.2))
    p[:, :, L:] = 0.0
    a = dict(kind=ACT, buf="a", off=0, sb=0, st=Lp, sc=1, T_in=L, C_in=Lp, Cpad=Lp, ksize=1, dil=1, pad=0, up=1,
             rows_per_batch=L, zs1=nh * L * Lp, zs2=L * Lp)
    b = dict(kind=ACT_T, buf="qkv", off=2 * I, st=3 * I, sc=1, T_in=L, rows=dh, zs1=L * 3 * I, zs2=dh)
    t = {"a": p.reshape(-1), "qkv": _randn((B * L * 3 * I,), seed + 2)}
    d = dict(M=L, N=dh, Kpad=_rup(Lp, 32), batch=B * nh, zdiv=nh, a=a, b=b, acc_scale=1.0, out_scale=1.0, accumulate=1,
             o_sb=0, o_st=I, o_sc=1, o_zs1=L * I + 24, o_zs2=dh, out_rows_per_batch=L, out_step=1)
    return finish(d, t, seed)


G, CV, SK = "gemm_kernel<{}, {}, {p}>", "conv_kernel<{}, {p}, {}>", "gemm_skinny_kernel<{p}>"
T64, T256_32, T256_64, T128 = "64, 32, 4, 1", "256, 32, 4, 1", "256, 64, 4, 1", "128, 128, 2, 2"
C64, C128 = "128, 64, 4, 1", "128, 128, 2, 2"
NOSKINNY = {"ALCM_GEMM_SKINNY": 0}


def _case(family, name, kernel, make, sw=None, **flags):
    return dict(family=family, name=name, kernel="alcm::" + kernel, make=make, sw=sw or {}, **flags)


def _cases():
    P = functools.partial
    c = []
    # 1: NCT input on the scalar loader, k = 5, dil 2, pad 4; NCT output + NCT residual, GELU (erf)
    for N, tile, sw in ((24, T64, None), (24, T256_32, NOSKINNY), (40, T256_64, None), (140, T128, None)):
        c.append(_case(1, f"nct_k5d2_N{N}" + ("_noskinny" if sw else ""), G.format(tile, "false, 0", p="{p}"),
                       P(conv_case, 3, 45, 20, N, 5, dil=2, nct=True, act=2, res="nct", out_nct=True, seed=100 + N), sw))
    # 2: channels-last vector loader, k = 3, Cpad 40: every epilogue stage at once
    for N, act, tile, sw in ((20, 1, T64, None), (20, 1, T256_32, NOSKINNY), (48, 3, T256_64, None),
                             (136, 4, T128, None)):
        c.append(_case(2, f"cl_k3_N{N}_act{act}" + ("_noskinny" if sw else ""), G.format(tile, "true, 0", p="{p}"),
                       P(conv_case, 2, 150, 40, N, 3, act=act, acc_scale=0.7, out_scale=0.5, accumulate=True, res="cl",
                         bias=0.5, seed=200 + N), sw))
    # 3: per-clip affine + SiLU prologue, |shift| ~ 3, on the nearest-x2 upsampled input
    c.append(_case(3, "affine_up2_C40", G.format(T128, "true, 0", p="{p}"),
                   P(conv_case, 2, 140, 40, 136, 3, up=2, pro="affine", shift=3.0, res="cl", seed=300), edge=True))
    for N, tile in ((64, C64), (136, C128)):
        c.append(_case(3, f"affine_up2_C64_N{N}", CV.format(tile, "true", p="{p}"),
                       P(conv_case, 2, 140, 64, N, 3, up=2, pro="affine", shift=3.0, res="cl", seed=310 + N), edge=True))
    # 4: LayerNorm prologue on rows of mean ~ 5 std, k = 9; (b) pins that the scalar loader's lanes >= C_in, which
    # hold (0 - mean) * rstd, meet a zero weight
    c.append(_case(4, "ln_k9_C64", CV.format(C128, "true", p="{p}"),
                   P(conv_case, 2, 130, 64, 136, 9, pro="ln", x_offset=5.0, seed=400), edge=True, window_pair=True))
    c.append(_case(4, "ln_k9_C20", G.format(T256_64, "false, 0", p="{p}"),
                   P(conv_case, 2, 130, 20, 40, 9, pro="ln", x_offset=5.0, seed=410), edge=True, window_pair=True))
    # 5: the window conv without prologue, halo 50 and 18, natural and forced N tiles
    for C, k, dil, N, tn, tile in ((32, 11, 5, 64, 0, C64), (96, 7, 3, 192, 0, C64), (32, 11, 5, 136, 0, C128),
                                   (96, 7, 3, 136, 64, C64), (32, 11, 5, 64, 128, C128)):
        c.append(_case(5, f"window_C{C}_k{k}_N{N}_tile{tn}", CV.format(tile, "false", p="{p}"),
                       P(conv_case, 2, 130, C, N, k, dil=dil, accumulate=True, out_scale=1.0 / 3.0, res="cl",
                         tile_n=tn, seed=500 + N + tn + k)))
    # 6: GEGLU 1 (erf) and 2 (tanh); act = 1 must be ignored; a gate pair ends every full tile
    for gg in (1, 2):
        ep = dict(geglu=gg, act=1, res="cl", out_scale=0.75, accumulate=True, w_scale=None, res_scale=0.3)
        c.append(_case(6, f"geglu{gg}_lin_N264", G.format(T128, "true, 0", p="{p}"),
                       P(conv_case, 1, 150, 72, 264, 1, seed=600 + gg, **ep)))
        c.append(_case(6, f"geglu{gg}_lin_N40", G.format(T256_64, "true, 0", p="{p}"),
                       P(conv_case, 1, 300, 72, 40, 1, seed=610 + gg, **ep)))
        c.append(_case(6, f"geglu{gg}_k9_N128", CV.format(C64, "false", p="{p}"),
                       P(conv_case, 2, 130, 64, 128, 9, tile_n=64, seed=620 + gg, **ep)))
        c.append(_case(6, f"geglu{gg}_k9_N264", CV.format(C128, "false", p="{p}"),
                       P(conv_case, 2, 130, 64, 264, 9, seed=630 + gg, **ep)))
    # 7: ConvTranspose1d phases (k = 8, s = 4 and k = 4, s = 2: Q = 2), each launched alone
    for k, s in ((8, 4), (4, 2)):
        for r in range(s):
            c.append(_case(7, f"convT_k{k}_s{s}_phase{r}", G.format(T64, "false, 0", p="{p}"),
                           P(transpose_phase_case, 2, 37, 48, 24, k, s, r, 700 + k), convT=(k, s, r)))
    # 8 / 9: the attention products on a packed qkv buffer, zdiv = nh = 3
    for dh in (72, 40):
        for L in (40, 77, 130):
            c.append(_case(8, f"qk_dh{dh}_L{L}", G.format(T256_64 if L <= 64 else T128, "true, 1", p="{p}"),
                           P(qk_case, 2, L, 3, dh, 800 + dh + L), pitch=True))
            c.append(_case(9, f"pv_dh{dh}_L{L}", G.format(T256_64 if dh <= 64 else T128, "true, 2", p="{p}"),
                           P(pv_case, 2, L, 3, dh, 900 + dh + L)))
    # 10: the skinny kernel and the MFMA tiles it replaces; row pitch > C_in; 32-row blocks across two clips
    for B, T, C, N, act, tile in ((1, 1, 36, 20, 0, T256_32 + ", false"), (1, 33, 256, 72, 1, T128 + ", true"),
                                  (2, 35, 768, 20, 2, T256_32 + ", true"), (1, 33, 36, 72, 3, T128 + ", false"),
                                  (2, 35, 256, 72, 4, T128 + ", true"), (1, 1, 768, 72, 1, T128 + ", true")):
        mk = P(conv_case, B, T, C, N, 1, a_pitch=4, rpb_gap=8, act=act, res="cl", out_scale=0.6, accumulate=True,
               seed=1000 + C + N + T)
        c.append(_case(10, f"skinny_M{B * T}_C{C}_N{N}_act{act}", SK, mk, skinny_pair=True))
        c.append(_case(10, f"skinny_M{B * T}_C{C}_N{N}_act{act}_noskinny", G.format(tile, "0", p="{p}"), mk, NOSKINNY))
    return c


CASES = _cases()
FAMILIES = sorted({c["family"] for c in CASES})


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(d, t) of a case, built once; the buffers are read-only."""
    c = next(c for c in CASES if c["name"] == name)
    d, t = c["make"]()
    for v in t.values():
        v.setflags(write=False)
    return d, t


@functools.lru_cache(maxsize=None)
def reference(name, round_operands=None):
    return evaluate(*case_data(name), round_operands=round_operands)


def mutant_tolerance(d):
    """The loosest bound the GPU test applies to a case at every precision: without a prologue each precision is also
    compared with the rounded-operand reference at SPLIT_TOL; with one, the per-precision bounds (bf16 the widest)."""
    return BF16_TOL if has_prologue(d) else SPLIT_TOL
