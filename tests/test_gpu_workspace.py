"""The workspace contract (include/audiolcm_hip.h, at the workspace queries): a forward reads only what it wrote.

Every model entry point carves a caller workspace into buffers that are reused on written-down rules (alcm_models.cpp:
the DiT's w.g / w.o / w.S / w.kp, the comment above VocWs), and operand planes wider than their channel count rely on
zeros their producer wrote.  With the wrappers' own cached torch.empty workspaces a read-before-write meets what the
same forward left there one run earlier, and a write past a buffer lands in its neighbour.  Here every forward takes
its workspace from tests/_wsguard.py instead: guard | exactly the queried bytes | guard.

Per case (the launch table of test_gpu_model_launches.py, whose cases reach every branch of the DiT, VAE, text and mel
forwards, and a subset of _windowed.VOC_CASES / HANDOFF_CASES for the vocoder, with the resblock streams on and off):

  (a) a reference run on a 0x00 workspace: finite, and within the whole-tensor bar the project states for the model and
      policy (BARS) against the float64 oracle on the very inputs the wrapper handed to the C entry.  Where no bar is
      stated (bf16 text / encoder / mel, the cut-down configurations) the error is printed and only finiteness asserted;
  (b) runs on 0xFF (NaN), on 0x7F (3.4e38 as fp32 / bf16, NaN as fp16) and on what another case of the same model left at
      the same base (`stale`): every output bit-identical to (a), guards and inputs untouched.  A difference under 0xFF
      alone is a stale lane times an exact zero; under both fills, a read-before-write;
  (c) once per model kind: half the queried size is refused with ALCM_E_WORKSPACE and the output keeps every byte.

A DiT case runs embed_context before its forward_cached: that call is guarded as a call of its own, with its own
arena, oracle line and bit comparison.  The forwards are deterministic (fixed order, no atomics), so bit identity needs
no tolerance.  The clips the B = 32 DiT case compares with the oracle are four of the 32 (0.5 s of float64 each; the
clips do not mix); every clip is in the bit comparison.

Below the models the same holds for the K-split scratch at exactly the planned size, for every producer of operand
planes (what the header says is written is written, padding as the header says, nothing else) and for
alcm_opconv_dense on planes whose padding channels hold poison.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _windowed as Wn
import _wsguard as G
import test_gpu_model_launches as ML
import test_gpu_voc_windows as VW
from conftest import golden, rel_l2

from audiolcm_amd import _hip, recipe
from audiolcm_amd import kernels as K
from audiolcm_amd._hip import check, lib, stream_handle
from oracle import alcm_oracle as O
from test_vocplan import switches

pytestmark = pytest.mark.gpu

ALCM_E_WORKSPACE = -4
# whole-tensor relative L2 the project states per model and policy: test_gpu_models.py (DiT, VAE decode, BigVGAN),
# test_gpu_text.py, test_gpu_audio_in.py (VAE encode, log-mel)
BARS = {"dit": dict(split=1e-4, mixed=5e-4, bf16=2e-2),
        "vae_decode": dict(split=1e-4, mixed=1e-3, bf16=3e-2),
        "vae_encode": dict(split=1e-4, mixed=2e-3),
        "text": dict(split=1e-4, mixed=3e-3),
        "mel": dict(split=1e-5)}
VOC_BAR = 1e-3

_W64 = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle_weights():
    yield
    _W64.clear()  # the text towers in float64 are 3.6 GB


def _w64(kind, cfg=()):
    if (kind, cfg) not in _W64:
        c = dict(cfg)
        if kind == "dit":
            W = recipe.dit_state(0, recipe.DiTConfig(**c))
        elif kind == "vae":
            W = {**recipe.vae_state(0), **recipe.vae_encoder_state(0)}
        else:
            W = recipe.text_state(0, recipe.TextConfig(**c))
        _W64[(kind, cfg)] = {k: v.double() for k, v in W.items()}
    return _W64[(kind, cfg)]


def _oracle(case, calls):
    """{call kind: (rows of the output compared, float64 reference of those rows)} from the inputs the calls got."""
    Wn._threads()
    cfg = tuple(sorted(case.get("cfg", {}).items()))
    inp = {k: [t.cpu() for t, _ in c.inputs] for k, c in calls.items()}
    B = case["B"]
    with torch.no_grad():
        if case["model"] == "dit":
            W, dc = _w64("dit", cfg), recipe.DiTConfig(**dict(cfg))
            sel = list(range(B)) if B <= 4 else [0, B // 3, 2 * B // 3, B - 1]
            ctx = inp["ctx"][0][sel].double()
            x, t = inp["fwd"][0][sel].double(), inp["fwd"][1][sel]
            wc = inp["fwd"][3][sel].double() if len(inp["fwd"]) > 3 else None
            pos = W["pos_emb.weight"][1:1 + dc.ctx_tokens]
            return {"ctx": (sel, O.dit_context_embed(W, ctx) + pos),
                    "fwd": (sel, O.dit_forward(W, x, t, ctx, wc, heads=dc.num_heads, depth=dc.depth))}
        if case["model"] == "vae_decode":
            return {"dec": (slice(None), O.vae_decode(_w64("vae"), inp["dec"][0].double()))}
        if case["model"] == "vae_encode":
            return {"enc": (slice(None), O.vae_encode_moments(_w64("vae"), inp["enc"][0].double()))}
        if case["model"] == "text":
            W, tc = _w64("text", cfg), recipe.TextConfig(**dict(cfg))
            a, b = inp["text"]
            uniq, inv = torch.unique(torch.cat([a, b], 1), dim=0, return_inverse=True)  # B = 32 repeats two prompts
            L = a.shape[1]
            ref = O.text_encode(W, uniq[:, :L], uniq[:, L:], tc.b_layers, tc.b_heads, tc.t_layers, tc.t_heads)
            return {"text": (slice(None), ref[inv])}
        basis = ML._model("mel", ()).mel_basis.double()
        return {"mel": (slice(None), O.mel_spectrogram(inp["mel"][0].double(), basis))}


def _assert_same(tag, got, ref):
    assert got.keys() == ref.keys(), (tag, sorted(got), sorted(ref))
    for kind in ref:
        a, b = got[kind], ref[kind]
        if G.same_bits(a, b):
            continue
        bad = (a.view(torch.int32) != b.view(torch.int32)).flatten()
        first = int(torch.nonzero(bad)[0])
        pytest.fail(f"{tag}: output of `{kind}` differs in {int(bad.sum())} of {bad.numel()} elements, first at flat "
                    f"index {first} ({float(a.flatten()[first])!r} for {float(b.flatten()[first])!r}); "
                    f"{int((~torch.isfinite(a)).sum())} not finite")


# ---------------------------------------------------------------------------------------------- DiT, VAE, text, mel
def _forward(cid, **kw):
    """One run_case of the launch table under a guard -> ({call kind: a copy of its output}, the guard), with the
    guards and the inputs of every call checked."""
    with G.guarded(**kw) as g:
        ML.run_case(ML.CASES[cid])
    torch.cuda.synchronize()
    g.check()
    _used(g)
    outs = {c.kind: c.out.clone() for c in g.calls}
    assert len(outs) == len(g.calls)
    return outs, g


def _used(g):
    """The forward did work in the guard's view (Call.inputs has checked that the C entry was given it)."""
    for c in g.calls:
        assert c.nbytes > 0 and bool((c.arena.ws[:c.nbytes] != c.arena.pattern).any()), c.kind


def _partner(cid):
    """The next case of the same model kind, in sorted order and cyclically, that differs in shape or policy."""
    key = lambda c: (c["B"], c["T"], c["policy"], tuple(sorted(c.get("cfg", {}).items())))
    ids = sorted(i for i in ML.CASES if ML.CASES[i]["model"] == ML.CASES[cid]["model"])
    at = ids.index(cid)
    for other in ids[at + 1:] + ids[:at]:
        if key(ML.CASES[other]) != key(ML.CASES[cid]):
            return other
    raise AssertionError(cid)


@pytest.mark.parametrize("cid", sorted(ML.CASES))
def test_model_forward_reads_only_what_it_wrote(cid):
    case = ML.CASES[cid]
    ref, g0 = _forward(cid, pattern=G.ZERO)
    bar = None if "cfg" in case else BARS[case["model"]].get(case["policy"])
    oracle = _oracle(case, {c.kind: c for c in g0.calls})
    assert oracle.keys() == ref.keys()
    for kind, (rows, want) in oracle.items():
        got = ref[kind]
        assert torch.isfinite(got).all(), (cid, kind)
        err = rel_l2(got[rows].cpu().numpy(), want.numpy())
        stated = bar if kind != "ctx" else None  # the bars are stated for the forwards' outputs
        print(f"reference {cid} {kind}: rel-L2 {err:.2e} (bar {stated})")
        assert np.isfinite(err) and (stated is None or err < stated), (cid, kind, err, stated)
    for pattern in G.POISONS:
        got, _ = _forward(cid, pattern=pattern)
        _assert_same(f"{cid} on {pattern:#04x}", got, ref)
    partner = _partner(cid)
    _, gp = _forward(partner, pattern=G.NAN, at_least=g0.sizes())
    got, gs = _forward(cid, arenas=gp.arenas())
    assert gs.sizes() == g0.sizes()
    _assert_same(f"{cid} on what {partner} left", got, ref)


# ---------------------------------------------------------------------------------------------- BigVGAN
def _voc_entries():
    e = [("tail", pol, B, M, ()) for pol in ("split", "mixed") for B, M in ((1, 1), (3, 33), (3, 129))]
    e += [("mid", pol, 3, 33, ()) for pol in ("split", "mixed")] + [("mid", "mixed", 4, 256, ())]
    e += [(name, pol, B, M, ()) for name, B, M in (("head", 2, 129), ("full", 2, 5)) for pol in ("split", "mixed")]
    assert all(c[:4] in Wn.VOC_CASES for c in e)
    return e + [c + ((("ALCM_WCONV3", 1),),) for c in Wn.HANDOFF_CASES]


VOC = _voc_entries()
_voc_id = lambda e: Wn.case_id(e[:4]) + ("-handoff" if e[4] else "")


def _voc_forward(entry, streams, **kw):
    name, policy, B, M, knobs = entry
    cfg, scale = Wn.VOC_CONFIGS[name]
    voc = VW._model(name)
    voc.set_resblock_streams(streams)
    try:
        with G.guarded(**kw) as g:
            wav, rows = VW.run(name, policy, Wn.voc_input(cfg, scale, B, M), dict(knobs))
    finally:
        voc.set_resblock_streams(True)
    torch.cuda.synchronize()  # the chains run on auxiliary streams
    g.check()
    _used(g)
    assert [c.kind for c in g.calls] == ["voc"]
    return {"voc": wav}, rows, g


def _voc_partner(entry):
    ids = sorted(e for e in VOC if e[0] == entry[0])
    at = ids.index(entry)
    for other in ids[at + 1:] + ids[:at]:
        if other[1:4] != entry[1:4]:
            return other
    raise AssertionError(entry)


@pytest.mark.parametrize("streams", [True, False], ids=["streams", "serial"])
@pytest.mark.parametrize("entry", VOC, ids=_voc_id)
def test_vocoder_forward_reads_only_what_it_wrote(entry, streams):
    name, policy, B, M, knobs = entry
    tag = f"{_voc_id(entry)}-{'streams' if streams else 'serial'}"
    ref, rows, g0 = _voc_forward(entry, streams, pattern=G.ZERO)
    assert (VW.SUM_ONE_LAUNCH in rows) == bool(knobs), sorted(rows)
    mel, exact = Wn.voc_exact(name, B, M)
    assert torch.equal(mel, g0.calls[0].inputs[0][0].cpu()) and torch.isfinite(ref["voc"]).all()
    err = rel_l2(ref["voc"].cpu().numpy(), exact)
    print(f"reference {tag}: rel-L2 {err:.2e} (bar {VOC_BAR})")
    assert err < VOC_BAR
    for pattern in G.POISONS:
        got, _, _ = _voc_forward(entry, streams, pattern=pattern)
        _assert_same(f"{tag} on {pattern:#04x}", got, ref)
    partner = _voc_partner(entry)
    _, _, gp = _voc_forward(partner, streams, pattern=G.NAN, at_least=g0.sizes())
    got, _, gs = _voc_forward(entry, streams, arenas=gp.arenas())
    assert gs.sizes() == g0.sizes()
    _assert_same(f"{tag} on what {_voc_id(partner)} left", got, ref)


# ---------------------------------------------------------------------------------------------- refusal
def _entry(kind):
    """-> (queried bytes, call(ws address, ws bytes) -> return code, the output tensor) of one C entry per model kind,
    at a launch-table shape."""
    L, s = lib(), stream_handle()
    rnd = lambda *shape: torch.randn(*shape, generator=torch.Generator().manual_seed(7)).cuda()
    p = _hip.ptr
    if kind == "dit":
        m, B, T = ML._model("dit", ()), 2, 40
        x, t, cemb, out = rnd(B, 20, T), torch.tensor([999, 499]).cuda(), rnd(B, 154, 576), rnd(B, 20, T)
        return (L.alcm_dit_workspace_bytes(m._handle, B, T), out, (x, t, cemb),
                lambda w, n: L.alcm_dit_forward(m._handle, p(x), p(t), p(cemb), None, p(out), B, T, w, n, s))
    if kind == "vae":
        m, B, T = ML._model("vae", ()), 2, 24
        z, out = rnd(B, 20, T), rnd(B, 80, 2 * T)
        return (L.alcm_vae_workspace_bytes(m._handle, B, T), out, (z,),
                lambda w, n: L.alcm_vae_decode(m._handle, p(z), 1.0, p(out), B, T, w, n, s))
    if kind == "bigvgan":
        m, B, M = VW._model("tail"), 3, 33
        mel = Wn.voc_input(Wn.VOC_CONFIGS["tail"][0], 0.2, B, M).cuda()
        out = rnd(B, 1, M * m.cfg.hop)
        return (L.alcm_bigvgan_workspace_bytes(m._handle, B, M), out, (mel,),
                lambda w, n: L.alcm_bigvgan_forward(m._handle, p(mel), p(out), B, M, w, n, s))
    if kind == "text":
        m, B, Lt = ML._model("text", ()), 1, 8
        g = golden("text_B2_L77.npz")
        a, b = (torch.from_numpy(g[k])[:B, :Lt].contiguous().cuda() for k in ("clap_ids", "t5_ids"))
        out = rnd(B, 2 * Lt, m.cfg.p_out)
        return (L.alcm_text_workspace_bytes(m._handle, B, Lt), out, (a, b),
                lambda w, n: L.alcm_text_encode(m._handle, p(a), p(b), p(out), B, Lt, w, n, s))
    m, B, n = ML._model("mel", ()), 2, 20 * 256
    wav, out = 0.1 * rnd(B, n), rnd(B, m.num_mels, n // m.hop_size)
    return (L.alcm_mel_workspace_bytes(m._handle, B, n), out, (wav,),
            lambda w, nb: L.alcm_mel_spectrogram(m._handle, p(wav), p(out), B, n, w, nb, s))


@pytest.mark.parametrize("kind", ["dit", "vae", "bigvgan", "text", "mel"])
def test_half_the_queried_workspace_is_refused(kind):
    nbytes, out, inputs, call = _entry(kind)
    assert nbytes > 512
    out.view(torch.uint8).fill_(G.NAN)
    before = [t.clone() for t in inputs]
    ar = G.arena(nbytes // 2, G.NAN)
    rc = call(ar.ws.data_ptr(), ar.ws.numel())
    torch.cuda.synchronize()
    assert rc == ALCM_E_WORKSPACE, (rc, lib().alcm_last_error().decode())
    assert bool((out.view(torch.uint8) == G.NAN).all()) and bool((ar.ws == G.NAN).all())
    ar.check_guards()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before))


# ---------------------------------------------------------------------------------------------- below the models
def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _filters():
    f = recipe.kaiser_sinc_filter1d(0.25, 0.3, 12).detach().reshape(-1).float().cpu().contiguous()
    return f


def _conv_args(pl, C_real, packed, N, k, dil, prec, bias):
    """alcm_opconv_args of a same-length conv on planes pl (NP, B, T, Cp), as kernels.opconv fills them."""
    _, B, T, Cp = pl.shape
    a = _hip.OpConvArgs()
    a.a, a.a_lo_off, a.B, a.T, a.C, a.Cp = pl.data_ptr(), B * T * Cp, B, T, C_real, Cp
    a.ksize, a.dil, a.pad = k, dil, (k - 1) * dil // 2
    a.w, a.w_lo_off, a.kpad, a.N = packed.data.data_ptr(), packed.lo_off, packed.kpad, N
    a.bias, a.out_scale, a.prec = _hip.ptr(bias), 1.0, int(prec)
    return a


def _planes(ar, shape):
    """A copy of an arena's workspace as int16 planes."""
    return ar.ws.clone().view(torch.int16).view(shape)


def _poison16(pattern):
    return torch.tensor([pattern, pattern], dtype=torch.uint8).view(torch.int16).item()


# B, T, C, N, k, accumulate: test_wconv3_ksplit_underfilled's and test_wconv2_ksplit_text_linears' shapes (test_gpu_ops.py)
KSPLIT = [(4, 467, 2304, 576, 9, False), (8, 467, 2304, 576, 9, True),
          (1, 2464, 1024, 1024, 1, False), (1, 2464, 3072, 768, 1, False), (1, 2464, 768, 768, 1, False)]


@pytest.mark.parametrize("B,T,Cin,N,k,acc", KSPLIT)
def test_ksplit_scratch_of_exactly_the_planned_size(B, T, Cin, N, k, acc):
    """ksplit_ws holds exactly ksplit * B * T * N floats (ksplit from the planner) inside an arena: the output does
    not depend on what the scratch held, nothing next to it is written, and the value is F.conv1d's on the fp16
    operands within the 1e-5 of the tests whose shapes these are."""
    x, w, bias = _r((B, T, Cin), 170, 0.5), _r((N, Cin, k), 171, 1.0 / np.sqrt(Cin * k)), _r((N,), 172, 0.05)
    r, o0 = _r((B, T, N), 173), _r((B, T, N), 174)
    pl, pw = K.operand_planes(x.cuda(), 2), K.pack_conv_weight(w.cuda())
    db, dr = bias.cuda(), r.cuda()
    a = _conv_args(pl, Cin, pw, N, k, 1, 2, db)
    a.res, a.out_scale, a.accumulate = dr.data_ptr(), 0.5, int(acc)
    a.out, a.ksplit_ws, a.ksplit_ws_floats = dr.data_ptr(), pl.data_ptr(), 8 * B * T * N  # (planning dereferences nothing)
    ks = K.conv_plan(a)[0]["ksplit"]
    assert ks > 1
    need = ks * B * T * N
    outs = []
    for pattern in (G.ZERO,) + G.POISONS:
        ar = G.arena(4 * need, pattern)
        out = o0.clone().cuda() if acc else torch.empty((B, T, N), device="cuda")
        a.out, a.ksplit_ws, a.ksplit_ws_floats = out.data_ptr(), ar.ws.data_ptr(), need
        plan = K.conv_plan(a)[0]
        assert plan["ksplit"] == ks and "ksplit_reduce" in plan["name"], plan
        check(lib().alcm_opconv(C.byref(a), stream_handle()), "opconv")
        torch.cuda.synchronize()
        ar.check_guards()
        outs.append(out)
    assert G.same_bits(outs[0], outs[1]), "the K-split output depends on its scratch (0xFF)"
    assert G.same_bits(outs[0], outs[2]), "the K-split output depends on its scratch (0x7F)"
    ref = (F.conv1d(x.half().float().permute(0, 2, 1), w.half().float(), bias, padding=k // 2).permute(0, 2, 1) + r) * 0.5
    err = rel_l2(outs[0].cpu().numpy(), (ref + o0 if acc else ref).numpy())
    print(f"ksplit B{B} T{T} C{Cin} N{N} k{k}: {ks} parts, vs F.conv1d {err:.2e}")
    assert err < 1e-5


def _act_params(Cn, nset, seed):
    return [tuple(t.contiguous() for t in K.snake_params(_r((Cn,), seed + 2 * i, 0.3).cuda(),
                                                         _r((Cn,), seed + 2 * i + 1, 0.3).cuda()))
            for i in range(nset)]


def _act_run(x, x_is_f16, params, B, T, Cn, Cp, prec, pattern, f):
    """alcm_activation1d_planes into one exactly-sized arena per set -> (plan, [planes (NP, B, T, Cp)])."""
    npl = 2 if prec == _hip.PREC_SPLIT else 1
    ars = [G.arena(npl * B * T * Cp * 2, pattern) for _ in params]
    a = _hip.ActArgs()
    a.x, a.x_is_f16, a.nset, a.B, a.T, a.C, a.Cp, a.prec = x.data_ptr(), int(x_is_f16), len(params), B, T, Cn, Cp, prec
    for i, (ae, ib) in enumerate(params):
        a.y[i], a.alpha_exp[i], a.inv_beta[i] = ars[i].ws.data_ptr(), ae.data_ptr(), ib.data_ptr()
    a.up_filter = a.down_filter = f.data_ptr()
    plan = K.act_plan(a)
    check(lib().alcm_activation1d_planes(C.byref(a), stream_handle()), "activation1d_planes")
    torch.cuda.synchronize()
    for ar in ars:
        ar.check_guards()
    return plan, [_planes(ar, (npl, B, T, Cp)) for ar in ars]


def _single_act(x, x_is_f16, ae, ib, B, T, Cn, Cp, prec, f):
    """One nset = 1 call into a torch.empty plane, as the kernels.py wrappers make it."""
    npl = 2 if prec == _hip.PREC_SPLIT else 1
    y = torch.empty((npl, B, T, Cp), dtype=torch.int16, device="cuda")
    fn = lib().alcm_activation1d_op_f16in if x_is_f16 else lib().alcm_activation1d_op
    check(fn(x.data_ptr(), y.data_ptr(), B, T, Cn, Cp, ae.data_ptr(), ib.data_ptr(), f.data_ptr(), f.data_ptr(), prec,
             stream_handle()), "activation1d_op")
    return y


@pytest.mark.parametrize("nset", [1, 3])
@pytest.mark.parametrize("prec", [1, 2, 0, 3])
@pytest.mark.parametrize("Cn,Cp,mfma", [(24, 32, 1), (48, 64, 1), (96, 96, 1), (96, 128, 1), (192, 192, 1),
                                        (192, 192, 0), (192, 224, 1)])
def test_activation_planes_are_written_whole(Cn, Cp, mfma, prec, nset):
    """alcm_activation1d_planes into 0xFF: every element of [B][T][Cp] of every plane is written (the arena's bytes
    equal those of a run into 0x00), channels >= C as 0, the SPLIT lo plane B*T*Cp behind the hi plane, nothing outside;
    and the planes are those of nset single calls bit for bit.  The planner names the kernel: the matrix-core ones at
    C = 192 = Cp in fp16, the cooperative one elsewhere and with ALCM_ACT_MFMA=0."""
    B, f = 2, _filters()
    for T in (3, 37):
        x = _r((B, T, Cn), 300 + T, 1.2).cuda()
        params = _act_params(Cn, nset, 310)
        with switches({"ALCM_ACT_MFMA": mfma}):
            _, zero = _act_run(x, False, params, B, T, Cn, Cp, prec, G.ZERO, f)
            plan, got = _act_run(x, False, params, B, T, Cn, Cp, prec, G.NAN, f)
            single = [_single_act(x, False, ae, ib, B, T, Cn, Cp, prec, f) for ae, ib in params]
        want = ("mfma" if nset == 1 else "mfma3") if (mfma and prec == 2 and Cn == Cp == 192) else "coop"
        assert plan["kernel"] == want and plan["nset"] == nset, plan
        for i in range(nset):
            assert torch.equal(got[i], zero[i]), f"set {i}, T {T}: an element of the plane was not written"
            assert torch.equal(got[i], single[i]), f"set {i}, T {T}: differs from the single call"
            assert bool((got[i][..., Cn:] == 0).all())
            dec = got[i][..., :Cn].view(torch.float16 if prec in (2, 3) else torch.bfloat16)
            assert torch.isfinite(dec.float()).all() and bool((dec.float().abs().amax((0, 1, 2)) > 0).all())


@pytest.mark.parametrize("Cn", [192, 256])
def test_activation_planes_from_an_fp16_plane_are_written_whole(Cn):
    """The x_is_f16 form (an fp16 plane in, C % 64 == 0, Cp == C, the matrix-core kernel)."""
    B, f = 2, _filters()
    for T in (3, 37):
        x16 = _r((B, T, Cn), 320 + T, 1.2).half().view(torch.int16).cuda()
        params = _act_params(Cn, 1, 330)
        _, zero = _act_run(x16, True, params, B, T, Cn, Cn, 2, G.ZERO, f)
        plan, got = _act_run(x16, True, params, B, T, Cn, Cn, 2, G.NAN, f)
        single = _single_act(x16, True, *params[0], B, T, Cn, Cn, 2, f)
        assert plan["kernel"] == "mfma" and plan["in16"] == 1, plan
        assert torch.equal(got[0], zero[0]) and torch.equal(got[0], single)
        assert torch.isfinite(got[0].view(torch.float16).float()).all()


# C = N, T, k, dil, prec, dense: N = 24 -> Cp' = 32 and N = 48 -> 64 on every precision alcm_opconv takes them at, and
# the resident-weight kernels of alcm_opconv_dense
ACT_EPILOGUE = [(24, 37, 3, 1, 2, False), (24, 300, 11, 5, 3, False), (48, 37, 7, 1, 0, False),
                (48, 300, 7, 3, 3, False), (48, 37, 3, 1, 1, False), (24, 300, 3, 1, 1, False),
                (24, 37, 3, 1, 3, True), (24, 300, 11, 5, 2, True), (48, 37, 11, 5, 3, True), (48, 300, 3, 1, 2, True)]
GAP = 128  # elements between the hi plane's end and the lo plane: act_plane_lo_off is the caller's to choose


@pytest.mark.parametrize("Cn,T,k,dil,prec,dense", ACT_EPILOGUE)
@pytest.mark.parametrize("res", [False, True], ids=["conv1", "conv2"])
def test_conv_activation_epilogue_writes_its_planes(Cn, T, k, dil, prec, dense, res):
    """The fused Activation1d epilogue into 0xFF (and 0x7F): alcm_opconv writes every element of [B][T][Cp'], channels
    >= N as 0, the SPLIT lo plane exactly act_plane_lo_off behind the hi plane and nothing between the two;
    alcm_opconv_dense writes channels < N and leaves channels >= N as they were.  The fp32 output, in an arena of its
    own, and the planes equal the kernels.py call's bit for bit."""
    B, N, f = 2, Cn, recipe.kaiser_sinc_filter1d(0.25, 0.3, 12)
    Cpo = K._round_up(N, 32)
    npl = 2 if prec == _hip.PREC_SPLIT else 1
    lo_off = B * T * Cpo + GAP
    x, w, bias = _r((B, T, Cn), 90), _r((N, Cn, k), 91, 0.7 / np.sqrt(Cn * k)).cuda(), _r((N,), 92, 0.05).cuda()
    r = _r((B, T, N), 93).cuda() if res else None
    al, bt = _r((N,), 94, 0.3).cuda(), _r((N,), 95, 0.3).cuda()
    pl = K.operand_planes(x.cuda(), prec)
    Cp = pl.shape[-1]
    packed = K.pack_conv_weight(w if dense else F.pad(w, (0, 0, 0, Cp - Cn)).contiguous())
    y_ref, pl_ref = K.opconv(pl, Cn, w, bias, dil, prec, residual=r, act=(al, bt, f, f), packed=packed, dense=dense,
                             fp32_out=res)
    ae, ib = (t.contiguous() for t in K.snake_params(al, bt))
    ff = _filters()
    seen = {}
    for pattern in (G.ZERO,) + G.POISONS:
        ap = G.arena(2 * (lo_off + B * T * Cpo if npl == 2 else B * T * Cpo), pattern)
        ao = G.arena(4 * B * T * N if res else 0, pattern)
        a = _conv_args(pl, Cn, packed, N, k, dil, prec, bias)
        a.res, a.out = _hip.ptr(r), ao.ws.data_ptr() if res else None
        a.act_plane, a.act_plane_lo_off = ap.ws.data_ptr(), lo_off
        a.act_alpha_exp, a.act_inv_beta = ae.data_ptr(), ib.data_ptr()
        a.act_up_filter = a.act_down_filter = ff.data_ptr()
        check((lib().alcm_opconv_dense if dense else lib().alcm_opconv)(C.byref(a), stream_handle()), "opconv")
        torch.cuda.synchronize()
        ap.check_guards()
        ao.check_guards()
        flat = ap.ws.clone().view(torch.int16)
        planes = [flat[i * lo_off:i * lo_off + B * T * Cpo].view(B, T, Cpo) for i in range(npl)]
        p16 = _poison16(pattern)
        if npl == 2:
            assert bool((flat[B * T * Cpo:lo_off] == p16).all()), "written between the hi and the lo plane"
        for i, p in enumerate(planes):
            assert torch.equal(p[..., :N], pl_ref[i][..., :N]), f"plane {i} on {pattern:#04x} differs from kernels.opconv's"
            pad = p[..., N:]
            assert bool((pad == (p16 if dense else 0)).all()), \
                f"plane {i} on {pattern:#04x}: channels >= N " + ("changed" if dense else "not written as 0")
        if res:
            out = ao.ws.clone().view(torch.float32).view(B, T, N)
            assert G.same_bits(out, y_ref), f"fp32 output on {pattern:#04x} differs from kernels.opconv's"
        seen[pattern] = planes
    assert all(torch.equal(seen[G.ZERO][i][..., :N], seen[p][i][..., :N]) for p in G.POISONS for i in range(npl))


# form, C, N, T, k, prec: the wide-layer kernel's GEGLU epilogue (N % 384 == 0) and the plane output on lin_plane
# (k = 1) and on wconv2 with a ragged last N tile (1024 = 5 x 192 + 64)
PLANE_EPILOGUE = [("geglu", 64, 384, 37, 3, 2), ("geglu", 128, 768, 300, 9, 0),
                  ("out", 64, 192, 37, 1, 2), ("out", 64, 192, 37, 1, 0), ("out", 64, 1024, 37, 3, 2),
                  ("out", 576, 1728, 196, 1, 2)]


@pytest.mark.parametrize("form,Cn,N,T,k,prec", PLANE_EPILOGUE)
def test_conv_plane_epilogues_write_their_plane_whole(form, Cn, N, T, k, prec):
    """geglu_plane [B][T][N/2] and out_plane [B][T][N] into 0xFF: every element written (the bytes of a run into
    0x00), nothing outside, and the plane kernels.opconv returns."""
    B = 2
    x, w, bias = _r((B, T, Cn), 110), _r((N, Cn, k), 111, 1.0 / np.sqrt(Cn * k)).cuda(), _r((N,), 112, 0.05).cuda()
    pl, packed = K.operand_planes(x.cuda(), prec), K.pack_conv_weight(w)
    No = N // 2 if form == "geglu" else N
    want = K.opconv(pl, Cn, w, bias, 1, prec, packed=packed, geglu=form == "geglu", out_plane=form == "out")
    got = {}
    for pattern in (G.ZERO, G.NAN):
        ar = G.arena(2 * B * T * No, pattern)
        a = _conv_args(pl, Cn, packed, N, k, 1, prec, bias)
        if form == "geglu":
            a.geglu_plane = ar.ws.data_ptr()
        else:
            a.out_plane = ar.ws.data_ptr()
        check(lib().alcm_opconv(C.byref(a), stream_handle()), "opconv")
        torch.cuda.synchronize()
        ar.check_guards()
        got[pattern] = _planes(ar, (1, B, T, No))
    assert torch.equal(got[G.NAN], got[G.ZERO]), "an element of the plane was not written"
    assert torch.equal(got[G.NAN], want)
    assert torch.isfinite(got[G.NAN].view(torch.float16 if prec == 2 else torch.bfloat16).float()).all()


@pytest.mark.parametrize("rows,Cn,prec", [(3, 64, 0), (74, 576, 2), (390, 192, 2), (515, 576, 0)])
def test_layer_norm_plane_is_written_whole(rows, Cn, prec):
    x, g, b = _r((1, rows, Cn), 120, 2.0).cuda(), _r((Cn,), 121).cuda(), _r((Cn,), 122).cuda()
    want = K.layer_norm_plane(x, g, b, prec)
    got = {}
    for pattern in (G.ZERO, G.NAN):
        ar = G.arena(2 * rows * Cn, pattern)
        check(lib().alcm_layer_norm_plane(x.data_ptr(), rows, Cn, Cn, 1e-5, g.data_ptr(), b.data_ptr(), ar.ws.data_ptr(),
                                          prec, stream_handle()), "layer_norm_plane")
        torch.cuda.synchronize()
        ar.check_guards()
        got[pattern] = _planes(ar, (1, 1, rows, Cn))
    assert torch.equal(got[G.NAN], got[G.ZERO]) and torch.equal(got[G.NAN], want)


@pytest.mark.parametrize("mode", ["conv1", "conv2", "last"])
@pytest.mark.parametrize("T", [37, 300])
@pytest.mark.parametrize("k,dil", [(3, 1), (11, 5)])
@pytest.mark.parametrize("Cn", [24, 48])
def test_dense_conv_ignores_the_padding_channels(Cn, k, dil, T, mode):
    """alcm_opconv_dense on planes with Cp > C whose channels >= C hold 0xFF, then 0x7F (NaN as fp16 both): the header
    says they are ignored, so each epilogue form gives the bits it gives on zero-padded planes."""
    B, prec, f = 2, 3, recipe.kaiser_sinc_filter1d(0.25, 0.3, 12)
    x, w, bias = _r((B, T, Cn), 60), _r((Cn, Cn, k), 61, 0.7 / np.sqrt(Cn * k)).cuda(), _r((Cn,), 62, 0.05).cuda()
    r, o0 = _r((B, T, Cn), 63).cuda(), _r((B, T, Cn), 66)
    al, bt = _r((Cn,), 64, 0.3).cuda(), _r((Cn,), 65, 0.3).cuda()
    packed = K.pack_conv_weight(w)
    base = K.operand_planes(x.cuda(), prec)
    assert base.shape[-1] > Cn

    def run(pl):
        if mode == "conv1":
            _, p = K.opconv(pl, Cn, w, bias, dil, prec, act=(al, bt, f, f), fp32_out=False, dense=True, packed=packed)
            return None, p
        if mode == "conv2":
            return K.opconv(pl, Cn, w, bias, dil, prec, residual=r, act=(al, bt, f, f), dense=True, packed=packed)
        o = o0.clone().cuda()
        K.opconv(pl, Cn, w, bias, dil, prec, residual=r, out_scale=1 / 3, accumulate_into=o, dense=True, packed=packed)
        return o, None

    y0, p0 = run(base)
    for pattern in G.POISONS:
        pl = base.clone()
        pl[..., Cn:] = _poison16(pattern)
        y, p = run(pl)
        torch.cuda.synchronize()
        if y0 is not None:
            assert torch.isfinite(y).all() and G.same_bits(y, y0), f"fp32 output reads the padding ({pattern:#04x})"
        if p0 is not None:
            assert torch.equal(p[..., :Cn], p0[..., :Cn]), f"Activation1d planes read the padding ({pattern:#04x})"
