"""tests/_wsguard.py on host tensors: the fills decode as its table says, the workspace view is 256-byte aligned and
exactly as long as asked, and check_guards sees one changed byte in either guard and nothing else."""
import math

import pytest
import torch

import _wsguard as G


def _decoded(pattern, dtype):
    return G.arena(64, pattern, "cpu").ws.view(dtype)


def test_zero_fill_is_zero_in_every_format():
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int64):
        assert bool((_decoded(G.ZERO, dt) == 0).all()), dt


def test_ff_fill_is_nan_and_minus_one():
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        assert bool(torch.isnan(_decoded(G.NAN, dt)).all()), dt
    assert bool((_decoded(G.NAN, torch.int64) == -1).all())


def test_7f_fill_is_huge_and_finite_except_as_fp16():
    for dt, about in ((torch.float32, 3.4e38), (torch.bfloat16, 3.4e38), (torch.float64, 1.4e306)):
        v = _decoded(G.HUGE, dt).double()
        assert bool(torch.isfinite(v).all()) and math.isclose(float(v[0]), about, rel_tol=0.02), (dt, float(v[0]))
    assert bool(torch.isnan(_decoded(G.HUGE, torch.float16)).all())
    # what tells a lane multiplied by an exact zero from a lane that is used
    z = torch.zeros(())
    assert float(_decoded(G.HUGE, torch.float32)[0] * z) == 0.0 and math.isnan(float(_decoded(G.NAN, torch.float32)[0] * z))


@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 4096, 100003])
def test_workspace_view_is_aligned_and_exact(nbytes):
    a = G.arena(nbytes, G.NAN, "cpu")
    head, tail = a.guards
    assert a.ws.numel() == nbytes and a.ws.dtype == torch.uint8 and a.ws.is_contiguous()
    assert (a.buf.data_ptr() + a.start) % G.ALIGN == 0 and (nbytes == 0 or a.ws.data_ptr() % G.ALIGN == 0)
    assert head.numel() >= G.GUARD and tail.numel() >= G.GUARD
    assert head.numel() + nbytes + tail.numel() == a.buf.numel()
    assert bool((a.buf == G.NAN).all())
    assert a.view(nbytes).data_ptr() == a.ws.data_ptr()
    a.check_guards()


def test_check_guards_is_silent_when_only_the_workspace_changes():
    for pattern in (G.ZERO, G.NAN, G.HUGE):
        a = G.arena(1000, pattern, "cpu")
        a.ws.fill_(0x5A)
        a.check_guards()


@pytest.mark.parametrize("where", ["first of head", "last of head", "first of tail", "last of tail"])
def test_check_guards_reports_one_changed_byte(where):
    a = G.arena(1000, G.NAN, "cpu")
    g = a.guards[0 if "head" in where else 1]
    g[0 if "first" in where else -1] = 0xFE
    with pytest.raises(AssertionError, match="head" if "head" in where else "tail"):
        a.check_guards()


def test_a_shorter_view_guards_what_lies_behind_it():
    a = G.arena(1000, G.NAN, "cpu")
    v = a.view(600)
    assert v.numel() == 600 and v.data_ptr() == a.ws.data_ptr()
    v.fill_(1)
    a.check_guards()
    a.ws[600] = 0
    with pytest.raises(AssertionError, match="behind a 600-byte view"):
        a.check_guards()


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    x = torch.tensor([0.0, float("nan"), 1.5])
    assert G.same_bits(x, x.clone())
    y = x.clone()
    y[0] = -0.0
    assert torch.equal(x[::2], y[::2]) and not G.same_bits(x, y)


def _wrapper(model, kind, nbytes, spoil_input=False):
    """What a models.py wrapper does around its C entry, on host tensors: query, _workspace, ptr of the inputs, of the
    one output and of the workspace, then the 'forward'."""
    from audiolcm_amd import models
    x, out = torch.arange(4.0), torch.empty(4)
    ws = model._workspace((kind, 1, 2), nbytes, "cpu")
    addresses = [models.ptr(x), models.ptr(None), models.ptr(out), models.ptr(ws)]
    assert addresses[1] is None and addresses[3] == ws.data_ptr() and ws.numel() == nbytes
    out.copy_(2 * x)
    ws[:8] = 1
    if spoil_input:
        x[0] = 7
    return out


def test_guarded_hands_out_exact_views_and_puts_the_wrappers_back():
    from audiolcm_amd import _hip, models
    m = models._HipModel()
    real = models._HipModel._workspace
    with G.guarded(G.NAN) as g:
        _wrapper(m, "ctx", 500)
        _wrapper(m, "fwd", 1000)
    assert models._HipModel._workspace is real and models.ptr is _hip.ptr
    g.check()
    assert g.sizes() == {"ctx": 500, "fwd": 1000} and [c.arena.nbytes for c in g.calls] == [500, 1000]
    assert [len(c.inputs) for c in g.calls] == [1, 1] and torch.equal(g.calls[1].out, 2 * torch.arange(4.0))


def test_guarded_stale_run_reuses_the_partners_arena_at_the_same_base():
    from audiolcm_amd import models
    m = models._HipModel()
    with G.guarded(G.NAN, at_least={"fwd": 3000}) as partner:
        _wrapper(m, "fwd", 800)
    partner.check()
    ar = partner.arenas()["fwd"]
    assert ar.nbytes == 3000 and bool((ar.ws[:8] == 1).all()) and bool((ar.ws[8:] == G.NAN).all())
    with G.guarded(arenas=partner.arenas()) as stale:
        _wrapper(m, "fwd", 1000)
    stale.check()
    assert stale.calls[0].arena is ar and stale.sizes() == {"fwd": 1000}
    ar.ws[2000] = 3  # behind the 1000 bytes the stale run was given
    with pytest.raises(AssertionError, match="behind a 1000-byte view"):
        stale.check()


def test_guard_check_reports_a_changed_input():
    from audiolcm_amd import models
    with G.guarded(G.ZERO) as g:
        _wrapper(models._HipModel(), "fwd", 64, spoil_input=True)
    with pytest.raises(AssertionError, match="input 0 changed"):
        g.check()
