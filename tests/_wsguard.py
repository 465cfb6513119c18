"""Poisoned, guarded workspaces: the yardstick of tests/test_gpu_workspace.py and its host twin.

The workspace contract (include/audiolcm_hip.h, at the workspace queries): what [ws, ws + ws_bytes) holds on entry is
irrelevant, nothing outside it is written, what it holds on exit is unspecified.  _HipModel._workspace hands out
torch.empty bytes cached per call kind, shape and stream, so a read-before-write meets what the same forward wrote one
run earlier, and a write past a sub-buffer lands in its neighbour: neither can show in a test that takes its workspace
from there.

arena(nbytes, pattern) is one uint8 tensor laid out guard | workspace | guard: each guard at least GUARD bytes, the
workspace 256-byte aligned and exactly nbytes long, every byte `pattern`.  The fills and what they decode to:

    0x00   0 in every format                                                          the reference run
    0xFF   NaN as fp32 / bf16 / fp16 / fp64, -1 as int64
    0x7F   3.4e38 as fp32 and as bf16, 1.4e306 as fp64 (finite); NaN as fp16

0xFF and 0x7F together tell "multiplied by an exact zero" (NaN x 0 = NaN shows under 0xFF; 3.4e38 x 0 = 0 does not show
under 0x7F on fp32 / bf16 lanes) from "used" (shows under both).  A `stale` run has no fill: the workspace is what
another case of the same model left at the same base.

guarded(...) replaces _HipModel._workspace for the duration of a block: every wrapper that takes its workspace there
(DiT embed_context and forward_cached, VAE decode and encode, MelNet, BigVGAN, the text encoder) gets the arena's view
of exactly the queried size, and passes ws.numel() on, so the C entry sees that size.  Nothing here touches a GPU at
import; with device="cpu" the arenas are host tensors (tests/test_wsguard_host.py).
"""
import contextlib

import torch

GUARD = 4096
ALIGN = 256
ZERO, NAN, HUGE = 0x00, 0xFF, 0x7F
POISONS = (NAN, HUGE)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


class Arena:
    """guard | workspace | guard in one uint8 tensor (see the module's docstring)."""

    def __init__(self, nbytes, pattern, device="cuda"):
        self.nbytes, self.pattern = int(nbytes), int(pattern)
        self.buf = torch.empty(GUARD + self.nbytes + GUARD + ALIGN, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.buf.data_ptr() + GUARD)) % ALIGN  # the head guard takes the alignment slack
        self.fill(pattern)
        self._lent, self._rest = self.nbytes, None

    def fill(self, pattern):
        self.pattern = int(pattern)
        self.buf.fill_(self.pattern)

    @property
    def ws(self):
        return self.buf[self.start:self.start + self.nbytes]

    @property
    def guards(self):
        return self.buf[:self.start], self.buf[self.start + self.nbytes:]

    def view(self, nbytes):
        """The first nbytes of the workspace (a stale run of the smaller of two cases); what lies behind them is
        guarded as well: check_guards compares it with what it held now."""
        nbytes = int(nbytes)
        assert 0 <= nbytes <= self.nbytes, (nbytes, self.nbytes)
        self._lent = nbytes
        self._rest = self.ws[nbytes:].clone() if nbytes < self.nbytes else None
        return self.ws[:nbytes]

    def check_guards(self):
        """Both guards keep every byte (and so does the workspace behind a shorter view).  Call it after
        torch.cuda.synchronize(): the BigVGAN chains run on auxiliary streams."""
        for name, g in zip(("head", "tail"), self.guards):
            bad = torch.nonzero(g != self.pattern).flatten()
            assert bad.numel() == 0, (f"{name} guard of a {self.nbytes}-byte workspace: {bad.numel()} bytes changed, "
                                      f"first at guard offset {int(bad[0])} ({int(g[bad[0]]):#04x} for {self.pattern:#04x})")
        if self._rest is not None:
            now = self.ws[self._lent:]
            bad = torch.nonzero(now != self._rest).flatten()
            assert bad.numel() == 0, (f"{bad.numel()} bytes changed behind a {self._lent}-byte view of a "
                                      f"{self.nbytes}-byte workspace, first at workspace offset {self._lent + int(bad[0])}")


def arena(nbytes, pattern, device="cuda"):
    return Arena(nbytes, pattern, device)


class Call:
    """One C entry that took its workspace from the guard: its kind (the first field of the wrapper's cache key),
    the queried size, the arena, and the tensors the wrapper handed to the C entry, in the wrapper's order (every
    wrapper passes its inputs, then the one output, then the workspace) with a copy of each taken as it was handed
    over."""

    def __init__(self, kind, nbytes, ar):
        self.kind, self.nbytes, self.arena, self.args = kind, nbytes, ar, []

    @property
    def inputs(self):
        assert len(self.args) >= 3 and self.args[-1][0].data_ptr() == self.arena.ws.data_ptr(), self.kind
        return self.args[:-2]

    @property
    def out(self):
        return self.args[-2][0]


class Guard:
    def __init__(self):
        self.calls = []

    def sizes(self):
        """{call kind: the largest size a call of that kind queried}"""
        s = {}
        for c in self.calls:
            s[c.kind] = max(s.get(c.kind, 0), c.nbytes)
        return s

    def arenas(self):
        return {c.kind: c.arena for c in self.calls}

    def check(self):
        """After torch.cuda.synchronize(): every arena's guards and every input of every call keep their bytes."""
        for c in self.calls:
            c.arena.check_guards()
            for i, (t, before) in enumerate(c.inputs):
                assert _same(t.view(torch.uint8), before.view(torch.uint8)), f"{c.kind}: input {i} changed"


def _ptr_modules():
    from audiolcm_amd import mel, models, text_encoder
    return [m for m in (models, mel, text_encoder) if hasattr(m, "ptr")]


@contextlib.contextmanager
def guarded(pattern=ZERO, arenas=None, at_least=None):
    """Within the block _HipModel._workspace returns an arena's workspace view of exactly the queried size.

    pattern: the fill of the arenas made here, one per call kind, each of exactly the queried size, or of
    at_least[kind] bytes where that is larger (the partner's run of a stale pair: the arena fits the larger case).
    arenas: {kind: Arena} to use as they are, without a refill (the stale run itself).
    -> a Guard: .calls lists what ran, .check() asserts guards and inputs."""
    from audiolcm_amd import _hip
    from audiolcm_amd.models import _HipModel
    g = Guard()
    made = dict(arenas or {})

    def workspace(self, key, nbytes, device):
        kind, nbytes = key[0], int(nbytes)
        ar = made.get(kind)
        if ar is None:
            ar = made[kind] = arena(max(nbytes, (at_least or {}).get(kind, 0)), pattern, device)
        g.calls.append(Call(kind, nbytes, ar))
        return ar.view(nbytes)

    def ptr(t):
        if t is not None and g.calls:
            c = g.calls[-1]
            c.args.append((t, None if t.data_ptr() == c.arena.ws.data_ptr() else t.clone()))
        return _hip.ptr(t)

    mods = _ptr_modules()
    old_ws, old_ptr = _HipModel._workspace, [m.ptr for m in mods]
    _HipModel._workspace = workspace
    for m in mods:
        m.ptr = ptr
    try:
        yield g
    finally:
        _HipModel._workspace = old_ws
        for m, p in zip(mods, old_ptr):
            m.ptr = p


def same_bits(a, b):
    """torch.equal on int32 views of two fp32 tensors: NaNs and signed zeros count."""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and \
        bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
