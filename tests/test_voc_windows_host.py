"""Host twin of tests/test_gpu_voc_windows.py and test_gpu_vae_windows.py (no GPU): the case tables of
tests/_windowed.py cannot drift from the stage planner, the emulation with no rounding is the oracle itself, no
reference sample of a vocoder case sits in tanh saturation, and window_errors cuts the windows it says it cuts.
"""
import numpy as np
import pytest
import torch

import _windowed as Wn
from audiolcm_amd import _hip
from audiolcm_amd import kernels as K
from oracle import alcm_oracle as O

S, F16, F16W2 = _hip.PREC_SPLIT, _hip.PREC_F16, _hip.PREC_F16W2

# (config, policy) -> per stage (prec, ups, amp, act3, sum3): what the windowed cases are meant to run
# (kernels.voc_plan(cfg, policy, True, B, M, 256), the same at every (B, M) of the case table)
PLANS = {
    # both stages ups2 with the fused AMPBlock and the three-set first Activation1d; the fused 24-channel head
    ("tail", "split"): [(S, "ups2", "fused", 1, 0), (S, "ups2", "fused", 1, 0)],
    # stage 0 upsampler on fp16 planes, stage 1 ups2; the tail kernels at fp16 (the loader accepts it; production
    # runs these widths at fp16 hi + lo weights)
    ("tail", "mixed"): [(F16, "planes", "fused_dense", 1, 0), (F16, "ups2", "fused_dense", 1, 0)],
    # phase-conv upsamplers, a wide stage closed by the sum form, then a fused C = 96 stage; the generic head
    ("mid", "split"): [(S, "phases", "wide", 0, 1), (S, "phases", "fused", 1, 0)],
    ("mid", "mixed"): [(F16, "planes", "wide", 1, 1), (F16, "planes", "fused_dense", 1, 0)],
    ("head", "split"): [(S, "phases", "wide", 0, 1)],
    ("head", "mixed"): [(F16, "planes", "wide", 1, 1)],
    ("full", "split"): [(S, "phases", "wide", 0, 1)] * 3 + [(S, "phases", "fused", 1, 0)] + [(S, "ups2", "fused", 1, 0)] * 2,
    # the only config where fp16 hi + lo weights (stages 4-5) meet ups2
    ("full", "mixed"): [(F16, "planes", "wide", 1, 1)] * 3 + [(F16, "planes", "fused_dense", 1, 0)]
                       + [(F16W2, "ups2", "fused_dense", 1, 0)] * 2,
}
# the fp16 conv1 hand-off of a wide stage is planned from B * To >= 1024 rows: these cases only
H16 = {("mid", "mixed", 4, 256): [1, 0], ("head", "mixed", 2, 129): [1], ("full", "mixed", 1, 33): [0, 0, 1, 0, 0, 0]}


def test_case_tables():
    assert len(Wn.VOC_CASES) == 2 * (24 + 12 + 2 + 3) + 1 and len(set(Wn.VOC_CASES)) == len(Wn.VOC_CASES)
    assert {(c[0], c[1]) for c in Wn.VOC_CASES} == set(PLANS)
    assert set(H16) <= set(Wn.VOC_CASES)
    assert len(Wn.VAE_CASES) == 14 + 4 and len(Wn.UPS2_GRID_CASES) == 6


@pytest.mark.parametrize("case", Wn.VOC_CASES + [c[:4] for c in Wn.UPS2_GRID_CASES[::3]], ids=Wn.case_id)
def test_planner_takes_the_intended_path(case):
    name, policy, B, M = case
    plans = K.voc_plan(Wn.VOC_CONFIGS[name][0], policy, True, B, M, Wn.NCU)
    assert [(p["prec"], p["ups"], p["amp"], p["act3"], p["sum3"]) for p in plans] == PLANS[(name, policy)]
    assert [p["h16"] for p in plans] == H16.get(case, [0] * len(plans))
    # the plane hand-off between wide stages starts far above these sizes
    assert not any(p["writes_next"] or p["planes_from_prev"] for p in plans)
    assert all(p["concurrent"] and p["own_bufs"] for p in plans)


def test_plane_handoff_starts_above_the_window_cases():
    """The smallest batches at which the default config's mixed plan has writes_next: about 2000 mel frames in all,
    30 s of float64 oracle per run.  By shape the hand-off stays with the whole-clip tests ..."""
    cfg = Wn.VOC_CONFIGS["full"][0]
    first = lambda B: next(M for M in range(1, 2000) if any(
        p["writes_next"] for p in K.voc_plan(cfg, "mixed", True, B, M, Wn.NCU)))
    assert (first(8), first(4), first(3)) == (241, 497, 673)


@pytest.mark.parametrize("case", Wn.HANDOFF_CASES, ids=Wn.case_id)
def test_plane_handoff_is_planned_with_wconv3_forced(case):
    """... and ALCM_WCONV3=1 plans it at the window cases' sizes: every wide stage followed by a planes upsampler of
    the same precision hands its output over as planes; nothing else in the plan moves."""
    from test_vocplan import switches
    name, policy, B, M = case
    cfg = Wn.VOC_CONFIGS[name][0]
    base = K.voc_plan(cfg, policy, True, B, M, Wn.NCU)
    with switches({"ALCM_WCONV3": 1}):
        forced = K.voc_plan(cfg, policy, True, B, M, Wn.NCU)
    want = {"mid": [1, 0], "full": [1, 1, 1, 0, 0, 0]}[name]
    assert [p["writes_next"] for p in forced] == want
    assert [p["planes_from_prev"] for p in forced] == [0] + want[:-1]
    strip = lambda ps: [{k: v for k, v in p.items() if k not in ("writes_next", "planes_from_prev")} for p in ps]
    assert strip(forced) == strip(base)


def test_layer_precisions_follow_the_plan():
    full = Wn.VOC_CONFIGS["full"][0]
    assert Wn.voc_layer_precisions(full, "mixed", 2, 5) == dict(
        pre="bf16x3", ups=["f16"] * 4 + ["bf16x3"] * 2, amp=["f16"] * 4 + ["f16w2"] * 2, post=None)
    assert Wn.voc_layer_precisions(Wn.VOC_CONFIGS["mid"][0], "split", 3, 129) == dict(
        pre="bf16x3", ups=["bf16x3"] * 2, amp=["bf16x3"] * 2, post="bf16x3")


def test_vae_roundings_follow_the_executor():
    """mixed: the 22 ResnetBlock1D convs and the Upsample1D conv on fp16, the other nine contractions' weights (and
    both attention products) bf16x3; split: bf16x3 everywhere."""
    from audiolcm_amd import recipe
    W = recipe.vae_state(0)
    convs = {k: v for k, v in W.items() if k.endswith(".weight") and v.dim() == 3}
    mixed, split = Wn.vae_chooser(W, "mixed"), Wn.vae_chooser(W, "split")
    f16 = {k for k, v in convs.items() if mixed("conv", v) == "f16"}
    assert len(f16) == 23 and all(W[k].shape[-1] == 3 for k in f16)
    assert set(convs) - f16 == {"post_quant_conv.weight", "decoder.conv_in.weight", "decoder.conv_out.weight",
                                "decoder.up.1.block.0.nin_shortcut.weight", "decoder.up.0.block.0.nin_shortcut.weight"} \
        | {f"decoder.mid.attn_1.{n}.weight" for n in ("q", "k", "v", "proj_out")}
    assert mixed("bmm", None) == "bf16x3" and {split("conv", v) for v in convs.values()} == {"bf16x3"}


def test_emulation_without_rounding_is_the_oracle():
    """Every patched call with precision None is the oracle's own call: bit for bit, vocoder and decoder."""
    cfg = Wn.VOC_CONFIGS["tail"][0]
    mel = Wn.voc_input(cfg, 0.2, 3, 33).double()
    W = Wn.voc_state64("tail")
    none = dict(pre=None, ups=[None, None], amp=[None, None], post=None)
    assert torch.equal(Wn.voc_oracle(W, mel, cfg, none), Wn.voc_oracle(W, mel, cfg))
    z, exact = Wn.vae_exact(2, 3)
    with torch.no_grad(), Wn.roundings(lambda kind, w: None):
        same = O.vae_decode(Wn._states["vae"], z.double())
    assert np.array_equal(same.numpy(), exact)


def test_emulated_roundings_reach_every_layer():
    """Each layer group's rounding moves the output, at the size its format predicts (bf16x3 ~2^-16, fp16 ~2^-11)."""
    cfg = Wn.VOC_CONFIGS["tail"][0]
    mel, exact = Wn.voc_exact("tail", 3, 33)
    W = Wn.voc_state64("tail")
    base = dict(pre=None, ups=[None, None], amp=[None, None], post=None)
    for grp, prec, lo, hi in (("pre", "bf16x3", 1e-7, 1e-4), ("post", "bf16x3", 1e-7, 1e-4), ("pre", "f16", 1e-5, 3e-3),
                              ("pre", "f16w2", 1e-5, 3e-3)):
        out = Wn.voc_oracle(W, mel.double(), cfg, dict(base, **{grp: prec})).numpy()
        assert lo < max(Wn.clip_l2(out, exact)) < hi, (grp, prec)
    for grp in ("ups", "amp"):
        for i in range(2):
            precs = dict(base, **{grp: [("f16" if j == i else None) for j in range(2)]})
            out = Wn.voc_oracle(W, mel.double(), cfg, precs).numpy()
            assert 1e-5 < max(Wn.clip_l2(out, exact)) < 3e-3, (grp, i)


@pytest.mark.parametrize("name", sorted(Wn.VOC_CONFIGS))
def test_no_reference_sample_in_saturation(name):
    """A saturated tanh hides every error upstream of it: |ref| <= 0.95 at every sample of every case, and the clips
    of a batch differ (different draws at gains x0.5, x1, x2)."""
    shapes = sorted({c[2:4] for c in Wn.VOC_CASES + Wn.UPS2_GRID_CASES if c[0] == name})
    for B, M in shapes:
        mel, ref = Wn.voc_exact(name, B, M)
        assert ref.shape == (B, 1, M * Wn.VOC_CONFIGS[name][0].hop)
        assert np.abs(ref).max() <= 0.95, (B, M, np.abs(ref).max())
        rms = np.sqrt((mel.numpy() ** 2).mean((1, 2)))
        for b in range(1, B):
            assert not np.allclose(mel[b].numpy() / rms[b], mel[0].numpy() / rms[0]), (B, M, b)
            assert abs(rms[b] / rms[0] / (Wn.GAINS[b % 3] / Wn.GAINS[0]) - 1) < 0.25, (B, M, b)


def test_window_errors_cuts_every_window():
    ref = np.ones((2, 3, 70))
    y = ref.copy()
    y[0, :, 69] += 0.3   # the last position of clip 0: in the ragged 7th window and in the closing one
    y[1, 1, 40] += 0.6   # one channel of one position of clip 1's second window (and of the closing one)
    e0, e1 = Wn.window_errors(y, ref, 32)
    assert len(e0) == len(e1) == 4  # [0, 32) [32, 64) [64, 70) and the last 32 positions
    np.testing.assert_allclose(e0, [0, 0, 0.3 / np.sqrt(6), 0.3 / np.sqrt(32)])
    np.testing.assert_allclose(e1, [0, 0.6 / np.sqrt(96), 0, 0.6 / np.sqrt(96)])
    short, = Wn.window_errors(y[:1, :, 60:], ref[:1, :, 60:], 32)  # shorter than a window: the one that covers it
    np.testing.assert_allclose(short, [0.3 / np.sqrt(10)])
    exact, = Wn.window_errors(y[:1, :, 6:], ref[:1, :, 6:], 32)    # a whole number of windows, plus the closing one
    assert len(exact) == 3 and exact[1] == exact[2]


def test_check_windows_sees_a_fault_the_whole_clip_bar_misses():
    """1 % on the six samples next to a clip end: 3e-4 of whole-clip L2 at M = 20, far beyond four times E."""
    g = np.random.default_rng(0)
    ref = g.standard_normal((1, 1, 20 * 256)) * 0.1
    emu = ref * (1 + 1e-5 * g.standard_normal(ref.shape))
    got = ref * (1 + 1e-5 * g.standard_normal(ref.shape))
    Wn.check_windows("clean", got, ref, emu, 32, 1e-3)
    got[0, 0, -6:] *= 1.01
    assert Wn.clip_l2(got, ref)[0] < 1e-3
    with pytest.raises(AssertionError, match="window 159 of 161"):
        Wn.check_windows("fault", got, ref, emu, 32, 1e-3)
