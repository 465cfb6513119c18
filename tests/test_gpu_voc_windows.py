"""Windowed float64 parity of the vocoder, stage by stage (the yardstick: tests/_windowed.py).

Several kernels of the vocoder have no entry point of their own (ups2, the fused output head, the three-set
Activation1d, the phase-conv upsamplers, the sum-form close as the executor builds it) and were reached only by
whole-clip comparisons, whose relative L2 cannot see a fault on a few samples at a clip end, a tile seam or a batch
boundary.  Vocoders cut down to one or two stages put each of them one or two layers from the output:

  tail  96 channels, rates (2, 2):  ups2 at both widths, the fused AMPBlock forms, the fused 24-channel head
  mid   384 channels, rates (2, 2): phase / plane upsamplers, a wide stage closed by the sum form, a C = 96 stage
  head  1536 channels, rate (4,):   the first stage alone with the generic head
  full  the default config at a few frames

Every window of W = 32 samples of every clip must stay within 4 x the largest window error E of the oracle with the
policy's operand roundings emulated (float64, CPU), and every clip within the whole-clip bar of test_gpu_models.py
(waveform rel-L2 < 1e-3).  Each case prints E, the device's largest window, their ratio and the whole-clip L2
(DESIGN.md §3 has the table).  The profile rows of each forward are checked for the kernels the case is about, so a
planner change cannot turn it into a test of something else (tests/test_voc_windows_host.py pins the plans themselves).
"""
import functools

import pytest
import torch

import _windowed as Wn
from audiolcm_amd import _hip
from test_vocplan import switches

pytestmark = pytest.mark.gpu

UPS2_96, UPS2_48, POST24 = "alcm::ups2_kernel<96, 48, 96>", "alcm::ups2_kernel<48, 32, 48>", "alcm::post_kernel<24>"
ACT1, ACT3_SPLIT, ACT3_F16 = "alcm::act_coop_kernel<1>", "alcm::act_coop_kernel<1>, x3", "alcm::act_coop_kernel<2>, x3"
ACT3_MFMA, ACT_MFMA, ACT_H16 = ("alcm::act_mfma3_kernel<64>", "alcm::act_mfma_kernel<64, true, false>",
                                "alcm::act_mfma_kernel<64, true, true>")
HEAD_N1 = "alcm::opconv_kernel<256, 16,"  # the generic head: conv_post (N = 1) as a plane conv
# (config, policy) -> profile rows every forward of it must contain: a whole row name, or, ending in a comma or a
# template argument, the start of one (tile shapes may move; the kernel family and its precision may not).
# ", x3" rows are the three-set first Activation1d; W1 / W2 = fp16 / fp16 hi + lo weights of the tail kernels.
LAUNCHED = {
    ("tail", "split"): {UPS2_96, UPS2_48, POST24, ACT3_SPLIT, "alcm::opconv_kernel<256, 48,", "alcm::opconv_kernel<256, 32,"},
    ("tail", "mixed"): {UPS2_48, POST24, ACT3_F16, "alcm::opconv_kernel<256, 48,", "alcm::tconv_kernel<C48, W1",
                        "alcm::tconv2_kernel<C24, W1"},
    # phase-conv upsamplers and conv_pre on conv_kernel; the wide stage's standalone Activation1d; its convs and the
    # three accumulating launches of its sum-form close on 192-column tiles (the one-launch kernel needs a full chip or
    # ALCM_WCONV3=1: test_plane_handoff below)
    ("mid", "split"): {ACT1, ACT3_SPLIT, "alcm::conv_kernel<128, 128,", "alcm::conv_kernel<128, 64,",
                       "alcm::opconv_kernel<128, 192,", "alcm::opconv_kernel<128, 96,", HEAD_N1},
    ("mid", "mixed"): {ACT3_MFMA, ACT_MFMA, ACT3_F16, "alcm::wconv2_kernel<2, false,", "alcm::tconv2_kernel<C96, W1",
                       HEAD_N1},
    ("head", "split"): {ACT1, "alcm::conv_kernel<128, 128,", "alcm::opconv_kernel<128, 96,", HEAD_N1},
    ("head", "mixed"): {ACT3_MFMA, ACT_MFMA, "alcm::wconv2_kernel<2, false,", HEAD_N1},
    ("full", "split"): {UPS2_96, UPS2_48, POST24, ACT1, ACT3_SPLIT, "alcm::conv_kernel<128, 64,",
                        "alcm::opconv_kernel<128, 192,"},
    ("full", "mixed"): {UPS2_96, UPS2_48, POST24, ACT3_MFMA, ACT_MFMA, ACT3_F16, "alcm::tconv2_kernel<C96, W1",
                        "alcm::tconv_kernel<C48, W2", "alcm::tconv2_kernel<C24, W2"},
}
# the cases whose plan has the fp16 conv1 hand-off (tests/test_voc_windows_host.py H16): the fp16-input Activation1d
H16_CASES = {("mid", "mixed", 4, 256), ("head", "mixed", 2, 129), ("full", "mixed", 1, 33)}
SUM_ONE_LAUNCH = "alcm::wconv3_kernel<2, 3, false>"


def missing_rows(required, rows):
    whole = lambda r: r.endswith(">") or r.endswith("x3")
    return {r for r in required if not (r in rows if whole(r) else any(n.startswith(r) for n in rows))}


@functools.lru_cache(maxsize=None)
def _model(name):
    from audiolcm_amd import models, recipe
    _hip.require_device(0)
    cfg = Wn.VOC_CONFIGS[name][0]
    return models.BigVGAN(cfg).load_state_dict(recipe.bigvgan_state(0, cfg))


def run(name, policy, mel, knobs=None):
    """One forward of config `name` -> (waveform (B, 1, T) on the device, {profile row: launches})."""
    voc = _model(name)
    with switches(knobs or {}):
        voc.set_split(policy)
        try:
            torch.cuda.synchronize()
            _hip.profile_begin()
            wav = voc(mel.cuda()).clone()
            torch.cuda.synchronize()
            rows = _hip.profile_end(1024)
        finally:
            voc.set_split(True)
    return wav, {r["name"]: r["launches"] for r in rows}


@pytest.mark.parametrize("case", Wn.VOC_CASES, ids=Wn.case_id)
def test_every_window_within_the_emulated_bar(case):
    name, policy, B, M = case
    mel, exact, emu = Wn.voc_references(name, policy, B, M)
    wav, rows = run(name, policy, mel)
    print(Wn.case_id(case), "rows:", sorted(rows))
    assert wav.shape == exact.shape
    missing = missing_rows(LAUNCHED[(name, policy)], rows)
    assert not missing, (missing, sorted(rows))
    assert (ACT_H16 in rows) == (case in H16_CASES) and SUM_ONE_LAUNCH not in rows, sorted(rows)
    Wn.check_windows(Wn.case_id(case), wav.cpu().numpy(), exact, emu, Wn.VOC_W, 1e-3)


@pytest.mark.parametrize("case", Wn.UPS2_GRID_CASES, ids=Wn.case_id)
def test_ups2_workgroup_cap(case):
    """ALCM_UPS2_GRID = 1, 2, 3: each workgroup walks several tiles, prefetching the next one's window, the first of
    the next clip included, while it computes; the output equals the uncapped run bit for bit and meets the same bar."""
    name, policy, B, M, cap = case
    mel, exact, emu = Wn.voc_references(name, policy, B, M)
    free, rows = run(name, policy, mel)
    capped, rows_c = run(name, policy, mel, {"ALCM_UPS2_GRID": cap})
    assert rows == rows_c and {UPS2_96, UPS2_48} <= set(rows)
    Wn.check_windows(Wn.case_id(case), capped.cpu().numpy(), exact, emu, Wn.VOC_W, 1e-3)
    assert torch.equal(capped, free)


@pytest.mark.parametrize("case", Wn.HANDOFF_CASES, ids=Wn.case_id)
def test_plane_handoff(case):
    """ALCM_WCONV3=1 plans, at these sizes, what the default plan takes from about 2000 mel frames: the wide stages
    close in the one-launch sum form, which writes the next stage's upsampler planes instead of the fp32 output
    (writes_next / planes_from_prev).  The roundings are the same, so are the references and the bar."""
    name, policy, B, M = case
    mel, exact, emu = Wn.voc_references(name, policy, B, M)
    wav, rows = run(name, policy, mel, {"ALCM_WCONV3": 1})
    assert SUM_ONE_LAUNCH in rows, sorted(rows)
    Wn.check_windows(Wn.case_id(case) + "-handoff", wav.cpu().numpy(), exact, emu, Wn.VOC_W, 1e-3)
