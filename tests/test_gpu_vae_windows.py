"""Windowed float64 parity of the VAE decoder (the yardstick: tests/_windowed.py), at lengths other than the goldens'
24, 312 and 936: affine_plane with and without the nearest-neighbour upsample, split_planes + sgemm_planes for the
1x1 convs, both upsample forms and both AttnBlock scratch choices have no entry point of their own.

A window is 4 output frames x 80 bins.  Every window of every clip must stay within 4 x the largest window error E of
oracle.vae_decode with the policy's operand roundings emulated (float64, CPU: bf16x3 everywhere under the split
policy; under mixed fp16 on the ResnetBlock1D / Upsample1D convs), and every clip within the whole-clip mel bars of
test_gpu_models.py (split < 1e-4, mixed < 1e-3).  Clips of a batch are different draws at gains x0.5, x1, x2.  The
two sizes either side of the 1024-row switch to the wide-layer kernel run under both policies.
"""
import functools

import pytest
import torch

import _windowed as Wn
from audiolcm_amd import _hip

pytestmark = pytest.mark.gpu

L2_BAR = {"split": 1e-4, "mixed": 1e-3}


@functools.lru_cache(maxsize=None)
def _vae():
    from audiolcm_amd import models
    _hip.require_device(0)
    return models.AutoencoderKL.from_recipe(0)


@pytest.mark.parametrize("case", Wn.VAE_CASES, ids=Wn.case_id)
def test_every_window_within_the_emulated_bar(case):
    policy, B, T = case
    z, exact, emu = Wn.vae_references(policy, B, T)
    vae = _vae()
    vae.set_split(policy)
    try:
        torch.cuda.synchronize()
        _hip.profile_begin()
        mel = vae.decode(z.cuda()).clone()
        torch.cuda.synchronize()
        rows = {r["name"] for r in _hip.profile_end(1024)}
    finally:
        vae.set_split(True)
    print(Wn.case_id(case), "rows:", sorted(rows))
    assert mel.shape == exact.shape == (B, 80, 2 * T)
    # the 1x1 convs on split planes under both policies; under mixed the plane convs below 1024 rows on opconv_kernel
    # (before the upsample at 3 x 341), from 1024 rows on the wide-layer kernel alone
    assert {"alcm::split_planes_kernel", "alcm::sgemm_planes_kernel<32, 2, 2>"} <= rows, sorted(rows)
    if policy == "mixed":
        assert "alcm::wconv2_kernel<2, false, 128, 192>" in rows, sorted(rows)
        assert any(r.startswith("alcm::opconv_kernel<") for r in rows) == (B * T < 1024), sorted(rows)
    Wn.check_windows(Wn.case_id(case), mel.cpu().numpy(), exact, emu, Wn.VAE_W, L2_BAR[policy])
