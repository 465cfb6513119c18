"""Executing the BigVGAN stage plans launches exactly what the forward launched before the planner existed.

tests/data/voc_launches.json holds, per case of tests/data/voc_plans.json (but the benchmark-sized ones), the profile
rows and launch counts of one vocoder forward on the recipe's weights with ALCM_PROF_SHAPES=1, recorded from the build
before the planner on an MI355X (256 compute units).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REPO, golden

from audiolcm_amd import _hip
from test_vocplan import load_table, switches

pytestmark = pytest.mark.gpu

with open(os.path.join(REPO, "tests", "data", "voc_launches.json")) as f:
    LAUNCHES = json.load(f)


@pytest.fixture(scope="module")
def voc():
    from audiolcm_amd import models
    _hip.require_device(0)
    return models.BigVGAN.from_recipe(0)


def test_every_small_case_is_recorded():
    cases = load_table()["cases"]
    assert set(LAUNCHES) == {cid for cid, c in cases.items() if c["B"] * c["M"] <= 80} and len(LAUNCHES) >= 26


@pytest.mark.parametrize("cid", sorted(LAUNCHES))
def test_forward_launches_the_recorded_rows(voc, cid):
    t = load_table()
    c = t["cases"][cid]
    assert torch.cuda.get_device_properties(0).multi_processor_count == t["ncu"]
    mel = np.tile(golden("bigvgan_M20.npz")["mel"], (c["B"], 1, (c["M"] + 19) // 20))[:, :, :c["M"]]
    mel = torch.from_numpy(np.ascontiguousarray(mel)).cuda()
    with switches(dict(c["knobs"], ALCM_PROF_SHAPES=1)):
        voc.set_split(c["policy"])
        voc.set_resblock_streams(bool(c["streams"]))
        try:
            _hip.profile_begin()
            wav = voc(mel)
            torch.cuda.synchronize()
            rows = _hip.profile_end(1024)
        finally:
            voc.set_split(True)
            voc.set_resblock_streams(True)
    assert torch.isfinite(wav).all()
    got = {r["name"]: r["launches"] for r in rows}
    assert got == LAUNCHES[cid], {k: (got.get(k), LAUNCHES[cid].get(k)) for k in set(got) ^ set(LAUNCHES[cid])
                                  | {k for k in set(got) & set(LAUNCHES[cid]) if got[k] != LAUNCHES[cid][k]}}
