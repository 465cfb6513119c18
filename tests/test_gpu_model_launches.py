"""The DiT, VAE, text and mel forwards launch exactly what they launched before they shared one set of launch helpers
(conv, lin, plane_args, plane_conv, conv_1x1, mha in audiolcm_amd/csrc/alcm_models.cpp).

tests/data/model_launches.json holds, per case of CASES, the profile rows and launch counts of one forward on the
recipe's weights with ALCM_PROF_SHAPES=1.  The table was recorded on an MI355X (256 compute units) from the library
built at the commit before the helpers were shared (8577839), by running this module as a script against that build:
run_case below is both what the test runs and what wrote the table.  Inputs are seeded random tensors (token ids from
tests/golden/text_B2_L77.npz); the rows do not depend on values.

Cases are the smallest shapes that reach every branch of the forwards: the two-GEMM attention and the split-plane 1x1
convs (split), plane q/k/v into flash attention and the plane linears (mixed, bf16), the DiT's fp32-qkv plane form
(L > 512), the VAE's nin_shortcut blocks, both upsample forms and both AttnBlock scratch choices, T5 wo on hi / lo
planes (mixed) and through lin (bf16), and the channels-last input copies switched off (ALCM_NCT_CL=0); two cases at
the benchmarked batch add the K-split projections, which the planner takes only there.  Two cases on cut-down
configurations whose head dims the fused attention does not take (recorded the same way from 09c2a2d, the commit before
the three forwards shared one attention sub-block) pin what no configured geometry reaches: the text towers' plane path
with the two-GEMM attention, and a DiT whose attention runs through conv + mha while its feed-forward stays on planes.
"""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

from conftest import REPO, golden

from audiolcm_amd import _hip, recipe
from test_vocplan import switches

pytestmark = pytest.mark.gpu

TABLE = os.path.join(REPO, "tests", "data", "model_launches.json")


def _cases():
    c = {}
    for pol in ("split", "mixed", "bf16"):
        for wc in (1, 0):
            c[f"dit-B2-T40-{pol}-{'w' if wc else 'now'}"] = dict(model="dit", B=2, T=40, policy=pol, w_cond=wc)
        c[f"vae_decode-B2-T24-{pol}"] = dict(model="vae_decode", B=2, T=24, policy=pol)
        c[f"vae_encode-B1-M40-{pol}"] = dict(model="vae_encode", B=1, T=40, policy=pol)
        c[f"text-B2-L77-{pol}"] = dict(model="text", B=2, T=77, policy=pol)
        c[f"text-B1-L8-{pol}"] = dict(model="text", B=1, T=8, policy=pol)
    c["dit-B2-T40-mixed-w-nct0"] = dict(model="dit", B=2, T=40, policy="mixed", w_cond=1, knobs={"ALCM_NCT_CL": 0})
    c["dit-B1-T360-mixed-w"] = dict(model="dit", B=1, T=360, policy="mixed", w_cond=1)  # L = 515 > 512
    c["vae_decode-B2-T24-mixed-nct0"] = dict(model="vae_decode", B=2, T=24, policy="mixed", knobs={"ALCM_NCT_CL": 0})
    for pol in ("split", "bf16"):
        c[f"mel-B2-L20-{pol}"] = dict(model="mel", B=2, T=20, policy=pol)
    # the benchmarked batch: the only shapes at which the planner takes the K-split forms of the DiT FFN
    # down-projection and of the text towers' out-projections
    c["dit-B32-T312-mixed-w"] = dict(model="dit", B=32, T=312, policy="mixed", w_cond=1)
    c["text-B32-L77-mixed"] = dict(model="text", B=32, T=77, policy="mixed")
    # head dims the fused attention does not take (96 and 144 > 72), one layer each: the text towers stay on planes
    # with the two-GEMM attention and to_planes between the plane linears; the DiT block's attention goes through
    # conv + mha in fp16 while its feed-forward stays on planes
    c["text_dh96-B1-L8-mixed"] = dict(model="text", B=1, T=8, policy="mixed", cfg=dict(
        b_layers=1, t_layers=1, b_hidden=192, b_heads=2, b_inter=256, t_d=128, p_out=128, t_heads=2, t_dkv=96,
        t_ff=128))
    c["dit_dh144-B1-T8-mixed-w"] = dict(model="dit", B=1, T=8, policy="mixed", w_cond=1,
                                        cfg=dict(depth=1, num_heads=4))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _model(kind, cfg=()):
    """The model of a case on the recipe's weights; cfg: (field, value) pairs that replace the configuration's."""
    from audiolcm_amd import models
    _hip.require_device(0)
    cfg = dict(cfg)
    if kind == "dit":
        return models.ConcatDiT2MLP(**cfg).load_state_dict(recipe.dit_state(0, recipe.DiTConfig(**cfg)))
    if kind == "vae":
        return models.AutoencoderKL().load_state_dict({**recipe.vae_state(0), **recipe.vae_encoder_state(0)})
    if kind == "text":
        from audiolcm_amd.text_encoder import CLAPT5TextEncoder
        return CLAPT5TextEncoder.from_recipe(0, cfg=recipe.TextConfig(**cfg))
    from audiolcm_amd.mel import MelNet
    return MelNet()


def run_case(c):
    """One forward of case c -> ({profile row name: launches}, the output tensor)."""
    B, T = c["B"], c["T"]
    gen = torch.Generator().manual_seed(1234)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda()
    kind = c["model"].split("_")[0]
    m = _model(kind, tuple(sorted(c.get("cfg", {}).items())))
    if kind == "dit":
        x, t, ctx = rnd(B, 20, T), torch.tensor([999, 499] * B)[:B].cuda(), recipe.synthetic_context(B).cuda()
        wc = rnd(B, 256) if c["w_cond"] else None
        fwd = lambda cemb: m.forward_cached(x, t, cemb, wc)
    elif c["model"] == "vae_decode":
        z = rnd(B, 20, T)
        fwd = lambda _: m.decode(z)
    elif c["model"] == "vae_encode":
        mel = rnd(B, 80, T)
        fwd = lambda _: m.encode(mel).parameters
    elif kind == "text":
        g = golden("text_B2_L77.npz")
        sel = torch.arange(B) % 2
        a, b = torch.from_numpy(g["clap_ids"])[sel, :T], torch.from_numpy(g["t5_ids"])[sel, :T]
        fwd = lambda _: m.encode_ids(a, b)
    else:
        wav = 0.1 * rnd(B, T * 256)
        fwd = lambda _: m(wav)
    with switches(dict(c.get("knobs", {}), ALCM_PROF_SHAPES=1)):
        m.set_split(c["policy"])
        try:
            pre = m.embed_context(ctx) if kind == "dit" else None  # outside the profile: forward_cached is the case
            torch.cuda.synchronize()
            _hip.profile_begin()
            out = fwd(pre)
            torch.cuda.synchronize()
            rows = _hip.profile_end(1024)
        finally:
            m.set_split(True)
    return {r["name"]: r["launches"] for r in rows}, out


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def test_every_case_is_recorded():
    assert set(load_table()["rows"]) == set(CASES) and len(CASES) == 27


@pytest.mark.parametrize("cid", sorted(CASES))
def test_forward_launches_the_recorded_rows(cid):
    t = load_table()
    assert torch.cuda.get_device_properties(0).multi_processor_count == t["ncu"]
    got, out = run_case(CASES[cid])
    assert torch.isfinite(out).all()
    want = t["rows"][cid]
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


if __name__ == "__main__":
    # python tests/test_gpu_model_launches.py TABLE.json: record the table (and print each output's SHA-256)
    table = dict(ncu=torch.cuda.get_device_properties(0).multi_processor_count, rows={})
    for cid in sorted(CASES):
        table["rows"][cid], out = run_case(CASES[cid])
        print(cid, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
