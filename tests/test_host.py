"""CPU tests: host logic (schedule, config/plugin surface, sharding, WAV), and the C-ABI library surface.

No compute runs here: the HIP library is only loaded and its exports checked.
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden

from audiolcm_amd import schedule, recipe


def test_schedule_matches_reference_fixtures():
    g = golden("schedule.npz")
    np.testing.assert_array_equal(schedule.alphas_cumprod().numpy(), g["alphas_cumprod"])
    for S in (1, 2, 4, 8):
        assert schedule.lcm_timesteps(S, 50) == list(g[f"timesteps_S{S}"])


def test_schedule_errors_match_reference():
    with pytest.raises(ValueError):
        schedule.lcm_timesteps(None, 50)
    with pytest.raises(ValueError):
        schedule.lcm_timesteps(2, 50, timesteps=[999, 499])
    with pytest.raises(ValueError):
        schedule.lcm_timesteps(60, 50)
    with pytest.raises(ValueError):
        schedule.lcm_timesteps(2, 2000)
    with pytest.raises(ValueError):
        schedule.lcm_timesteps(None, 50, timesteps=[499, 999])
    assert schedule.lcm_timesteps(None, 50, timesteps=[999, 500, 3]) == [999, 500, 3]


def test_step_coeffs_match_oracle():
    from oracle import alcm_oracle as O
    ac = schedule.alphas_cumprod()
    for t, pt in ((999, 499), (499, 499), (759, 499), (259, 259)):
        sc = O.lcm_step_scalars(t, pt, ac)
        ref = [float(sc[k]) for k in ("sqrt_a", "sqrt_b", "c_out", "c_skip", "sqrt_a_prev", "sqrt_b_prev")]
        assert schedule.step_coeffs(t, pt, ac) == ref


def test_sample_plan():
    p = schedule.sample_plan(2)
    assert [x["t"] for x in p] == [999, 499] and [x["add_noise"] for x in p] == [True, False]
    p4 = schedule.sample_plan(4)
    assert [x["prev_t"] for x in p4] == [759, 499, 259, 259]


def test_frequency_tables_match_reference():
    """Tables equal the reference's up to the last ulp of exp (platform dependent in torch itself):
    at t = 999 / w*1000 = 4000 one ulp of a frequency moves the embedding by <= 3e-5 / 3e-4."""
    g = golden("schedule.npz")
    t = torch.from_numpy(g["t"])
    ref_t = torch.exp(-math.log(10000) * torch.arange(0, 128, dtype=torch.float32) / 128)
    assert (schedule.timestep_freqs() - ref_t).abs().max() <= 1.2e-7 * ref_t.abs().max()
    args = t[:, None].float() * schedule.timestep_freqs()[None]
    np.testing.assert_allclose(torch.cat([torch.cos(args), torch.sin(args)], 1).numpy(), g["timestep_emb"],
                               atol=5e-5)
    w = torch.tensor(4).repeat(3) * 1000.0
    a = w[:, None] * schedule.guidance_freqs()[None]
    np.testing.assert_allclose(torch.cat([torch.sin(a), torch.cos(a)], 1).numpy(), g["guidance_w4"], atol=3e-4)


def test_recipe_keys_and_shapes():
    assert len(recipe.dit_specs()) == 128
    names = [s[0] for s in recipe.bigvgan_specs()]
    assert len(names) == len(set(names)) == 784
    vae = {s[0]: s[1] for s in recipe.vae_decoder_specs()}
    assert vae["decoder.conv_in.weight"] == (1536, 20, 5)
    assert vae["decoder.up.1.upsample.conv.weight"] == (768, 768, 3)
    assert "decoder.up.0.block.0.nin_shortcut.weight" in vae


def test_config_surface_builds_hip_classes():
    from audiolcm_amd import config
    cfg = config.load_config(os.path.join(REPO, "configs", "audiolcm.yaml"))
    assert cfg.model.target == "ldm.models.diffusion.lcm_audio.LCM_audio"
    assert config.get_obj_from_str(cfg.model.params.unet_config.target).__module__ == "audiolcm_amd.models"
    assert config.get_obj_from_str(cfg.model.params.first_stage_config.target).__name__ == "AutoencoderKL"
    assert config.get_obj_from_str("ldm.models.diffusion.lcm_audio.LCM_audio").__module__ == "audiolcm_amd.lcm"
    with pytest.raises(ImportError):
        config.get_obj_from_str("ldm.models.diffusion.ddpm_audio.LatentDiffusion_audio")
    with pytest.raises(KeyError):
        config.instantiate_from_config({"params": {}})


def test_reference_targets_are_accepted():
    """Every `target:` of configs/audiolcm.yaml (the reference's own dotted strings, kept unchanged in the project's
    copy of the model section) resolves to an MI355X class, and the training-only targets the reference's file also
    names are accepted as inert."""
    from audiolcm_amd import config
    cfg = config.load_config(os.path.join(REPO, "configs", "audiolcm.yaml"))
    for key in ("unet_config", "first_stage_config", "cond_stage_config"):
        assert cfg.model.params[key].target.startswith("ldm.")
        cls = config.get_obj_from_str(cfg.model.params[key].target)
        assert cls.__module__.startswith("audiolcm_amd")
    assert cfg.vocoder.target.startswith("vocoder.")
    assert config.get_obj_from_str(cfg.vocoder.target).__name__ == "VocoderBigVGAN"
    assert config.instantiate_from_config({"target": "ldm.lr_scheduler.LambdaLinearScheduler",
                                           "params": {"warm_up_steps": [10000]}}) is None
    assert config.instantiate_from_config(cfg.model.params.first_stage_config.params.lossconfig).__class__.__name__ \
        == "Identity"


def test_shard_range_partitions():
    from audiolcm_amd.distributed import shard_range
    for n in (0, 1, 7, 32, 256, 257):
        for w in (1, 2, 3, 8):
            spans = [shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [h - l for l, h in spans]
            assert max(sizes) - min(sizes) <= 1


def test_all_gather_two_ranks_gloo():
    """world_size-2 gloo run of the waveform all-gather used by the multi-GPU path."""
    script = os.path.join(REPO, "tests", "_dist_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr=127.0.0.1", "--master-port=29577", script], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GATHER_OK" in r.stdout


def test_wav_writer_roundtrip(tmp_path):
    from audiolcm_amd import wavio
    from oracle import alcm_oracle as O
    w = np.sin(np.linspace(0, 100, 16000)).astype(np.float32) * 0.7
    p = str(tmp_path / "x.wav")
    wavio.write_pcm16(p, w)
    data, sr = wavio.read_pcm16(p)
    assert sr == 16000 and data.tobytes() == O.pcm16_bytes(w)


def test_header_declares_every_binding():
    """include/audiolcm_hip.h and the ctypes binding list the same entry points."""
    from audiolcm_amd import _hip
    hdr = open(os.path.join(REPO, "include", "audiolcm_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:const char\*|int|size_t)\s+(alcm_\w+)\s*\(", hdr, re.M))
    assert declared == set(_hip.EXPORTED), declared ^ set(_hip.EXPORTED)


def test_library_exports_every_symbol():
    """The built libaudiolcm_hip.so loads (no GPU needed) and exports every declared symbol."""
    from audiolcm_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    L = _hip.lib()
    for name in _hip.EXPORTED:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    for name in _hip.EXPORTED:
        assert re.search(rf"\bT {name}\b", out), name
    assert L.alcm_version() == 1


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "audiolcm_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in re.findall(r"^\s*(?:from|import)\s+(\w+)", src, re.M), f


def test_product_fails_loudly_without_library(monkeypatch):
    from audiolcm_amd import _hip
    monkeypatch.setattr(_hip, "LIB_PATH", "/nonexistent/libaudiolcm_hip.so")
    monkeypatch.setattr(_hip, "_lib", None)
    with pytest.raises(ImportError):
        _hip.lib()


def test_yaml_instantiates_lcm_model_without_gpu():
    from audiolcm_amd import config, lcm, models, text_encoder
    cfg = config.load_config(os.path.join(REPO, "configs", "audiolcm.yaml"))
    m = config.instantiate_from_config(cfg.model, split=True)
    assert isinstance(m, lcm.LCM_audio)
    assert isinstance(m.unet.diffusion_model, models.ConcatDiT2MLP)
    assert m.unet.diffusion_model.cfg.hidden_size == 576 and m.unet.diffusion_model.cfg.depth == 4
    assert isinstance(m.first_stage_model, models.AutoencoderKL)
    assert m.first_stage_model.cfg.upsample_levels == (1,)
    assert isinstance(m.cond_stage_model, text_encoder.FrozenCLAPFLANEmbedder)
    assert m.cond_stage_model.clap_tokenizer is None  # no vocabulary offline, and no silent stand-in
    with pytest.raises(RuntimeError, match="tokenizer"):
        m.cond_stage_model.tokenize(["a dog barks"], ["<a dog barks& all>"])
    m.cond_stage_model.use_synthetic_tokenizer()  # explicit opt-in (recipe weights / tests)
    a, b = m.cond_stage_model.tokenize(["a dog barks"], ["<a dog barks& all>"])
    assert a.shape == b.shape == (1, 77)
    assert not m.cond_stage_model.model.loaded
    assert not m.unet.diffusion_model.loaded
    with pytest.raises(RuntimeError):
        m.unet.diffusion_model.forward_cached(torch.zeros(1, 20, 8), torch.zeros(1), None, None)


def test_api_requires_checkpoints(tmp_path):
    from audiolcm_amd.infer_api import AudioLCMBatchInfer
    with pytest.raises(FileNotFoundError):
        AudioLCMBatchInfer(["x"], config_path=os.path.join(REPO, "configs", "audiolcm.yaml"),
                           model_path=str(tmp_path / "missing.ckpt"), outpath=str(tmp_path))


def test_roofline_model_reproduces_survey():
    """audiolcm_amd/roofline.py (bench.py's path_roofline_frac_model) reproduces SURVEY.md §8(d) / BASELINE.md §3:
    C2 47,763 GFLOP / 20.9 ms, C4 ~153.4k GFLOP / 65.3 ms, C5 57,243 GFLOP / 25.45 ms."""
    from audiolcm_amd import roofline as RL
    c2 = RL.summary(RL.path_layers(**RL.CONFIGS[2]))
    c4 = RL.summary(RL.path_layers(**RL.CONFIGS[4]))
    c5 = RL.summary(RL.path_layers(**RL.CONFIGS[5]))
    assert abs(c2["gflop"] - 47763) / 47763 < 1e-3 and abs(c2["t_roof_ms"] - 20.9) < 0.1
    assert abs(c4["gflop"] - 153400) / 153400 < 5e-3 and abs(c4["t_roof_ms"] - 65.3) < 0.3
    assert abs(c5["gflop"] - 57243) / 57243 < 1e-3 and abs(c5["t_roof_ms"] - 25.45) < 0.1
    dit = RL.summary(RL.dit_layers(1, 312))
    assert abs(dit["gflop"] - 150.6) < 0.5           # per sample-step
    assert abs(RL.summary(RL.vae_layers(1, 312))["gflop"] - 65.8) < 0.2
    assert abs(RL.summary(RL.bigvgan_layers(1, 624))["gflop"] - 1125.5) < 0.5


def test_t5_relative_bucket_matches_transformers():
    """The bucket table the HIP T5 encoder is packed with == transformers' own T5Attention rule."""
    from transformers.models.t5.modeling_t5 import T5Attention
    from audiolcm_amd.text_encoder import relative_position_bucket
    for L in (7, 77, 300):
        rel = torch.arange(L)[None, :] - torch.arange(L)[:, None]
        ref = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128)
        assert torch.equal(relative_position_bucket(L), ref)


def test_synthetic_tokenizer_layout():
    from audiolcm_amd.text_encoder import SyntheticTokenizer
    b = SyntheticTokenizer("bert", 30522)(["A dog barks.", "a dog barks"], max_length=8)["input_ids"]
    assert b.shape == (2, 8) and b[0, 0] == 101 and b[0, 5] == 102 and b[0, 6:].tolist() == [0, 0]
    assert torch.equal(b[0, 1:4], b[1, 1:4])          # lower-cased words map to the same ids
    t = SyntheticTokenizer("t5", 32128)(["<a dog& all>"], max_length=77)["input_ids"]
    n = int((t[0] != 0).sum())
    assert t[0, n - 1] == 1 and int(t.max()) < 32128  # </s> then padding
    long = SyntheticTokenizer("bert", 30522)(["w " * 200], max_length=77)["input_ids"]
    assert long.shape == (1, 77) and long[0, -1] == 102  # truncated, [SEP] kept


AUDIOCAPS_ROWS = (  # three rows of the reference's audiocaps_test_16000_struct.tsv (data), one name repeated
    "name\tdataset\tori_cap\tmel_path\tcaption\taudio_path\n"
    "Y7fmOlUlwoNg\taudiocaps\tConstant rattling noise and sharp vibrations\taudiocaps_mels/test/Y7fmOlUlwoNg_mel.npy\t"
    "<constant rattling noise& all>@<sharp vibrations& all>\tdata/audiocaps/test/Y7fmOlUlwoNg.wav\n"
    "Y6BJ455B1aAs\taudiocaps\tA rocket flies by followed by a loud explosion and fire crackling as a truck engine "
    "runs idle\taudiocaps_mels/test/Y6BJ455B1aAs_mel.npy\t<rocket flying by& start>@<loud explosion& mid>@<fire "
    "crackling& mid>@<truck engine idle& mid>\tdata/audiocaps/test/Y6BJ455B1aAs.wav\n"
    "Y7fmOlUlwoNg\taudiocaps\tRattling and vibrating\taudiocaps_mels/test/Y7fmOlUlwoNg_mel.npy\t"
    "<rattling& all>@<vibrating& all>\tdata/audiocaps/test/Y7fmOlUlwoNg.wav\n")


def test_tsv_dataset_struct(tmp_path):
    """ldm/data/tsvdataset.py TSVDatasetStruct: running _<num> suffix per repeated name, caption dict; absent mels
    are None (generation needs captions only); instantiated through the YAML test_dataset target."""
    from audiolcm_amd import config
    tsv = tmp_path / "caps.tsv"
    tsv.write_text(AUDIOCAPS_ROWS)
    mel = np.arange(80 * 10, dtype=np.float32).reshape(80, 10)
    (tmp_path / "audiocaps_mels" / "test").mkdir(parents=True)
    np.save(tmp_path / "audiocaps_mels" / "test" / "Y6BJ455B1aAs_mel.npy", mel)
    cfg = config.load_config(os.path.join(REPO, "configs", "audiolcm.yaml"))
    d = dict(cfg["test_dataset"])
    d["params"] = dict(d["params"], tsv_path=str(tsv))
    ds = config.instantiate_from_config(d)
    assert len(ds) == 3
    names = [ds[i]["f_name"] for i in range(3)]
    assert names == ["Y7fmOlUlwoNg_0", "Y6BJ455B1aAs_0", "Y7fmOlUlwoNg_1"]
    assert ds[1]["caption"]["ori_caption"].startswith("A rocket") and ds[1]["caption"]["struct_caption"].startswith("<rocket")
    assert ds[0]["image"] is None and ds[1]["image"].shape == (80, 624) and np.array_equal(ds[1]["image"][:, :10], mel)


def test_cli_arguments_match_reference():
    """scripts/txt2audio_for_lcm.py argument surface (reference :48-152) with the reference defaults."""
    from audiolcm_amd.cli import parse_args
    o = parse_args([])
    assert (o.prompt_txt, o.sample_rate, o.test_dataset, o.outdir, o.ddim_steps, o.n_iter, o.H, o.W, o.n_samples,
            o.scale, o.resume, o.vocoder_ckpt) == ("prompt.txt", 22050, "none", "outputs/txt2audio-samples", 100, 1, 20,
                                                   312, 1, 5.0, "", "vocoder/logs/audioset")
    o = parse_args(["--test-dataset", "audiocaps", "--ddim_steps", "2", "-r", "x.ckpt", "-b", "c.yaml",
                    "--vocoder-ckpt", "bigvgan", "--sample_rate", "16000"])
    assert o.test_dataset == "audiocaps" and o.ddim_steps == 2 and o.resume == "x.ckpt" and o.base == "c.yaml"


class _StubSampler:
    def __init__(self):
        self.seeds = []

    def sample(self, S, conditioning, batch_size, shape, seeds, **kw):
        self.seeds.extend(seeds)
        return torch.tensor(seeds, dtype=torch.float32)[:, None], None


class _StubModel:
    channels = 0

    def get_learned_conditioning(self, text):
        return torch.zeros(len(text["ori_caption"]), 1)

    def decode_first_stage(self, z):
        return z


def test_cli_seeds_do_not_depend_on_batching():
    """Per-clip seeds come from (global prompt index, iteration, sample), so --batch-size 1 and 4 give every clip
    the same seed with --n_iter 2 --n_samples 2 (a running counter made them depend on the chunking)."""
    from audiolcm_amd.cli import GenSamples, parse_args
    prompts = [dict(ori_caption=f"p{i}", struct_caption=f"<p{i}& all>") for i in range(5)]
    per_clip = []
    for bs in (1, 4):
        opt = parse_args(["--n_iter", "2", "--n_samples", "2", "--seed", "11"])
        samp = _StubSampler()
        gen = GenSamples(opt, samp, _StubModel(), "/nonexistent", None, save_mel=False, save_wav=False)
        for lo in range(0, len(prompts), bs):
            gen.gen_batch(prompts[lo:lo + bs], [p["ori_caption"] for p in prompts[lo:lo + bs]], lo)
        per_clip.append(sorted(samp.seeds))
    assert per_clip[0] == per_clip[1] == list(range(11, 11 + 5 * 2 * 2))


class _HParams:  # stands in for a Lightning checkpoint's OmegaConf / Namespace hyper_parameters
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_checkpoint_loader_is_safe_and_keeps_tensors(tmp_path):
    """A Lightning-shaped .ckpt with non-tensor objects (hyper_parameters object, callback class keys, optimizer
    state) loads through torch.load(weights_only=True) with inert placeholders: tensors intact, no class of the
    file imported or constructed."""
    from audiolcm_amd.ckpt import OpaqueObject, load_checkpoint, state_dict_of
    sd = {"unet.diffusion_model.proj_in.weight": torch.randn(4, 2, 5), "scale_factor": torch.tensor(0.5)}
    ck = {"state_dict": sd, "hyper_parameters": _HParams(lr=1e-4, cfg={"a": 1}), "callbacks": {_HParams: {"k": 1}},
          "epoch": 3, "optimizer_states": [{"state": {}, "param_groups": [{"lr": 1.0}]}]}
    path = str(tmp_path / "m.ckpt")
    torch.save(ck, path)
    with pytest.raises(Exception):
        torch.load(path, weights_only=True)   # the plain safe loader refuses such a file
    out = load_checkpoint(path)
    assert isinstance(out["hyper_parameters"], OpaqueObject) and type(out["hyper_parameters"]) is not _HParams
    got = state_dict_of(out)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert out["epoch"] == 3
