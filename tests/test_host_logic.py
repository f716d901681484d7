"""CPU: host-side logic of the product package and the C-ABI boundary (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from univid_amd import _lib, detinit, parallel
from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
from univid_amd.wan import fm_solvers_unipc, textimage2video
from univid_amd.wan.model import WanModel
from univid_amd.wan.vae2_2 import WanVAE_


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "univid_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(uv_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    """The shared library loads and exports exactly the entry points include/univid_hip.h declares."""
    if not os.path.exists(_lib.LIB_PATH):
        from univid_amd import build
        build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _header_functions()
    assert len(declared) >= 28
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert sorted(_lib.SIGNATURES) == declared, "ctypes signature table and header disagree"
    assert lib.uv_version() >= 100


def test_developer_options_are_explicit_calls_not_environment(monkeypatch):
    """Round-3 verdict / advisor: kernel-selection knobs are set through uv_set_option (host-only, atomic), never read from the
    environment per call: defaults, set / get / reset, loud rejection of unknown keys and out-of-range values, and no getenv left in
    the kernel sources."""
    lib = _lib.load()
    _lib.reset_options()
    assert (_lib.get_option(_lib.OPT_CONV_HALO), _lib.get_option(_lib.OPT_GEMM_GM), _lib.get_option(_lib.OPT_ATTN_CUT)) == (-1, 0, 0)
    monkeypatch.setenv("UV_CONV_HALO", "0")
    monkeypatch.setenv("UV_GEMM_GM", "16")
    assert _lib.get_option(_lib.OPT_CONV_HALO) == -1 and _lib.get_option(_lib.OPT_GEMM_GM) == 0      # the environment is not consulted
    _lib.set_option(_lib.OPT_CONV_HALO, 1)
    _lib.set_option(_lib.OPT_GEMM_GM, 8)
    _lib.set_option(_lib.OPT_ATTN_CUT, 7)
    assert (_lib.get_option(_lib.OPT_CONV_HALO), _lib.get_option(_lib.OPT_GEMM_GM), _lib.get_option(_lib.OPT_ATTN_CUT)) == (1, 8, 7)
    for key, bad in ((_lib.OPT_CONV_HALO, 2), (_lib.OPT_GEMM_GM, -1), (_lib.OPT_ATTN_CUT, -3), (99, 0)):
        with pytest.raises(_lib.UnividHipError):
            _lib.set_option(key, bad)
    assert _lib.get_option(_lib.OPT_CONV_HALO) == 1, "a rejected call must not change anything"
    _lib.reset_options()
    assert (_lib.get_option(_lib.OPT_CONV_HALO), _lib.get_option(_lib.OPT_GEMM_GM), _lib.get_option(_lib.OPT_ATTN_CUT)) == (-1, 0, 0)
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(csrc, f)).read()
            assert "getenv(" not in text.replace("(getenv racing", ""), f"{f} reads the environment"


def test_no_fallback_without_gpu():
    """Product path must fail loudly when there is no device / extension (no CPU fallback)."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = WanModel(model_type="ti2v", in_dim=48, out_dim=48, dim=256, ffn_dim=512, num_heads=4, num_layers=1, text_len=32, text_dim=64)
    with pytest.raises(_lib.UnividHipError):
        m([torch.randn(48, 1, 4, 4)], torch.tensor([5.0]), [torch.randn(3, 64)], 4)
    with pytest.raises(_lib.UnividHipError):
        _lib.load("/nonexistent/libunivid_hip.so") if False else _lib.init()


def test_product_does_not_import_oracle():
    """Only tests/, smoke and bench's cpu_baseline may touch oracle/."""
    bad = []
    for top in ("univid_amd", "tools"):
        for dp, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py") and re.search(r"^\s*(from|import)\s+oracle\b", open(os.path.join(dp, f)).read(), flags=re.M):
                    bad.append(os.path.join(top, f))
    assert not bad, bad
    # bench.py: the oracle appears only inside the cpu_baseline functions; __graft_entry__: inside smoke(), and build() checks that it imports
    src = open(os.path.join(ROOT, "bench.py")).read()
    for m in re.finditer(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
        head = src[:m.start()]
        fn = re.findall(r"^def (\w+)", head, flags=re.M)[-1]
        assert fn.startswith("cpu_baseline"), f"bench.py imports the oracle inside {fn}()"
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    for m in re.finditer(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
        assert re.findall(r"^def (\w+)", src[:m.start()], flags=re.M)[-1] in ("smoke", "build")   # build() only imports the checker


def test_detinit_is_deterministic_and_device_independent():
    a = detinit.uniform_pm1("blocks.0.ffn.0.weight", 1000, seed=3)
    b = detinit.uniform_pm1("blocks.0.ffn.0.weight", 1000, seed=3)
    c = detinit.uniform_pm1("blocks.0.ffn.2.weight", 1000, seed=3)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.min() >= -1 and a.max() < 1 and abs(a.mean()) < 0.1
    # known answers pin the generator itself (fixtures store seeds, not weights)
    assert [round(v, 6) for v in detinit.uniform_pm1("x", 4, 0).tolist()] == [round(v, 6) for v in detinit.uniform_pm1("x", 8, 0)[:4].tolist()]


def test_wanmodel_module_tree_contract():
    """The names UniVid's code relies on (model_pipeline.py:474-493, 578-592, 1745-1807)."""
    m = WanModel(model_type="ti2v", in_dim=48, out_dim=48, dim=256, ffn_dim=512, num_heads=4, num_layers=2, text_len=32, text_dim=64)
    assert isinstance(m.blocks, torch.nn.ModuleList) and len(m.blocks) == 2
    names = dict(m.named_modules())
    for p in ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "cross_attn.q", "cross_attn.k", "cross_attn.v",
              "cross_attn.o", "ffn.0", "ffn.2"):
        assert isinstance(names[f"blocks.1.{p}"], torch.nn.Linear)
    ca = [n for n, mod in m.named_modules() if mod.__class__.__name__ == "WanCrossAttention"]
    assert ca == ["blocks.0.cross_attn", "blocks.1.cross_attn"]
    assert m.freqs.dtype == torch.complex128 and tuple(m.freqs.shape) == (1024, 32)
    assert any("text_embedding" in k for k, _ in m.named_parameters())
    assert m.patch_embedding.weight.shape == (256, 48, 1, 2, 2)
    sd = m.state_dict()
    for k in ("blocks.0.modulation", "blocks.0.norm3.weight", "blocks.0.self_attn.norm_q.weight", "head.head.weight",
              "head.modulation", "time_projection.1.weight", "time_embedding.0.weight", "text_embedding.2.bias"):
        assert k in sd
    assert "blocks.0.norm1.weight" not in sd          # norm1 / norm2 have no affine parameters (model.py:203,211)


def test_vae_state_dict_matches_reference_names():
    with torch.device("meta"):
        v = WanVAE_(dim=160, dec_dim=256, z_dim=48, dim_mult=[1, 2, 4, 4], temperal_downsample=[False, True, True])
    sd = v.state_dict()
    assert len(sd) == 196
    assert tuple(sd["decoder.upsamples.0.upsamples.3.time_conv.weight"].shape) == (2048, 1024, 3, 1, 1)
    assert tuple(sd["encoder.conv1.weight"].shape) == (160, 12, 3, 3, 3)
    assert tuple(sd["decoder.head.2.weight"].shape) == (12, 256, 3, 3, 3)
    assert tuple(sd["encoder.middle.1.to_qkv.weight"].shape) == (1920, 640, 1, 1)


def test_unipc_host_schedule_matches_golden(golden):
    g = golden("unipc")
    for steps, shift in ((50, 5.0), (10, 5.0), (40, 3.0)):
        s = fm_solvers_unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
        s.set_timesteps(steps, device="cpu", shift=shift)
        assert torch.equal(s.timesteps, g[f"timesteps_{steps}_{shift}"])
        assert torch.equal(s.sigmas, g[f"sigmas_{steps}_{shift}"])
    with pytest.raises(NotImplementedError):
        fm_solvers_unipc.FlowUniPCMultistepScheduler(solver_order=3)


def test_unipc_host_coefficients_match_oracle():
    from oracle import unipc as ou
    s = fm_solvers_unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
    s.set_timesteps(10, device="cpu", shift=5.0)
    o = ou.FlowUniPC(1000, shift=1)
    o.set_timesteps(10, shift=5.0)
    for si in range(1, 9):
        a = s._coeffs(si + 1, si, 2, [si - 1])
        b = o._coeffs(si + 1, si, 2, [si - 1])
        assert a["r"] == (b["sigma_t"] / b["sigma_s0"]).item()
        assert a["c1"] == (b["alpha_t"] * b["h_phi_1"]).item()
        assert a["c2"] == (b["alpha_t"] * b["B_h"]).item()
        assert a["rk"] == b["rks"][0].item()


def test_masks_like_and_output_size(golden):
    g = golden("masks_like")
    x = [torch.zeros(3, 4, 2, 2)]
    b1, b2 = textimage2video.masks_like(x, zero=True)
    assert torch.equal(b1[0], g["zero1"]) and torch.equal(b2[0], g["zero2"])
    ow, oh = textimage2video.best_output_size(1920, 1080, 32, 32, 704 * 1280)
    assert ow % 32 == 0 and oh % 32 == 0 and ow * oh <= 704 * 1280
    assert textimage2video.best_output_size(1280, 704, 32, 32, 704 * 1280) == (1280, 704)


def test_text_weight_schedule_of_wrapper():
    import json
    import logging
    from conftest import GOLDEN
    tab = json.load(open(os.path.join(GOLDEN, "text_weight.json")))

    class _P:
        model = torch.nn.Module()

    for schedule, total, ratio, enabled, step, w in tab["rows"][::7]:
        cfg = CrossAttentionConfig(use_dynamic_text_weight=bool(enabled), total_sampling_steps=total,
                                   text_weight_transition_ratio=ratio, text_weight_schedule=schedule)
        wr = Wan22ContextWrapper(_P(), None, logging.getLogger("t"), cfg)
        assert wr._calculate_text_weight(step) == w


def test_config_defaults_match_reference():
    c = CrossAttentionConfig()
    assert (c.bagel_sequence_length, c.wan_text_length, c.total_sampling_steps) == (128, 512, 25)
    assert (c.text_weight_max, c.text_weight_min, c.text_weight_schedule, c.text_weight_transition_ratio) == (1.3, 1.0, "cosine", 0.4)
    assert c.video_size == (1280, 704) and c.video_length == 121 and c.bagel_cross_attn_layers == [8, 15, 22, 28]


def test_shard_range_partitions_the_batch():
    for n in (1, 7, 8, 13):
        for ws in (1, 2, 4, 8):
            if n < ws:
                continue
            spans = [parallel.shard_range(n, r, ws) for r in range(ws)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_checkpoint_roundtrip_diffusers_layout(tmp_path):
    """config.json + (sharded) safetensors: what WanModel.from_pretrained reads in the reference (textimage2video.py:103)."""
    from univid_amd.wan import checkpoint
    m = WanModel(model_type="ti2v", in_dim=48, out_dim=48, dim=256, ffn_dim=512, num_heads=4, num_layers=2, text_len=32, text_dim=64)
    detinit.init_module_(m, 5)
    for name, shard in (("single", 1 << 40), ("sharded", 1 << 20)):
        d = tmp_path / name
        checkpoint.save_wan_model(m, str(d), max_shard_bytes=shard)
        files = sorted(os.listdir(d))
        assert "config.json" in files
        assert ("diffusion_pytorch_model.safetensors.index.json" in files) == (name == "sharded")
        m2 = WanModel.from_pretrained(str(d))
        assert m2.num_layers == 2 and m2.patch_size == (1, 2, 2) and m2.model_type == "ti2v"
        sd, sd2 = m.state_dict(), m2.state_dict()
        assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    import json
    bad = tmp_path / "bad"
    checkpoint.save_wan_model(m, str(bad))
    cfg = json.load(open(bad / "config.json"))
    cfg["num_layers"] = 3
    json.dump(cfg, open(bad / "config.json", "w"))
    with pytest.raises(RuntimeError, match="does not match"):
        WanModel.from_pretrained(str(bad))


def test_mmr_select_matches_reference_golden():
    """univid_amd.understanding.mmr_select against the outputs of the reference's own function (eval_understanding.py:225-240)."""
    from conftest import load_golden
    from univid_amd.understanding.eval_understanding import mmr_select
    g = load_golden("siglip2_tiny")
    for K, lam, key in ((5, 0.5, "mmr_5_05"), (12, 0.2, "mmr_12_02"), (20, 0.9, "mmr_20_09")):
        assert mmr_select(g["mmr_embs"], g["mmr_query"], K, lam) == g[key].tolist()
    assert mmr_select(g["mmr_embs"][:0], g["mmr_query"], 3) == []


def test_siglip2_state_dict_is_hf_compatible():
    """Parameter names / shapes are transformers.Siglip2Model's (checkpoints load key for key)."""
    from oracle import siglip2 as osl
    from univid_amd.understanding import Siglip2Model
    m = Siglip2Model(osl.TINY_CFG)
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("logit_")}
    assert mine == {k: tuple(v) for k, v in osl.state_dict_shapes(osl.TINY_CFG).items()}
    with pytest.raises(NotImplementedError):
        Siglip2Model(dict(vision=dict(osl.TINY_CFG["vision"], hidden_size=192, num_attention_heads=3), text=osl.TINY_CFG["text"]))


def test_tokenizer_wrapper_cleaning_and_padding(tmp_path):
    """univid_amd.wan.tokenizers.HuggingfaceTokenizer (reference tokenizers.py:38-82): cleaning modes, padding / truncation to seq_len,
    the (ids, mask) pair T5EncoderModel consumes. The tokenizer files are a tiny word-level vocabulary built here."""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from univid_amd.wan.tokenizers import HuggingfaceTokenizer, clean_text
    assert clean_text("  a &amp;amp; b\n\n c  ", "whitespace") == "a & b c"
    assert clean_text(" Hello   World ", "lower") == "hello world"
    assert clean_text("A_cat, sitting! (on) a_mat.", "canonicalize") == "a cat sitting on a mat"
    assert clean_text("  keep  me ", None) == "  keep  me "
    with pytest.raises(ValueError):
        clean_text("x", "shout")
    vocab = {"<pad>": 0, "</s>": 1, "<unk>": 2, "a": 3, "cat": 4, "on": 5, "mat": 6, "&": 7}
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    PreTrainedTokenizerFast(tokenizer_object=tok, pad_token="<pad>", eos_token="</s>", unk_token="<unk>").save_pretrained(tmp_path)
    t = HuggingfaceTokenizer(str(tmp_path), seq_len=6, clean="whitespace")
    ids, mask = t(["a   cat  on a mat on a mat", "cat &amp; dog"], return_mask=True, add_special_tokens=True)
    assert ids.shape == (2, 6) and mask.shape == (2, 6)
    assert ids[0].tolist() == [3, 4, 5, 3, 6, 5] and mask[0].tolist() == [1] * 6          # truncated to seq_len
    assert ids[1].tolist() == [4, 7, 2, 0, 0, 0] and mask[1].tolist() == [1, 1, 1, 0, 0, 0]  # cleaned, unknown word, padded
    assert t("a cat").shape == (1, 6) and t.vocab_size == len(vocab)


def test_lora_wrapped_linear_is_rejected_not_ignored():
    """PEFT's lora.Linear exposes `.weight` = base_layer.weight (reference LoRAManager, model_pipeline.py:340-380): reading it
    would drop the adapter silently; the weight preparation must refuse it and say how to merge."""
    from univid_amd.wan.model import _Prepared

    class FakeLoraLinear(torch.nn.Module):      # the attribute surface of peft.tuners.lora.Linear
        def __init__(self, base):
            super().__init__()
            self.base_layer = base
            self.lora_A = torch.nn.ModuleDict({"default": torch.nn.Linear(base.in_features, 4, bias=False)})
            self.lora_B = torch.nn.ModuleDict({"default": torch.nn.Linear(4, base.out_features, bias=False)})

        @property
        def weight(self):
            return self.base_layer.weight

        @property
        def bias(self):
            return self.base_layer.bias

    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        _Prepared(FakeLoraLinear(torch.nn.Linear(8, 8)))
    m = WanModel(model_type="ti2v", in_dim=48, out_dim=48, dim=256, ffn_dim=512, num_heads=4, num_layers=1, text_len=32, text_dim=64)
    m.blocks[0].self_attn.q = FakeLoraLinear(m.blocks[0].self_attn.q)
    with pytest.raises(NotImplementedError, match="LoRA"):
        m.blocks[0].self_attn.prepare()


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """A .so built from other kernel sources than the tree's (old local objects after a pull) must not load silently."""
    from univid_amd import build
    lib = _lib.load()
    assert lib.uv_build_id().decode() == build.source_id()
    monkeypatch.setattr(build, "source_id", lambda: "0" * 24)
    with pytest.raises(_lib.UnividHipError, match="rebuild"):
        _lib._check_build_id(lib, _lib.LIB_PATH)


def test_calls_refuse_host_or_mixed_device_pointers():
    """Every entry point runs on the device of its tensors; a host tensor (or tensors of two GPUs) is an error, not a launch."""
    a = torch.zeros(4, 8)
    with pytest.raises(_lib.UnividHipError, match="ONE GPU"):
        _lib.call("uv_cast_f32_bf16", _lib.ptr(a), _lib.ptr(a), 32, _lib.stream_ptr())
    p, q = _lib.ptr(a), _lib.ptr(a)
    p.dev, q.dev = 0, 1
    with pytest.raises(_lib.UnividHipError, match="ONE GPU"):
        _lib.call("uv_cast_f32_bf16", p, q, 32, _lib.stream_ptr())


def test_bench_bare_multi_gpu_invocation_starts_one_rank_per_gpu():
    """`python bench.py --gpus N` without a launcher: the parent (which never touches the GPU) starts
    `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` as a CHILD and relays its output; under the
    launcher, WORLD_SIZE must equal --gpus. Dry run: the ranks print their environment and exit before any GPU call."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, UV_BENCH_DRYRUN="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert sorted(l["rank"] for l in lines) == [0, 1] and all(l["world"] == 2 and l["gpus"] == 2 for l in lines), r.stdout
    # a launcher world that disagrees with --gpus is an error, not a silent run
    env2 = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2")
    env2.pop("UV_BENCH_DRYRUN", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env2, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2 but --gpus 4" in (r.stderr + r.stdout)


def test_lora_adapter_directory_is_parsed_merged_and_unloaded(tmp_path):
    """univid_amd.lora on the host: PEFT key formats (with / without the adapter name, safetensors / .bin / the reference's manual
    lora_weights.pt), scaling rules, merged weight == peft's get_delta_weight arithmetic (oracle/lora.py), bit-exact unload, loud errors."""
    import json
    from safetensors.torch import save_file
    from oracle import lora as ora, wan_dit
    from univid_amd import lora
    cfg = dict(wan_dit.TINY_CFG)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(wan_dit.make_state_dict(cfg, 0))
    g = torch.Generator().manual_seed(0)
    r = 4
    tgt = {"blocks.0.cross_attn.q": (256, 256), "blocks.1.self_attn.o": (256, 256), "blocks.1.ffn.0": (512, 256)}
    fac = {n: (torch.randn(r, i, generator=g), torch.randn(o, r, generator=g)) for n, (o, i) in tgt.items()}
    base = {n: dict(m.named_modules())[n].weight.detach().clone() for n in tgt}

    def write(d, mid, fmt, **over):
        d.mkdir()
        (d / "adapter_config.json").write_text(json.dumps({**dict(r=r, lora_alpha=8, use_rslora=False, use_dora=False, bias="none"), **over}))
        t = {}
        for n, (a, b) in fac.items():
            t[f"base_model.model.{n}.lora_A{mid}.weight"], t[f"base_model.model.{n}.lora_B{mid}.weight"] = a, b
        if fmt == "safetensors":
            save_file(t, str(d / "adapter_model.safetensors"))
        else:
            torch.save(t, str(d / fmt))
        return str(d)

    for i, (mid, fmt, over, scale) in enumerate([("", "safetensors", {}, 2.0), (".default", "adapter_model.bin", {}, 2.0),
                                                  (".default", "lora_weights.pt", {"use_rslora": True}, 4.0)]):
        mgr = lora.LoRAManager()
        assert mgr.load_lora_weights(write(tmp_path / f"a{i}", mid, fmt, **over), m) is m
        assert m._prep is None, "merging must drop the prepared bf16 operands"
        for n, (a, b) in fac.items():
            assert torch.equal(dict(m.named_modules())[n].weight, ora.merged_weight(base[n], a, b, scale)), (fmt, n)
        assert mgr.get_statistics()["lora_modules"] == 3
        mgr.unload()
        for n in tgt:
            assert torch.equal(dict(m.named_modules())[n].weight, base[n]), "unload() restores the base weights bit for bit"
    with pytest.raises(NotImplementedError):
        lora.LoRAManager().load_lora_weights(write(tmp_path / "dora", "", "safetensors", use_dora=True), m)
    with pytest.raises(FileNotFoundError):
        lora.LoRAManager().load_lora_weights(str(tmp_path / "missing"), m)
    with pytest.raises(NotImplementedError):
        lora.LoRAManager().apply_lora_to_dit(m)
    with pytest.raises(KeyError):
        lora.merge_adapter_(m, {"blocks.0.norm3": fac["blocks.0.cross_attn.q"]}, dict(r=r, lora_alpha=8))
    with pytest.raises(ValueError):
        lora.adapter_factors({"base_model.model.blocks.0.cross_attn.q.lora_A.weight": fac["blocks.0.cross_attn.q"][0]})
    # no config file / no lora_alpha / per-module patterns: the scaling cannot be guessed (peft refuses too; its default alpha is 8, not r)
    nocfg = tmp_path / "nocfg"
    write(nocfg, ".default", "lora_weights.pt")
    (nocfg / "adapter_config.json").unlink()
    with pytest.raises(ValueError, match="lora_alpha"):
        lora.LoRAManager().load_lora_weights(str(nocfg), m)
    with pytest.raises(ValueError, match="lora_alpha"):
        lora.merge_adapter_(m, fac, dict(r=r))
    with pytest.raises(NotImplementedError, match="rank_pattern"):
        lora.LoRAManager().load_lora_weights(write(tmp_path / "rp", "", "safetensors", rank_pattern={"blocks.0.cross_attn.q": 8}), m)
    with pytest.raises(NotImplementedError, match="alpha_pattern"):
        lora.LoRAManager().load_lora_weights(write(tmp_path / "ap", "", "safetensors", alpha_pattern={"blocks.1.ffn.0": 32}), m)
    # an error on the LAST module must not leave the first ones merged (validation precedes mutation)
    with pytest.raises(KeyError):
        lora.merge_adapter_(m, {**fac, "blocks.0.norm3": fac["blocks.0.cross_attn.q"]}, dict(r=r, lora_alpha=8))
    for n in tgt:
        assert torch.equal(dict(m.named_modules())[n].weight, base[n]), "failed loads must leave the model untouched"


def test_context_cache_is_scoped_and_survives_inference_tensors():
    """the context cache keys on tensor identity + version counter, so it is OFF for the bare reference-signature forward and
    switched on only inside `context_cached()` (WanTI2V.denoise, bench.py); tensors made under torch.inference_mode() have no version
    counter and must not crash the key; the graph key uses a monotonic prepared-weights generation, not id()."""
    from oracle import wan_dit
    from univid_amd.wan.model import tensor_version
    m = WanModel.from_config(dict(wan_dit.TINY_CFG, model_type="ti2v"))
    assert m.cache_context is False
    with m.context_cached():
        assert m.cache_context is True
        with m.context_cached():
            assert m.cache_context is True
        assert m.cache_context is True, "the inner scope must not switch the outer one off"
    assert m.cache_context is False and m._ctx_cache is None
    with pytest.raises(ZeroDivisionError):
        with m.context_cached():
            1 / 0
    assert m.cache_context is False, "the scope must end on an exception too"
    with torch.inference_mode():
        u = torch.zeros(3)
    assert tensor_version(u) == -1 and tensor_version(torch.zeros(3)) == 0
    g0 = m._prep_gen
    m.invalidate()
    assert m._prep_gen == g0 + 1


def test_vt_cols_is_the_attention_kernels_layout():
    """_lib.vt_cols(batch, L): every sample but the last takes L columns, the last runs up to its 64-key tile bound."""
    want = {(1, 1): 64, (1, 64): 64, (1, 65): 128, (2, 512): 1024, (3, 8): 80}
    assert {k: _lib.vt_cols(*k) for k in want} == want


def test_context_kv_is_refused_before_any_device_work():
    """WanModel.forward(context_kv=): a wrong number of (k, V^T) pairs, mixed shapes and a re-assigned cross-attention forward raise
    their own errors on a model that has no device (preparing its weights would raise UnividHipError)."""
    from oracle import wan_dit
    cfg = wan_dit.TINY_CFG
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    x, small = torch.zeros(cfg["in_dim"], 4, 16, 16), torch.zeros(cfg["in_dim"], 2, 8, 8)
    kv = [(None, None)] * len(m.blocks)
    with pytest.raises(ValueError, match=r"1 \(k, V\^T\) pair\(s\) for 2 block"):
        m([x, x], None, None, 256, context_kv=kv[:1])
    with pytest.raises(ValueError, match="one shape"):
        m([x, small], None, None, 256, context_kv=kv)
    m.blocks[1].cross_attn.forward = lambda *a, **k: None
    with pytest.raises(NotImplementedError, match="re-assigned"):
        m([x, x], None, None, 256, context_kv=kv)
    del m.blocks[1].cross_attn.forward
    with pytest.raises(_lib.UnividHipError):
        m([x, x], None, None, 256, context_kv=kv)


def test_sample_offset_lives_on_a_module_for_the_hooked_call_only(monkeypatch):
    """The sample offset of per-sample adapter weights is an argument everywhere but in a re-assigned cross_attn.forward, which the block
    serves through WanCrossAttention._s0 for the length of that call: a closure sees it, and after a forward that raises midway - inside
    the closure, or before any block ran - no attention module carries a non-zero offset."""
    from oracle import wan_dit
    from univid_amd.wan import model as M

    class NoLaunch:                  # every entry point a no-op: the host path of a block runs without a device
        vt_cols = staticmethod(_lib.vt_cols)

        def __getattr__(self, name):
            return lambda *a, **k: None
    cfg = wan_dit.TINY_CFG
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))

    def offsets():
        return [mod._s0 for mod in m.modules() if hasattr(mod, "_s0")]
    assert offsets() == [0] * len(m.blocks) and not hasattr(m.blocks[0].self_attn, "_s0")
    with pytest.raises(_lib.UnividHipError):
        m([torch.zeros(cfg["in_dim"], 4, 16, 16)], torch.zeros(1), [torch.zeros(4, cfg["text_dim"])], 256)
    assert offsets() == [0] * len(m.blocks)
    monkeypatch.setattr(M, "_lib", NoLaunch())
    blk, seen, attn_kw = m.blocks[0], [], []
    blk.self_attn._self_attn = lambda *a, **k: attn_kw.append(k)

    def closure(x, context, context_lens=None):
        seen.append(blk.cross_attn._s0)
        raise RuntimeError("boom")
    blk.cross_attn.forward = closure
    C, Ls = cfg["dim"], 256
    with pytest.raises(RuntimeError, match="boom"):
        blk._run(torch.zeros(2 * Ls, C), Ls, torch.zeros(1, 6 * C), None, (4, 8, 8), None, torch.zeros(2 * 8, C, dtype=torch.bfloat16), False,
                 batch=2, s0=1)
    assert seen == [1] and attn_kw == [{"s0": 1}]
    assert offsets() == [0] * len(m.blocks)


def test_vae_pass_length_falls_back_when_memory_runs_out():
    """WanVAE_._with_pass_length: an out-of-memory error at `frames_per_pass` frames retries with half the pass length down to the
    reference's 1 (the result does not depend on it), with the engine and its workspace arena released first; at 1 the error propagates."""
    import types
    m = WanVAE_(dim=32, dec_dim=32, z_dim=48, dim_mult=(1, 2, 4, 4), temperal_downsample=(False, True, True))
    m._engine = types.SimpleNamespace(scratch={"k": 1})
    m._pool = object()
    m.frames_per_pass = 8
    seen = []

    def body(G, tag):
        seen.append(G)
        if G > 2:
            raise torch.cuda.OutOfMemoryError("simulated")
        return (tag, G)

    # (round 5: the engine's cached frames and rings live in the VAE's workspace arena: both are dropped before the retry)
    assert m._with_pass_length(body, "x") == ("x", 2) and seen == [8, 4, 2] and m._engine is None and m._pool is None

    def always(G):
        raise torch.cuda.OutOfMemoryError("simulated")

    with pytest.raises(torch.cuda.OutOfMemoryError):
        m._with_pass_length(always)


def test_pw4_attention_isa_audit():
    """The hand-placed diagnostic self-attention kernel (tools/diag/attn_pw4.hip) owns accumulator registers behind hipcc's back and places its own wait
    states: the compiled ISA must show no compiler access to the asm-owned a[0:215] outside the asm statements and no vector-ALU write directly in
    front of an MFMA that reads it (tools/diag/pw4_audit.py; both slips produced wrong tiles during development)."""
    import importlib.util, os, tempfile
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "diag", "pw4_audit.py")
    spec = importlib.util.spec_from_file_location("pw4_audit", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "attn_pw4.s")
        mod.compile_to_asm(out)
        findings = mod.audit(out)
        text = open(out).read()
    assert not findings, findings[:5]
    assert "scratch_" not in text.split("flash_attn_pw4_kernel")[1].split(".amdhsa_")[0], "the pw4 kernel must not touch scratch memory"


def test_upsample_phase_weights_reproduce_the_3x3_convolution_on_cpu():
    """Host logic of the round-4 phase decomposition (univid_amd/wan/vae2_2.py: _ConvOp.phases): Resample's "nearest-exact 2x + Conv2d 3x3"
    (vae2_2.py:86-96, 153-155) equals four 2x2 convolutions of the SOURCE image - output pixels (2y + a, 2x + b) from the taps' pre-summed
    weights with padding (1 - a, 1 - b) - checked here with plain torch ops on the CPU, incl. the zero padding at all four borders."""
    import torch.nn as nn
    import torch.nn.functional as F
    from univid_amd.wan.vae2_2 import _ConvOp
    torch.manual_seed(5)
    conv = nn.Conv2d(40, 24, 3, padding=1).double()
    op = _ConvOp(conv, is2d=True)                      # weights re-laid as [Cout, 3, 3, Cin_pad] (Cin padded 40 -> 64)
    x = torch.randn(2, 40, 5, 7, dtype=torch.float64)
    up = F.interpolate(x, scale_factor=2.0, mode="nearest-exact")
    ref = conv(up)
    out = torch.zeros(2, 24, 10, 14, dtype=torch.float64)
    for k, ph in enumerate(op.phases()):
        a, b = k >> 1, k & 1
        assert (ph.kt, ph.kh, ph.kw, ph.cout, ph.cin_pad) == (1, 2, 2, 24, 64)
        w = ph.w.view(24, 2, 2, 64)[..., :40].permute(0, 3, 1, 2).double()      # [Cout, Cin, 2, 2]
        # rows y + i - (1 - a), i in {0, 1}: pad (1 - a) rows on top and a rows at the bottom (the kernel's out-of-range taps read zero)
        xp = F.pad(x, (1 - b, b, 1 - a, a))
        out[:, :, a::2, b::2] = F.conv2d(xp, w, conv.bias)
    # the phase weights are the f32 roundings of fp64 sums of f32-rounded taps: compare against the convolution with THOSE taps
    conv32 = nn.Conv2d(40, 24, 3, padding=1).double()
    conv32.weight.data = conv.weight.data.float().double()
    conv32.bias.data = conv.bias.data.float().double()
    ref32 = conv32(up)
    assert (out - ref32).abs().max() <= 1e-6 * ref32.abs().max(), float((out - ref32).abs().max())
    assert (out - ref).abs().max() <= 1e-5 * ref.abs().max()


def test_f16x3_weight_scale_rule():
    """f16_weight_scale: a power of two, max |w| * scale in [2^13, 2^14) for every magnitude, 1.0 for zero / non-finite tensors."""
    import math
    from univid_amd.wan.vae2_2 import f16_weight_scale
    for mx in (1e-8, 3.1e-4, 0.02, 0.5, 1.0, 1.9999, 2.0, 77.0, 6.0e4, 1e9):
        sc = f16_weight_scale(mx)
        assert math.frexp(sc)[0] == 0.5 and 2.0 ** 13 <= mx * sc < 2.0 ** 14, (mx, sc)
    assert f16_weight_scale(0.0) == 1.0 and f16_weight_scale(float("inf")) == 1.0 and f16_weight_scale(float("nan")) == 1.0


def test_ctypes_signatures_match_the_header_argument_by_argument():
    """Every entry point's ctypes argument list (univid_amd/_lib.py: SIGNATURES) against its C declaration in include/univid_hip.h: same
    argument COUNT and the same class per argument (pointer / long / int / float) - a drifted signature would pass garbage through the
    C ABI without any loader error."""
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "univid_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)

    def cls_c(arg):
        arg = arg.strip()
        if "*" in arg:
            return "p"
        t = arg.split()[:-1] if len(arg.split()) > 1 else arg.split()
        t = " ".join(x for x in t if x != "const")
        return {"long": "l", "int": "i", "float": "f", "int32_t": "i"}.get(t, "?" + t)

    def cls_py(t):
        if t in (_lib._P, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
            return "p"
        return {_lib._L: "l", _lib._I: "i", _lib._F: "f"}.get(t, "?" + repr(t))

    n = 0
    for m in re.finditer(r"\b(?:int|long|const char\*)\s+(uv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        name, args = m.group(1), m.group(2).strip()
        c = [] if args in ("", "void") else [cls_c(a) for a in args.split(",")]
        py = [cls_py(t) for t in _lib.SIGNATURES[name]]
        assert c == py, f"{name}: header {c} vs ctypes {py}"
        n += 1
    assert n == len(_lib.SIGNATURES)



def test_ffn0_row_padding_never_adds_a_round_of_tiles():
    """WanAttentionBlock runs the first FFN projection on rows rounded up to whole 256-row tiles only where the padded row tile rides in
    the last, partial round of 256 x 256 tiles (univid_amd.wan.model._ffn0_rows): never an extra round, never for small problems."""
    from univid_amd.wan import model as M
    M._ncu["cpu-test"] = 256
    assert M._ffn0_rows(22880, 14336, "cpu-test") == 23040          # the metric's CFG pair: 19.47 -> 19.69 rounds
    assert M._ffn0_rows(54560, 14336, "cpu-test") == 54784          # UniVid's default workload
    assert M._ffn0_rows(22784, 14336, "cpu-test") == 22784          # whole tiles already
    assert M._ffn0_rows(22235, 14336, "cpu-test") == 22235          # 18.81 -> 19.03 rounds: the pad would cost a round
    assert M._ffn0_rows(1000, 14336, "cpu-test") == 1000            # under two rounds of tiles: the small-tile path
    assert M._ffn0_rows(22880, 14400, "cpu-test") == 22880          # columns not in whole tiles: not the persistent kernel's shape
    for L in range(2048, 60000, 997):
        Lp = M._ffn0_rows(L, 14336, "cpu-test")
        assert Lp == L or (Lp % 256 == 0 and 0 < Lp - L < 256 and -(-(Lp // 256 * 56) // 256) == -(-(L // 256 * 56) // 256))


def test_splitk_workspace_size_follows_the_gemm_plan():
    """uv_gemm_splitk_ws_bytes is one of the GEMM launch plan's two externally visible outputs (the other: uv_gemm_plan, pinned in
    test_gemm_launch_plan_is_pinned): the bytes the split-K strip of a tile_cfg 0
    call needs (4 096 + strip tiles x 4 slices x 256 KiB), 0 where the plan has no such strip. Without a device the library plans
    for 256 CUs, which is also what an MI355X reports."""
    lib = _lib.load()
    for M, N, K, want in [
        (22880, 3072, 14336, 62918656),     # 1 080 tiles = 4 rounds + 56 (under 45 % of a round): 21 760 rows persistent, a 1 120-row strip of 5 x 12 tiles
        (22880, 3072, 3072, 0),             # K < 8 192: the strip stays on the 128x128 ring
        (1024, 3072, 14336, 0),             # small shape
        (54560, 3072, 14336, 12587008),     # 32-row strip: 12 tiles
        (22784, 3072, 14336, 50335744),     # whole row tiles, short round: a 1 024-row strip
        (22235, 3072, 14336, 25169920),
        (22880, 3000, 14336, 0),            # N not in whole tiles
    ]:
        assert lib.uv_gemm_splitk_ws_bytes(M, N, K) == want, (M, N, K)


def test_gemm_launch_plan_is_pinned():
    """uv_gemm_plan is plan_gemm's (csrc/gemm_bf16.hip) externally visible output: which rows of a uv_gemm_bf16_nt / uv_gemm_f16_nt call go to
    which kernel, in one or two steps. Without a device the library plans for 256 CUs, which is also what an MI355X reports.
    tests/test_gemm_kernels.py asserts the plan of every case it launches; here every threshold of plan_gemm is pinned from both sides."""
    lib = _lib.load()
    BF, GELU, F32, RES, GATE, TR, SSQ = range(7)
    BIG = 1 << 40

    def plan(M, N, K, epi=BF, ldo=None, cfg=0, f16=False, ws=0):
        return [(s["kernel"], s["m0"], s["rows"]) for s in _lib.gemm_plan(M, N, K, epi, ldo, cfg, f16, ws)]

    # the name table next to enum GemmKernel
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "gemm_bf16.hip")).read()
    names = re.findall(r'"([^"]+)"', re.search(r"kGemmKernelName\[[^\]]*\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1))
    assert names == ["PERSIST", "PINGPONG", "RING128", "T128", "T256", "T256x192", "SPLITK4", "SPLITK2", "DIAG"]

    # ---- the numbered configurations: the whole problem on one kernel, whatever the shape
    for cfg, name in ((1, "T128"), (5, "T256"), (6, "T256x192"), (7, "PINGPONG"), (12, "RING128"), (17, "PERSIST"), (19, "SPLITK4"), (20, "SPLITK2"),
                      (2, "DIAG2"), (3, "DIAG3"), (4, "DIAG4"), (10, "DIAG10"), (11, "DIAG11"), (13, "DIAG13"), (14, "DIAG14")):
        for M, N, K in ((1, 16, 64), (4156, 4096, 384)):
            assert plan(M, N, K, cfg=cfg) == [(name, 0, M)], (cfg, M, N, K)
    # 8 / 9: the whole rounds of 256 x 256 tiles, the rest as a strip. 17 x 16 tiles = one round of 256 and 16 tiles: 4 096 rows + 60
    assert plan(4156, 4096, 256, cfg=8) == [("PINGPONG", 0, 4096), ("RING128", 4096, 60)]
    assert plan(4156, 4096, 256, cfg=9) == [("T256", 0, 4096), ("RING128", 4096, 60)]
    assert plan(4352, 4096, 256, cfg=8) == [("PINGPONG", 0, 4096), ("RING128", 4096, 256)]
    assert plan(1000, 512, 256, cfg=8) == [("PINGPONG", 0, 1000)]            # under one round: a cut of 0
    assert plan(4095, 4096, 256, cfg=9) == [("T256", 0, 4095)]               # 255 tiles: a cut of 0
    assert plan(4096, 4096, 256, cfg=8) == [("PINGPONG", 0, 4096)]           # exactly one round: the cut is M
    assert plan(4000, 4096, 256, cfg=9) == [("T256", 0, 4000)]               # 16 x 16 tiles, the last row tile ragged: cut 4 096 >= M
    # 18: the persistent kernel on the whole 256-row tiles; in whole tiles, the whole-rounds cut
    assert plan(4156, 4096, 384, cfg=18) == [("PERSIST", 0, 4096), ("RING128", 4096, 60)]
    assert plan(700, 1024, 384, cfg=18) == [("PERSIST", 0, 512), ("RING128", 512, 188)]
    assert plan(4352, 4096, 384, cfg=18) == [("PERSIST", 0, 4096), ("RING128", 4096, 256)]
    assert plan(200, 1024, 384, cfg=18) == [("PERSIST", 0, 200)]             # no whole tile, under one round: a cut of 0
    assert plan(4096, 4096, 384, cfg=18) == [("PERSIST", 0, 4096)]           # whole tiles, exactly one round: the cut is M

    # ---- tile_cfg 0, the large path (persistent / ping-pong kernel): on and off at each of its conditions
    assert plan(2048, 1024, 384) == [("PINGPONG", 0, 2048)]
    assert plan(2047, 1024, 384) == [("RING128", 0, 2047)]                   # M < 2 048: 16 x 8 tiles of 128
    assert plan(2048, 768, 384) == [("RING128", 0, 2048)]                    # N < 1 024
    assert plan(2048, 1280, 384) == [("PINGPONG", 0, 2048)]
    assert plan(2048, 1264, 384) == [("T256", 0, 2048)]                      # N % 256
    assert plan(2048, 1024, 448) == [("T256", 0, 2048)]                      # K % 128
    assert plan(2048, 1024, 256) == [("T256", 0, 2048)]                      # K < 384
    # ldo % 8 by epilogue class: 16-bit row-major outputs need it, the f32 ones and the transposed one do not (the transposed one falls
    # back from the persistent to the one-tile kernel instead)
    for epi in (BF, GELU):
        assert plan(8192, 4096, 384, epi, ldo=4096 + 8) == [("PERSIST", 0, 8192)]
        assert plan(8192, 4096, 384, epi, ldo=4096 + 4) == [("T256", 0, 8192)]
    for epi in (F32, RES, GATE):
        assert plan(8192, 4096, 384, epi, ldo=4096 + 4) == [("PERSIST", 0, 8192)]
    assert plan(8192, 4096, 384, SSQ, ldo=4096 + 8) == [("PERSIST", 0, 8192)]
    with pytest.raises(_lib.UnividHipError, match="ldo"):
        plan(8192, 4096, 384, SSQ, ldo=4096 + 4)
    assert plan(8192, 4096, 384, TR, ldo=8192 + 8) == [("PERSIST", 0, 8192)]
    assert plan(8192, 4096, 384, TR, ldo=8192 + 4) == [("PINGPONG", 0, 8192)]
    # two rounds of whole tiles: 511 tiles (73 x 7) the one-tile kernel, 512 (64 x 8) the persistent one
    assert plan(18688, 1792, 384) == [("PINGPONG", 0, 18688)]
    assert plan(16384, 2048, 384) == [("PERSIST", 0, 16384)]
    assert plan(18944, 1792, 384) == [("PINGPONG", 0, 18688), ("RING128", 18688, 256)]       # 518 tiles = 2 rounds + 6: short round, 511 tiles before the cut
    assert plan(8292, 4096, 384) == [("PERSIST", 0, 8192), ("RING128", 8192, 100)]           # 33 x 16 = 2 rounds + 16
    assert plan(4156, 4096, 384) == [("PINGPONG", 0, 4096), ("RING128", 4096, 60)]           # 17 x 16 = 1 round + 16
    assert plan(8392, 4096, 384) == [("PERSIST", 0, 8192), ("RING128", 8192, 200)]           # no short round without a whole round: rows beyond the last whole tile
    assert plan(2100, 1024, 384) == [("PINGPONG", 0, 2100)]                                  # under one round: never a short round
    # the short round: a partial round under 45 % of the CUs (115 of 256 tiles) is cut off with its rows, 116 tiles are not
    assert plan(17152, 4352, 384) == [("PERSIST", 0, 15360), ("RING128", 15360, 1792)]       # 67 x 17 = 4 x 256 + 115
    assert plan(24320, 3072, 384) == [("PERSIST", 0, 24320)]                                 # 95 x 12 = 4 x 256 + 116
    assert plan(24300, 3072, 384) == [("PERSIST", 0, 24064), ("RING128", 24064, 236)]        # the same tiles, ragged: only the rows beyond the last whole tile

    # ---- the split-K strip (needs a workspace; K >= 8 192, K % 512 == 0, 4 x strip tiles <= CUs, epilogues 0 / 3 / 4, bf16)
    need = 4096 + 5 * 12 * 4 * 262144
    for epi in (BF, RES, GATE):
        assert plan(22880, 3072, 14336, epi, ws=need) == [("PERSIST", 0, 21760), ("SPLITK4", 21760, 1120)]
    for epi in (GELU, F32, TR, SSQ):
        assert plan(22880, 3072, 14336, epi, ldo=22880 if epi == TR else None, ws=need) == [("PERSIST", 0, 21760), ("RING128", 21760, 1120)]
    assert plan(22880, 3072, 14336, RES, ws=need - 1) == [("PERSIST", 0, 21760), ("RING128", 21760, 1120)]
    assert plan(22880, 3072, 14336, RES) == [("PERSIST", 0, 21760), ("RING128", 21760, 1120)]
    assert plan(22880, 3072, 14336, RES, f16=True, ws=need) == [("PERSIST", 0, 21760), ("RING128", 21760, 1120)]
    assert plan(22880, 3072, 8192, RES, ws=need) == [("PERSIST", 0, 21760), ("SPLITK4", 21760, 1120)]
    assert plan(22880, 3072, 8064, RES, ws=need) == [("PERSIST", 0, 21760), ("RING128", 21760, 1120)]          # K < 8 192
    assert plan(22880, 3072, 8192 + 128, RES, ws=need) == [("PERSIST", 0, 21760), ("RING128", 21760, 1120)]    # K % 512
    assert plan(54560, 3072, 14336, GATE, ws=BIG) == [("PERSIST", 0, 54528), ("SPLITK4", 54528, 32)]           # no short round: the ragged rows
    assert plan(9216, 4096, 8192, RES, ws=BIG) == [("PERSIST", 0, 8192), ("SPLITK4", 8192, 1024)]              # 4 x 16 = 64 strip tiles: 256 workgroups
    assert plan(16384, 3328, 8192, RES, ws=BIG) == [("PERSIST", 0, 15104), ("RING128", 15104, 1280)]           # 5 x 13 = 65 strip tiles
    # the seven sizes test_splitk_workspace_size_follows_the_gemm_plan pins: the workspace of the plan's last step
    for M, N, K, want in [(22880, 3072, 14336, 62918656), (22880, 3072, 3072, 0), (1024, 3072, 14336, 0), (54560, 3072, 14336, 12587008),
                          (22784, 3072, 14336, 50335744), (22235, 3072, 14336, 25169920), (22880, 3000, 14336, 0)]:
        if N % 16:              # a shape the call itself refuses (uv_gemm_splitk_ws_bytes has no error return: 0)
            with pytest.raises(_lib.UnividHipError, match="multiple of 16"):
                plan(M, N, K, RES, ws=BIG)
            last = (None, 0, 0)
        else:
            last = plan(M, N, K, RES, ws=BIG)[-1]
        size = 4096 + -(-last[2] // 256) * -(-N // 256) * 4 * 262144 if last[0] == "SPLITK4" else 0
        assert size == want == lib.uv_gemm_splitk_ws_bytes(M, N, K), (M, N, K, last)

    # ---- tile_cfg 0, M < 2 048 or N < 1 024
    # tall and narrow: whole 256-row tiles, M >= 4 096, 512 <= N, K % 128 == 0, K >= 256, ldo % 8 == 0 and at least half a round of tiles
    assert plan(16384, 512, 256) == [("PINGPONG", 0, 16384)]                 # 2 x 64 x 2 = 256
    assert plan(16128, 512, 256) == [("RING128", 0, 16128)]                  # 2 x 63 x 2 = 252 (an even number: 255 cannot occur); 126 x 4 = 504 tiles of 128
    assert plan(11008, 768, 256) == [("PINGPONG", 0, 11008)]                 # 2 x 43 x 3 = 258
    assert plan(10752, 768, 256) == [("RING128", 0, 10752)]                  # 2 x 42 x 3 = 252; 84 x 6 = 504
    assert plan(11008, 768, 256, ldo=772) == [("T128", 0, 11008)]            # 86 x 6 = 516 tiles of 128
    assert plan(11008, 768, 192) == [("T128", 0, 11008)]
    assert plan(11009, 768, 256) == [("T128", 0, 11009)]
    assert plan(16384, 528, 256) == [("T128", 0, 16384)]
    assert plan(16384, 256, 256) == [("RING128", 0, 16384)]                  # N < 512: 128 x 2 tiles of 128
    # tiles of 128: at most two per CU on the 8-wave ring, more on the 4-wave kernel
    assert plan(1024, 8192, 64) == [("RING128", 0, 1024)]                    # 8 x 64 = 512
    assert plan(1152, 7296, 64) == [("T128", 0, 1152)]                       # 9 x 57 = 513
    assert plan(1, 16, 64) == [("RING128", 0, 1)]

    # ---- tile_cfg 0, everything else: 256 x 192 tiles where they cost less than 256 x 256
    assert plan(2048, 1152, 64) == [("T256x192", 0, 2048)]
    assert plan(2048, 1168, 64) == [("T256", 0, 2048)]                       # N % 192
    assert plan(2048, 1152, 4096) == [("T256x192", 0, 2048)]
    assert plan(2048, 1152, 4160) == [("T256", 0, 2048)]                     # K > 4 096
    assert plan(2048, 1152, 64, SSQ) == [("T256", 0, 2048)]                  # 48 columns per wave: no whole 32-column groups
    assert plan(2048, 1152, 64, f16=True) == [("T256", 0, 2048)]             # not built for fp16
    assert plan(4096, 3072, 64) == [("T256x192", 0, 4096)]                   # 16 x 16 = 256 tiles of 192 columns: one round x 0.78
    assert plan(4352, 3072, 64) == [("T256", 0, 4352)]                       # 17 x 16 = 272: two rounds x 0.78 against one of 256 x 256
    # fp16: the same plan on the five kernels built for it
    assert plan(8292, 4096, 384, f16=True) == [("PERSIST", 0, 8192), ("RING128", 8192, 100)]
    assert plan(1152, 7296, 64, f16=True) == [("T128", 0, 1152)]
    assert plan(2048, 1024, 384, f16=True) == [("PINGPONG", 0, 2048)]

    # ---- the shape checks of the call itself
    for bad, match in ((dict(M=0), "bad shape"), (dict(K=96), "multiple of 64"), (dict(N=24), "multiple of 16"), (dict(ldo=514), "ldo"),
                       (dict(epi=7), "epilogue"), (dict(epi=SSQ, N=528, ldo=528), "N %"), (dict(f16=True, cfg=7), "fp16")):
        a = dict(M=300, N=512, K=256)
        a.update(bad)
        with pytest.raises(_lib.UnividHipError, match=match):
            plan(**a)
    n = ctypes.c_int()
    assert lib.uv_gemm_plan(300, 512, 256, 0, 512, 0, 0, 0, ctypes.byref(n), None, 32, None, None) != 0


def test_attention_launch_plan_is_pinned():
    """uv_flash_attn_plan is plan_attn's (csrc/attn_args.h) externally visible output: the kernel, the query blocks per (sample, head), how
    many of them own 12 units and the grid of an attention launch. Without a device the library plans for 256 CUs, which is also what an
    MI355X reports. The numeric cuts are what the list-scheduling model gave before it moved into plan_attn."""
    lib = _lib.load()
    _lib.reset_options()

    def plan(B, H, Lq, Lk, D=128, f16=False, ldk=None):
        buf, qb, n12, grid = ctypes.create_string_buffer(96), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ldvt = (B - 1) * Lk + (Lk + 63) // 64 * 64
        rc = lib.uv_flash_attn_plan(B, Lq, Lk, H, D, H * D if ldk is None else ldk, ldvt, int(f16), buf, 96, ctypes.byref(qb), ctypes.byref(n12),
                                    ctypes.byref(grid))
        assert rc == 0, lib.uv_last_error()
        return buf.value.decode(), n12.value, qb.value - n12.value, grid.value        # kernel, n12, n8 (fwd12) / blocks of 128 queries, grid

    F12, F3 = "flash_attn_fwd12_kernel", "flash_attn_fwd3_kernel"
    assert plan(2, 24, 11440, 11440) == (F12, 26, 6, 1536)        # the bench shape
    assert plan(1, 24, 11440, 11440) == (F12, 30, 0, 720)
    assert plan(2, 24, 27280, 27280) == (F12, 69, 4, 3504)        # UniVid's default workload
    assert plan(1, 24, 27280, 27280) == (F12, 72, 0, 1728)
    assert plan(2, 2, 500, 2104) == (F12, 0, 2, 8)
    assert plan(1, 24, 11440, 2047) == (F3, 0, 90, 90 * 24)       # one Lk below the threshold: 4-wave workgroups, ceil(Lq / 128) blocks
    assert plan(1, 3, 129, 2047) == (F3, 0, 2, 6)
    assert plan(1, 24, 11440, 2048)[0] == F12
    assert plan(2, 4, 260, 2104, D=64) == ("flash_attn_fwd_kernel<64>", 0, 3, 24)
    assert plan(2, 4, 260, 2104, f16=True) == ("flash_attn_fwd_kernel<128>", 0, 3, 24)
    assert plan(1, 4, 260, 2104, ldk=1 << 24) == ("flash_attn_fwd_kernel<128>", 0, 3, 12)      # 64 * ldk >= 2^30: past the 32-bit lane offsets
    assert plan(1, 4, 260, 2104, ldk=(1 << 24) - 8)[0] == F12
    assert _lib.attn_plan(11440, 11440, 128, batch=2, H=24) == dict(kernel=F12, q_blocks=32, n12=26, grid=1536)
    assert _lib.attn_kernel_name(11440, 512, 128, 2, H=24) == F3
    try:
        for Lq, H, B in ((11440, 24, 2), (500, 4, 2), (500, 2, 2), (33, 1, 1)):
            nwu = -(-Lq // 32)
            for v in (1, 2, 3, 4, 7, 45, 46, 60):
                _lib.set_option(_lib.OPT_ATTN_CUT, v)
                n8 = v - 1
                n12 = max(0, -(-(nwu - 8 * n8) // 12))
                assert plan(B, H, Lq, 2104) == (F12, n12, n8, (n12 + n8) * H * B), (Lq, v)
                assert plan(B, H, Lq, 512)[1:] == (0, -(-Lq // 128), -(-Lq // 128) * H * B), "the option only concerns the 12-wave kernel"
    finally:
        _lib.reset_options()
    assert plan(2, 24, 11440, 11440) == (F12, 26, 6, 1536)
    assert lib.uv_flash_attn_plan(1, 0, 64, 1, 128, 128, 64, 0, ctypes.create_string_buffer(8), 8, None, None, None) != 0


def test_conv_launch_plan_is_pinned():
    """uv_conv3d_plan is plan_conv's (csrc/conv_args.h) externally visible output: which of the 23 convolution kernels a uv_conv3d_* call
    launches, on how many row tiles (halo kernels: pixel patches) x output-channel tiles. Without a device the library plans for 256 CUs,
    which is also what an MI355X reports; the big-tile thresholds are literal numbers either way. tests/test_conv_kernels.py asserts the
    plan of every case it launches; here the thresholds themselves are pinned from both sides."""
    lib = _lib.load()
    _lib.reset_options()

    def plan(prec, Tout, Hout, Wout, Hin, Win, Cin, Cout, kt, kh, kw, **kw_):
        p = _lib.conv_plan(prec, Tout, Hout, Wout, Hin, Win, Cin, Cout, kt, kh, kw, **kw_)
        return p["kernel"], p["tiles_m"], p["tiles_n"]

    # the name table next to enum ConvKernel: 23 distinct names
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "conv_args.h")).read()
    names = re.findall(r'"([^"]+)"', re.search(r"kConvKernelName\[[^\]]*\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1))
    assert len(names) == 23 and len(set(names)) == 23

    down = dict(sh=2, sw=2)        # Resample's stride-2 1x3x3 behind ZeroPad2d(0, 1, 0, 1)
    for prec in (1, 2, 4):
        # case A: 32 600 pixels = 128 tiles of 256 rows; x 2 column tiles = 256 workgroups, the threshold itself
        assert plan(prec, 1, 163, 200, 326, 400, 32, 160, 1, 3, 3, **down) == (f"G256x128+{prec}", 128, 2)
        assert plan(prec, 1, 163, 200, 326, 400, 32, 320, 1, 3, 3, **down) == (f"G256x256+{prec}", 128, 2)
        # case B: 32 437 pixels = 127 tiles of 256 rows: 254 workgroups, one row tile below the threshold
        assert plan(prec, 1, 163, 199, 326, 398, 32, 160, 1, 3, 3, **down) == (f"G128x128+{prec}", 254, 2)
        # case C: 127 row tiles x 2 tiles of 256 columns = 254 misses by two; x 3 tiles of 128 columns does not
        assert plan(prec, 1, 127, 256, 254, 512, 32, 320, 1, 3, 3, **down) == (f"G256x128+{prec}", 127, 3)
        assert plan(prec, 1, 127, 256, 254, 512, 32, 128, 1, 3, 3, **down) == (f"G128x128+{prec}", 254, 1)
        # Cout < 256 never takes the 256-wide tile, however many rows
        assert plan(prec, 2, 163, 200, 326, 400, 32, 252, 1, 3, 3, **down) == (f"G256x128+{prec}", 255, 2)
        # the other launch forms plan alike: time_conv with interleave, an output-phase launch, 1x1x1
        assert plan(prec, 1, 163, 200, 163, 200, 32, 512, 3, 1, 1, interleave=1) == (f"G256x256+{prec}", 128, 2)
        assert plan(prec, 1, 163, 200, 163, 200, 32, 320, 1, 2, 2, ph=1, pw=0, up=3) == (f"G256x256+{prec}", 128, 2)
        assert plan(prec, 1, 110, 200, 110, 200, 32, 640, 1, 1, 1) == (f"G256x256+{prec}", 86, 3)
        assert plan(prec, 1, 108, 200, 108, 200, 32, 640, 1, 1, 1) == (f"G256x128+{prec}", 85, 5)      # 85 x 3 = 255
    # narrow and 160-wide outputs, 3 x 19 x 23 = 1 311 pixels
    small = (3, 19, 23, 19, 23, 64)
    for prec in (0, 3, 4):
        assert plan(prec, *small, 12, 3, 3, 3, ph=1, pw=1) == (f"G256x16+{prec}", 6, 1)
        assert plan(prec, *small, 16, 3, 3, 3, ph=1, pw=1) == (f"G256x16+{prec}", 6, 1)
        assert plan(prec, *small, 20, 3, 3, 3, ph=1, pw=1) == (f"G128x128+{prec}", 11, 1)
    for prec in (1, 2):
        assert plan(prec, *small, 12, 3, 3, 3, ph=1, pw=1) == (f"G128x128+{prec}", 11, 1)
    assert plan(0, *small, 160, 3, 3, 3, ph=1, pw=1) == ("G160+0", 11, 1)            # 128 rows per tile
    assert plan(0, *small, 320, 3, 3, 3, ph=1, pw=1) == ("G160+0", 11, 2)
    assert plan(3, *small, 160, 3, 3, 3, ph=1, pw=1) == ("G160+3", 21, 1)            # 64 rows per tile
    assert plan(3, *small, 320, 3, 3, 3, ph=1, pw=1) == ("G160+3", 21, 2)
    assert plan(0, *small, 640, 3, 3, 3, ph=1, pw=1) == ("G128x128+0", 11, 5)        # a multiple of 128 as well: 128-wide tiles
    for prec in (1, 2, 4):
        assert plan(prec, *small, 160, 3, 3, 3, ph=1, pw=1) == (f"G128x128+{prec}", 11, 2)
    # automatic: a halo kernel where four frames of patches fill 256 CUs (exact f32: twice that)
    assert plan(4, 1, 45, 80, 45, 80, 64, 128, 3, 3, 3, ph=1, pw=1) == ("G128x128+4", 29, 1)        # 4 x 15 patches
    assert plan(4, 1, 360, 640, 360, 640, 64, 128, 3, 3, 3, ph=1, pw=1) == ("HALO_F16_128", 900, 1)     # 920 square patches against 900
    assert plan(0, 1, 64, 128, 64, 128, 64, 128, 3, 3, 3, ph=1, pw=1) == ("G128x128+0", 64, 1)          # 4 x 64 patches of 8 x 16 < 512
    assert plan(0, 1, 64, 256, 64, 256, 64, 128, 3, 3, 3, ph=1, pw=1) == ("HALO_F32_128", 128, 1)       # 4 x 128 = 512
    try:
        _lib.set_option(_lib.OPT_CONV_HALO, 1)
        halo = lambda prec, T, H, W, ci, co, kt, up=0: plan(prec, T, H * (2 if up == 1 else 1), W * (2 if up == 1 else 1), H, W, ci, co, kt, 3, 3, ph=1, pw=1, up=up)
        assert halo(4, 2, 8, 32, 64, 128, 3) == ("HALO_F16_128", 2, 1)               # kt * Cin / 32 = 6
        assert halo(4, 2, 8, 32, 64, 256, 1) == ("HALO_F16_128", 2, 2)               # 2
        assert halo(4, 2, 8, 32, 32, 128, 3) == ("G128x128+4", 4, 1)                 # 3: odd, the gather kernel
        assert halo(4, 2, 8, 32, 96, 128, 1) == ("G128x128+4", 4, 1)                 # 3
        assert halo(4, 2, 8, 32, 96, 128, 3) == ("G128x128+4", 4, 1)                 # 9
        assert halo(4, 2, 16, 16, 64, 128, 3) == ("HALO_F16_SQUARE", 2, 1)           # one 16 x 16 patch against two 8 x 32
        assert halo(4, 2, 45, 80, 64, 128, 3) == ("HALO_F16_SQUARE", 30, 1)          # 15 against 18
        assert halo(4, 1, 13, 48, 64, 256, 1) == ("HALO_F16_SQUARE", 3, 2)           # 3 against 4
        assert halo(4, 2, 19, 23, 64, 128, 3) == ("HALO_F16_128", 6, 1)              # 4 against 3
        assert halo(4, 2, 19, 23, 64, 160, 3) == ("HALO_F16_160", 6, 1)
        assert halo(4, 2, 19, 23, 32, 320, 3) == ("HALO_F16_160", 6, 2)              # no parity rule on the 160-wide kernel
        assert halo(4, 3, 19, 40, 64, 12, 3) == ("HALO_F16_N16", 18, 1)
        assert halo(4, 3, 19, 40, 64, 16, 1) == ("HALO_F16_N16", 18, 1)
        assert halo(4, 3, 19, 40, 64, 12, 1, up=1) == ("G256x16+4", 36, 1)           # the narrow halo kernel: plain geometry only
        assert halo(4, 3, 19, 40, 64, 96, 3) == ("G128x128+4", 18, 1)                # neither 128- nor 160-wide tiles
        assert halo(4, 2, 9, 13, 64, 128, 1, up=1) == ("HALO_F16_128", 6, 1)         # 18 x 26 upsampled: 3 patches a frame
        assert halo(0, 2, 19, 23, 64, 160, 3) == ("HALO_F32_160", 12, 1)             # exact f32: 8 x 16 patches
        assert halo(0, 2, 19, 23, 64, 320, 3) == ("HALO_F32_160", 12, 2)
        assert halo(0, 2, 19, 23, 32, 128, 3) == ("HALO_F32_128", 12, 1)
        assert halo(0, 2, 19, 23, 32, 384, 1) == ("HALO_F32_128", 12, 3)
        assert halo(0, 2, 19, 23, 32, 12, 3) == ("G256x16+0", 4, 1)
        assert halo(3, 2, 19, 23, 64, 128, 3) == ("HALO_BF16X6", 6, 1)
        assert halo(3, 2, 19, 23, 64, 256, 1) == ("HALO_BF16X6", 6, 2)
        assert halo(3, 2, 19, 23, 64, 160, 3) == ("G160+3", 14, 1)                   # bf16x6: whole 128-wide tiles only
        assert halo(3, 2, 19, 23, 64, 12, 3) == ("G256x16+3", 4, 1)
        for prec in (1, 2):
            assert halo(prec, 2, 19, 23, 64, 128, 3) == (f"G128x128+{prec}", 7, 1)   # bf16x3 has no halo kernel
        for prec in (0, 3, 4):
            # the halo geometry, but an output-phase launch (halo kernels store to plain positions) or interleave, a stride, another padding
            for up in (2, 3, 4, 5):
                assert plan(prec, 2, 19, 23, 19, 23, 64, 128, 1, 3, 3, ph=1, pw=1, up=up) == (f"G128x128+{prec}", 7, 1), (prec, up)
            assert plan(prec, 2, 19, 23, 19, 23, 64, 128, 3, 3, 3, ph=1, pw=1, interleave=1) == (f"G128x128+{prec}", 7, 1)
            assert plan(prec, 2, 19, 23, 19, 23, 64, 128, 3, 3, 3, ph=1, pw=1, st=2)[0] == f"G128x128+{prec}"
            assert plan(prec, 2, 19, 23, 19, 23, 64, 128, 3, 3, 3, ph=0, pw=1)[0] == f"G128x128+{prec}"
            assert plan(prec, 2, 10, 12, 19, 23, 64, 128, 1, 3, 3, ph=1, pw=1, sh=2, sw=2)[0] == f"G128x128+{prec}"
        _lib.set_option(_lib.OPT_CONV_HALO, 0)
        for prec in (0, 3, 4):
            assert halo(prec, 2, 19, 23, 64, 128, 3) == (f"G128x128+{prec}", 7, 1)
            assert halo(prec, 1, 360, 640, 64, 128, 3) == (("G256x128+4", 900, 1) if prec == 4 else (f"G128x128+{prec}", 1800, 1))
        assert halo(4, 3, 19, 40, 64, 12, 3) == ("G256x16+4", 9, 1)
        assert halo(0, 2, 19, 23, 64, 160, 3) == ("G160+0", 7, 1)
    finally:
        _lib.reset_options()
    # what conv_common refuses, the query refuses
    for bad in (dict(Cin=48), dict(Cout=10), dict(Tout=0), dict(up=6), dict(up=2, sh=2), dict(interleave=1, Cout=12), dict(prec=5)):
        a = dict(prec=0, Tout=2, Hout=19, Wout=23, Hin=19, Win=23, Cin=64, Cout=128, kt=1, kh=3, kw=3)
        a.update(bad)
        with pytest.raises(_lib.UnividHipError):
            _lib.conv_plan(**a)
    assert lib.uv_conv3d_plan(0, 2, 19, 23, 19, 23, 64, 128, 1, 3, 3, 1, 1, 1, 1, 1, 0, 0, None, 0, None, None) != 0


def test_graph_runner_cache_policy():
    """WanTI2V keeps the `max_graph_runners` most recently used captured graphs (host logic only - stand-ins for the runners; the replay
    itself is tests/test_gpu_parity.py::test_graph_runner_serves_new_prompts_without_recapture_and_never_goes_stale): a hit moves the
    runner to the most-recently-used end and builds nothing; a miss evicts the least recently used BEFORE building (the old graph's pool is
    free when the new capture allocates); another prepared-weights generation or text_len drops every held runner; a failing capture
    leaves nothing behind; `_runner` reads the last used one and can only be cleared."""
    import collections
    pipe = textimage2video.WanTI2V.__new__(textimage2video.WanTI2V)
    pipe._runners, pipe.max_graph_runners = collections.OrderedDict(), 2
    assert pipe._runner is None
    built, alive = [], set()

    class Runner:
        def __init__(self, name):
            self.name = name
            alive.add(name)

    def make(name, expect_alive=None):
        def f():
            if expect_alive is not None:
                assert {r.name for r in pipe._runners.values()} == expect_alive, "eviction must happen before the capture"
            built.append(name)
            return Runner(name)
        return f
    t2v, i2v, short = ((48, 13, 44, 80), False, 3, 512), ((48, 13, 44, 80), True, 3, 512), ((48, 4, 44, 80), False, 3, 512)
    a, fresh = pipe._runner_for(t2v, make("t2v"))
    assert fresh and pipe._runner is a
    b, fresh = pipe._runner_for(i2v, make("i2v", {"t2v"}))
    assert fresh and pipe._runner is b and list(pipe._runners) == [t2v, i2v]
    a2, fresh = pipe._runner_for(t2v, make("never"))
    assert a2 is a and not fresh and pipe._runner is a and list(pipe._runners) == [i2v, t2v] and built == ["t2v", "i2v"]
    c, fresh = pipe._runner_for(short, make("short", {"t2v"}))             # i2v is the least recently used: gone before the capture
    assert fresh and list(pipe._runners) == [t2v, short]
    # a capture that fails: the eviction it needed has happened, nothing is stored under its key
    def boom():
        raise RuntimeError("capture failed")
    with pytest.raises(RuntimeError):
        pipe._runner_for(i2v, boom)
    assert i2v not in pipe._runners and list(pipe._runners) == [short]
    # new prepared weights (generation 4): every held graph belongs to the old ones
    d, fresh = pipe._runner_for(((48, 13, 44, 80), False, 4, 512), make("regen", set()))
    assert fresh and len(pipe._runners) == 1 and pipe._runner is d
    pipe.max_graph_runners = 0                                              # never below one: the runner in use is always held
    e, _ = pipe._runner_for(((48, 13, 44, 80), True, 4, 512), make("one", set()))
    assert list(pipe._runners.values()) == [e]
    with pytest.raises(ValueError):
        pipe._runner = e
    pipe._runner = None
    assert pipe._runner is None and not pipe._runners


def test_fusion_pipeline_config_only_construction_refuses_loudly(tmp_path):
    """CrossAttentionFusionPipeline(config) as inference.py:196 calls it (model_pipeline.py:2112-2131): a missing checkpoint directory is
    the reference's FileNotFoundError (:2178-2180); an enabled BAGEL extraction without a registered extractor is an error naming
    `register_bagel_extractor`, never a silent stub; the registered factory receives the reference's four keyword arguments (:2153-2158);
    a GPU index this process does not have is named by its config field. No GPU is touched."""
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline, register_bagel_extractor
    with pytest.raises(FileNotFoundError, match="Wan2.2 model path not found"):
        CrossAttentionFusionPipeline(CrossAttentionConfig(wan_model_path=str(tmp_path / "missing")))
    cfg = CrossAttentionConfig(wan_model_path=str(tmp_path), bagel_model_path="/m/bagel", bagel_gpu=0, wan_gpu=0, cross_attn_gpu=0)
    prev = register_bagel_extractor(None)
    try:
        with pytest.raises(RuntimeError, match="register_bagel_extractor"):
            CrossAttentionFusionPipeline(cfg)
        seen = {}
        assert register_bagel_extractor(lambda **kw: seen.update(kw) or object()) is None
        with pytest.raises(RuntimeError, match="cross_attn_gpu"):      # 0 GPUs here: the next thing the constructor needs
            CrossAttentionFusionPipeline(cfg)
        assert seen == dict(model_path="/m/bagel", device_id=0, use_bfloat16=True, config=cfg)
    finally:
        register_bagel_extractor(prev)


def test_rank_host_policy_is_explicit_and_a_no_op_without_a_gpu():
    """univid_amd.parallel: the host-scheduling policy of a one-rank-per-GPU job is data the LAUNCHER applies (RANK_ENV, exported before the ranks
    import torch) plus an explicit per-device call (host_policy -> uv_host_blocking_sync); importing the package sets neither, and on a CPU
    device (the gloo tests) host_policy does nothing."""
    import univid_amd.parallel as par
    assert par.RANK_ENV == {"AMD_DIRECT_DISPATCH": "0", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    before = dict(os.environ)
    par.host_policy("cpu")
    par.host_policy(torch.device("cpu"), blocking_sync=False)
    assert dict(os.environ) == before and not par._blocking_set


def test_raw_pointer_calls_are_confined_to_lib():
    """univid_amd/_lib.py is the only file of the package that marshals pointers, leading dimensions and the stream: nothing else under
    univid_amd/ calls the C ABI raw, and every entry point of the signature table is reached by a wrapper or helper inside _lib.py."""
    pkg = os.path.join(ROOT, "univid_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            path = os.path.join(d, f)
            if f.endswith(".py") and path != os.path.join(pkg, "_lib.py"):
                txt = open(path).read()
                for raw in ("_lib.call(", "_lib.ptr(", "stream_ptr("):
                    assert raw not in txt, f"{os.path.relpath(path, ROOT)} contains {raw}"
    src = open(os.path.join(pkg, "_lib.py")).read()
    code = src[src.index("_RESTYPE ="):].split("\n", 1)[1]         # behind the signature tables
    for name in set(_lib.SIGNATURES) - {"uv_version"}:      # (read by the loaders' own sanity checks, nothing to wrap)
        assert re.search(rf'"{name}"|\.{name}\(', code), f"{name}: no wrapper or helper in _lib.py reaches it"


def _short(t, need):
    """t's shape and strides over a storage of need - 1 elements (one row fewer in the shape, so that the view itself is legal)."""
    shape = (t.shape[0] - 1,) + tuple(t.shape[1:])
    return torch.empty(need - 1, dtype=t.dtype).as_strided(shape, t.stride())


def _checker_cases():
    """(wrapper, positional arguments, {index of the argument to spoil: its name}, index and extent of the argument to shorten), one per
    shape class: rows + leading dimension, flat n, the convolution, the epilogue-dependent GEMM output."""
    f32, bf16 = torch.float32, torch.bfloat16
    z = torch.zeros
    w1 = z(4, 32)
    return {
        "linear_rows": (_lib.linear_rows, [z(3, 8), z(4, 8), z(4), z(3, 4)], {0: "x", 1: "W", 2: "b", 3: "out"}, (3, 12)),
        "vae_rms_silu": (_lib.vae_rms_silu, [z(2, 3, 2, 8), z(8), z(2, 3, 2, 8)], {0: "x", 1: "gamma", 2: "out"}, (2, 96)),
        "add_bf16": (_lib.add_bf16, [z(4, 8, dtype=bf16), z(4, 8, dtype=bf16), z(4, 8, dtype=bf16)], {0: "x", 1: "y"}, (0, 32)),
        "cfg_convert": (_lib.cfg_convert, [z(2, 4, 4), z(2, 4, 4), z(2, 4, 4), 3.0, 0.5, None, z(2, 4, 4)], {0: "cond", 1: "uncond", 2: "sample"},
                        (1, 32)),
        "conv3d": (lambda src, w, b, out, resid: _lib.conv3d("fp32", src, lambda kind: (w, 1.0), b, out, 3, 2, 2, 3, 2, 2, 32, 4, 1, 1, 1, resid=resid),
                   [z(3, 2, 2, 32), w1, z(4), z(3, 2, 2, 4), None], {0: "src", 1: "weights", 2: "bias", 3: "out"}, (3, 48)),
        "gemm_bf16": (lambda a, w, bias, out: _lib.gemm_bf16(a, w, bias, out, _lib.EPI_BF16),
                      [z(4, 64, dtype=bf16), z(16, 64, dtype=bf16), None, z(4, 16, dtype=bf16)], {0: "a", 1: "w", 3: "out"}, (3, 64)),
    }


@pytest.mark.parametrize("case", sorted(_checker_cases()))
def test_wrappers_check_dtype_layout_and_extent_before_the_library_is_touched(case, monkeypatch):
    """Every pointer argument of a wrapper is checked from tensor metadata - dtype, then layout, then that the extent the kernel addresses
    fits in the tensor's STORAGE - and only then the device, so CPU tensors exercise the first three: each failure is a UnividHipError that
    names wrapper and argument, optional arguments may be None, and nothing is launched or even loaded."""
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a rejected call reached the library"))
    fn, args, names, (si, need) = _checker_cases()[case]
    E = _lib.UnividHipError
    with pytest.raises(E, match=rf"{case}\.{names[0]}: tensor must live on the GPU"):      # well-formed: only the device is wrong
        fn(*args)
    for i, name in names.items():
        bad = list(args)
        bad[i] = args[i].to(torch.float64)
        with pytest.raises(E, match=rf"{case}\.{name}: expected"):
            fn(*bad)
        if args[i].dim() >= 2:
            bad[i] = args[i].transpose(-1, -2).contiguous().transpose(-1, -2)             # same shape, innermost stride != 1
            with pytest.raises(E, match=rf"{case}\.{name}: (innermost dimension )?must be contiguous"):
                fn(*bad)
    bad = list(args)
    bad[si] = _short(args[si], need)
    with pytest.raises(E, match=rf"{case}\.{names[si]}: the kernel addresses {need} elements, the tensor's storage holds {need - 1}"):
        fn(*bad)
    bad[si] = torch.empty(need, dtype=args[si].dtype).as_strided(bad[si].shape, bad[si].stride())    # the same view over enough storage
    with pytest.raises(E, match="must live on the GPU"):
        fn(*bad)


def test_gemm_output_dtype_and_shape_follow_the_epilogue():
    """gemm_bf16's `out` is checked against what the epilogue writes: 16-bit rows, f32 rows, or the [N, M] transpose."""
    bf16 = torch.bfloat16
    a, w = torch.zeros(4, 64, dtype=bf16), torch.zeros(16, 64, dtype=bf16)
    o16, o32, oT = torch.zeros(4, 16, dtype=bf16), torch.zeros(4, 16), torch.zeros(16, 4, dtype=bf16)
    E = _lib.UnividHipError
    for epi, good, wrong in ((_lib.EPI_BF16, o16, o32), (_lib.EPI_GELU_BF16, o16, o32), (_lib.EPI_F32_FROM_BF16, o32, o16),
                             (_lib.EPI_RESID_F32, o32, o16), (_lib.EPI_GATE_RESID_F32, o32, o16), (_lib.EPI_BF16_T, oT, o32)):
        with pytest.raises(E, match="gemm_bf16.out: expected"):
            _lib.gemm_bf16(a, w, None, wrong, epi)
        with pytest.raises(E, match="gemm_bf16.a: tensor must live on the GPU"):
            _lib.gemm_bf16(a, w, None, good, epi)
    with pytest.raises(E, match="gemm_bf16.out: the kernel addresses 64 elements"):      # [N, M]: 15 rows of 4 apart + 4
        _lib.gemm_bf16(a, w, None, torch.zeros(15, 4, dtype=bf16), _lib.EPI_BF16_T)
    with pytest.raises(E, match="gemm_bf16.out: the kernel addresses 244 elements"):     # [M, N] where [N, M] is written
        _lib.gemm_bf16(a, w, None, o16, _lib.EPI_BF16_T)
    with pytest.raises(E, match="gemm_bf16.gate_tid: expected torch.int32"):
        _lib.gemm_bf16(a, w, None, o32, _lib.EPI_GATE_RESID_F32, gate=torch.zeros(2, 16), gate_tid=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(E, match="gemm_bf16.bias: the kernel addresses 16 elements"):
        _lib.gemm_bf16(a, w, torch.zeros(15, dtype=bf16), o16, _lib.EPI_BF16)


def test_wrappers_measure_views_against_their_storage_and_keep_optionals_optional():
    """A correctly sized view whose rows are wider than its shape - the LoRA slot buf[:, K:], V^T columns vt[:, col0:], the row tail
    a[j * L:] - passes dtype, layout and extent (measured to the end of the storage, not numel()) and fails only for living on the CPU;
    the same view one column further along is one element short. None stays accepted for optional arguments."""
    bf16 = torch.bfloat16
    E = _lib.UnividHipError
    buf, A, scale = torch.zeros(4, 64 + 128, dtype=bf16), torch.zeros(3, 64, dtype=bf16), torch.zeros(3)
    with pytest.raises(E, match="lora_down.buf: tensor must live on the GPU"):
        _lib.lora_down(buf, 64, A, scale)
    a, w = buf[:, 128:], torch.zeros(16, 64, dtype=bf16)                # 4 rows of 64 columns, 192 apart: ends with the storage
    out = torch.zeros(4, 24, dtype=bf16)[:, 8:]
    for kw in ({}, dict(gate=None, gate_tid=None, ws=None)):
        with pytest.raises(E, match="gemm_bf16.a: tensor must live on the GPU"):
            _lib.gemm_bf16(a, w, None, out, _lib.EPI_BF16, **kw)
    with pytest.raises(E, match="gemm_bf16.a: the kernel addresses 640 elements, the tensor's storage holds 639"):
        _lib.gemm_bf16(buf[:, 129:], w, None, out, _lib.EPI_BF16, M=4)
    vt = torch.zeros(8, 64 + 24, dtype=bf16)
    with pytest.raises(E, match="transpose_16.rows: tensor must live on the GPU"):
        _lib.transpose_16(torch.zeros(24, 8, dtype=bf16), vt[:, 24:], 24, 8, 64)
    with pytest.raises(E, match="transpose_16.out: the kernel addresses"):
        _lib.transpose_16(torch.zeros(24, 8, dtype=bf16), vt[:, 25:], 24, 8, 64)
    rows = torch.zeros(6, 16, dtype=bf16)
    with pytest.raises(E, match="patchify.x: tensor must live on the GPU"):
        _lib.patchify(torch.zeros(4, 1, 2, 4), rows[4:], (1, 2, 2))                       # 2 patches -> the last 2 rows
    with pytest.raises(E, match="patchify.out: the kernel addresses 32 elements, the tensor's storage holds 16"):
        _lib.patchify(torch.zeros(4, 1, 2, 4), rows[5:], (1, 2, 2))
    x = torch.zeros(2, 4, 4)
    for fn, args in ((_lib.unipc_predictor, (x, x, None, x, 1., 1., 1., 1., 1)), (_lib.dpmpp_update, (x, x, None, x, 1., 1., 1., 1)),
                     (_lib.unipc_corrector, (x, x, None, x, x, 1., 1., 1., 1., 1., 1., 1)),
                     (_lib.layernorm_mod, (torch.zeros(4, 256), torch.zeros(4, 256, dtype=bf16), 4, 256, 1e-6))):
        with pytest.raises(E, match="must live on the GPU"):
            fn(*args)
    with pytest.raises(E, match="unipc_predictor.m_prev: a tensor is required"):             # order 2 reads the older x0
        _lib.unipc_predictor(x, x, None, x, 1., 1., 1., 1., 2)


def test_vae_arena_pauses_the_collector_and_restores_it():
    """WanVAE_._arena runs with Python's cyclic collector off (a dropped VAE's memory pool must not be finalised while allocations are
    routed to another pool) and puts back whatever state it found, also when the body raises."""
    import contextlib
    import gc
    from univid_amd.wan.vae2_2 import _gc_paused
    seen = []
    inner = contextlib.contextmanager(lambda: (yield seen.append("in")))
    was = gc.isenabled()
    try:
        for state in (True, False):
            gc.enable() if state else gc.disable()
            with _gc_paused(inner()):
                assert not gc.isenabled()
            assert gc.isenabled() == state
            with pytest.raises(KeyError):
                with _gc_paused(inner()):
                    raise KeyError("body")
            assert gc.isenabled() == state
        assert seen == ["in"] * 4
    finally:
        gc.enable() if was else gc.disable()
