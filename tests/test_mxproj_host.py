"""Host-side behaviour of the opt-in MXFP8 mode of the attention projections (WanModel.set_proj_precision) - no GPU needed: the guards and
that they leave the state alone, the generation bump that makes captured graphs and cached K / V^T unusable, the un-merged adapter
conflict in both orders, the config pass-through, the refusal of the sequence-parallel forward, and the new wrappers' argument checks."""
import pytest
import torch

BF16, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
LORA_CFG = dict(r=4, lora_alpha=8)


def _model(**over):
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG, **over)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    if not over:
        m.load_state_dict(wan_dit.make_state_dict(cfg, 0))
    return m.eval()


def _state(m):
    return (m.proj_precision, tuple((b.proj_precision, b.self_attn.proj_precision, b.cross_attn.proj_precision) for b in m.blocks), m._prep_gen,
            m.ffn_precision, m.attn_precision,
            {n: sorted(getattr(l, "_uv_lora", {})) for n, l in m.named_modules() if isinstance(l, torch.nn.Linear)})


def _all(m, mode):
    return m.proj_precision == mode and all(b.proj_precision == mode and b.self_attn.proj_precision == mode and
                                            b.cross_attn.proj_precision == mode for b in m.blocks)


def _factors(names, dim=256, r=4):
    g = torch.Generator().manual_seed(1)
    return {n: (torch.randn(r, dim, generator=g), torch.randn(dim, r, generator=g)) for n in names}


def test_default_unknown_values_and_generation():
    from univid_amd.wan.model import PROJ_PRECISIONS
    assert PROJ_PRECISIONS == ("bf16", "mxfp8")
    m = _model()
    assert _all(m, "bf16")
    before = _state(m)
    for bad in ("fp8", "MXFP8", "mxfp8_qk", None, 8):
        with pytest.raises(ValueError):
            m.set_proj_precision(bad)
        with pytest.raises(ValueError):
            m.blocks[0].set_proj_precision(bad)
    assert _state(m) == before
    gen = m._prep_gen
    m.set_proj_precision("mxfp8")
    assert m._prep_gen > gen and _all(m, "mxfp8")
    assert all(b.self_attn._prep is None and b.cross_attn._prep is None and not b.cross_attn._kv_cache for b in m.blocks)
    assert m.ffn_precision == "bf16" and m.attn_precision == "bf16", "the modes are independent"
    m.set_ffn_precision("mxfp8")
    assert _all(m, "mxfp8")
    gen = m._prep_gen
    m.set_proj_precision("bf16")
    assert m._prep_gen > gen and _all(m, "bf16") and m.ffn_precision == "mxfp8"


def test_every_mode_combination_is_legal():
    from univid_amd.wan.model import ATTN_PRECISIONS, FFN_PRECISIONS, PROJ_PRECISIONS
    m = _model(num_heads=2)                                        # dim 256, head_dim 128: every attention mode applies
    for a in ATTN_PRECISIONS:
        for f in FFN_PRECISIONS:
            for p in PROJ_PRECISIONS:
                m.set_attn_precision(a), m.set_ffn_precision(f), m.set_proj_precision(p)
                assert (m.attn_precision, m.ffn_precision, m.proj_precision) == (a, f, p)


def test_dim_320_is_refused_with_state_unchanged():
    m = _model(dim=320, num_heads=5, ffn_dim=512)
    before = _state(m)
    with pytest.raises(ValueError, match="256"):
        m.set_proj_precision("mxfp8")
    assert _state(m) == before
    with pytest.raises(ValueError, match="256"):
        m.blocks[0].set_proj_precision("mxfp8")
    assert _state(m) == before


@pytest.mark.parametrize("target", ["blocks.0.self_attn.q", "blocks.1.cross_attn.o"])
def test_unmerged_adapter_conflicts_in_both_orders(target):
    from univid_amd.lora import attach_adapter_, detach_adapter_
    m = _model()
    # mode first, adapter second
    m.set_proj_precision("mxfp8")
    before = _state(m)
    with pytest.raises(NotImplementedError) as ei:
        attach_adapter_(m, "P", _factors([target, "blocks.0.cross_attn.k"]), LORA_CFG)
    assert "mxfp8" in str(ei.value) and "merge=False" in str(ei.value) and _state(m) == before
    # adapter first, mode second
    m.set_proj_precision("bf16")
    attach_adapter_(m, "P", _factors([target]), LORA_CFG)
    before = _state(m)
    with pytest.raises(NotImplementedError) as ei:
        m.set_proj_precision("mxfp8")
    assert "mxfp8" in str(ei.value) and "merge=False" in str(ei.value) and _state(m) == before
    with pytest.raises(NotImplementedError):
        m.blocks[int(target.split(".")[1])].set_proj_precision("mxfp8")
    assert _state(m) == before
    detach_adapter_(m, "P")
    m.set_proj_precision("mxfp8")
    assert _all(m, "mxfp8")


def test_unmerged_adapter_on_cross_attn_k_is_accepted():
    from univid_amd.lora import attach_adapter_
    m = _model()
    m.set_proj_precision("mxfp8")
    attach_adapter_(m, "K", _factors(["blocks.0.cross_attn.k", "blocks.1.cross_attn.v"]), LORA_CFG)
    assert sorted(m.blocks[0].cross_attn.k._uv_lora) == ["K"]
    m.set_proj_precision("bf16")
    m.set_proj_precision("mxfp8")                                  # ... and in the other order
    assert _all(m, "mxfp8")


def test_config_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    assert CrossAttentionConfig().proj_precision == "bf16"
    pipe = WanTI2V(TI2VConfig, model=_model(), device="cpu", proj_precision="mxfp8")
    assert _all(pipe.model, "mxfp8") and pipe.model.ffn_precision == "bf16" and pipe.model.attn_precision == "bf16"
    with pytest.raises(ValueError):
        WanTI2V(TI2VConfig, model=_model(), device="cpu", proj_precision="int8")
    plain = WanTI2V(TI2VConfig, model=_model(), device="cpu")
    assert _all(plain.model, "bf16")
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(proj_precision="mxfp8", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert _all(fused.dit_model, "mxfp8") and fused.dit_model.ffn_precision == "bf16"


def test_sequence_parallel_forward_is_refused_in_the_mode():
    m = _model()
    m.set_proj_precision("mxfp8")
    sa = m.blocks[0].self_attn
    with pytest.raises(NotImplementedError, match="proj_precision 'mxfp8'"):
        sa._self_attn_sp(torch.empty(0, 256, dtype=BF16), 0, (1, 1, 1), None, None, None, None, 1, (None, 8, 0))
    with pytest.raises(NotImplementedError, match="proj_precision 'mxfp8'"):
        sa._self_attn(torch.empty(0, 256, dtype=BF16), 0, (1, 1, 1), None, None, None, None, 1, sp=(None, 8, 0))


def _wrapper_cases():
    from univid_amd import _lib
    z = torch.zeros
    M, N, K = 8, 256, 128
    a, a_s, w, w_s = z(M, K, dtype=U8), z(M, K // 32, dtype=U8), z(N, K, dtype=U8), z(N, K // 32, dtype=U8)
    return {
        "layernorm_mod_mx": (lambda x, c, s, tab: _lib.layernorm_mod_mx(x, c, s, 4, 256, 1e-6, mode=1, tab=tab, shift_off=0, scale_off=256),
                             [z(4, 256), z(4, 256, dtype=U8), z(4, 8, dtype=U8), z(1, 512)], {0: "x", 1: "codes", 2: "scales", 3: "tab"}, (1, 4 * 256)),
        "gemm_mxfp8_t": (lambda a_, as_, w_, ws_, o: _lib.gemm_mxfp8_t(a_, as_, w_, ws_, None, o),
                         [a, a_s, w, w_s, z(N, M, dtype=BF16)], {0: "a", 1: "a_scale", 2: "w", 3: "w_scale", 4: "out_t"}, (4, N * M)),
        "gemm_mxfp8_ssq": (lambda a_, as_, w_, ws_, o, q: _lib.gemm_mxfp8_ssq(a_, as_, w_, ws_, None, o, q),
                           [a, a_s, w, w_s, z(M, N, dtype=BF16), z(M, N // 32)], {0: "a", 2: "w", 4: "out", 5: "ssq"}, (5, M * (N // 32))),
    }


@pytest.mark.parametrize("case", sorted(_wrapper_cases()))
def test_new_wrappers_check_before_the_library_is_touched(case, monkeypatch):
    """A wrong-dtype operand and a too-short output are UnividHipErrors naming wrapper and argument, raised from tensor metadata: nothing
    is launched or even loaded (CPU tensors: a well-formed call fails on the device check only)."""
    from univid_amd import _lib
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a rejected call reached the library"))
    fn, args, names, (si, need) = _wrapper_cases()[case]
    E = _lib.UnividHipError
    with pytest.raises(E, match=rf"{case}\.{names[min(names)]}: tensor must live on the GPU"):
        fn(*args)
    for i, name in names.items():
        bad = list(args)
        bad[i] = args[i].to(torch.float64)
        with pytest.raises(E, match=rf"{case}\.{name}: expected"):
            fn(*bad)
    t = args[si]
    short = list(args)
    short[si] = torch.empty(need - 1, dtype=t.dtype).as_strided((t.shape[0] - 1,) + tuple(t.shape[1:]), t.stride())
    with pytest.raises(E, match=rf"{case}\.{names[si]}: the kernel addresses {need} elements"):
        fn(*short)
