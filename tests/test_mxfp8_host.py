"""Host-side behaviour of the opt-in MXFP8 FFN mode (WanModel.set_ffn_precision) - no GPU needed: the guards, the generation bump that
makes captured graphs re-capture, the config pass-through, and the properties of the format's CPU emulation the GPU tests rely on."""
import pytest
import torch

from test_mxfp8 import mx_dequant, mx_quant_ref

pytestmark = []          # (test_mxfp8 is imported for its emulation only; nothing here carries its gpu mark)

BF16 = torch.bfloat16


def _tiny():
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(wan_dit.make_state_dict(cfg, 0))
    return cfg, m.eval()


def _factors(cfg, names, r=4):
    g = torch.Generator().manual_seed(1)
    shapes = {"ffn.0": (cfg["ffn_dim"], cfg["dim"]), "ffn.2": (cfg["dim"], cfg["ffn_dim"])}
    out = {}
    for n in names:
        o, i = next((v for k, v in shapes.items() if n.endswith(k)), (cfg["dim"], cfg["dim"]))
        out[n] = (torch.randn(r, i, generator=g), torch.randn(o, r, generator=g))
    return out


LORA_CFG = dict(r=4, lora_alpha=8)


def _state(m):
    return (m.ffn_precision, tuple(b.ffn_precision for b in m.blocks), m._prep_gen,
            {n: sorted(getattr(l, "_uv_lora", {})) for n, l in m.named_modules() if isinstance(l, torch.nn.Linear)})


def test_unknown_mode_and_generation():
    cfg, m = _tiny()
    assert m.ffn_precision == "bf16" and all(b.ffn_precision == "bf16" for b in m.blocks)
    before = _state(m)
    for bad in ("fp8", "MXFP8", None, 8):
        with pytest.raises(ValueError):
            m.set_ffn_precision(bad)
    assert _state(m) == before
    gen = m._prep_gen
    m.set_ffn_precision("mxfp8")
    assert m._prep_gen > gen and m.ffn_precision == "mxfp8" and all(b.ffn_precision == "mxfp8" and b._prep is None for b in m.blocks)
    gen = m._prep_gen
    m.set_ffn_precision("bf16")
    assert m._prep_gen > gen and all(b.ffn_precision == "bf16" for b in m.blocks)


def test_shapes_the_kernel_cannot_take_are_refused():
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    m = WanModel.from_config(dict(wan_dit.TINY_CFG, ffn_dim=384, model_type="ti2v"))
    with pytest.raises(ValueError):
        m.set_ffn_precision("mxfp8")
    assert m.ffn_precision == "bf16"


def test_unmerged_ffn_adapter_conflicts_in_both_orders():
    from univid_amd.lora import attach_adapter_, detach_adapter_
    cfg, m = _tiny()
    ffn = _factors(cfg, ["blocks.0.ffn.0", "blocks.1.ffn.2", "blocks.0.self_attn.q"])
    attn = _factors(cfg, ["blocks.0.self_attn.q", "blocks.1.cross_attn.o"])
    # mode first, adapter second
    m.set_ffn_precision("mxfp8")
    before = _state(m)
    with pytest.raises(NotImplementedError) as ei:
        attach_adapter_(m, "F", ffn, LORA_CFG)
    assert "mxfp8" in str(ei.value) and "merge=False" in str(ei.value) and _state(m) == before
    attach_adapter_(m, "A", attn, LORA_CFG)                    # attention projections: fine in both modes
    detach_adapter_(m, "A")
    # adapter first, mode second
    m.set_ffn_precision("bf16")
    attach_adapter_(m, "F", ffn, LORA_CFG)
    before = _state(m)
    with pytest.raises(NotImplementedError) as ei:
        m.set_ffn_precision("mxfp8")
    assert "mxfp8" in str(ei.value) and "merge=False" in str(ei.value) and _state(m) == before
    detach_adapter_(m, "F")
    m.set_ffn_precision("mxfp8")
    assert m.ffn_precision == "mxfp8"


def test_config_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    assert CrossAttentionConfig().ffn_precision == "bf16"
    cfg, m = _tiny()
    pipe = WanTI2V(TI2VConfig, model=m, device="cpu", ffn_precision="mxfp8")
    assert pipe.model.ffn_precision == "mxfp8" and all(b.ffn_precision == "mxfp8" for b in pipe.model.blocks)
    with pytest.raises(ValueError):
        WanTI2V(TI2VConfig, model=_tiny()[1], device="cpu", ffn_precision="int8")
    cfg, m2 = _tiny()
    plain = WanTI2V(TI2VConfig, model=m2, device="cpu")
    assert plain.model.ffn_precision == "bf16"
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(ffn_precision="mxfp8", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.dit_model.ffn_precision == "mxfp8"


def test_emulation_properties():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 256, generator=g) * torch.logspace(-6, 6, 64).unsqueeze(1)).to(BF16)
    x[3, 32:64] = 0
    codes, scales = mx_quant_ref(x)
    assert int(scales[3, 1]) == 0 and int(codes[3, 32:64].sum()) == 0, "an all-zero block: scale byte 0, codes 0"
    assert not ((codes & 0x7F) == 0x7F).any()
    deq = mx_dequant(codes, scales)
    amax = x.double().reshape(64, 8, 32).abs().amax(-1)
    dmax = deq.reshape(64, 8, 32).abs().amax(-1)
    nz = amax > 0
    r = dmax[nz] / amax[nz]
    # amax scales into [256, 512) and is clamped at 448 (else rounded to 4 significant bits: at most 1/16 up): the dequantised amax lies
    # in (448 / 512, 1 + 1/16] of the original
    assert float(r.min()) > 448 / 512 and float(r.max()) <= 1 + 1 / 16
    # [1, 2) x 448 / 512: the dequantised amax never exceeds 448 x scale, and scale x 256 <= amax < scale x 512
    sc = torch.exp2(scales.double() - 127)[nz]
    assert (dmax[nz] <= 448 * sc).all() and (amax[nz] >= 256 * sc).all() and (amax[nz] < 512 * sc).all()
    # relative error of the elements that matter (within 2^-5 of the block amax): e4m3's 3 mantissa bits -> 2^-4 relative at most, except the clamp
    big = (x.double().abs().reshape(64, 8, 32) >= amax.unsqueeze(-1) / 32) & nz.unsqueeze(-1)
    rel = ((deq - x.double()).abs() / x.double().abs().clamp_min(1e-300)).reshape(64, 8, 32)[big]
    assert float(rel.max()) <= 1 - 448 / 512 + 1e-12
