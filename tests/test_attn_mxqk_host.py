"""Host-side behaviour of the opt-in MXFP8 q / k mode of the self-attention (WanModel.set_attn_precision) - no GPU needed: the guards, the
generation bump that makes captured graphs re-capture, the config pass-through, the launch plans of every Lk of the GPU table
(tests/test_attn_mxqk.py) as the library reports them for 256 CUs, and the conditions of the table's designed operands - every one must
survive the MXFP8 rule exactly, and the fp64 reference must stay inside its family's own conditions."""
import math

import pytest
import torch

from test_attn_mxqk import CASES, D, KNAME, _ops, assert_plan, mx_exact

pytestmark = []          # (test_attn_mxqk is imported for its table and builders only; nothing here carries its gpu mark)


@pytest.fixture(autouse=True)
def _default_options():
    from univid_amd import _lib
    _lib.reset_options()
    yield
    _lib.reset_options()


def _model(**over):
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG, **over)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(wan_dit.make_state_dict(cfg, 0))
    return m.eval()


def _state(m):
    return m.attn_precision, tuple(b.self_attn.attn_precision for b in m.blocks), m._prep_gen


# ---- mode plumbing ----------------------------------------------------------------------------------------------------------------
def test_default_unknown_values_and_generation():
    m = _model(num_heads=2)                                        # dim 256: head_dim 128
    assert m.attn_precision == "bf16" and all(b.self_attn.attn_precision == "bf16" for b in m.blocks)
    before = _state(m)
    for bad in ("mxfp8", "MXFP8_QK", "fp8", None, 8):
        with pytest.raises(ValueError):
            m.set_attn_precision(bad)
    assert _state(m) == before
    gen = m._prep_gen
    m.set_attn_precision("mxfp8_qk")
    assert m._prep_gen > gen and m.attn_precision == "mxfp8_qk" and all(b.self_attn.attn_precision == "mxfp8_qk" for b in m.blocks)
    assert m.ffn_precision == "bf16" and all(b.ffn_precision == "bf16" for b in m.blocks), "the two modes are independent"
    m.set_ffn_precision("mxfp8")
    assert m.attn_precision == "mxfp8_qk" and all(b.self_attn.attn_precision == "mxfp8_qk" for b in m.blocks)
    gen = m._prep_gen
    m.set_attn_precision("bf16")
    assert m._prep_gen > gen and all(b.self_attn.attn_precision == "bf16" for b in m.blocks) and m.ffn_precision == "mxfp8"


def test_head_dim_64_is_refused_with_state_unchanged():
    m = _model()                                                   # the tiny config: 4 heads of 64
    before = _state(m)
    with pytest.raises(ValueError, match="mxfp8_qk"):
        m.set_attn_precision("mxfp8_qk")
    assert _state(m) == before
    with pytest.raises(ValueError, match="mxfp8_qk"):
        m.blocks[0].set_attn_precision("mxfp8_qk")
    assert _state(m) == before


def test_config_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    assert CrossAttentionConfig().attn_precision == "bf16"
    pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_precision="mxfp8_qk")
    assert pipe.model.attn_precision == "mxfp8_qk" and all(b.self_attn.attn_precision == "mxfp8_qk" for b in pipe.model.blocks)
    assert pipe.model.ffn_precision == "bf16"
    with pytest.raises(ValueError):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_precision="int8")
    with pytest.raises(ValueError):
        WanTI2V(TI2VConfig, model=_model(), device="cpu", attn_precision="mxfp8_qk")         # head_dim 64
    plain = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu")
    assert plain.model.attn_precision == "bf16"
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(attn_precision="mxfp8_qk", ffn_precision="mxfp8", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.dit_model.attn_precision == "mxfp8_qk" and fused.dit_model.ffn_precision == "mxfp8"


def test_sequence_parallel_forward_is_refused_in_the_mode():
    m = _model(num_heads=2)
    m.set_attn_precision("mxfp8_qk")
    sa = m.blocks[0].self_attn
    with pytest.raises(NotImplementedError, match="mxfp8_qk"):
        sa._self_attn_sp(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, (None, 8, 0))
    with pytest.raises(NotImplementedError, match="mxfp8_qk"):
        sa._self_attn(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, sp=(None, 8, 0))


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def test_plans_of_the_gpu_table_and_the_threshold():
    from univid_amd import _lib
    for c in CASES:
        assert_plan(c, 256)
    _lib.reset_options()
    assert {c.kern for c in CASES} == {"mx4", "mx12"}
    assert _lib.attn_mxqk_plan(500, 2047, D, 2, 4) == dict(kernel=KNAME["mx4"], q_blocks=4, n12=0, grid=32)
    assert _lib.attn_mxqk_plan(500, 2048, D, 2, 4)["kernel"] == KNAME["mx12"]
    # the same cut and grid as the bf16 plan of the shape: plan_attn stays the one place that chooses
    for Lq, Lk, B, H in ((500, 2048, 2, 4), (11440, 11440, 2, 24), (11440, 11440, 1, 24), (150, 200, 1, 2)):
        mx, bf = _lib.attn_mxqk_plan(Lq, Lk, D, B, H), _lib.attn_plan(Lq, Lk, D, B, H)
        assert (mx["q_blocks"], mx["n12"], mx["grid"]) == (bf["q_blocks"], bf["n12"], bf["grid"])
        assert mx["kernel"] == {"flash_attn_fwd12_kernel": KNAME["mx12"], "flash_attn_fwd3_kernel": KNAME["mx4"]}[bf["kernel"]]
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_mxqk_plan: head_dim 64"):
        _lib.attn_mxqk_plan(150, 200, 64, 1, 2)


# ---- operand builders ---------------------------------------------------------------------------------------------------------------
def test_designed_operands_are_exact_in_mxfp8():
    """Every operand set of the GPU table: q and k survive mx_quant_ref / mx_dequant exactly (+-1, 0, 0 / 1 beside a 6 or a 10, 40 x (+-1):
    asserted element for element), so the fp64 reference of tests/test_attn_kernels.py's builders IS the softmax of the dequantised operands;
    the builders' own conditions (scale equality, span < 2^24, at most 0.5 % excepted, the spikes' pattern, the selector's gap >= 300) are
    asserted inside them. The table keeps a ragged last tile, both spikes and the production-scale selector for both kernels."""
    worst = dict(excluded_share=0.0, span_log2=0.0, selector_gap=math.inf)
    for c in CASES:
        o = _ops(c)
        mx_exact(o.q), mx_exact(o.k)
        assert o.ref.shape == (c.B * c.Lq, c.H * D) and o.ref.dtype == torch.bfloat16
        for key, val in o.stats.items():
            worst[key] = min(worst[key], val) if key == "selector_gap" else max(worst[key], val)
    assert worst["excluded_share"] <= 0.005 and worst["span_log2"] < 24 and worst["selector_gap"] >= 300
    for kern in ("mx4", "mx12"):
        assert {"A", "spike10", "spike6", "B"} == {c.fam for c in CASES if c.kern == kern}, kern
        assert any(c.Lk % 64 for c in CASES if c.kern == kern and c.fam == "A")
        assert {c.ld for c in CASES if c.kern == kern} == {"dense", "slice", "vt+64", "vt+8", "ldo+8", "ldo+4"}, kern
    assert {c.cut for c in CASES if c.kern == "mx12" and c.Lq == 500 and c.H * c.B == 8} == {0, 1, 2, 3}
    assert {c.cut for c in CASES if c.kern == "mx12" and c.H == 3} == {0, 1, 2, 3}
    assert {(c.Lq, c.Lk) for c in CASES if c.kern == "mx4" and c.ld == "dense" and c.fam == "A" and c.B == 1} == \
        {(lq, lk) for lk in (5, 63, 64, 65, 128, 129, 200, 2040) for lq in (1, 33, 150)}
    assert all(c.B == 1 or c.Lk % 8 == 0 for c in CASES)
