"""Host-side behaviour of the opt-in MXFP8 q / k + P.V mode of the self-attention (WanModel.set_attn_precision("mxfp8_qk_pv")) - no GPU needed:
the guards, the generation bump, the config pass-through, the refusal of the sequence-parallel forward, the launch plans of the GPU table
(tests/test_attn_mxpv.py) as the library reports them for 256 CUs, the stated V^T layout's round trip, and the exactness conditions of every
designed operand of that table - q, k along the head dimension, V along the keys, every P a normal power-of-two code - with the fp64
reference inside its family's own cap."""
import math

import pytest
import torch

from test_attn_mxpv import CASES, D, DEFER_PV, KNAME, PERM34, PSHIFT, _ops, assert_plan, check_exactness, tail_gap, vt_pack, vt_ref, vt_unpack
from test_attn_mxqk_host import _model, _state

pytestmark = []          # (test_attn_mxpv is imported for its table and builders only; nothing here carries its gpu mark)
MODE = "mxfp8_qk_pv"


@pytest.fixture(autouse=True)
def _default_options():
    from univid_amd import _lib
    _lib.reset_options()
    yield
    _lib.reset_options()


# ---- mode plumbing ----------------------------------------------------------------------------------------------------------------
def test_the_mode_is_accepted_and_unknown_values_are_not():
    from univid_amd.wan.model import ATTN_PRECISIONS
    assert ATTN_PRECISIONS == ("bf16", "mxfp8_qk", MODE)
    m = _model(num_heads=2)                                        # dim 256: head_dim 128
    before = _state(m)
    for bad in ("mxfp8", "fp8", "mxfp8_pv", "MXFP8_QK_PV", None, 8):
        with pytest.raises(ValueError):
            m.set_attn_precision(bad)
    assert _state(m) == before
    gen = m._prep_gen
    m.set_attn_precision(MODE)
    assert m._prep_gen > gen and m.attn_precision == MODE and all(b.self_attn.attn_precision == MODE for b in m.blocks)
    assert m.ffn_precision == "bf16" and all(b.ffn_precision == "bf16" for b in m.blocks), "the modes are independent"
    gen = m._prep_gen
    m.set_attn_precision("mxfp8_qk")                               # between the two narrow modes the generation moves too: graphs re-capture
    assert m._prep_gen > gen and all(b.self_attn.attn_precision == "mxfp8_qk" for b in m.blocks)
    gen = m._prep_gen
    m.set_attn_precision("bf16")
    assert m._prep_gen > gen and all(b.self_attn.attn_precision == "bf16" for b in m.blocks)


def test_head_dim_64_is_refused_with_state_unchanged():
    m = _model()                                                   # the tiny config: 4 heads of 64
    before = _state(m)
    with pytest.raises(ValueError, match=MODE):
        m.set_attn_precision(MODE)
    assert _state(m) == before
    with pytest.raises(ValueError, match=MODE):
        m.blocks[0].set_attn_precision(MODE)
    assert _state(m) == before


def test_config_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_precision=MODE)
    assert pipe.model.attn_precision == MODE and all(b.self_attn.attn_precision == MODE for b in pipe.model.blocks)
    assert pipe.model.ffn_precision == "bf16"
    with pytest.raises(ValueError):
        WanTI2V(TI2VConfig, model=_model(), device="cpu", attn_precision=MODE)         # head_dim 64
    plain = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu")
    assert plain.model.attn_precision == "bf16"
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(attn_precision=MODE, use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.dit_model.attn_precision == MODE and fused.dit_model.ffn_precision == "bf16"


def test_sequence_parallel_forward_is_refused_in_the_mode():
    m = _model(num_heads=2)
    m.set_attn_precision(MODE)
    sa = m.blocks[0].self_attn
    with pytest.raises(NotImplementedError, match=MODE):
        sa._self_attn_sp(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, (None, 8, 0))
    with pytest.raises(NotImplementedError, match="mxfp8_qk"):
        sa._self_attn(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, sp=(None, 8, 0))


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def test_plans_of_the_gpu_table_and_the_threshold():
    from univid_amd import _lib
    for c in CASES:
        assert_plan(c, 256)                                        # the mxqk plan's geometry, the mxpv kernel's name
    _lib.reset_options()
    assert {c.kern for c in CASES} == {"mx4", "mx12"}
    assert _lib.attn_mxpv_plan(500, 2047, D, 2, 4) == dict(kernel=KNAME["mx4"], q_blocks=4, n12=0, grid=32)
    assert _lib.attn_mxpv_plan(500, 2048, D, 2, 4)["kernel"] == KNAME["mx12"]
    for Lq, Lk, B, H in ((500, 2048, 2, 4), (11440, 11440, 2, 24), (11440, 11440, 1, 24), (150, 200, 1, 2)):
        pv, qk = _lib.attn_mxpv_plan(Lq, Lk, D, B, H), _lib.attn_mxqk_plan(Lq, Lk, D, B, H)
        assert (pv["q_blocks"], pv["n12"], pv["grid"]) == (qk["q_blocks"], qk["n12"], qk["grid"])
        assert pv["kernel"] == qk["kernel"].replace("mxqk", "mxpv")
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_mxpv_plan: head_dim 64"):
        _lib.attn_mxpv_plan(150, 200, 64, 1, 2)


# ---- the format's constants and layout ------------------------------------------------------------------------------------------------
def test_constants_and_layout_round_trip():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "univid_hip.h")).read()
    assert f"#define UV_ATT_MXPV_DEFER {DEFER_PV}\n" in hdr and f"#define UV_ATT_MXPV_PSHIFT {PSHIFT}\n" in hdr
    assert DEFER_PV + PSHIFT == 8, "the largest P code is 2^8 = 256 < 448"
    assert PERM34.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 22, 23, 8, 9, 10, 11, 12, 13, 14, 15, 24, 25, 26, 27, 28, 29, 30, 31]
    B, Lk, H = 2, 72, 2
    v = (torch.arange(B * Lk * H * D).reshape(B * Lk, H * D) % 13 - 6).to(torch.bfloat16)
    codes, sc = vt_ref(v, B, Lk)
    assert codes.shape == (H * D, 256) and sc.shape == (H * D, 8)
    assert int(codes[:, 72:128].sum()) == 0 and bool((sc[:, 3] == 127).all()) and bool((sc[:, 2] != 127).all())   # block 2 holds keys 64..71
    pc, ps = vt_pack(codes, sc, H)
    assert ps.shape == (H, 4 * 256)
    # byte 4 (r + 32 k) + d of tile t of head h is the scale of channel 32 d + r, key half k
    h, t, k, r, d = 1, 2, 1, 5, 3
    assert int(ps[h, t * 256 + 4 * (r + 32 * k) + d]) == int(sc[h * D + 32 * d + r, 2 * t + k])
    assert int(pc[7, 32 + 8]) == int(codes[7, 32 + 16]) and int(pc[7, 32 + 16]) == int(codes[7, 32 + 8])
    c2, s2 = vt_unpack(pc, ps, H)
    assert torch.equal(c2, codes) and torch.equal(s2, sc)


# ---- operand builders ---------------------------------------------------------------------------------------------------------------
def test_designed_operands_hold_their_exactness_conditions():
    """Every operand set of the GPU table: q / k exact in MXFP8 along the head dimension, V along the keys, every P a power of two inside the
    normal e4m3 range under PSHIFT for any admissible reference maximum (check_exactness states the argument); family A and the spikes keep
    the reference alone inside the 0.5 % cap of excepted elements; the tail family carries at least 0.97 of the peak's mass in codes of 2^-G."""
    worst = dict(excluded_share=0.0, span=0.0)
    for c in CASES:
        o = _ops(c)
        worst["span"] = max(worst["span"], check_exactness(c, o)["span"])
        assert o.ref.shape == (c.B * c.Lq, c.H * D) and o.ref.dtype == torch.bfloat16
        if c.fam in ("A", "spike10", "spike6"):
            assert o.near is not None and float(o.near.double().mean()) == o.stats["excluded_share"]
            worst["excluded_share"] = max(worst["excluded_share"], o.stats["excluded_share"])
        else:
            assert o.near is None
        if c.fam == "tail":
            G = tail_gap(c.Lk)
            assert o.stats["tail_mass"] >= 0.97 and PSHIFT - G >= -6 and c.Lk * 2.0 ** -G >= 1
    assert worst["excluded_share"] <= 0.005 and 11 <= worst["span"] <= PSHIFT + 6
    assert tail_gap(2104) == 11 and tail_gap(200) == 7
    for kern in ("mx4", "mx12"):
        assert {"A", "spike10", "spike6", "B", "tail"} == {c.fam for c in CASES if c.kern == kern}, kern
        assert {c.ld for c in CASES if c.kern == kern} == {"dense", "slice", "vt+64", "vt+8", "ldo+8", "ldo+4"}, kern
    assert {c.cut for c in CASES if c.kern == "mx12" and c.Lq == 500 and c.H * c.B == 8} == {0, 1, 2, 3}
    assert all(c.B == 1 or c.Lk % 8 == 0 for c in CASES)
    assert math.log2(448) > DEFER_PV + PSHIFT
