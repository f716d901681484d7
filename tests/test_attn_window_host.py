"""Host-side behaviour of the opt-in sliding-window / causal self-attention (WanModel.set_attn_window) - no GPU needed: plan_attn_win through
`attn_win_plan` for 256 CUs (the 12-wave rule from both sides, the cut of `attn_plan`), every guard with its message and its order, the
keyword pass-through on a CPU model, and the conditions of the designed operands of every row of the GPU table (tests/test_attn_window.py)."""
import pytest
import torch

from test_attn_window import CASES, D, IDS, KNAME, assert_plan, expected_plan, kern_of, ops_of, poison_rows, span_of, window_mask

pytestmark = []          # (test_attn_window is imported for its table and builders only; nothing here carries its gpu mark)


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
    return (m.attn_precision, m.window_size, m.attn_window, m.config["window_size"], tuple(b.self_attn.attn_precision for b in m.blocks),
            tuple((b.self_attn.attn_window, b.self_attn.window_size, b.window_size) for b in m.blocks), m._prep_gen)


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_rule_from_both_sides_and_the_dense_cut():
    from univid_amd import _lib
    for c in CASES:
        assert_plan(c, 256)
    _lib.reset_options()
    assert {kern_of(c) for c in CASES} == {"win4", "win12"}
    # span = min(L, 384 + left + right), an unbounded side counted as L; the 12-wave form from 2048 on
    for n, win, kern in ((2104, (1663, 0), "win4"), (2104, (1664, 0), "win12"), (2104, (0, 1663), "win4"), (2104, (832, 832), "win12"),
                         (2104, (832, 831), "win4"), (2047, (-1, -1), "win4"), (2048, (-1, -1), "win12"), (2048, (-1, 0), "win12"),
                         (2048, (0, -1), "win12"), (11440, (1760, 1760), "win12"), (11440, (800, 800), "win4"), (27280, (1760, 1760), "win12"),
                         (11440, (-1, 0), "win12"), (2304, (576, 576), "win4"), (2304, (1152, 1152), "win12"), (100, (5000, 5000), "win4")):
        assert span_of(n, win) >= 2048 if kern == "win12" else span_of(n, win) < 2048
        assert _lib.attn_win_plan(n, D, 2, 24, win)["kernel"] == KNAME[kern], (n, win)
    assert _lib.attn_win_plan(500, D, 2, 4, (100, 100)) == dict(kernel=KNAME["win4"], q_blocks=4, n12=0, grid=32)
    # the same cut and grid as the dense plan of (L, batch, H): plan_attn stays the one place that chooses
    for n, B, H in ((2104, 2, 4), (11440, 2, 24), (11440, 1, 24), (27280, 1, 24), (2504, 1, 3)):
        for cut in (0, 1, 2, 3):
            _lib.set_option(_lib.OPT_ATTN_CUT, cut)
            w, d = _lib.attn_win_plan(n, D, B, H, (1760, 1760)), _lib.attn_plan(n, n, D, B, H)
            assert w["kernel"] == KNAME["win12"] and d["kernel"] == "flash_attn_fwd12_kernel"
            assert (w["q_blocks"], w["n12"], w["grid"]) == (d["q_blocks"], d["n12"], d["grid"])
    _lib.reset_options()
    # OPT_ATTN_WIN_FORM (A/B tools): either form whatever the span; the 12-wave cut is still the dense plan's
    assert _lib.get_option(_lib.OPT_ATTN_WIN_FORM) == 0
    for form, kern in ((1, "win12"), (2, "win4")):
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, form)
        for n, win in ((200, (4, 4)), (11440, (1760, 1760)), (11440, (100, 100)), (2104, (-1, -1))):
            assert _lib.attn_win_plan(n, D, 2, 24, win)["kernel"] == KNAME[kern]
        if form == 1:
            w, d = _lib.attn_win_plan(11440, D, 2, 24, (100, 100)), _lib.attn_plan(11440, 11440, D, 2, 24)
            assert (w["q_blocks"], w["n12"], w["grid"]) == (d["q_blocks"], d["n12"], d["grid"])
    with pytest.raises(_lib.UnividHipError, match="UV_OPT_ATTN_WIN_FORM"):
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, 3)
    _lib.reset_options()
    assert _lib.get_option(_lib.OPT_ATTN_WIN_FORM) == 0
    for bad, match in (((-2, 0), r"window \(-2, 0\)"), ((0, -5), r"window \(0, -5\)")):
        with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_win_plan: " + match):
            _lib.attn_win_plan(200, D, 1, 2, bad)
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_win_plan: head_dim 64"):
        _lib.attn_win_plan(200, 64, 1, 2, (4, 4))


# ---- guards -----------------------------------------------------------------------------------------------------------------------
def test_setter_constructor_and_generation():
    m = _model(num_heads=2)                                        # dim 256: head_dim 128
    assert m.window_size == (-1, -1) and m.attn_window is None and all(b.self_attn.attn_window is None for b in m.blocks)
    gen = m._prep_gen
    m.set_attn_window((64, 32))
    assert m._prep_gen > gen and m.window_size == (64, 32) and m.attn_window == (64, 32) and m.config["window_size"] == (64, 32)
    assert all(b.self_attn.attn_window == (64, 32) and b.window_size == (64, 32) and b.cross_attn.attn_window is None for b in m.blocks)
    assert m.ffn_precision == "bf16" and m.proj_precision == "bf16" and m.attn_precision == "bf16"
    m.set_ffn_precision("mxfp8")                                   # independent of the window
    m.set_proj_precision("mxfp8")
    assert m.window_size == (64, 32) and all(b.self_attn.attn_window == (64, 32) for b in m.blocks)
    m.set_ffn_precision("bf16")
    m.set_proj_precision("bf16")
    m.set_attn_window([-1, 0])                                     # causal, as a list (config.json)
    assert m.window_size == (-1, 0) and all(b.self_attn.attn_window == (-1, 0) for b in m.blocks)
    gen = m._prep_gen
    for off in (None, (-1, -1)):
        m.set_attn_window(off)
        assert m._prep_gen > gen and m.window_size == (-1, -1) and m.attn_window is None and all(b.self_attn.attn_window is None for b in m.blocks)
        gen = m._prep_gen
    built = _model(num_heads=2, window_size=(64, 32))              # the constructor lands in the setter's state
    m.set_attn_window((64, 32))
    assert _state(built)[:6] == _state(m)[:6]


def test_bad_windows_raise_value_error_with_state_unchanged():
    from univid_amd.wan.model import WanAttentionBlock, WanModel, WanSelfAttention
    m = _model(num_heads=2)
    m.set_attn_window((8, 8))
    before = _state(m)
    for bad in ((-2, 0), (0, -2), (4,), (1, 2, 3), "ab", 5, (1.5, 2), (None, 3), ("a", "b")):
        with pytest.raises(ValueError, match="window_size"):
            m.set_attn_window(bad)
        with pytest.raises(ValueError, match="window_size"):
            m.blocks[0].set_attn_window(bad)
        assert _state(m) == before
    with pytest.raises(ValueError, match="window_size"):
        WanSelfAttention(256, 2, (-3, 0))
    with pytest.raises(ValueError, match="window_size"):
        WanAttentionBlock(256, 512, 2, (0, -2))
    with pytest.raises(ValueError, match="window_size"):
        _model(num_heads=2, window_size=(-2, -2))
    with pytest.raises(NotImplementedError, match="qk_norm"):
        WanSelfAttention(256, 2, (4, 4), qk_norm=False)            # still not built
    # a bad tuple is a ValueError even where the mode would refuse a good one: validation comes first
    m.set_attn_window(None)
    m.set_attn_precision("mxfp8_qk")
    with pytest.raises(ValueError, match="window_size"):
        m.set_attn_window((-2, 0))


def test_head_dim_64_is_refused_with_state_unchanged():
    m = _model()                                                   # the tiny config: 4 heads of 64
    before = _state(m)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        m.set_attn_window((8, 8))
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        m.blocks[0].set_attn_window((8, 8))
    assert _state(m) == before
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        _model(window_size=(8, 8))
    m.set_attn_window((-1, -1))                                    # global attention is what it runs
    assert m.window_size == (-1, -1)


@pytest.mark.parametrize("mode", ["mxfp8_qk", "mxfp8_qk_pv"])
def test_window_and_mxfp8_attention_refuse_each_other_either_way_round(mode):
    m = _model(num_heads=2)
    m.set_attn_window((64, 64))
    before = _state(m)
    with pytest.raises(NotImplementedError, match=rf"window_size \(64, 64\) with attn_precision '{mode}'"):
        m.set_attn_precision(mode)
    with pytest.raises(NotImplementedError, match=rf"window_size \(64, 64\) with attn_precision '{mode}'"):
        m.blocks[1].set_attn_precision(mode)
    assert _state(m) == before
    m.set_attn_window(None)
    m.set_attn_precision(mode)
    before = _state(m)
    with pytest.raises(NotImplementedError, match=rf"window_size \(64, 64\) with attn_precision '{mode}'"):
        m.set_attn_window((64, 64))
    with pytest.raises(NotImplementedError, match=rf"window_size \(64, 64\) with attn_precision '{mode}'"):
        m.blocks[1].set_attn_window((64, 64))
    assert _state(m) == before
    m.set_attn_window(None)                                        # switching the window OFF is always legal
    m.set_attn_precision("bf16")
    m.set_attn_window((64, 64))
    assert m.window_size == (64, 64)


def test_sequence_parallel_forward_is_refused_with_a_window():
    m = _model(num_heads=2)
    m.set_attn_window((64, 0))
    sa = m.blocks[0].self_attn
    with pytest.raises(NotImplementedError, match=r"window_size \(64, 0\) is not built for the sequence-parallel forward"):
        sa._self_attn_sp(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, (None, 8, 0))
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        sa._self_attn(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, sp=(None, 8, 0))


def test_reference_signature_forward_refuses_padding_with_a_window():
    from univid_amd.wan.model import WanSelfAttention
    sa = WanSelfAttention(256, 2, (16, 16))
    x = torch.zeros(2, 40, 256)
    with pytest.raises(NotImplementedError, match="call WanModel.forward, which strips the padding"):
        sa(x, torch.tensor([40, 33]), torch.tensor([[1, 5, 8], [1, 3, 11]]), None)


def test_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    assert CrossAttentionConfig().attn_window is None
    pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_window=(64, 64))
    assert pipe.model.window_size == (64, 64) and all(b.self_attn.attn_window == (64, 64) for b in pipe.model.blocks)
    assert pipe.model.attn_precision == "bf16" and pipe.model.ffn_precision == "bf16"
    kept = WanTI2V(TI2VConfig, model=_model(num_heads=2, window_size=(32, 0)), device="cpu")        # None keeps what the model came with
    assert kept.model.window_size == (32, 0)
    off = WanTI2V(TI2VConfig, model=_model(num_heads=2, window_size=(32, 0)), device="cpu", attn_window=(-1, -1))
    assert off.model.window_size == (-1, -1) and off.model.attn_window is None
    with pytest.raises(ValueError, match="window_size"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_window=(-2, 4))
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        WanTI2V(TI2VConfig, model=_model(), device="cpu", attn_window=(8, 8))
    with pytest.raises(NotImplementedError, match="with attn_precision 'mxfp8_qk'"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_precision="mxfp8_qk", attn_window=(8, 8))
    plain = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu")
    assert plain.model.window_size == (-1, -1)
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(attn_window=(128, 0), ffn_precision="mxfp8", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.dit_model.window_size == (128, 0) and fused.dit_model.ffn_precision == "mxfp8"


def test_seam_argument_order_without_a_gpu():
    """The seam refuses host tensors first (no CPU path), as before; window validation does not move that."""
    from univid_amd import _lib
    from univid_amd.wan.attention import flash_attention
    q = torch.zeros(1, 8, 1, 128)
    with pytest.raises(_lib.UnividHipError):
        flash_attention(q, q, q, window_size=(2, 2))


# ---- operand builders ---------------------------------------------------------------------------------------------------------------
def test_designed_operands_hold_their_conditions_for_every_row():
    """Every row of the GPU table, on the CPU: the scale equality, the span below 2^24, the excepted share at or below 0.5 % (the cap is a
    condition of the operands: the 64-seed loop replaces a seed that misses it), the spikes' score pattern under the mask, the poison keys
    hidden from every query but the zeroed ones (all asserted inside the builders) - and the table's coverage."""
    worst = dict(excluded_share=0.0, span_log2=0.0)
    for c in CASES:
        o = ops_of(c)
        assert o.ref.shape == (c.B * c.L, c.H * D) and o.ref.dtype == torch.bfloat16
        assert o.stats["excluded_share"] <= 0.005 and o.stats["span_log2"] < 24, IDS[CASES.index(c)]
        for key, val in o.stats.items():
            worst[key] = max(worst[key], val)
        assert (o.poison is not None) == (c.fam == "A" and poison_rows(c.L, c.win) is not None)
    print(f"{len(CASES)} rows: largest excepted share {worst['excluded_share']:.4%}, largest span 2^{worst['span_log2']:.2f}")
    assert worst["excluded_share"] <= 0.005 and worst["span_log2"] < 24
    rows = {(c.B, c.L, c.win) for c in CASES}
    for want in ((1, 1, (0, 0)), (1, 33, (1, 0)), (1, 65, (0, 1)), (1, 150, (31, 0)), (1, 200, (32, 32)), (1, 200, (63, 64)), (1, 321, (100, -1)),
                 (1, 321, (-1, 0)), (1, 321, (100, 0)), (2, 200, (5, 70)), (3, 200, (64, 63)), (1, 321, (400, 400)), (2, 2504, (1100, 1100)),
                 (1, 2504, (-1, 0)), (1, 2104, (2047, 0)), (2, 2104, (0, 2047)), (1, 2504, (70, 5)), (1, 200, (0, 0)), (1, 64, (63, 0)),
                 (1, 64, (0, 63)), (1, 128, (63, 0)), (1, 128, (0, 63)), (1, 321, (64, 63)), (1, 321, (63, 64)), (1, 2504, (100, 0)),
                 (1, 2504, (100, -1)), (1, 321, (-1, -1)), (2, 2104, (-1, -1))):
        assert want in rows, want
    for kern in ("win4", "win12"):
        mine = [c for c in CASES if kern_of(c) == kern]
        assert {c.ld for c in mine} == {"dense", "slice", "vt+64", "vt+8", "ldo+8", "ldo+4"}, kern
        assert {"A", "spike10", "spike6"} == {c.fam for c in mine}, kern
        assert any(c.B > 1 and c.L % 64 for c in mine) and any(c.win == (-1, -1) for c in mine) and any(c.win == (-1, 0) and c.L % 64 for c in mine)
        assert any(c.win[0] == 100 for c in mine), "the hazard row"
        assert any(ops_of(c).poison is not None for c in mine), "no row of the form carries poison inside the sample"
    for win in ((-1, -1), (-1, 0)):
        assert {c.cut for c in CASES if c.L == 2104 and c.win == win and c.B * c.H == 8} == {0, 1, 2, 3}
        assert {c.cut for c in CASES if c.L == 2104 and c.win == win and c.H == 3} == {0, 1, 2, 3}
    assert {span_of(c.L, c.win) for c in CASES} >= {2047, 2048}
    # forced cuts with blocks behind the head's last unit, under a bounded left, on the 12-wave form
    empty = [c for c in CASES if kern_of(c) == "win12" and c.cut and c.win[0] >= 0 and (12 * expected_plan(c, 256)["n12"]
             + 8 * (expected_plan(c, 256)["q_blocks"] - expected_plan(c, 256)["n12"] - 1)) * 32 >= c.L]
    assert {c.cut for c in empty} == {3, 9} and {c.win for c in empty} == {(0, 2047), (32, -1), (64, 1700)}
    assert all(c.B == 1 or c.L % 8 == 0 for c in CASES) and all(c.H <= 4 and c.L <= 2504 for c in CASES) and len(set(IDS)) == len(IDS)
    for c in CASES:                                                 # the spike rows: the window holds the spike for some queries only
        if c.fam != "A":
            col = window_mask(c.L, c.win)[:, 64 + (c.L - 64) * 2 // 3]
            assert bool(col.any()) and not bool(col.all())
