"""The DiT's five opt-in forward settings together (ffn_precision, proj_precision, attn_precision, attn_window, attn_block_mask) - no GPU
needed. Every combination goes through the named setters of WanModel and of one WanAttentionBlock, in the pipelines' order and in its
reverse; what each call must do is computed HERE from the table of DESIGN.md section 8 (`refusal` below), never from the code under
test: the call succeeds or raises the table's error type, a refused call leaves every mirror of the state and the prepared-weights
generation alone, and after a successful one the mirrors on model, block and attention modules agree. Then: blocks that differ from their
model, and the "apply what was asked for" rule at both pipeline constructors."""
import itertools
import types

import pytest
import torch

ORDER = ("ffn_precision", "attn_precision", "attn_window", "attn_block_mask", "proj_precision")       # the pipelines' order
SETTER = {"ffn_precision": "set_ffn_precision", "attn_precision": "set_attn_precision", "attn_window": "set_attn_window",
          "attn_block_mask": "set_attn_block_mask", "proj_precision": "set_proj_precision"}
DEFAULT = dict(ffn_precision="bf16", proj_precision="bf16", attn_precision="bf16", attn_window=None, attn_block_mask=None)


def _mask256():
    return torch.tensor([[True, True, False, False], [False, False, True, True]])      # 2 x 4 tiles of 128 x 64: L = 256


MASK = _mask256()
COMBOS = [dict(ffn_precision=f, proj_precision=p, attn_precision=a, attn_window=w, attn_block_mask=k)
          for f, p, a, w, k in itertools.product(("bf16", "mxfp8"), ("bf16", "mxfp8"), ("bf16", "mxfp8_qk", "mxfp8_qk_pv"), (None, (8, 8)),
                                                 (None, MASK))]
assert len(COMBOS) == 48


def _model(**over):
    """oracle.wan_dit.TINY_CFG: dim 256, ffn_dim 512, two blocks; num_heads=2 -> head_dim 128, the default 4 heads -> 64."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    return WanModel.from_config(dict(wan_dit.TINY_CFG, model_type="ti2v", **over)).eval()


def refusal(name, value, cur, head_dim, dim=256, ffn_dim=512):
    """The table: the error type that setting `name` to the (well-formed) `value` raises while the other settings are `cur`, or None."""
    if name == "ffn_precision":
        return ValueError if value == "mxfp8" and (dim % 256 or ffn_dim % 256) else None
    if name == "proj_precision":
        return ValueError if value == "mxfp8" and dim % 256 else None
    if name == "attn_precision":
        if value == "bf16":
            return None
        if head_dim != 128:
            return ValueError
        return NotImplementedError if cur["attn_window"] is not None or cur["attn_block_mask"] is not None else None
    other = "attn_block_mask" if name == "attn_window" else "attn_window"
    if value is None:
        return None
    return NotImplementedError if head_dim != 128 or cur["attn_precision"] != "bf16" or cur[other] is not None else None


def _attn_state(a):
    return a.attn_precision, a.proj_precision, a.attn_window, a.window_size, a.attn_block_mask


def _block_state(b):
    return (b.ffn_precision, b.proj_precision, b.window_size, _attn_state(b.self_attn), _attn_state(b.cross_attn))


def _state(m):
    """The prepared-weights generation and every mirror of the five settings (a resolver compares by identity)."""
    return (m._prep_gen, m.ffn_precision, m.proj_precision, m.attn_precision, m.attn_window, m.window_size, m.config["window_size"],
            m.attn_block_mask, tuple(_block_state(b) for b in m.blocks))


def _assert_block(b, want, resolver=None):
    """One block's mirrors of the logical state `want`; `resolver`: the object its self-attention must hold (a model-level mask)."""
    sa, ca = b.self_attn, b.cross_attn
    win = want["attn_window"] or (-1, -1)
    assert b.ffn_precision == want["ffn_precision"]
    assert b.proj_precision == sa.proj_precision == ca.proj_precision == want["proj_precision"]
    assert sa.attn_precision == want["attn_precision"]
    assert sa.attn_window == want["attn_window"] and sa.window_size == b.window_size == win
    if want["attn_block_mask"] is None:
        assert sa.attn_block_mask is None
    else:
        assert sa.attn_block_mask.spec is want["attn_block_mask"] and (resolver is None or sa.attn_block_mask is resolver)
    # the cross-attention's window, mask and attn_precision never move
    assert (ca.attn_precision, ca.attn_window, ca.window_size, ca.attn_block_mask) == ("bf16", None, (-1, -1), None)


def _assert_model(m, want):
    win = want["attn_window"] or (-1, -1)
    assert (m.ffn_precision, m.proj_precision, m.attn_precision) == (want["ffn_precision"], want["proj_precision"], want["attn_precision"])
    assert m.attn_window == want["attn_window"] and m.window_size == m.config["window_size"] == win
    assert (m.attn_block_mask is None) == (want["attn_block_mask"] is None)
    for b in m.blocks:
        _assert_block(b, want, m.attn_block_mask)


def _plant(m):
    """Stand-ins for prepared operands and cached K / V^T, so that a setter's drops can be seen on a CPU."""
    for b in m.blocks:
        b._prep = b.self_attn._prep = b.cross_attn._prep = {"planted": 1}
        b.self_attn._kv_cache, b.cross_attn._kv_cache = {"planted": 1}, {"planted": 1}


def _assert_dropped(b, name):
    """What a successful setter of `name` must have dropped on block b (the attention-core settings prepare nothing)."""
    if name == "ffn_precision":
        assert b._prep is None
    if name == "proj_precision":
        assert b.self_attn._prep is None and b.cross_attn._prep is None and not b.self_attn._kv_cache and not b.cross_attn._kv_cache


@pytest.mark.parametrize("level", ["model", "block"])
@pytest.mark.parametrize("order", ["pipeline", "reverse"])
@pytest.mark.parametrize("heads", [2, 4])
def test_every_combination_in_two_orders_follows_the_table(heads, order, level):
    head_dim = 256 // heads
    names = ORDER if order == "pipeline" else ORDER[::-1]
    for combo in COMBOS:
        m = _model(num_heads=heads)
        target = m if level == "model" else m.blocks[1]
        cur = dict(DEFAULT)
        for name in names:
            value, what = combo[name], f"{level}.{SETTER[name]}({combo[name]!r}) after {cur}, head_dim {head_dim}"
            err = refusal(name, value, cur, head_dim)
            _plant(m)
            before = _state(m)
            if err is not None:
                with pytest.raises(err) as ei:
                    getattr(target, SETTER[name])(value)
                assert type(ei.value) is err, what
                assert _state(m) == before, what + ": a refused call changed the state"
                continue
            getattr(target, SETTER[name])(value)              # (a refusal the table does not hold fails here)
            cur[name] = value
            if level == "model":
                assert m._prep_gen > before[0], what
                _assert_model(m, cur)
                assert m._prep is None and all(b._prep is None and b.self_attn._prep is None and b.cross_attn._prep is None and
                                               not b.cross_attn._kv_cache for b in m.blocks), what
            else:
                assert m._prep_gen == before[0], what + ": a block-level setter moved the model's generation"
                _assert_block(target, cur)
                _assert_dropped(target, name)
                assert _block_state(m.blocks[0]) == before[8][0] and _state(m)[1:8] == before[1:8], what + ": another block or the model moved"


def test_refusals_carry_the_tables_type_exactly():
    """pytest.raises accepts subclasses; the table names the types themselves (NotImplementedError is no ValueError, but it IS a
    RuntimeError): one call per row of the table, with the type compared exactly."""
    m64, m128 = _model(), _model(num_heads=2)
    m320 = _model(dim=320, num_heads=5, ffn_dim=512)
    for call, err in ((lambda: m64.set_attn_precision("mxfp8_qk"), ValueError), (lambda: m64.set_attn_window((8, 8)), NotImplementedError),
                      (lambda: m64.set_attn_block_mask(MASK), NotImplementedError), (lambda: m320.set_ffn_precision("mxfp8"), ValueError),
                      (lambda: m320.set_proj_precision("mxfp8"), ValueError), (lambda: m128.set_attn_window((8,)), ValueError),
                      (lambda: m128.set_attn_block_mask("frames"), TypeError),
                      (lambda: m128.set_attn_block_mask(torch.ones(3, 2, 4, dtype=torch.bool)), ValueError),
                      (lambda: m128.set_ffn_precision("fp8"), ValueError), (lambda: m128.set_proj_precision("fp8"), ValueError),
                      (lambda: m128.set_attn_precision("fp8"), ValueError)):
        with pytest.raises(Exception) as ei:
            call()
        assert type(ei.value) is err


def test_a_model_level_mask_is_one_resolver_and_a_resolver_is_reused():
    from univid_amd.wan.model import AttnBlockMask
    m = _model(num_heads=2)
    m.set_attn_block_mask(MASK)
    r = m.attn_block_mask
    assert isinstance(r, AttnBlockMask) and r.spec is MASK and all(b.self_attn.attn_block_mask is r for b in m.blocks)
    m.set_attn_block_mask(None)
    m.set_attn_block_mask(r)                                       # an existing resolver passed as a spec: reused, with its cache
    assert m.attn_block_mask is r and all(b.self_attn.attn_block_mask is r for b in m.blocks)
    m.blocks[0].set_attn_block_mask(None)
    m.blocks[0].set_attn_block_mask(r)
    assert m.blocks[0].self_attn.attn_block_mask is r


# ---- blocks that differ from the model ----------------------------------------------------------------------------------------------
def test_a_block_with_its_own_mask_refuses_conflicting_model_setters_only():
    m = _model(num_heads=2)
    m.blocks[1].set_attn_block_mask(MASK)
    own = m.blocks[1].self_attn.attn_block_mask
    before = _state(m)
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(8, 8\)"):
        m.set_attn_window((8, 8))
    assert _state(m) == before
    for mode in ("mxfp8_qk", "mxfp8_qk_pv"):
        with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
            m.set_attn_precision(mode)
        assert _state(m) == before
    # what does not conflict succeeds, and leaves the block's own mask where it is
    for call in (lambda: m.set_ffn_precision("mxfp8"), lambda: m.set_proj_precision("mxfp8"), lambda: m.set_attn_window(None),
                 lambda: m.set_attn_precision("bf16")):
        gen = m._prep_gen
        call()
        assert m._prep_gen > gen and m.blocks[1].self_attn.attn_block_mask is own and m.blocks[0].self_attn.attn_block_mask is None
    assert m.ffn_precision == "mxfp8" and m.proj_precision == "mxfp8" and all(b.ffn_precision == "mxfp8" for b in m.blocks)
    m.set_attn_block_mask(_mask256())                               # a model-level mask replaces it: one resolver for every block
    assert all(b.self_attn.attn_block_mask is m.attn_block_mask for b in m.blocks) and m.attn_block_mask is not own


@pytest.mark.parametrize("mode", ["mxfp8_qk", "mxfp8_qk_pv"])
def test_a_block_with_its_own_mxfp8_attention_refuses_conflicting_model_setters_only(mode):
    m = _model(num_heads=2)
    m.blocks[1].set_attn_precision(mode)
    before = _state(m)
    with pytest.raises(NotImplementedError, match=rf"window_size \(8, 8\) with attn_precision '{mode}'"):
        m.set_attn_window((8, 8))
    assert _state(m) == before
    with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
        m.set_attn_block_mask(MASK)
    assert _state(m) == before
    for call in (lambda: m.set_ffn_precision("mxfp8"), lambda: m.set_proj_precision("mxfp8"), lambda: m.set_attn_window((-1, -1)),
                 lambda: m.set_attn_block_mask(None)):
        gen = m._prep_gen
        call()
        assert m._prep_gen > gen and m.blocks[1].self_attn.attn_precision == mode and m.blocks[0].self_attn.attn_precision == "bf16"
    m.set_attn_precision("bf16")                                   # the model-level setter brings the block back
    m.set_attn_window((8, 8))
    _assert_model(m, dict(DEFAULT, ffn_precision="mxfp8", proj_precision="mxfp8", attn_window=(8, 8)))


# ---- the application rule at both pipeline call sites ---------------------------------------------------------------------------------
def _fusion(cfg_kw, wan_pipeline):
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    return CrossAttentionFusionPipeline(CrossAttentionConfig(use_lora=False, enable_bagel_extraction=False, **cfg_kw), wan_pipeline=wan_pipeline,
                                        context_projector=lambda *a, **k: None)


def _non_default_model():
    m = _model(num_heads=2)
    m.set_ffn_precision("mxfp8"), m.set_proj_precision("mxfp8"), m.set_attn_window((8, 8))
    return m


NON_DEFAULT = dict(DEFAULT, ffn_precision="mxfp8", proj_precision="mxfp8", attn_window=(8, 8))
SWITCHES = (("ffn_precision", "mxfp8"), ("attn_precision", "mxfp8_qk"), ("attn_precision", "mxfp8_qk_pv"), ("attn_window", (8, 8)),
            ("attn_window", [-1, 0]), ("attn_block_mask", MASK), ("proj_precision", "mxfp8"))


def test_wan_ti2v_applies_what_was_asked_for():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    kept = WanTI2V(TI2VConfig, model=_non_default_model(), device="cpu")                     # None keeps the model's mode
    _assert_model(kept.model, NON_DEFAULT)
    m = _non_default_model()
    gen = m._prep_gen
    same = WanTI2V(TI2VConfig, model=m, device="cpu", ffn_precision="mxfp8", proj_precision="mxfp8", attn_precision="bf16", attn_window=(8, 8))
    _assert_model(same.model, NON_DEFAULT)
    assert m._prep_gen == gen, "a keyword equal to the model's mode called its setter"
    for name, value in SWITCHES:                                                             # a differing value switches
        pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", **{name: value})
        _assert_model(pipe.model, dict(DEFAULT, **{name: tuple(value) if name == "attn_window" else value}))
    back = WanTI2V(TI2VConfig, model=_non_default_model(), device="cpu", ffn_precision="bf16", proj_precision="bf16", attn_window=(-1, -1))
    _assert_model(back.model, DEFAULT)


def test_fusion_pipeline_applies_what_was_asked_for():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    m = _non_default_model()
    gen = m._prep_gen
    fused = _fusion({}, WanTI2V(TI2VConfig, model=m, device="cpu"))          # injected, and the config holds the defaults: left alone
    _assert_model(fused.dit_model, NON_DEFAULT)
    assert fused.dit_model is m and m._prep_gen == gen
    for name, value in SWITCHES:
        fused = _fusion({name: value}, WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu"))
        _assert_model(fused.dit_model, dict(DEFAULT, **{name: tuple(value) if name == "attn_window" else value}))
    # a DiT object without the setters is tolerated, whatever the config asks for
    bare = types.SimpleNamespace(model=torch.nn.Module(), vae=None, text_encoder=None)
    fused = _fusion(dict(ffn_precision="mxfp8", proj_precision="mxfp8", attn_precision="mxfp8_qk", attn_window=(8, 8), attn_block_mask=MASK), bare)
    assert fused.dit_model is bare.model


@pytest.mark.parametrize("site", ["wan_ti2v", "fusion"])
def test_conflicting_keywords_are_applied_one_at_a_time_in_the_pipelines_order(site):
    """ffn, attn_precision, attn_window, attn_block_mask, proj - each through its named setter: the window meets the MXFP8 attention that
    was set just before it and is refused as today; what came before it is applied, what comes after it is not."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    for kw, match, after in (
            (dict(ffn_precision="mxfp8", attn_precision="mxfp8_qk", attn_window=(8, 8), attn_block_mask=MASK, proj_precision="mxfp8"),
             r"window_size \(8, 8\) with attn_precision 'mxfp8_qk'", dict(DEFAULT, ffn_precision="mxfp8", attn_precision="mxfp8_qk")),
            (dict(ffn_precision="mxfp8", attn_precision="mxfp8_qk_pv", attn_block_mask=MASK, proj_precision="mxfp8"),
             r"attn_block_mask with attn_precision 'mxfp8_qk_pv'", dict(DEFAULT, ffn_precision="mxfp8", attn_precision="mxfp8_qk_pv")),
            (dict(attn_window=(8, 8), attn_block_mask=MASK, proj_precision="mxfp8"),
             r"attn_block_mask with window_size \(8, 8\)", dict(DEFAULT, attn_window=(8, 8)))):
        m = _model(num_heads=2)
        with pytest.raises(NotImplementedError, match=match):
            if site == "wan_ti2v":
                WanTI2V(TI2VConfig, model=m, device="cpu", **kw)
            else:
                _fusion(kw, WanTI2V(TI2VConfig, model=m, device="cpu"))
        _assert_model(m, after)
