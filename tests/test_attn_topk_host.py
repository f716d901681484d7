"""Host-side behaviour of the data-dependent block-sparse self-attention (univid_amd.wan.attention.TopKBlockMask) - no GPU needed: the
spec's validation and immutability, a float top_k resolving to a count per grid, keep caching per grid, every refusal with state unchanged,
the keyword reaching the model from WanTI2V and CrossAttentionConfig, the seam's guards, the three entry points' ctypes signatures against
the header, and the reference selection function of the GPU tests (tests/test_attn_topk.py) holding its own invariants on designed inputs,
with the conditions of that file's designed operands."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from test_attn_topk import (D, KB, KEEPS, QB, SEL_CASES, SEL_NKB, lists_of, mask_of, nblocks, ref_rank, ref_select, sel_expected, sel_keep,
                            sel_len, sel_operands, sel_rank, split_operands)

pytestmark = []          # (test_attn_topk is imported for its references and builders only; nothing here carries its gpu mark)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**over):
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG, **over)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(wan_dit.make_state_dict(cfg, 0))
    return m.eval()


def _state(m):
    return (m.attn_precision, m.window_size, m.attn_window, m.attn_block_mask, tuple(b.self_attn.attn_precision for b in m.blocks),
            tuple((b.self_attn.attn_window, b.self_attn.attn_block_mask) for b in m.blocks), m._prep_gen)


def _keep256():
    return torch.tensor([[True, False, False, False], [False, False, True, False]])


# ---- the spec --------------------------------------------------------------------------------------------------------------------------
def test_spec_validation_immutability_and_float_top_k():
    from univid_amd.wan.attention import TopKBlockMask
    s = TopKBlockMask(3)
    assert (s.top_k, s.keep, s.q_block, s.k_block) == (3, None, 128, 64) and s.count(200) == 3 and s.count(64) == 3
    assert "top_k=3" in repr(s) and "keep=None" in repr(s)
    for name, value in (("top_k", 5), ("keep", None), ("other", 1)):
        with pytest.raises(AttributeError, match="immutable"):
            setattr(s, name, value)
    with pytest.raises(AttributeError, match="immutable"):
        del s.top_k
    # a fraction of the key tiles, rounded up, per sequence length: ceil(f * nkb)
    f = TopKBlockMask(0.18)
    for n in (64, 200, 256, 11440, 27280, 176400):
        nkb = nblocks(n)[1]
        assert f.count(n) == math.ceil(0.18 * nkb) >= 1, n
    assert f.count(11440) == 33 and f.count(27280) == 77 and f.count(64) == 1
    assert TopKBlockMask(1.0).count(200) == 4 and TopKBlockMask(0.5).count(200) == 2 and TopKBlockMask(0.26).count(200) == 2
    assert TopKBlockMask(1e-9).count(27280) == 1
    for bad, err in ((0, ValueError), (-2, ValueError), (0.0, ValueError), (1.5, ValueError), (-0.1, ValueError), (float("nan"), ValueError),
                     (True, TypeError), ("3", TypeError), (None, TypeError), (torch.tensor(3), TypeError)):
        with pytest.raises(err, match="TopKBlockMask"):
            TopKBlockMask(bad)
    for bad in (_keep256().float(), torch.ones(4, dtype=torch.bool), torch.ones(1, 1, 2, 4, dtype=torch.bool), "frames", 5):
        with pytest.raises(TypeError, match="TopKBlockMask: .*keep"):
            TopKBlockMask(2, bad)
    for kw in (dict(q_block=64), dict(k_block=96), dict(q_block=0)):
        with pytest.raises(ValueError, match="multiple of 128 and k_block"):
            TopKBlockMask(2, _keep256(), **kw)
    with pytest.raises(TypeError):
        TopKBlockMask(2, None, 256)                                # the block sizes are keyword-only
    assert TopKBlockMask(2, _keep256()).keep.dtype == torch.bool and callable(TopKBlockMask(2, lambda F, H, W, nh: None).keep)


def test_resolver_caches_keep_per_grid():
    from univid_amd.wan.attention import TopKBlockMask, video_block_mask
    from univid_amd.wan.model import AttnTopKMask
    calls = []

    def keep(F, H, W, nh):
        calls.append((F, H, W, nh))
        return video_block_mask((F, H, W), frames=(0, 0))

    cpu = torch.device("cpu")
    r = AttnTopKMask(TopKBlockMask(0.5, keep), 2)
    a = r.resolve((4, 8, 8), 256, cpu)
    assert r.resolve((4, 8, 8), 256, cpu) is a and calls == [(4, 8, 8, 2)]
    assert (a.top_k, a.L) == (2, 256) and a.keep.dtype == torch.uint8 and tuple(a.keep.shape) == (1, 2, 4)
    assert a.mask.tolist() == [[[True, True, False, False], [False, False, True, True]]] and torch.equal(a.keep.bool(), a.mask)
    b = r.resolve((2, 8, 8), 128, cpu)
    assert (b.top_k, b.L) == (1, 128) and r.prepare((2, 8, 8), "cpu") is b and r.resolve((4, 8, 8), 256, cpu) is a
    assert calls == [(4, 8, 8, 2), (2, 8, 8, 2)] and set(r.prepared()) == {((4, 8, 8), cpu), ((2, 8, 8), cpu)}
    fixed = AttnTopKMask(TopKBlockMask(3, _keep256()), 2)
    assert fixed.resolve((4, 8, 8), 256, cpu) is fixed.resolve((1, 16, 16), 256, cpu)          # a tensor belongs to an L, whatever the grid
    with pytest.raises(ValueError, match="does not belong to L = 64"):
        fixed.resolve((1, 8, 8), 64, cpu)
    none = AttnTopKMask(TopKBlockMask(3), 2)                       # nothing to upload: any grid resolves, keyed by L
    p = none.resolve((4, 8, 8), 256, cpu)
    assert p.keep is None and p.mask is None and p.top_k == 3 and none.resolve((1, 16, 16), 256, cpu) is p
    assert none.resolve((1, 8, 8), 64, cpu).top_k == 3
    with pytest.raises(ValueError, match="a per-head keep mask needs 2 heads, got 3"):
        AttnTopKMask(TopKBlockMask(1, lambda F, H, W, nh: torch.ones(3, 2, 4, dtype=torch.bool)), 2).resolve((4, 8, 8), 256, cpu)
    coarse = AttnTopKMask(TopKBlockMask(1, torch.tensor([[True, False]]), q_block=256, k_block=128), 2).resolve((4, 8, 8), 256, cpu)
    assert coarse.mask.tolist() == [[[True, True, False, False]] * 2]
    with pytest.raises(NotImplementedError, match="4097 key tiles; the top-k selection kernel sorts at most 4096"):
        none.resolve((1, 1, 4096 * 64 + 1), 4096 * 64 + 1, cpu)
    empty_rows = AttnTopKMask(TopKBlockMask(1, torch.zeros(2, 4, dtype=torch.bool)), 2).resolve((4, 8, 8), 256, cpu)      # legal: top-k fills every row
    assert not bool(empty_rows.mask.any())


def test_prepare_keep_mask_shapes_and_refusals():
    from univid_amd import _lib
    keep, mask = _lib.prepare_keep_mask(_keep256(), 256, "cpu")
    assert keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (1, 2, 4) and torch.equal(keep.bool(), mask)
    keep3, _ = _lib.prepare_keep_mask(_keep256()[None].repeat(3, 1, 1), 256, "cpu")
    assert tuple(keep3.shape) == (3, 2, 4)
    with pytest.raises(TypeError, match="prepare_keep_mask: the mask must be a torch.bool tensor"):
        _lib.prepare_keep_mask(_keep256().float(), 256, "cpu")
    with pytest.raises(ValueError, match="prepare_keep_mask: mask shape .* does not belong to L = 200"):
        _lib.prepare_keep_mask(torch.ones(2, 3, dtype=torch.bool), 200, "cpu")


# ---- the setters' guards -----------------------------------------------------------------------------------------------------------------
def test_setter_accepts_the_spec_and_moves_the_generation():
    from univid_amd.wan.attention import TopKBlockMask
    from univid_amd.wan.model import AttnBlockMask, AttnTopKMask
    m = _model(num_heads=2)
    for spec in (TopKBlockMask(2), TopKBlockMask(0.25, _keep256()), TopKBlockMask(1, _keep256()[None].repeat(2, 1, 1)),
                 TopKBlockMask(1, lambda F, H, W, nh: _keep256())):
        gen = m._prep_gen
        m.set_attn_block_mask(spec)
        assert m._prep_gen > gen and isinstance(m.attn_block_mask, AttnTopKMask) and m.attn_block_mask.spec is spec
        assert all(b.self_attn.attn_block_mask is m.attn_block_mask and b.cross_attn.attn_block_mask is None for b in m.blocks)
        assert m.window_size == (-1, -1) and m.attn_precision == "bf16"
    m.set_ffn_precision("mxfp8")                                   # independent of the spec
    m.set_proj_precision("mxfp8")
    assert all(b.self_attn.attn_block_mask is m.attn_block_mask for b in m.blocks)
    m.set_ffn_precision("bf16")
    m.set_proj_precision("bf16")
    m.blocks[1].set_attn_block_mask(_keep256() | True)              # a block of its own: a static mask beside the others' top-k
    assert isinstance(m.blocks[1].self_attn.attn_block_mask, AttnBlockMask) and isinstance(m.blocks[0].self_attn.attn_block_mask, AttnTopKMask)
    m.blocks[1].set_attn_block_mask(TopKBlockMask(4))
    assert isinstance(m.blocks[1].self_attn.attn_block_mask, AttnTopKMask) and m.blocks[1].self_attn.attn_block_mask is not m.attn_block_mask
    gen = m._prep_gen
    m.set_attn_block_mask(None)
    assert m._prep_gen > gen and m.attn_block_mask is None and all(b.self_attn.attn_block_mask is None for b in m.blocks)


def test_refusals_leave_the_state_unchanged():
    from univid_amd.wan.attention import TopKBlockMask
    spec = TopKBlockMask(2, _keep256())
    m = _model()                                                   # the tiny config: 4 heads of 64
    before = _state(m)
    for target in (m, m.blocks[0]):
        with pytest.raises(NotImplementedError, match="head_dim 128"):
            target.set_attn_block_mask(spec)
    assert _state(m) == before
    m = _model(num_heads=2)
    m.set_attn_block_mask(spec)
    before = _state(m)
    with pytest.raises(ValueError, match="needs 2 heads"):
        m.set_attn_block_mask(TopKBlockMask(2, torch.ones(3, 2, 4, dtype=torch.bool)))
    with pytest.raises(ValueError, match="needs 2 heads"):
        m.blocks[0].set_attn_block_mask(TopKBlockMask(2, torch.ones(3, 2, 4, dtype=torch.bool)))
    assert _state(m) == before
    for mode in ("mxfp8_qk", "mxfp8_qk_pv"):
        for target in (m, m.blocks[1]):
            with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
                target.set_attn_precision(mode)
    for target in (m, m.blocks[1]):
        with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(64, 64\)"):
            target.set_attn_window((64, 64))
    assert _state(m) == before
    # the other way round
    m.set_attn_block_mask(None)
    for setup, undo, match in ((lambda: m.set_attn_precision("mxfp8_qk"), lambda: m.set_attn_precision("bf16"), "attn_block_mask with attn_precision 'mxfp8_qk'"),
                               (lambda: m.set_attn_precision("mxfp8_qk_pv"), lambda: m.set_attn_precision("bf16"), "attn_block_mask with attn_precision 'mxfp8_qk_pv'"),
                               (lambda: m.set_attn_window((64, 64)), lambda: m.set_attn_window(None), r"attn_block_mask with window_size \(64, 64\)")):
        setup()
        before = _state(m)
        for target in (m, m.blocks[1]):
            with pytest.raises(NotImplementedError, match=match):
                target.set_attn_block_mask(spec)
        assert _state(m) == before
        undo()
    m.set_attn_block_mask(spec)
    assert m.attn_block_mask is not None


def test_sequence_parallel_and_padded_samples_are_refused():
    from univid_amd.wan.attention import TopKBlockMask
    m = _model(num_heads=2)
    m.set_attn_block_mask(TopKBlockMask(1))
    sa = m.blocks[0].self_attn
    with pytest.raises(NotImplementedError, match="attn_block_mask is not built for the sequence-parallel forward"):
        sa._self_attn_sp(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, (None, 8, 0))
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        sa._self_attn(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, sp=(None, 8, 0))
    x = torch.zeros(2, 40, 256)
    with pytest.raises(NotImplementedError, match="attn_block_mask with padded samples .* call WanModel.forward, which strips the padding"):
        sa(x, torch.tensor([40, 33]), torch.tensor([[1, 5, 8], [1, 3, 11]]), None)


def test_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.attention import TopKBlockMask
    from univid_amd.wan.model import AttnTopKMask
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    spec = TopKBlockMask(0.5, _keep256())
    pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_block_mask=spec)
    assert isinstance(pipe.model.attn_block_mask, AttnTopKMask) and pipe.model.attn_block_mask.spec is spec
    assert all(b.self_attn.attn_block_mask is pipe.model.attn_block_mask for b in pipe.model.blocks)
    assert pipe.model.attn_precision == "bf16" and pipe.model.ffn_precision == "bf16" and pipe.model.window_size == (-1, -1)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        WanTI2V(TI2VConfig, model=_model(), device="cpu", attn_block_mask=spec)
    with pytest.raises(NotImplementedError, match="attn_block_mask with attn_precision 'mxfp8_qk'"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_precision="mxfp8_qk", attn_block_mask=spec)
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(8, 8\)"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_window=(8, 8), attn_block_mask=spec)
    plain = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu")
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(attn_block_mask=spec, ffn_precision="mxfp8", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.dit_model.attn_block_mask.spec is spec and fused.dit_model.ffn_precision == "mxfp8"


def test_seam_guards_without_a_gpu():
    """The seam refuses host tensors first (no CPU path), the keyword stays keyword-only and last, and TopKBlockMask is exported."""
    from univid_amd import _lib
    from univid_amd.wan import attention as att
    q = torch.zeros(1, 8, 1, 128)
    with pytest.raises(_lib.UnividHipError):
        att.flash_attention(q, q, q, block_mask=att.TopKBlockMask(1))
    for fn in (att.flash_attention, att.attention):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "block_mask" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default is None
    assert "TopKBlockMask" in att.__all__


def test_wrappers_check_their_tensors_before_the_library_is_touched(monkeypatch):
    from univid_amd import _lib
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a rejected call reached the library"))
    n, H = 200, 2
    nqb, nkb = nblocks(n)
    q = torch.zeros(n, H * D, dtype=torch.bfloat16)
    qbar, kbar = torch.zeros(1, H, nqb, D), torch.zeros(1, H, nkb, D)
    idx, cnt = torch.zeros(1, H, nqb, nkb, dtype=torch.int32), torch.zeros(1, H, nqb, dtype=torch.int32)
    for bad, match in (((q.float(), q, qbar, kbar), r"attn_pool_qk\.q: expected"), ((q, q[:100].clone(), qbar, kbar), r"attn_pool_qk\.k: the kernel addresses"),
                       ((q, q, qbar.double(), kbar), r"attn_pool_qk\.qbar: expected"), ((q, q, qbar, kbar[:, :, :3]), r"attn_pool_qk\.kbar: ")):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.attn_pool_qk(*bad, n, H, D)
    keep = torch.ones(1, nqb, nkb, dtype=torch.uint8)
    for bad, match in (((qbar[:, :1].clone(), kbar, None, 2, idx, cnt), r"attn_bs_select\.qbar: "), ((qbar, kbar, keep.bool(), 2, idx, cnt), r"attn_bs_select\.keep: expected"),
                       ((qbar, kbar, keep[:, :, :3], 2, idx, cnt), r"attn_bs_select\.keep: expected uint8 \[1 or 2, 2, 4\]"),
                       ((qbar, kbar, None, 2, idx.long(), cnt), r"attn_bs_select\.tile_idx: expected"), ((qbar, kbar, None, 2, idx, cnt[:, :1].clone()), r"attn_bs_select\.tile_cnt: ")):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.attn_bs_select(*bad, n, H)
    vt = torch.zeros(H * D, 256, dtype=torch.bfloat16)
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_bs_lists\.tile_idx: the kernel addresses"):
        _lib.flash_attn_bs_lists(q, q, vt, q.clone(), n, H, D, 1.0, idx[:, :1].clone(), cnt, H, 1)
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_bs_lists\.tile_cnt: expected"):
        _lib.flash_attn_bs_lists(q, q, vt, q.clone(), n, H, D, 1.0, idx, cnt.long(), H, 1)
    with pytest.raises(_lib.UnividHipError, match=r"must live on the GPU"):
        _lib.flash_attn_bs_lists(q, q, vt, q.clone(), n, H, D, 1.0, idx, cnt, H, 1)


def test_ctypes_signatures_match_the_header():
    from univid_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "univid_hip.h")).read(), flags=re.S)
    cls_py = {_lib._P: "p", _lib._L: "l", _lib._I: "i", _lib._F: "f"}
    want = {"uv_attn_pool_qk": "plplppiiiip", "uv_attn_bs_select": "pppiippiiip", "uv_flash_attn_bs_lists_bf16": "plplplpliiiifppiip"}
    for name, classes in want.items():
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in the header"
        c = "".join("p" if "*" in a else {"long": "l", "int": "i", "float": "f"}[a.split()[-2]] for a in m.group(1).split(","))
        py = "".join(cls_py[t] for t in _lib.SIGNATURES[name])
        assert c == py == classes, f"{name}: header {c}, ctypes {py}, expected {classes}"
    # uv_flash_attn_bs_bf16 keeps its signature: the new entry is the same plus mask_samples in front of the stream
    old, new = _lib.SIGNATURES["uv_flash_attn_bs_bf16"], _lib.SIGNATURES["uv_flash_attn_bs_lists_bf16"]
    assert new == old[:-1] + [_lib._I] + old[-1:]
    assert _lib.BS_SELECT_MAX_TILES == 4096 and isinstance(ctypes.c_int(0), _lib._I)


# ---- the reference selection and the designed operands -----------------------------------------------------------------------------------
def test_reference_selection_holds_its_invariants_on_designed_inputs():
    s = torch.tensor([[5.0, 7.0, 7.0, 1.0, 7.0, 5.0, -2.0, 0.0]])
    none = torch.zeros(1, 8, dtype=torch.bool)
    assert lists_of(ref_select(s, none, 1))[0][0, :1].tolist() == [1]                          # the lowest index of the tied maximum
    assert lists_of(ref_select(s, none, 2))[0][0, :2].tolist() == [1, 2]                       # a tie across the cut: 4 stays out
    assert lists_of(ref_select(s, none, 3))[0][0, :3].tolist() == [1, 2, 4]
    assert lists_of(ref_select(s, none, 4))[0][0, :4].tolist() == [0, 1, 2, 4]                 # 0 before 5 among the tied 5.0
    assert lists_of(ref_select(s, none, 8))[1].tolist() == [8] and lists_of(ref_select(s, none, 13))[1].tolist() == [8]
    keep = torch.tensor([[False, True, False, False, False, False, True, False]])
    idx, cnt = lists_of(ref_select(s, keep, 2))
    assert cnt.tolist() == [4] and idx[0, :4].tolist() == [1, 2, 4, 6] and idx[0, 4:].tolist() == [-1] * 4      # kept 1, 6; best others 2, 4
    assert lists_of(ref_select(s, keep, 7))[1].tolist() == [8]                                 # fewer candidates than top_k: all
    full = torch.ones(1, 8, dtype=torch.bool)
    assert ref_select(s, full, 1).all()
    rank, ncand = ref_rank(s, keep)
    assert ncand.tolist() == [6] and rank[0, [2, 4, 0, 5, 3, 7]].tolist() == [0, 1, 2, 3, 4, 5]
    # the invariants, on every designed case: ascending lists, the count formula, kept tiles listed, the tie rule at the cut
    seen_kinds, ragged = set(), {}
    for c in SEL_CASES:
        _, _, sc = sel_operands(c.nkb, c.B, c.H)
        rank, ncand, kb = sel_rank(c.keep, c.nkb, c.B, c.H)
        want = sel_expected(c)
        idx, cnt = lists_of(want)
        assert torch.equal(mask_of(idx, cnt), want)                                            # (mask_of asserts range and strict ascent)
        kx = kb[None].expand_as(want)
        assert torch.equal(cnt.long(), kx.sum(-1) + (~kx).sum(-1).clamp(max=c.top_k)) and int(cnt.min()) >= 1
        assert bool((want | ~kx).all())
        listed, out = want & ~kx, ~want
        lo = sc.masked_fill(~listed, math.inf).amin(-1)
        hi = sc.masked_fill(~out, -math.inf).amax(-1)
        assert bool((lo >= hi).all())
        tied = (lo == hi)[..., None] & (sc == lo[..., None])                                    # tiles at the cut's score, where the cut splits a tie
        first_out = torch.where(tied & out, torch.arange(c.nkb), c.nkb).amin(-1)
        last_in = torch.where(tied & listed, torch.arange(c.nkb), -1).amax(-1)
        assert bool((last_in < first_out).all()), "a tie at the cut did not go to the lower index"
        ragged.setdefault(c.nkb, set()).update({bool(want[..., -1].any()), bool(want[..., -1].all())} if c.top_k < c.nkb else set())
        if c.nkb >= 179 and c.top_k <= 2:
            assert bool((lo == hi).any()), f"{c}: no row's cut splits a tie"
            inside = (sc.masked_fill(~listed, math.nan) == lo[..., None]).sum(-1)
            assert c.top_k == 1 or bool((inside >= 2).any()), f"{c}: no tie inside the cut"
            assert bool(want[..., -1].any()) and not bool(want[..., -1].all()), f"{c}: the ragged last tile is not both listed and unlisted"
        if c.keep != "none":
            seen_kinds.update((c.nkb, k) for k in ("empty", "full", "partial")
                              if bool({"empty": ~kb.any(-1), "full": kb.all(-1), "partial": kb.any(-1) & ~kb.all(-1)}[k].any()))
    for nkb in SEL_NKB[3:]:
        assert {(nkb, k) for k in ("empty", "full", "partial")} <= seen_kinds, f"nkb = {nkb}: keep rows are not empty, full and partial"
    assert {k for _, k in seen_kinds} == {"empty", "full", "partial"}
    assert {c.nkb for c in SEL_CASES} == set(SEL_NKB) and {c.keep for c in SEL_CASES} == set(KEEPS)
    for nkb in SEL_NKB:
        assert {c.top_k for c in SEL_CASES if c.nkb == nkb} == {k for k in (1, 2, nkb - 1, nkb, nkb + 5) if k >= 1}
        assert nblocks(sel_len(nkb))[1] == nkb and sel_len(nkb) % KB == 8
    assert any(c.B == 2 for c in SEL_CASES)
    q0, _, s2 = sel_operands(179, 2, 2)
    assert not torch.equal(s2[0], s2[1]) and q0.dtype == torch.float32 and torch.equal(q0, q0.round())


def test_split_operands_rank_their_halves_apart():
    """The designed attention operands (tests/test_attn_topk.py, B = 2, L = 200): in fp64 the pooled scores of each sample's '+u' tiles are
    above its '-u' tiles' by far more than any fp32 error, and the halves swap between the samples."""
    from test_attn_topk import ref_pool
    B, n, H = 2, 200, 2
    for seed in (41, 45):
        q, k, _ = split_operands(B, n, H, seed)
        s = ref_pool(q, B, n, H, QB) @ ref_pool(k, B, n, H, KB).transpose(-1, -2)             # [B, H, 2, 4]
        assert float(s[0, ..., :2].min()) > 10 > -10 > float(s[0, ..., 2:].max()) and float(s[1, ..., 2:].min()) > 10 > -10 > float(s[1, ..., :2].max())
