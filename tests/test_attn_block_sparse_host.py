"""Host-side behaviour of the opt-in block-sparse self-attention (WanModel.set_attn_block_mask) - no GPU needed: `prepare_block_mask`'s
bookkeeping and refusals, `video_block_mask` against an O(L^2) brute force, the plan, every model / seam / pipeline guard with its message
and its order (raised before any state changes), and the conditions of the designed operands of every row of the GPU table
(tests/test_attn_block_sparse.py)."""
import pytest
import torch

from test_attn_block_sparse import CASES, D, IDS, KB, KNAME, QB, assert_plan, block_mask, expand_mask, expected_plan, nblocks, ops_of, unvisited_tiles

pytestmark = []          # (test_attn_block_sparse is imported for its table and builders only; nothing here carries its gpu mark)


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


# ---- prepare_block_mask ---------------------------------------------------------------------------------------------------------------
def _lists(bm):
    return [[bm.tile_idx[h, q, :int(bm.tile_cnt[h, q])].tolist() for q in range(bm.tile_idx.shape[1])] for h in range(bm.heads)]


def test_prepare_block_mask_lists_counts_and_immutability():
    from univid_amd import _lib
    n = 640
    nqb, nkb = nblocks(n)
    m = block_mask("rand0.5", 3, n)
    bm = _lib.prepare_block_mask(m, n, "cpu")
    assert isinstance(bm, _lib.PreparedBlockMask) and (bm.L, bm.heads) == (n, 3) and bm.density == float(m.double().mean())
    assert bm.tile_idx.dtype == torch.int32 and tuple(bm.tile_idx.shape) == (3, nqb, nkb) and bm.tile_idx.is_contiguous()
    assert bm.tile_cnt.dtype == torch.int32 and tuple(bm.tile_cnt.shape) == (3, nqb) and bm.tile_cnt.is_contiguous()
    assert bm.mask.device.type == "cpu" and bm.mask.dtype == torch.bool and torch.equal(bm.mask, m)
    assert torch.equal(bm.tile_cnt.long(), m.sum(-1)) and int(bm.tile_cnt.min()) >= 1
    for h, per_head in enumerate(_lists(bm)):
        for q, lst in enumerate(per_head):
            assert lst == m[h, q].nonzero().flatten().tolist() and lst == sorted(lst), (h, q)
    shared = _lib.prepare_block_mask(m[1], n, "cpu")                          # one mask for all heads against the same mask per head
    assert shared.heads == 1 and tuple(shared.tile_idx.shape) == (1, nqb, nkb) and _lists(shared)[0] == _lists(bm)[1]
    per_head = _lib.prepare_block_mask(m[1][None].expand(3, -1, -1), n, "cpu")
    assert per_head.heads == 3 and all(lst == _lists(shared)[0] for lst in _lists(per_head))
    ones = _lib.prepare_block_mask(torch.ones(1, 1, dtype=torch.bool), 1, "cpu")
    assert ones.density == 1.0 and _lists(ones) == [[[0]]]
    for name, value in (("L", 5), ("tile_idx", None), ("other", 1)):
        with pytest.raises(AttributeError, match="immutable"):
            setattr(bm, name, value)
    with pytest.raises(AttributeError, match="immutable"):
        del bm.mask
    with pytest.raises(TypeError, match="built by prepare_block_mask"):
        _lib.PreparedBlockMask(n, 1, bm.tile_idx, bm.tile_cnt, bm.mask, 1.0)


@pytest.mark.parametrize("qblk, kblk", [(128, 128), (256, 64), (256, 192), (128, 64)])
@pytest.mark.parametrize("n", [640, 600, 65])
def test_prepare_block_mask_expands_coarser_blocks_exactly(qblk, kblk, n):
    from univid_amd import _lib
    g = torch.Generator().manual_seed(qblk + kblk + n)
    shape = (-(-n // qblk), -(-n // kblk))
    m = torch.rand(2, *shape, generator=g) < 0.5
    m[:, :, 0] |= ~m.any(-1)
    bm = _lib.prepare_block_mask(m, n, "cpu", q_block=qblk, k_block=kblk)
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    want = m[:, i // qblk, j // kblk]                                         # element mask of the coarse blocks
    assert torch.equal(expand_mask(bm.mask, 2, n), want), "the 128 x 64 tiles do not cover exactly the coarse mask's elements"
    assert tuple(bm.mask.shape) == (2, *nblocks(n))


def test_prepare_block_mask_refusals_name_the_limit():
    from univid_amd import _lib
    n = 640
    ok = torch.ones(*nblocks(n), dtype=torch.bool)
    empty = ok.clone()
    empty[3] = False
    with pytest.raises(ValueError, match=r"query block 3 of mask head 0 \(queries 384\.\.\) has no key tile"):
        _lib.prepare_block_mask(empty, n, "cpu")
    per_head = ok[None].repeat(2, 1, 1)
    per_head[1, 4] = False
    with pytest.raises(ValueError, match=r"query block 4 of mask head 1"):
        _lib.prepare_block_mask(per_head, n, "cpu")
    for bad in (ok[:4], ok[:, :9], ok[None, None], ok.flatten(), torch.ones(0, *nblocks(n), dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"mask shape|must be \[nqb, nkb\]|at least one head"):
            _lib.prepare_block_mask(bad, n, "cpu")
    for bad in (ok.float(), ok.to(torch.uint8), ok.int(), ok.tolist(), None):
        with pytest.raises(TypeError, match="must be a torch.bool tensor"):
            _lib.prepare_block_mask(bad, n, "cpu")
    for wrong in (641, 512, 1281):                                            # a wrong L: another number of blocks
        with pytest.raises(ValueError, match=rf"does not belong to L = {wrong}"):
            _lib.prepare_block_mask(ok, wrong, "cpu")
    with pytest.raises(ValueError, match="must be positive"):
        _lib.prepare_block_mask(ok, 0, "cpu")
    for kw in (dict(q_block=64), dict(q_block=192), dict(k_block=32), dict(k_block=96), dict(q_block=0)):
        with pytest.raises(ValueError, match="multiple of 128 and k_block"):
            _lib.prepare_block_mask(ok, n, "cpu", **kw)


def test_plan_is_one_kernel_on_128_query_blocks():
    from univid_amd import _lib
    for c in CASES:
        assert_plan(c)
    assert _lib.attn_bs_plan(11440, D, 2, 24) == dict(kernel=KNAME, q_blocks=90, grid=4320)
    assert _lib.attn_bs_plan(27280, D, 1, 24) == dict(kernel=KNAME, q_blocks=214, grid=5136)
    assert _lib.attn_bs_plan(1) == dict(kernel=KNAME, q_blocks=1, grid=1) == expected_plan(1, 1, 1)
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_bs_plan: head_dim 64"):
        _lib.attn_bs_plan(200, 64, 1, 2)
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_bs_plan: bad shape"):
        _lib.attn_bs_plan(0, D, 1, 2)


# ---- video_block_mask -------------------------------------------------------------------------------------------------------------------
def _brute(grid, frames, rows, cols):
    F, H, W = grid
    n = F * H * W
    i = torch.arange(n)
    f, h, w = i // (H * W), (i // W) % H, i % W
    df, dh, dw = f[None, :] - f[:, None], (h[None, :] - h[:, None]).abs(), (w[None, :] - w[:, None]).abs()      # key - query
    ok = torch.ones(n, n, dtype=torch.bool)
    if frames[0] >= 0:
        ok &= df >= -frames[0]
    if frames[1] >= 0:
        ok &= df <= frames[1]
    if rows >= 0:
        ok &= dh <= rows
    if cols >= 0:
        ok &= dw <= cols
    m = torch.zeros(*nblocks(n), dtype=torch.bool)
    qi, kj = ok.nonzero(as_tuple=True)
    m[qi // QB, kj // KB] = True
    return m, ok


@pytest.mark.parametrize("grid", [(3, 6, 10), (4, 8, 12), (2, 5, 7)])
def test_video_block_mask_is_the_block_cover_of_the_neighbourhood(grid):
    from univid_amd import _lib
    from univid_amd.wan.attention import video_block_mask
    n = grid[0] * grid[1] * grid[2]
    seen = set()
    for frames, rows, cols in (((1, 1), 2, 3), ((-1, -1), 1, -1), ((0, 2), -1, 2), ((2, 0), 1, 1), ((0, 0), 0, 0), ((-1, 0), -1, -1),
                               ((1, -1), 0, -1), ((-1, -1), -1, -1), ((0, 0), -1, -1)):
        got = video_block_mask(grid, frames=frames, rows=rows, cols=cols)
        want, elems = _brute(grid, frames, rows, cols)
        assert got.dtype == torch.bool and tuple(got.shape) == nblocks(n) and torch.equal(got, want), (grid, frames, rows, cols)
        assert bool((expand_mask(got, 1, n)[0] | ~elems).all()), "the cover must contain the element-exact neighbourhood"
        assert bool(got.any(-1).all())
        seen.add(float(got.double().mean()))
        _lib.prepare_block_mask(got, n, "cpu")
    assert max(seen) == 1.0 and (len(seen) > 2 or nblocks(n) == (1, 2))          # (2, 5, 7): 70 tokens, one query block - every cover is full
    per_head = video_block_mask(grid, frames=(1, 0), rows=1, cols=1, num_heads=3)
    assert tuple(per_head.shape) == (3, *nblocks(n)) and all(torch.equal(per_head[h], _brute(grid, (1, 0), 1, 1)[0]) for h in range(3))
    assert torch.equal(video_block_mask(grid, (1, 1), 2, 3, q_block=256, k_block=128),
                       _lib.prepare_block_mask(video_block_mask(grid, (1, 1), 2, 3, q_block=256, k_block=128), n, "cpu", 256, 128).mask[0][::2, ::2])
    for kw in (dict(frames=(-2, 0)), dict(rows=-2), dict(cols=-3)):
        with pytest.raises(ValueError, match="video_block_mask"):
            video_block_mask(grid, **kw)
    with pytest.raises(ValueError, match="video_block_mask"):
        video_block_mask((0, 4, 4))


# ---- guards -----------------------------------------------------------------------------------------------------------------------
def _mask256():
    return torch.tensor([[True, True, False, False], [False, False, True, True]])


def test_setter_specs_and_generation():
    from univid_amd import _lib
    from univid_amd.wan.model import AttnBlockMask
    m = _model(num_heads=2)                                        # dim 256: head_dim 128
    assert m.attn_block_mask is None and all(b.self_attn.attn_block_mask is None for b in m.blocks)
    for spec in (_mask256(), _mask256()[None].repeat(2, 1, 1), _lib.prepare_block_mask(_mask256(), 256, "cpu"), lambda F, H, W, nh: _mask256()):
        gen = m._prep_gen
        m.set_attn_block_mask(spec)
        assert m._prep_gen > gen and isinstance(m.attn_block_mask, AttnBlockMask) and m.attn_block_mask.spec is spec
        assert all(b.self_attn.attn_block_mask is m.attn_block_mask and b.cross_attn.attn_block_mask is None for b in m.blocks)
        assert m.window_size == (-1, -1) and m.attn_precision == "bf16"
    m.set_ffn_precision("mxfp8")                                   # independent of the mask
    m.set_proj_precision("mxfp8")
    assert all(b.self_attn.attn_block_mask is m.attn_block_mask for b in m.blocks)
    m.set_ffn_precision("bf16")
    m.set_proj_precision("bf16")
    gen = m._prep_gen
    m.set_attn_block_mask(None)
    assert m._prep_gen > gen and m.attn_block_mask is None and all(b.self_attn.attn_block_mask is None for b in m.blocks)


def test_resolver_caches_per_grid_and_refuses_another_length():
    from univid_amd import _lib
    from univid_amd.wan.model import AttnBlockMask
    calls = []

    def spec(F, H, W, nh):
        calls.append((F, H, W, nh))
        return torch.ones(*nblocks(F * H * W), dtype=torch.bool)

    cpu = torch.device("cpu")
    r = AttnBlockMask(spec, 2)
    a = r.resolve((4, 8, 8), 256, cpu)
    assert r.resolve((4, 8, 8), 256, cpu) is a and calls == [(4, 8, 8, 2)] and a.L == 256
    b = r.resolve((2, 8, 8), 128, cpu)
    assert b.L == 128 and r.prepare((2, 8, 8), "cpu") is b and r.resolve((4, 8, 8), 256, cpu) is a and calls == [(4, 8, 8, 2), (2, 8, 8, 2)]
    fixed = AttnBlockMask(_mask256(), 2)
    assert fixed.resolve((4, 8, 8), 256, cpu) is fixed.resolve((1, 16, 16), 256, cpu)          # a tensor belongs to an L, whatever the grid
    with pytest.raises(ValueError, match="does not belong to L = 64"):
        fixed.resolve((1, 8, 8), 64, cpu)
    prepared = AttnBlockMask(_lib.prepare_block_mask(_mask256(), 256, "cpu"), 2)
    assert prepared.resolve((4, 8, 8), 256, cpu) is prepared.spec
    with pytest.raises(ValueError, match=r"prepared for L = 256; this forward has L = 128"):
        prepared.resolve((2, 8, 8), 128, cpu)
    with pytest.raises(ValueError, match="lives on cpu"):
        prepared.resolve((4, 8, 8), 256, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="a per-head mask needs 2 heads, got 3"):
        AttnBlockMask(lambda F, H, W, nh: torch.ones(3, 2, 4, dtype=torch.bool), 2).resolve((4, 8, 8), 256, cpu)


def test_bad_specs_raise_with_state_unchanged():
    m = _model(num_heads=2)
    m.set_attn_block_mask(_mask256())
    before = _state(m)
    for bad, err, match in ((_mask256().float(), TypeError, "torch.bool"), (torch.ones(4, dtype=torch.bool), TypeError, "torch.bool"), ("frames", TypeError, "got str"),
                            (5, TypeError, "got int"), (torch.ones(3, 2, 4, dtype=torch.bool), ValueError, "needs 2 heads")):
        with pytest.raises(err, match=match):
            m.set_attn_block_mask(bad)
        with pytest.raises(err, match=match):
            m.blocks[0].set_attn_block_mask(bad)
        assert _state(m) == before


def test_head_dim_64_is_refused_with_state_unchanged():
    m = _model()                                                   # the tiny config: 4 heads of 64
    before = _state(m)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        m.set_attn_block_mask(_mask256())
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        m.blocks[0].set_attn_block_mask(_mask256())
    assert _state(m) == before
    m.set_attn_block_mask(None)                                    # global attention is what it runs
    assert m.attn_block_mask is None


@pytest.mark.parametrize("mode", ["mxfp8_qk", "mxfp8_qk_pv"])
def test_mask_and_mxfp8_attention_refuse_each_other_either_way_round(mode):
    m = _model(num_heads=2)
    m.set_attn_block_mask(_mask256())
    before = _state(m)
    with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
        m.set_attn_precision(mode)
    with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
        m.blocks[1].set_attn_precision(mode)
    assert _state(m) == before
    m.set_attn_block_mask(None)
    m.set_attn_precision(mode)
    before = _state(m)
    with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
        m.set_attn_block_mask(_mask256())
    with pytest.raises(NotImplementedError, match=rf"attn_block_mask with attn_precision '{mode}'"):
        m.blocks[1].set_attn_block_mask(_mask256())
    assert _state(m) == before
    m.set_attn_block_mask(None)                                    # switching the mask OFF is always legal
    m.set_attn_precision("bf16")
    m.set_attn_block_mask(_mask256())
    assert m.attn_block_mask is not None


def test_mask_and_window_refuse_each_other_either_way_round():
    m = _model(num_heads=2)
    m.set_attn_block_mask(_mask256())
    before = _state(m)
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(64, 64\)"):
        m.set_attn_window((64, 64))
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(64, 64\)"):
        m.blocks[1].set_attn_window((64, 64))
    assert _state(m) == before
    m.set_attn_window(None)                                        # (global attention beside a mask: legal, nothing to refuse)
    m.set_attn_block_mask(None)
    m.set_attn_window((64, 64))
    before = _state(m)
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(64, 64\)"):
        m.set_attn_block_mask(_mask256())
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(64, 64\)"):
        m.blocks[1].set_attn_block_mask(_mask256())
    assert _state(m) == before
    m.set_attn_block_mask(None)
    m.set_attn_window(None)
    m.set_attn_block_mask(_mask256())
    assert m.attn_block_mask is not None and m.attn_window is None


def test_sequence_parallel_forward_is_refused_with_a_mask():
    m = _model(num_heads=2)
    m.set_attn_block_mask(_mask256())
    sa = m.blocks[0].self_attn
    with pytest.raises(NotImplementedError, match="attn_block_mask is not built for the sequence-parallel forward"):
        sa._self_attn_sp(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, (None, 8, 0))
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        sa._self_attn(torch.empty(0, 256, dtype=torch.bfloat16), 0, (1, 1, 1), None, None, None, None, 1, sp=(None, 8, 0))


def test_reference_signature_forward_refuses_padding_with_a_mask():
    m = _model(num_heads=2)
    m.set_attn_block_mask(lambda F, H, W, nh: torch.ones(1, 1, dtype=torch.bool))
    sa = m.blocks[0].self_attn
    x = torch.zeros(2, 40, 256)
    with pytest.raises(NotImplementedError, match="attn_block_mask with padded samples .* call WanModel.forward, which strips the padding"):
        sa(x, torch.tensor([40, 33]), torch.tensor([[1, 5, 8], [1, 3, 11]]), None)


def test_keyword_reaches_the_model():
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    assert CrossAttentionConfig().attn_block_mask is None
    spec = _mask256()
    pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_block_mask=spec)
    assert pipe.model.attn_block_mask.spec is spec and all(b.self_attn.attn_block_mask is pipe.model.attn_block_mask for b in pipe.model.blocks)
    assert pipe.model.attn_precision == "bf16" and pipe.model.ffn_precision == "bf16" and pipe.model.window_size == (-1, -1)
    plain = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu")
    assert plain.model.attn_block_mask is None
    with pytest.raises(TypeError, match="attn_block_mask"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_block_mask="frames")
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        WanTI2V(TI2VConfig, model=_model(), device="cpu", attn_block_mask=spec)
    with pytest.raises(NotImplementedError, match="attn_block_mask with attn_precision 'mxfp8_qk'"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_precision="mxfp8_qk", attn_block_mask=spec)
    with pytest.raises(NotImplementedError, match=r"attn_block_mask with window_size \(8, 8\)"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", attn_window=(8, 8), attn_block_mask=spec)
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(attn_block_mask=spec, ffn_precision="mxfp8", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.dit_model.attn_block_mask.spec is spec and fused.dit_model.ffn_precision == "mxfp8"


def test_seam_guards_without_a_gpu():
    """The seam refuses host tensors first (no CPU path), as before; the keyword does not move that, and it is keyword-only: the reference's
    positional signature is unchanged."""
    import inspect
    from univid_amd import _lib
    from univid_amd.wan.attention import attention, flash_attention
    q = torch.zeros(1, 8, 1, 128)
    with pytest.raises(_lib.UnividHipError):
        flash_attention(q, q, q, block_mask=torch.ones(1, 1, dtype=torch.bool))
    for fn, last in ((flash_attention, "version"), (attention, "fa_version")):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "block_mask" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default is None
        assert params[-2].name == last and [p.name for p in params[:5]] == ["q", "k", "v", "q_lens", "k_lens"]


# ---- operand builders ---------------------------------------------------------------------------------------------------------------
def test_designed_operands_hold_their_conditions_for_every_row():
    """Every row of the GPU table, on the CPU: the scale equality, the span below 2^24, every P exact, the excepted share at or below 0.5 %
    (the cap is a condition of the operands: the 64-seed loop replaces a seed that misses it), the spikes' score pattern under the mask, the
    poisoned tiles hidden from every query (all asserted inside the builders) - and the table's coverage."""
    worst = dict(excluded_share=0.0, span_log2=0.0)
    for c in CASES:
        o = ops_of(c)
        assert o.ref.shape == (c.B * c.L, c.H * D) and o.ref.dtype == torch.bfloat16
        assert o.stats["excluded_share"] <= 0.005 and o.stats["span_log2"] < 24, IDS[CASES.index(c)]
        for key in worst:
            worst[key] = max(worst[key], o.stats[key])
        if c.fam == "A":
            assert o.poison == unvisited_tiles(block_mask(c.mask, c.H, c.L), c.H)
    print(f"{len(CASES)} rows: largest excepted share {worst['excluded_share']:.4%}, largest span 2^{worst['span_log2']:.2f}")
    assert worst["excluded_share"] <= 0.005 and worst["span_log2"] < 24
    rows = {(c.B, c.H, c.L, c.mask) for c in CASES if c.fam == "A" and c.ld == "dense"}
    for want in ((1, 2, 1, "ones"), (1, 2, 65, "ones"), (1, 2, 65, "first"), (1, 2, 65, "last"), (1, 2, 200, "diag"), (1, 2, 200, "anti"),
                 (1, 2, 200, "last"), (1, 2, 200, "checker"), (1, 2, 321, "last"), (1, 2, 321, "first+last"), (2, 2, 200, "checker"),
                 (3, 2, 200, "anti"), (1, 3, 640, "rand0.5"), (1, 2, 640, "checker"), (2, 4, 2504, "rand0.3"), (1, 2, 2504, "diag")):
        assert want in rows, want
    assert {c.ld for c in CASES if (c.B, c.H, c.L, c.mask) == (2, 2, 200, "checker")} == {"dense", "slice", "vt+64", "vt+8", "ldo+8", "ldo+4"}
    assert {(c.fam, c.L) for c in CASES if c.fam != "A"} == {(f, n) for f in ("spike10", "spike6") for n in (321, 640)}
    assert any(c.fam == "A" and any(ops_of(c).poison) for c in CASES), "no row carries poison inside the sample"
    assert all(c.B == 1 or c.L % 8 == 0 for c in CASES) and all(c.H <= 4 and c.L <= 2504 for c in CASES) and len(set(IDS)) == len(IDS)
    counts = block_mask("rand0.5", 3, 640).sum(-1)                              # the per-head random row: odd and even counts, ragged densities
    assert bool((counts % 2 == 0).any()) and bool((counts % 2 == 1).any()) and int(counts.min()) >= 1
    assert abs(float(block_mask("rand0.5", 3, 640).double().mean()) - 0.5) < 0.1 and abs(float(block_mask("rand0.3", 4, 2504).double().mean()) - 0.3) < 0.05
    for c in CASES:                                                 # a stacked sample whose V^T columns start off a tile boundary
        if c.B == 3:
            assert c.L % KB != 0 and c.L % QB != 0
