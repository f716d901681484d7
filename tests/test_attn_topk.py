"""Data-dependent block-sparse self-attention (univid_amd.wan.attention.TopKBlockMask): uv_attn_pool_qk, uv_attn_bs_select and
uv_flash_attn_bs_lists_bf16 through their `_lib` wrappers, the operator seam and the small model - against references written HERE in fp64
torch (pooling: the mean of a block's valid rows; selection: `ref_select`, the keep tiles plus the top_k best of the others under (score
descending, tile index ascending); attention: `flash_attn_bs` at batch 1 under the static mask rebuilt from a sample's read-back lists).

Everything is bit-exact except two checks with stated bounds:
  pooling, ragged block   the fp32 sum of small integers is exact; its division by a count that is no power of two is within 1 ulp of fp32 of
                          the fp64 mean (the division may be compiled as a multiplication by a reciprocal); full blocks (128 / 64 rows) are
                          exact.
  selection, random fp32  an fp32 dot product of D = 128 terms in any order differs from the exact one by at most gamma_D sum_d |q_d k_d| <
                          (D + 2) 2^-24 sum_d |q_d k_d| =: e_j for the pair (block, tile j). A listed non-kept tile t beat an unlisted one u
                          in fp32, so in fp64 s_t >= s_u - (e_t + e_u), evaluated per pair - never more than 2 (D + 2) 2^-24 max(S_t, S_u).
Designed selection operands are small integers: every fp32 score is exact, so lists and counts equal the reference exactly, ties included.
The builders' own conditions are asserted without a GPU in tests/test_attn_topk_host.py."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import load_golden

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
DEV = "cuda"
D = 128
QB, KB = 128, 64
SENT = -7.25
ISENT = -77
PAD = 64          # sentinel elements in front of and behind a buffer (64 fp32 / int32 = 256 bytes: the view stays 16-byte aligned)


@pytest.fixture(scope="module")
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


def gpu(f):
    return pytest.mark.gpu(pytest.mark.usefixtures("_init")(f))


def L():
    from univid_amd import _lib
    return _lib


def nblocks(n):
    return (n + QB - 1) // QB, (n + KB - 1) // KB


# ---------------------------------------------------------------------------------------------------------------
# the fp64 references
# ---------------------------------------------------------------------------------------------------------------
def ref_pool(x, B, n, H, block):
    """x [B*n, H*D] (any float dtype) -> fp64 [B, H, ceil(n / block), D]: the mean of each block's valid rows."""
    nb = -(-n // block)
    out = torch.empty(B, H, nb, D, dtype=F64)
    for b in range(B):
        xs = x[b * n:(b + 1) * n].double().view(n, H, D)
        for i in range(nb):
            out[b, :, i] = xs[i * block:min(n, (i + 1) * block)].mean(0)
    return out


def ref_rank(s, keep):
    """s fp64 [..., nkb] (finite), keep bool broadcastable to it -> (rank, ncand): rank[..., j] = position of tile j among its row's
    NON-kept tiles under (score descending, tile index ascending); kept tiles rank behind all of them."""
    keep = keep.expand_as(s)
    order = torch.sort(s.masked_fill(keep, -math.inf), dim=-1, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(-1, order, torch.arange(s.shape[-1]).expand_as(order).contiguous())
    return rank, (~keep).sum(-1)


def ref_select(s, keep, top_k):
    """The selected mask, bool like s: kept tiles, plus the min(top_k, candidates) best non-kept ones of each row."""
    rank, ncand = ref_rank(s, keep)
    return keep.expand_as(s) | (rank < ncand.clamp(max=top_k)[..., None])


def lists_of(sel):
    """bool [..., nkb] -> (tile_idx int32 [..., nkb] with the selected tiles ascending and -1 behind, tile_cnt int32 [...])"""
    nkb = sel.shape[-1]
    cnt = sel.sum(-1, dtype=I32)
    order = torch.sort((~sel).to(torch.uint8), dim=-1, stable=True).indices.to(I32)
    return torch.where(torch.arange(nkb, dtype=I32) < cnt[..., None], order, torch.full_like(order, -1)), cnt


def mask_of(idx, cnt):
    """read-back lists -> bool mask [..., nkb]; asserts the lists' own guarantees: count in [1, nkb], entries in range, strictly ascending"""
    idx, cnt = idx.cpu().long(), cnt.cpu().long()
    nkb = idx.shape[-1]
    assert int(cnt.min()) >= 1 and int(cnt.max()) <= nkb, f"counts outside [1, {nkb}]: {int(cnt.min())} .. {int(cnt.max())}"
    live = torch.arange(nkb) < cnt[..., None]
    assert bool(((idx >= 0) & (idx < nkb))[live].all()), "a listed entry is out of range"
    asc = (idx[..., 1:] > idx[..., :-1]) | ~live[..., 1:]
    assert bool(asc.all()), "a list is not strictly ascending"
    hits = torch.zeros(idx.shape, dtype=torch.int64)
    hits.scatter_add_(-1, idx.clamp(0, nkb - 1), live.long())             # (entries behind the count add 0 wherever they point)
    assert int(hits.max()) <= 1
    return hits > 0


# ---------------------------------------------------------------------------------------------------------------
# designed selection operands
# ---------------------------------------------------------------------------------------------------------------
SelCase = namedtuple("SelCase", "nkb top_k keep B H")
SEL_NKB = (1, 2, 4, 179, 1030, 4096)
KEEPS = ("none", "shared", "perhead")


def _sel_cases():
    out = []
    for nkb in SEL_NKB:
        B, H = (1, 2) if nkb == 4096 else (2, 2)
        for top_k in sorted({k for k in (1, 2, nkb - 1, nkb, nkb + 5) if k >= 1}):
            for keep in KEEPS:
                out.append(SelCase(nkb, top_k, keep, B, H))
    return out


SEL_CASES = _sel_cases()
SEL_IDS = [f"nkb{c.nkb}-k{c.top_k}-{c.keep}-B{c.B}" for c in SEL_CASES]


def sel_len(nkb):
    """the sequence length of a designed case: nkb tiles, the last one ragged (8 keys)"""
    return (nkb - 1) * KB + 8


@lru_cache(maxsize=None)
def sel_operands(nkb, B, H):
    """Integer-valued qbar [B, H, nqb, D], kbar [B, H, nkb, D] in -3 .. 3 (every fp32 product and partial sum is an exact integer below
    2^11) whose scores differ per sample and tie in plenty: kbar rows are drawn from a pool of nkb / 3 + 1 distinct rows, so every score
    value is shared by about three tiles of a row. From 4 tiles on, the ragged last tile's row is query block 0's own qbar: that block
    scores it highest (sum q^2) and lists it under any top_k, the other blocks see one more random row."""
    n = sel_len(nkb)
    nqb = nblocks(n)[0]
    g = torch.Generator().manual_seed(7000 + nkb)
    qbar = torch.randint(-3, 4, (B, H, nqb, D), generator=g).to(F32)
    pool = torch.randint(-3, 4, (B, H, nkb // 3 + 1, D), generator=g).to(F32)
    pick = torch.randint(0, pool.shape[2], (B, H, nkb), generator=g)
    kbar = torch.gather(pool, 2, pick[..., None].expand(-1, -1, -1, D)).contiguous()
    if nkb >= 4:
        kbar[:, :, nkb - 1] = qbar[:, :, 0]
    s = qbar.double() @ kbar.double().transpose(-1, -2)                 # [B, H, nqb, nkb]
    assert float(s.abs().max()) < 2 ** 11
    return qbar, kbar, s


@lru_cache(maxsize=None)
def sel_keep(name, nkb, H):
    """None, or bool [1 or H, nqb, nkb]: rows cycle through empty / full / partial (p = 0.3) with the query block and the head"""
    if name == "none":
        return None
    nqb = nblocks(sel_len(nkb))[0]
    heads = H if name == "perhead" else 1
    g = torch.Generator().manual_seed(7100 + nkb + heads)
    m = torch.rand(heads, nqb, nkb, generator=g) < 0.3
    kind = (torch.arange(nqb)[None, :] + 2 * torch.arange(heads)[:, None] + 2) % 3          # 0 empty, 1 full, 2 partial
    m[kind == 0] = False
    m[kind == 1] = True
    return m


@lru_cache(maxsize=None)
def sel_rank(name, nkb, B, H):
    """(rank, ncand, keep as [1 or H, nqb, nkb] bool) of a designed case's scores: shared by the top_k values of the table"""
    _, _, s = sel_operands(nkb, B, H)
    keep = sel_keep(name, nkb, H)
    kb = torch.zeros(1, *s.shape[2:], dtype=torch.bool) if keep is None else keep
    rank, ncand = ref_rank(s, kb[None])
    return rank, ncand, kb


def sel_expected(c):
    rank, ncand, kb = sel_rank(c.keep, c.nkb, c.B, c.H)
    return kb[None].expand_as(rank) | (rank < ncand.clamp(max=c.top_k)[..., None])


def _guarded(shape, dtype, fill):
    """a contiguous tensor of `shape` with PAD sentinel elements on both sides: (view, check())"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(shape)

    def check(what, untouched=False):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all()), f"{what}: a sentinel beside the buffer changed"
        if untouched:
            assert bool((buf == fill).all()), f"{what}: a rejected call wrote to its output"
    return view, check


# ---------------------------------------------------------------------------------------------------------------
# 1. pooling
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("B, n", [(1, 200), (2, 200), (1, 64), (2, 64), (1, 321)])
def test_pooling_of_small_integer_operands(B, n, strided):
    _lib = L()
    H = 2
    C = H * D
    g = torch.Generator().manual_seed(100 * n + B)
    q, k = (torch.randint(-8, 9, (B * n, C), generator=g).to(BF16) for _ in range(2))
    if strided:         # q and k as column slices of one wider buffer whose other columns would ruin every mean
        wide = torch.full((B * n, 2 * C + 24), 1000.0, dtype=BF16, device=DEV)
        wide[:, 8:8 + C], wide[:, 16 + C:16 + 2 * C] = q.to(DEV), k.to(DEV)
        qd, kd = wide[:, 8:8 + C], wide[:, 16 + C:16 + 2 * C]
        assert qd.stride(0) == 2 * C + 24 and qd.stride(0) % 8 == 0
    else:
        qd, kd = q.to(DEV), k.to(DEV)
    nqb, nkb = nblocks(n)
    qbar, qcheck = _guarded((B, H, nqb, D), F32, SENT)
    kbar, kcheck = _guarded((B, H, nkb, D), F32, SENT)
    _lib.attn_pool_qk(qd, kd, qbar, kbar, n, H, D, batch=B)
    torch.cuda.synchronize()
    qcheck("qbar"), kcheck("kbar")
    for name, got, src, blk in (("qbar", qbar, q, QB), ("kbar", kbar, k, KB)):
        want = ref_pool(src, B, n, H, blk)
        got = got.cpu()
        nb = got.shape[2]
        full = nb if n % blk == 0 else nb - 1
        assert torch.equal(got[:, :, :full].double(), want[:, :, :full]), f"{name}: a full block's mean is not exact"
        if full < nb:
            w = want[:, :, full:].numpy()
            ulp = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
            err = np.abs(got[:, :, full:].double().numpy() - w)
            print(f"{name} ragged block of {n - full * blk} rows: max error {float((err / ulp).max()):.3f} ulp")
            assert bool((err <= ulp).all()), f"{name}: the ragged block is off by {float((err / ulp).max()):.3f} ulp (bound 1)"


# ---------------------------------------------------------------------------------------------------------------
# 2. selection on designed integer operands
# ---------------------------------------------------------------------------------------------------------------
def _select(c, qbar, kbar, keep, top_k=None, n=None):
    _lib = L()
    n = sel_len(c.nkb) if n is None else n
    nqb, nkb = nblocks(n)
    idx, icheck = _guarded((c.B, c.H, nqb, nkb), I32, ISENT)
    cnt, ccheck = _guarded((c.B, c.H, nqb), I32, ISENT)
    kd = None if keep is None else keep.to(torch.uint8).to(DEV)
    _lib.attn_bs_select(qbar.to(DEV), kbar.to(DEV), kd, c.top_k if top_k is None else top_k, idx, cnt, n, c.H, batch=c.B)
    torch.cuda.synchronize()
    icheck("tile_idx"), ccheck("tile_cnt")
    return idx, cnt


@gpu
@pytest.mark.parametrize("c", SEL_CASES, ids=SEL_IDS)
def test_selection_on_designed_operands_equals_the_reference(c):
    qbar, kbar, _ = sel_operands(c.nkb, c.B, c.H)
    idx, cnt = _select(c, qbar, kbar, sel_keep(c.keep, c.nkb, c.H))
    want = sel_expected(c)
    widx, wcnt = lists_of(want)
    idx, cnt = idx.cpu(), cnt.cpu()
    assert torch.equal(cnt, wcnt), "counts differ from the reference"
    live = torch.arange(c.nkb) < wcnt[..., None]
    assert torch.equal(torch.where(live, idx, torch.full_like(idx, -1)), widx), "lists differ from the reference"
    assert bool(((idx == ISENT) | live).all()), "an entry behind the count was written"      # stronger than the contract asks: stays inside the row
    assert torch.equal(mask_of(idx, cnt), want)


@gpu
def test_selection_rejections_write_nothing():
    _lib = L()
    c = SelCase(4, 2, "none", 2, 2)
    qbar, kbar, _ = sel_operands(4, 2, 2)
    n = sel_len(4)
    nqb, nkb = nblocks(n)
    idx, icheck = _guarded((2, 2, nqb, nkb), I32, ISENT)
    cnt, ccheck = _guarded((2, 2, nqb), I32, ISENT)
    qd, kd = qbar.to(DEV), kbar.to(DEV)
    with pytest.raises(_lib.UnividHipError, match="top_k=0 must be >= 1"):
        _lib.attn_bs_select(qd, kd, None, 0, idx, cnt, n, 2, batch=2)
    with pytest.raises(_lib.UnividHipError, match="keep_heads=3 must be 1"):
        _lib.attn_bs_select(qd, kd, torch.ones(3, nqb, nkb, dtype=torch.uint8, device=DEV), 2, idx, cnt, n, 2, batch=2)
    p = _lib.ptr
    with pytest.raises(_lib.UnividHipError, match="keep_heads=0 must be 1"):
        _lib.call("uv_attn_bs_select", p(qd), p(kd), None, 0, 2, p(idx), p(cnt), 2, n, 2, _lib.stream_ptr())
    with pytest.raises(_lib.UnividHipError, match="null pointer"):
        _lib.call("uv_attn_bs_select", p(qd), None, None, 1, 2, p(idx), p(cnt), 2, n, 2, _lib.stream_ptr())
    with pytest.raises(_lib.UnividHipError, match="16-byte aligned"):
        _lib.call("uv_attn_bs_select", p(qd.flatten()[1:]), p(kd), None, 1, 2, p(idx), p(cnt), 2, n, 2, _lib.stream_ptr())
    # 4097 key tiles: one more than the row sort holds (buffers of the right size, so only the limit can refuse)
    n_big = 4096 * KB + 1
    nqb_b, nkb_b = nblocks(n_big)
    assert nkb_b == 4097
    big_idx, bcheck = _guarded((1, 1, nqb_b, nkb_b), I32, ISENT)
    big_cnt, bccheck = _guarded((1, 1, nqb_b), I32, ISENT)
    with pytest.raises(_lib.UnividHipError, match="4097 key tiles"):
        _lib.attn_bs_select(torch.zeros(1, 1, nqb_b, D, device=DEV), torch.zeros(1, 1, nkb_b, D, device=DEV), None, 2, big_idx, big_cnt, n_big, 1)
    with pytest.raises(_lib.UnividHipError, match=r"attn_bs_select\.tile_idx: "):
        _lib.attn_bs_select(qd, kd, None, 2, torch.empty(2 * 2 * nqb * nkb - 1, dtype=I32, device=DEV), cnt, n, 2, batch=2)
    torch.cuda.synchronize()
    icheck("tile_idx", True), ccheck("tile_cnt", True), bcheck("tile_idx (4097)", True), bccheck("tile_cnt (4097)", True)


@gpu
def test_pool_and_lists_rejections_write_nothing():
    _lib = L()
    n, H = 72, 2
    C = H * D
    q = torch.zeros(2 * n, C, dtype=BF16, device=DEV)
    vt = torch.zeros(C, n + 128, dtype=BF16, device=DEV)
    out = torch.full((2 * n, C), SENT, dtype=BF16, device=DEV)
    nqb, nkb = nblocks(n)
    qbar, qcheck = _guarded((2, H, nqb, D), F32, SENT)
    kbar, kcheck = _guarded((2, H, nkb, D), F32, SENT)
    p = _lib.ptr

    def pool(match, hd=D, batch=1, n=n, ldq=C, qq=q, qb=qbar):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call("uv_attn_pool_qk", p(qq), ldq, p(q), C, p(qb), p(kbar), batch, n, H, hd, _lib.stream_ptr())

    pool("head_dim 64 unsupported", hd=64)
    pool("needs L % 8", batch=2, n=68)
    pool("multiples of 8", ldq=C + 4)
    pool("cover H\\*128", ldq=C - 8)
    pool("null pointer", qb=None)
    pool("16-byte aligned", qq=q.flatten()[4:])
    pool("bad shape", n=0)
    with pytest.raises(_lib.UnividHipError, match=r"attn_pool_qk\.qbar: "):
        _lib.attn_pool_qk(q, q, torch.empty(2 * H * nqb * D - 1, device=DEV), kbar, n, H, D, batch=2)
    bm = _lib.prepare_block_mask(torch.ones(1, 2, dtype=torch.bool), n, DEV)

    def lists(match, ms=1, mh=1, batch=2, hd=D, idx=bm.tile_idx):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call("uv_flash_attn_bs_lists_bf16", p(q), C, p(q), C, p(vt), vt.stride(0), p(out), C, batch, n, H, hd, 1.0, p(idx), p(bm.tile_cnt),
                      mh, ms, _lib.stream_ptr())

    lists("mask_samples=3 must be 1", ms=3)
    lists("mask_samples=0 must be 1", ms=0)
    lists("mask_samples=2 must be 1", ms=2, batch=1)
    lists("mask_heads=3 must be 1", mh=3)
    lists("head_dim 64 unsupported", hd=64)
    lists("null pointer", idx=None)
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_bs_lists\.tile_idx: "):          # lists of one sample under mask_samples = batch
        _lib.flash_attn_bs_lists(q, q, vt, out, n, H, D, 1.0, bm.tile_idx, bm.tile_cnt, 1, 2, batch=2)
    torch.cuda.synchronize()
    qcheck("qbar", True), kcheck("kbar", True)
    assert bool((out == SENT).all()), "a rejected call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------
# 3. selection on random fp32 operands
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_selection_on_random_operands_is_within_the_dot_product_bound():
    B, H, nkb, top_k = 2, 2, 179, 20
    n = sel_len(nkb)
    nqb = nblocks(n)[0]
    g = torch.Generator().manual_seed(31)
    qbar, kbar = torch.randn(B, H, nqb, D, generator=g), torch.randn(B, H, nkb, D, generator=g)
    keep = torch.rand(1, nqb, nkb, generator=g) < 0.1
    c = SelCase(nkb, top_k, "shared", B, H)
    idx, cnt = _select(c, qbar, kbar, keep)
    sel = mask_of(idx, cnt)                                                                    # the structure, exactly
    kb = keep[None].expand_as(sel)
    assert bool((sel | ~kb).all()), "a kept tile is not listed"
    assert torch.equal(cnt.cpu().long(), (kb.sum(-1) + (~kb).sum(-1).clamp(max=top_k))), "the count is not keepcount + min(top_k, candidates)"
    s = qbar.double() @ kbar.double().transpose(-1, -2)
    e = (D + 2) * 2.0 ** -24 * (qbar.double().abs() @ kbar.double().abs().transpose(-1, -2))
    listed, unlisted = sel & ~kb, ~sel
    # per pair (t listed, u unlisted): s_t + e_t >= s_u - e_u; the worst pair of a row is min over t against max over u
    lo = (s + e).masked_fill(~listed, math.inf).amin(-1)
    hi = (s - e).masked_fill(~unlisted, -math.inf).amax(-1)
    margin = (lo - hi).min()
    print(f"smallest margin of a listed tile over an unlisted one: {float(margin):.3e} (bound 0); largest e {float(e.max()):.3e}")
    assert bool((lo >= hi).all()), f"a listed tile's score is below an unlisted one's by more than the fp32 dot-product bound ({float(margin):.3e})"


@gpu
def test_selection_of_nan_and_inf_scores_gives_valid_lists():
    B, H, nkb, top_k = 2, 2, 179, 7
    n = sel_len(nkb)
    nqb = nblocks(n)[0]
    g = torch.Generator().manual_seed(32)
    qbar, kbar = torch.randn(B, H, nqb, D, generator=g), torch.randn(B, H, nkb, D, generator=g)
    qbar[0, 0, 0] = math.nan                       # a row of NaN scores
    qbar[0, 1, 1, 5] = math.inf                    # +-inf and NaN (inf - inf) scores in one row
    kbar[1, 0, 3] = math.inf                       # one +inf / -inf / NaN column in every row of (1, 0)
    kbar[1, 1, ::2] = -math.inf
    kbar[1, 1, 7, 9] = math.nan
    keep = torch.rand(H, nqb, nkb, generator=g) < 0.05
    idx, cnt = _select(SelCase(nkb, top_k, "perhead", B, H), qbar, kbar, keep)
    sel = mask_of(idx, cnt)
    kb = keep[None].expand_as(sel)
    assert bool((sel | ~kb).all())
    assert torch.equal(cnt.cpu().long(), kb.sum(-1) + (~kb).sum(-1).clamp(max=top_k))
    idx2, cnt2 = _select(SelCase(nkb, top_k, "perhead", B, H), qbar, kbar, keep)
    assert torch.equal(mask_of(idx2, cnt2), sel), "the selection is not deterministic"
    # -0 ties with +0: a row of zero scores of both signs lists the lowest indices
    z = torch.zeros(1, 1, 1, D)                    # qbar = +0: tile 0's products 0 * -1 are all -0 (their sum is -0), tile 1's are +0
    kz = torch.zeros(1, 1, 2, D)
    kz[0, 0, 0, :] = -1.0
    i3, c3 = _select(SelCase(2, 1, "none", 1, 1), z, kz, None, n=72)
    assert i3.cpu()[0, 0, 0, :1].tolist() == [0] and int(c3.cpu()[0, 0, 0]) == 1, "-0 did not tie with +0"


# ---------------------------------------------------------------------------------------------------------------
# 4. attention under device-built lists
# ---------------------------------------------------------------------------------------------------------------
def _vt(v, B, n, C):
    vt = torch.zeros(C, L().vt_cols(B, n), dtype=BF16, device=DEV)
    vt[:, :B * n] = v.to(DEV).t()
    return vt


def split_operands(B, n, H, seed):
    """q, k, v bf16 [B*n, H*D] in which sample b's queries point along +u and its keys along +u in one half of the tiles and -u in the
    other, the halves swapped between even and odd samples (noise on top): the pooled scores are about +-D/4 and every sample's top
    tiles are the +u half - different tiles for neighbouring samples."""
    g = torch.Generator().manual_seed(seed)
    C = H * D
    nkb = nblocks(n)[1]
    q = 0.5 + 0.25 * torch.randn(B * n, C, generator=g)
    k = 0.25 * torch.randn(B * n, C, generator=g)
    tile = (torch.arange(n) // KB)
    for b in range(B):
        plus = (tile < (nkb + 1) // 2) if b % 2 == 0 else (tile >= (nkb + 1) // 2)
        k[b * n:(b + 1) * n] += torch.where(plus, 0.5, -0.5)[:, None]
    v = torch.randn(B * n, C, generator=g) + 0.25
    return q.to(BF16), k.to(BF16), v.to(BF16)


def _random(B, n, H, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B * n, H * D, generator=g).to(BF16) for _ in range(3))
    return q, k, v + 0.25


def _topk_run(q, k, v, B, n, H, top_k, keep):
    from univid_amd.wan.attention import topk_attention
    C = H * D
    out = torch.empty(B * n, C, dtype=BF16, device=DEV)
    kd = None if keep is None else (keep[None] if keep.dim() == 2 else keep).to(torch.uint8).to(DEV)
    idx, cnt = topk_attention(q.to(DEV), k.to(DEV), _vt(v, B, n, C), out, n, H, D, D ** -0.5, top_k, kd, B)
    return out, idx, cnt


def _static_run(q, k, v, n, H, mask):
    _lib = L()
    out = torch.empty(n, H * D, dtype=BF16, device=DEV)
    _lib.flash_attn_bs(q.to(DEV), k.to(DEV), _vt(v, 1, n, H * D), out, n, H, D, D ** -0.5, _lib.prepare_block_mask(mask, n, DEV))
    return out


def _assert_samples_equal_static(q, k, v, B, n, H, out, idx, cnt):
    sel = mask_of(idx, cnt)                                            # [B, H, nqb, nkb]
    for b in range(B):
        rs = slice(b * n, (b + 1) * n)
        assert torch.equal(out[rs], _static_run(q[rs], k[rs], v[rs], n, H, sel[b])), \
            f"sample {b} differs from flash_attn_bs at batch 1 under the static mask rebuilt from its list"
    return sel


@gpu
def test_attention_under_device_built_lists_samples_select_different_tiles():
    B, n, H, top_k = 2, 200, 2, 2
    q, k, v = split_operands(B, n, H, 41)
    out, idx, cnt = _topk_run(q, k, v, B, n, H, top_k, None)
    sel = _assert_samples_equal_static(q, k, v, B, n, H, out, idx, cnt)
    assert bool((cnt.cpu() == top_k).all())
    assert sel[0].all(0).all(0).tolist() == [True, True, False, False] and sel[1].all(0).all(0).tolist() == [False, False, True, True], \
        f"the designed samples did not select different tiles: {sel.tolist()}"
    # the pooled operands on the way: within fp32 summation error of the fp64 means (random bf16 rows: not exact)
    nqb, nkb = nblocks(n)
    qbar, kbar = torch.empty(B, H, nqb, D, device=DEV), torch.empty(B, H, nkb, D, device=DEV)
    L().attn_pool_qk(q.to(DEV), k.to(DEV), qbar, kbar, n, H, D, batch=B)
    assert torch.allclose(qbar.cpu().double(), ref_pool(q, B, n, H, QB), rtol=0, atol=128 * 2.0 ** -24 * 2)
    assert torch.allclose(kbar.cpu().double(), ref_pool(k, B, n, H, KB), rtol=0, atol=64 * 2.0 ** -24 * 2)


@gpu
def test_attention_under_device_built_lists_random_with_a_diagonal_keep():
    B, n, H, top_k = 2, 2104, 2, 5
    nqb, nkb = nblocks(n)
    q, k, v = _random(B, n, H, 42)
    keep = torch.arange(nkb)[None, :] // 2 == torch.arange(nqb)[:, None]
    out, idx, cnt = _topk_run(q, k, v, B, n, H, top_k, keep)
    sel = _assert_samples_equal_static(q, k, v, B, n, H, out, idx, cnt)
    assert bool((sel | ~keep).all()) and torch.equal(cnt.cpu().long(), (keep.sum(-1) + top_k).expand(B, H, nqb))
    assert not torch.equal(sel[0], sel[1]) and not torch.equal(sel[:, 0], sel[:, 1]), "random samples / heads chose the same tiles"
    assert bool(sel[..., nkb - 1].any()) and not bool(sel[..., nkb - 1].all()), "the ragged last tile should be listed by some rows only"


@gpu
@pytest.mark.parametrize("n", [200, 2104])
def test_a_covering_top_k_equals_the_dense_kernels_bit_for_bit(n):
    _lib = L()
    B, H = 2, 2
    C = H * D
    nkb = nblocks(n)[1]
    q, k, v = _random(B, n, H, 43 + n)
    dense = torch.empty(B * n, C, dtype=BF16, device=DEV)
    _lib.flash_attn(q.to(DEV), k.to(DEV), _vt(v, B, n, C), dense, n, n, H, D, D ** -0.5, batch=B)
    for top_k in (nkb, nkb + 5):
        out, idx, cnt = _topk_run(q, k, v, B, n, H, top_k, None)
        assert bool((cnt.cpu() == nkb).all()) and torch.equal(out, dense), f"top_k = {top_k} >= nkb = {nkb} differs from the dense launch"


@gpu
def test_shared_lists_through_the_new_entry_equal_the_old_entry():
    from test_attn_block_sparse import block_mask
    _lib = L()
    B, n, H = 2, 200, 2
    C = H * D
    q, k, v = _random(B, n, H, 44)
    qd, kd, vt = q.to(DEV), k.to(DEV), _vt(v, B, n, C)
    for mask in (block_mask("checker", H, n), block_mask("rand0.5", H, n)):
        bm = _lib.prepare_block_mask(mask, n, DEV)
        old, new = (torch.empty(B * n, C, dtype=BF16, device=DEV) for _ in range(2))
        _lib.flash_attn_bs(qd, kd, vt, old, n, H, D, D ** -0.5, bm, batch=B)
        _lib.flash_attn_bs_lists(qd, kd, vt, new, n, H, D, D ** -0.5, bm.tile_idx, bm.tile_cnt, bm.heads, 1, batch=B)
        assert torch.equal(new, old)
        # the same lists given once per sample
        rep = torch.empty(B * n, C, dtype=BF16, device=DEV)
        _lib.flash_attn_bs_lists(qd, kd, vt, rep, n, H, D, D ** -0.5, bm.tile_idx[None].expand(B, -1, -1, -1).contiguous(),
                                 bm.tile_cnt[None].expand(B, -1, -1).contiguous(), bm.heads, B, batch=B)
        assert torch.equal(rep, old)


# ---------------------------------------------------------------------------------------------------------------
# 5. the operator seam
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_seam_top_k_block_mask():
    from univid_amd.wan.attention import TopKBlockMask, attention, flash_attention
    B, n, N = 2, 200, 2
    nqb, nkb = nblocks(n)
    q, k, v = split_operands(B, n, N, 45)
    q4, k4, v4 = (t.view(B, n, N, D).to(DEV) for t in (q, k, v))
    keep = torch.zeros(nqb, nkb, dtype=torch.bool)
    keep[:, 0] = True                                                  # a sink tile
    for spec, kp, top_k in ((TopKBlockMask(2), None, 2), (TopKBlockMask(1, keep), keep, 1), (TopKBlockMask(0.3, keep[None].expand(N, -1, -1).clone()), keep, 2)):
        want, idx, cnt = _topk_run(q, k, v, B, n, N, top_k, kp)
        _assert_samples_equal_static(q, k, v, B, n, N, want, idx, cnt)
        got = flash_attention(q4, k4, v4, block_mask=spec)
        assert got.dtype == BF16 and tuple(got.shape) == (B, n, N, D) and torch.equal(got.view(B * n, N * D), want), repr(spec)
        assert torch.equal(attention(q4, k4, v4, k_lens=torch.tensor([n] * B), block_mask=spec), got)
    got = flash_attention(q4, k4, v4, block_mask=TopKBlockMask(2))
    wide = flash_attention(q4.float(), k4.float(), v4.float(), block_mask=TopKBlockMask(2))       # fp32 in: cast, fp32 out on the bf16 grid
    assert wide.dtype == F32 and torch.equal(wide, got.float())
    dense = flash_attention(q4, k4, v4)
    assert torch.equal(flash_attention(q4, k4, v4, block_mask=TopKBlockMask(1.0)), dense) and not torch.equal(got, dense)
    # one sample at an L that is no multiple of 8, and two of them (one launch per sample)
    odd = flash_attention(q4[:, :197].contiguous(), k4[:, :197].contiguous(), v4[:, :197].contiguous(), block_mask=TopKBlockMask(2))
    one = flash_attention(q4[1:, :197].contiguous(), k4[1:, :197].contiguous(), v4[1:, :197].contiguous(), block_mask=TopKBlockMask(2))
    assert torch.equal(odd[1:], one) and torch.isfinite(odd.float()).all()
    for match, args in (("fp16", (q4.half(), k4.half(), v4.half(), {})),
                        ("head size 64", (q4[..., :64].contiguous(), k4[..., :64].contiguous(), v4[..., :64].contiguous(), {})),
                        ("Lq != Lk", (q4[:, :100].contiguous(), k4, v4, {})),
                        ("ragged k_lens", (q4, k4, v4, dict(k_lens=torch.tensor([n, 77])))),
                        ("causal / window_size", (q4, k4, v4, dict(causal=True))),
                        ("causal / window_size", (q4, k4, v4, dict(window_size=(8, 8))))):
        a, b, c, kw = args
        with pytest.raises(NotImplementedError, match=match):
            flash_attention(a, b, c, block_mask=TopKBlockMask(2), dtype=torch.float16 if a.dtype == torch.float16 else BF16, **kw)
    with pytest.raises(TypeError, match="keep is a callable needs a patch grid"):
        flash_attention(q4, k4, v4, block_mask=TopKBlockMask(2, lambda F, H, W, nh: keep))
    with pytest.raises(ValueError, match="does not belong to L = 200"):
        flash_attention(q4, k4, v4, block_mask=TopKBlockMask(2, torch.ones(3, 5, dtype=torch.bool)))
    with pytest.raises(ValueError, match="keep has 3 heads"):
        flash_attention(q4, k4, v4, block_mask=TopKBlockMask(2, torch.ones(3, nqb, nkb, dtype=torch.bool)))


# ---------------------------------------------------------------------------------------------------------------
# 6. the small model
# ---------------------------------------------------------------------------------------------------------------
def _small_model(seed=0, **over):
    """The tiny golden model has head_dim 64: dim 256 with 2 heads instead, weights from detinit (as tests/test_attn_block_sparse.py)."""
    from test_gpu_parity import _tiny_model
    return _tiny_model(seed, num_heads=2, **over)


def sink_keep(F, H, W, num_heads):
    """the callable keep of the small-model tests: the first key tile (a sink), for every query block"""
    sink_keep.calls.append((F, H, W, num_heads))
    nqb, nkb = nblocks(F * H * W)
    m = torch.zeros(nqb, nkb, dtype=torch.bool)
    m[:, 0] = True
    return m


sink_keep.calls = []


@gpu
def test_small_model_covering_top_k_is_dense_and_small_top_k_is_not():
    from univid_amd.wan.attention import TopKBlockMask
    from univid_amd.wan.model import AttnTopKMask
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    Lt = 256                                                           # grid (4, 8, 8): 2 query blocks, 4 key tiles
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        for spec in (TopKBlockMask(4), TopKBlockMask(9), TopKBlockMask(1.0), TopKBlockMask(3, sink_keep)):
            gen = m._prep_gen
            m.set_attn_block_mask(spec)
            assert m._prep_gen > gen and isinstance(m.attn_block_mask, AttnTopKMask) and m.attn_block_mask.spec is spec
            assert all(b.self_attn.attn_block_mask is m.attn_block_mask and b.cross_attn.attn_block_mask is None for b in m.blocks)
            assert torch.equal(m([x], t, [ctx], Lt)[0], base), f"{spec!r} covers every tile and must equal the dense forward"
        sink_keep.calls.clear()
        m.set_attn_block_mask(TopKBlockMask(1, sink_keep))
        got = m([x], t, [ctx], Lt)[0]
        assert not torch.equal(got, base) and torch.isfinite(got).all()
        assert torch.equal(m([x], t, [ctx], Lt)[0], got) and sink_keep.calls == [(4, 8, 8, 2)], "the keep callable runs once per grid"
        ctx2 = (ctx * 0.5).contiguous()
        x2 = x.flip(1).contiguous()
        other = m([x2], t, [ctx2], Lt)[0]
        pair = m([x, x2], torch.cat([t, t]), [ctx, ctx2], Lt)
        assert torch.equal(pair[0], got) and torch.equal(pair[1], other), "the stacked pair differs from single forwards (per-sample lists)"
        m.set_ffn_precision("mxfp8")                                   # independent of the spec: the two combine
        both = m([x], t, [ctx], Lt)[0]
        assert not torch.equal(both, got) and torch.isfinite(both).all()
        m.set_ffn_precision("bf16")
        one = m([x[:, :2].contiguous()], t[:, :128].contiguous(), [ctx], 128)[0]      # another grid resolves beside the first
        assert sink_keep.calls == [(4, 8, 8, 2), (2, 8, 8, 2)] and torch.isfinite(one).all()
        m.set_attn_block_mask(None)
        assert m.attn_block_mask is None and torch.equal(m([x], t, [ctx], Lt)[0], base)


@gpu
def test_small_model_denoise_graph_replays_two_latents_through_one_capture():
    """The lists are rebuilt by the captured kernels in every replay: two different latents through ONE capture equal their eager runs bit
    for bit (lists frozen at capture time would reproduce the first latent's tiles for the second), and the tiles they select differ."""
    from univid_amd.wan import model as wm
    from univid_amd.wan.attention import TopKBlockMask
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (2, g["shift"], g["guide_scale"])
    cfg, sd, m = _small_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV, attn_block_mask=TopKBlockMask(1, sink_keep))
    noise_a = g["noise"].to(DEV)
    noise_b = torch.randn(noise_a.shape, generator=torch.Generator().manual_seed(5)).to(noise_a.dtype).to(DEV) * 2

    def gen(noise, graph):
        with torch.no_grad():
            return pipe.denoise(noise, [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    def lists_now():
        return [t.clone() for k, (t, _) in wm._zero_cache.items() if k[0] == "topk_idx"]

    eager_a = gen(noise_a, False)
    la = lists_now()
    eager_b = gen(noise_b, False)
    lb = lists_now()
    assert len(la) == 1 and len(lb) == 1 and la[0].shape[0] == 2, "the CFG pair runs as one stacked forward with per-sample lists"
    assert not torch.equal(la[0][..., :2], lb[0][..., :2]), "the two latents select the same tiles: the replay check would show nothing"
    graph_a = gen(noise_a, True)
    runner = pipe._runner
    assert runner is not None
    graph_b = gen(noise_b, True)
    assert pipe._runner is runner and len(pipe._runners) == 1, "the second latent was not replayed through the first capture"
    assert torch.equal(graph_a, eager_a), "graph != eager under a TopKBlockMask"
    assert torch.equal(graph_b, eager_b), "the second latent through the same capture differs from eager: lists frozen at capture time?"
    assert torch.equal(gen(noise_a, True), eager_a) and not torch.equal(eager_a, eager_b)
    pipe._runner = None


@gpu
def test_unmerged_lora_works_with_top_k(tmp_path):
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    from univid_amd.wan.attention import TopKBlockMask
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    m.set_attn_block_mask(TopKBlockMask(1, sink_keep))
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    attn = [f"blocks.{i}.self_attn.{p}" for i in range(cfg["num_layers"]) for p in ("q", "k", "v")]
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, attn, 8, 6, b_std=0.2), 8, 16)
    mgr = LoRAManager()
    with torch.no_grad():
        base = m([x], t, [ctx], 256)[0]
        mgr.load_lora_weights(str(tmp_path / "A"), m, merge=False, name="A")
        with_a = m([x], t, [ctx], 256)[0]
        assert not torch.equal(with_a, base) and torch.isfinite(with_a).all()
        mgr.unload("A")
        assert torch.equal(m([x], t, [ctx], 256)[0], base), "unload does not restore the bits"
