"""Block-sparse self-attention from a key-tile mask: uv_flash_attn_bs_bf16 (flash_attn_bs4_kernel), the operator seam under `block_mask=`,
and WanModel.set_attn_block_mask - called through `_lib.flash_attn_bs` and compared with an fp64 softmax of the same operands under the
EXPANDED boolean mask: query i of head h attends key j iff mask[h][i // 128][j // 64] (and j < L).

The kernel part is driven by ONE table (CASES). Every row asserts `attn_bs_plan(...)` - kernel name, query blocks, grid - before it launches
(-m gpu); the operand builders' own conditions are asserted for every row without a GPU (tests/test_attn_block_sparse_host.py).

Operand families (tests/test_attn_window.py's, restated, with the block mask applied in the fp64 reference):
  A        softmax_scale = float32(ln 2): scale * log2(e) is exactly 1 in f32 (asserted), k dense +-1, q rows four +-1 whose columns rotate with
           the row, v integers in -2 .. 2: every P is a power of two and every partial sum of P v and of P is exact in f32 in ANY order (span
           max sum_j 2^(s_ij - min s) |v_jd| < 2^24 over the VISIBLE keys, asserted). Gate: bit-identical to the fp64 softmax rounded to bf16,
           except the elements whose fp64 value lies within relative 2^-18 of a rounding boundary; at most 0.5 % of a case's elements may be
           excepted (a condition of the operands: a seed that misses it is replaced, the cap is never raised).
  spike10  scores in {0, 1} and one key 10 above them for two queries of three, in a tile that SOME query blocks visit and others do not: the
  spike6   rescale branch (10 > UV_ATT_DEFER) / P up to 2^7 without a move (6), after skipped tiles.
  A mask that leaves ONE key (last-only at L = 65 and 321: the ragged tile holds key L - 1 alone): the result must EQUAL that v row as a bit
  pattern (checked against v itself).
Poison INSIDE the sample (family A): every key row of a tile that NO query block of that head visits holds +-64 patterns (rows in pairs, the
second the negative of the first): such a row wins the softmax of any query that wrongly sees it.
Around every launch, as in tests/test_attn_window.py: 8 slack rows (and slack columns where ldo > C) filled with SENT that must come back
unchanged, 8 poison rows behind q and k, 1000 in the V^T columns behind the last sample, poison around column slices."""
import contextlib
import json
import math
import time
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import bf16_ulp, load_golden, record_margin

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
DEV = "cuda"
D = 128
QB, KB = 128, 64
SENT = -7.25
KNAME = "flash_attn_bs4_kernel"


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


def _up(x, m):
    return (x + m - 1) // m * m


def nblocks(n):
    return (n + QB - 1) // QB, (n + KB - 1) // KB


# ---------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------
def block_mask(name, H, n):
    """The table's masks by name -> bool [nqb, nkb] (shared by the heads) or [H, nqb, nkb] (the random ones: per head). No row is empty."""
    nqb, nkb = nblocks(n)
    qb, kb = torch.arange(nqb)[:, None], torch.arange(nkb)[None, :]
    if name == "ones":
        return torch.ones(nqb, nkb, dtype=torch.bool)
    if name == "first":
        return (kb == 0).expand(nqb, nkb).clone()
    if name == "last":
        return (kb == nkb - 1).expand(nqb, nkb).clone()
    if name == "first+last":
        return ((kb == 0) | (kb == nkb - 1)).expand(nqb, nkb).clone()
    if name == "diag":                      # a query block's own keys
        return kb // 2 == qb
    if name == "anti":                      # the keys of the mirrored query block
        return kb // 2 == nqb - 1 - qb
    if name == "checker":
        return (qb + kb) % 2 == 0
    if name.startswith("rand"):             # "rand0.5": per head, each tile with that probability, an empty row gets one tile
        p = float(name[4:])
        g = torch.Generator().manual_seed(3000 + int(p * 1000) + 31 * n + H)
        m = torch.rand(H, nqb, nkb, generator=g) < p
        pick = torch.randint(0, nkb, (H, nqb), generator=g)
        empty = ~m.any(-1)
        m[empty, pick[empty]] = True
        return m
    raise KeyError(name)


def expand_mask(m, H, n):
    """[nqb, nkb] or [H, nqb, nkb] -> [H, n, n] bool: query i (row) of head h sees key j (column)"""
    m = m[None].expand(H, -1, -1) if m.dim() == 2 else m
    return m.repeat_interleave(QB, 1)[:, :n].repeat_interleave(KB, 2)[:, :, :n]


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
# mask: a name of block_mask; fam: operand family; ld: "dense", "slice" (q and k column slices of one [rows, 3 C + 16] buffer),
# "vt+64" / "vt+8" (ldvt wider than required), "ldo+8" (the store through LDS into a wider row) / "ldo+4" (the direct store)
Case = namedtuple("Case", "B H L mask fam ld")
CASES = []


def _c(n, mask, B=1, H=2, fam="A", ld="dense"):
    c = Case(B, H, n, mask, fam, ld)
    if c not in CASES:
        CASES.append(c)


_c(1, "ones")
for _m in ("ones", "first", "last"):        # last: ONE key (64) - the ragged tile alone
    _c(65, _m)
for _m in ("diag", "anti", "last", "checker"):
    _c(200, _m)
for _m in ("last", "first+last"):           # last: ONE key (320)
    _c(321, _m)
_c(200, "checker", B=2)
_c(200, "anti", B=3)                        # V^T columns of samples 1, 2 start off a tile boundary
_c(640, "rand0.5", H=3)                     # per head; odd and even counts (asserted by the host test)
_c(640, "checker")
_c(2504, "rand0.3", B=2, H=4)               # eight (sample, head)s: the XCD-contiguous id order
_c(2504, "diag")
for _ld in ("slice", "vt+64", "vt+8", "ldo+8", "ldo+4"):
    _c(200, "checker", B=2, ld=_ld)
for _fam in ("spike10", "spike6"):          # spike key 64 + (L - 64) 2 // 3 = 235 (tile 3) / 448 (tile 7): the odd query blocks visit it
    _c(321, "checker", fam=_fam)
    _c(640, "checker", fam=_fam)


def _id(i, c):
    return f"{i:03d}-{c.fam}-B{c.B}H{c.H}-L{c.L}-{c.mask}" + ("" if c.ld == "dense" else "-" + c.ld)


IDS = [_id(i, c) for i, c in enumerate(CASES)]


def _layout(c):
    C = c.H * D
    ldq = ldk = ldo = C
    ldvt = (c.B - 1) * c.L + _up(c.L, 64)
    if c.ld == "slice":
        ldq = ldk = 3 * C + 16
    elif c.ld in ("vt+64", "vt+8"):
        ldvt += int(c.ld[3:])
    elif c.ld in ("ldo+8", "ldo+4"):
        ldo += int(c.ld[4:])
    return ldq, ldk, ldvt, ldo


def expected_plan(B, H, n):
    """plan_attn_bs, restated: one 4-wave workgroup per (sample, head, 128-query block), whatever the mask"""
    return dict(kernel=KNAME, q_blocks=nblocks(n)[0], grid=nblocks(n)[0] * H * B)


def assert_plan(c):
    plan = L().attn_bs_plan(c.L, D, c.B, c.H)
    assert plan == expected_plan(c.B, c.H, c.L), f"planned {plan}, the row expects {expected_plan(c.B, c.H, c.L)}"
    return plan


# ---------------------------------------------------------------------------------------------------------------
# operands and references (CPU; shared by the rows that differ in the layout only)
# ---------------------------------------------------------------------------------------------------------------
Ops = namedtuple("Ops", "q k v scale ref near strict stats poison mask")


def _near_boundary(x, rel):
    """fp64 x -> which elements lie within rel |x| of a bf16 rounding boundary (the midpoint of two neighbours), ties included"""
    bits, emin = 8, -126
    m, e = torch.frexp(x.abs())
    e = e.clamp_min(emin + 1)
    scaled = torch.ldexp(x.abs(), bits - e)
    frac = scaled - scaled.floor()
    return (frac - 0.5).abs() <= rel * scaled


def _rint(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def unvisited_tiles(m, H):
    """per head: the key tiles no query block of that head visits"""
    m = m[None].expand(H, -1, -1) if m.dim() == 2 else m
    return [(~m[h].any(0)).nonzero().flatten().tolist() for h in range(H)]


class _OtherSeed(Exception):
    """the operands of this seed miss a condition that depends on the seed alone: the next one is tried"""


@lru_cache(maxsize=None)
def _operands(fam, B, H, n, mask):
    base = 7919 * n + 5 * B + H + 104729 * sum(map(ord, mask)) + {"A": 0, "spike10": 1, "spike6": 2}[fam]
    why = []
    for attempt in range(64):
        g = torch.Generator().manual_seed(base + 15485863 * attempt)
        try:
            return _integer_exponents(g, fam, B, H, n, mask)
        except _OtherSeed as ex:
            why.append(str(ex))
    raise AssertionError(f"no seed holds the conditions: {why[-1]}")


def _integer_exponents(g, fam, B, H, n, mask_name):
    C = H * D
    rq = torch.arange(B * n) % n
    scale = np.float32(math.log(2.0))
    sl2 = float(np.float32(scale) * np.float32(1.4426950408889634))       # the f32 product the entry point hands to the kernel
    assert sl2 == 1.0, "scale * log2(e) is not exactly 2^0 in f32"
    bmask = block_mask(mask_name, H, n)
    emask = expand_mask(bmask, H, n)
    assert bool(emask.any(-1).all()), "a query without a visible key: no empty rows"
    q = torch.zeros(B * n, C, dtype=F64)
    poison = None
    js = 64 + (n - 64) * 2 // 3
    if fam == "A":
        k = _rint(g, (B * n, C), 0, 1) * 2 - 1
        v = _rint(g, (B * n, C), -2, 2)
        for h in range(H):
            for j in range(4):
                q[torch.arange(B * n), h * D + (rq + 7 * h + D // 4 * j) % D] = _rint(g, (B * n,), 0, 1) * 2 - 1
        poison = unvisited_tiles(bmask, H)
        for h, tiles in enumerate(poison):
            for t in tiles:
                lo, hi = t * KB, min(n, (t + 1) * KB)
                assert not bool(emask[h][:, lo:hi].any()), "a query sees a poisoned key"
                for b in range(B):
                    pat = _rint(g, (hi - lo, D), 0, 1) * 128 - 64
                    pat[1::2] = -pat[0:(hi - lo) - (hi - lo) % 2:2]
                    k[b * n + lo:b * n + hi, h * D:(h + 1) * D] = pat
    else:
        gap = 10.0 if fam == "spike10" else 6.0
        assert 64 <= js < n, "the spike belongs into the second or a later tile"
        k = _rint(g, (B * n, C), 0, 1)
        v = _rint(g, (B * n, C), -1, 1)
        for h in range(H):
            k[:, h * D + D - 1] = 0
            k[torch.arange(B) * n + js, h * D + D - 1] = gap
            q[torch.arange(B * n), h * D + (rq + 5 * h) % (D - 1)] = 1
            q[:, h * D + D - 1] = (rq % 3 != 0).double()          # two queries of three see the spike - where their block visits its tile
        for h in range(H):
            inside = emask[h][:, js]
            blocks = bmask if bmask.dim() == 2 else bmask[h]
            assert bool(blocks[:, js // KB].any()) and not bool(blocks[:, js // KB].all()), "the spike's tile must be visited by some query blocks only"
            assert bool(blocks[blocks[:, js // KB]][:, :js // KB].logical_not().any()), "no tile is skipped in front of the spike"
            assert bool((inside & (torch.arange(n) % 3 != 0)).any()) and bool((inside & (torch.arange(n) % 3 == 0)).any())
    ref = torch.empty(B * n, C, dtype=F64)
    strict = torch.empty(B * n, C, dtype=BF16)
    span = 0.0
    for b in range(B):
        for h in range(H):
            rs, cs = slice(b * n, (b + 1) * n), slice(h * D, (h + 1) * D)
            mask = emask[h]
            S = q[rs, cs] @ k[rs, cs].t()                        # exact integers
            X = (S * sl2).masked_fill(~mask, -math.inf)
            P = torch.exp2(X - X.max(-1, keepdim=True).values)
            ref[rs, cs] = (P @ v[rs, cs]) / P.sum(-1, keepdim=True)
            smin = S.masked_fill(~mask, math.inf).min()
            E = torch.exp2(S - smin).masked_fill(~mask, 0.0)     # every visible P in units of the smallest one: exact powers of two
            span = max(span, float((E @ v[rs, cs].abs()).max()), float(E.sum(-1).max()))
            if fam != "A":
                vis = S.masked_fill(~mask, -math.inf)
                rest = torch.cat((vis[:, :js], vis[:, js + 1:]), 1)
                sees = (q[rs, h * D + D - 1] == 1) & mask[:, js]
                fin = torch.isfinite(rest)
                assert float(rest[fin].max()) == 1 and float(rest[fin].min()) == 0
                assert bool((vis[sees, js] - rest.max(-1).values[sees] >= gap - 1).all()) and bool((vis[sees, js] >= gap).all())
                assert bool((vis[~sees, js] <= 1).all())
            O, l = P @ v[rs, cs], P.sum(-1)
            assert torch.equal(O.float().double(), O) and torch.equal(l.float().double(), l)
            strict[rs, cs] = (O.float() * (1.0 / l.float())[:, None]).to(BF16)
    assert span < 2 ** 24, f"span 2^{math.log2(span):.2f}: a partial sum could round in fp32"
    near = _near_boundary(ref, 2.0 ** -18)
    share = float(near.double().mean())
    if share > 0.005:
        raise _OtherSeed(f"{share:.4%} of the elements lie at a rounding boundary (at most 0.5 % may be excepted)")
    for t in (q, k, v):
        assert torch.equal(t.to(BF16).double(), t)
    if mask_name == "last" and n % KB == 1:
        assert torch.equal(ref, v.view(B, n, C)[:, n - 1:].expand(B, n, C).reshape(B * n, C)), "one visible key: the reference is its v row"
    return Ops(q.to(BF16), k.to(BF16), v.to(BF16), float(scale), ref.to(BF16), near, strict,
               dict(excluded_share=share, span_log2=math.log2(max(span, 1.0)), density=float(expand_mask(bmask, H, n).double().mean())), poison, bmask)


def ops_of(c):
    return _operands(c.fam, c.B, c.H, c.L, c.mask)


# ---------------------------------------------------------------------------------------------------------------
# the launch: operands in the row's memory layout, poison around them, sentinels around the output
# ---------------------------------------------------------------------------------------------------------------
def _poison(rows, cols, g):
    p = (torch.randint(0, 2, (rows, cols), generator=g, device=DEV) * 128 - 64).to(BF16)
    p[1::2] = -p[0:rows - rows % 2:2]
    return p


def _launch(c, o):
    """One flash_attn_bs call of the row -> the dense result [B L, C] on the CPU; the sentinels are asserted here."""
    _lib = L()
    C, rows = c.H * D, c.B * c.L
    ldq, ldk, ldvt, ldo = _layout(c)
    g = torch.Generator(device=DEV).manual_seed(CASES.index(c))
    if c.ld == "slice":
        buf = _poison(rows + 8, ldq, g)
        q, k = buf[:rows, :C], buf[:rows, C + 8:2 * C + 8]
        q.copy_(o.q.to(DEV))
        k.copy_(o.k.to(DEV))
    else:
        qb, kb = _poison(rows + 8, C, g), _poison(rows + 8, C, g)
        qb[:rows] = o.q.to(DEV)
        kb[:rows] = o.k.to(DEV)
        q, k = qb[:rows], kb[:rows]
    vt = torch.full((C, ldvt), 1000.0, dtype=BF16, device=DEV)
    vt[:, :rows] = o.v.to(DEV).t()
    full = torch.full((rows + 8, ldo), SENT, dtype=BF16, device=DEV)
    out = full[:rows, :C]
    assert (q.stride(0), k.stride(0), vt.stride(0), out.stride(0)) == (ldq, ldk, ldvt, ldo)
    bm = _lib.prepare_block_mask(o.mask, c.L, DEV)
    _lib.flash_attn_bs(q, k, vt, out, c.L, c.H, D, o.scale, bm, batch=c.B)
    torch.cuda.synchronize()
    host = full.cpu()
    stray = int((host != SENT).sum()) - int((host[:rows, :C] != SENT).sum())
    assert stray == 0, f"{stray} elements outside the [{rows}, {C}] result were written (buffer {tuple(host.shape)})"
    assert not bool((host[:rows, :C] == SENT).any()), "part of the result was not written"
    return host[:rows, :C].contiguous()


def _where(c, i, j):
    return (f"(row {i} = sample {i // c.L} query {i % c.L}: block {i % c.L // QB} unit {i % c.L // 32} lane {i % 32}; column {j} = head {j // D} "
            f"d {j % D})")


def _compare(o, got):
    diff = (got.view(torch.int16) != o.ref.view(torch.int16)) & ~((got == 0) & (o.ref == 0))
    strict = (got.view(torch.int16) != o.strict.view(torch.int16)) & ~((got == 0) & (o.strict == 0))
    return diff & ~o.near, int((diff & o.near).sum()), int(strict.sum())


@gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_block_sparse_kernel_is_bit_exact_on_designed_operands(c):
    """The planned kernel (asserted), launched once on the row's designed operands: bit-identical to the masked fp64 softmax rounded to bf16
    outside the excepted elements (at most 0.5 %: asserted by the builder); a mask of ONE key EQUAL to that v row as a bit pattern; sentinels
    and poison as the file's docstring says."""
    plan = assert_plan(c)
    o = ops_of(c)
    got = _launch(c, o)
    bad, in_band, strict = _compare(o, got)
    name = IDS[CASES.index(c)]
    print(f"{name}: {plan}; {o.stats}; poisoned tiles per head {o.poison}; mismatches in the excepted band {in_band}, against the strict prediction {strict}")
    record_margin(f"attn_block_sparse/{name}", kernel=plan["kernel"], band_mismatches=in_band, strict_mismatches=strict, **o.stats)
    if c.mask == "last" and c.L % KB == 1:
        want = o.v.view(c.B, c.L, -1)[:, c.L - 1:].expand(c.B, c.L, c.H * D).reshape(c.B * c.L, c.H * D)
        same = (got.view(torch.int16) == want.contiguous().view(torch.int16)) | ((got == 0) & (want == 0))
        assert bool(same.all()), f"{name}: one visible key must return its v row itself; {int((~same).sum())} elements differ"
    if bad.any():
        i, j = (int(x) for x in bad.nonzero()[0])
        rows = sorted({int(x) for x in bad.nonzero()[:, 0]})
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the reference, in {len(rows)} rows (first rows {rows[:8]}); "
                             f"first at {_where(c, i, j)}: got {got[i, j].item()!r}, expected {o.ref[i, j].item()!r}")


# ---------------------------------------------------------------------------------------------------------------
# random operands: the dense kernels' bits, independence of the launch, the fp64 truth
# ---------------------------------------------------------------------------------------------------------------
def _random(B, n, H, seed):
    g = torch.Generator().manual_seed(seed)
    C = H * D
    q, k, v = (torch.randn(B * n, C, generator=g).to(BF16) for _ in range(3))
    v += 0.25
    return q, k, v


def _vt(v, B, n, C):
    vt = torch.zeros(C, L().vt_cols(B, n), dtype=BF16, device=DEV)
    vt[:, :B * n] = v.to(DEV).t()
    return vt


def _run(q, k, v, B, n, H, mask, dense=False):
    _lib = L()
    C = H * D
    vt = _vt(v, B, n, C)
    out = torch.empty(B * n, C, dtype=BF16, device=DEV)
    if dense:
        _lib.flash_attn(q.to(DEV), k.to(DEV), vt, out, n, n, H, D, D ** -0.5, batch=B)
    else:
        _lib.flash_attn_bs(q.to(DEV), k.to(DEV), vt, out, n, H, D, D ** -0.5, _lib.prepare_block_mask(mask, n, DEV), batch=B)
    return out


@gpu
@pytest.mark.parametrize("n", [200, 2104])
def test_all_ones_mask_equals_the_dense_kernels_bit_for_bit(n):
    """The all-ones mask - shared and per head - is torch.equal to flash_attn on random operands (fwd3 at L = 200, fwd12 at 2104)."""
    B, H = 2, 2
    q, k, v = _random(B, n, H, 5 + n)
    dense = _run(q, k, v, B, n, H, None, dense=True)
    assert L().attn_bs_plan(n, D, B, H) == expected_plan(B, H, n)
    assert L().attn_plan(n, n, D, B, H)["kernel"] == ("flash_attn_fwd12_kernel" if n >= 2048 else "flash_attn_fwd3_kernel")
    for mask in (block_mask("ones", H, n), block_mask("ones", H, n)[None].expand(H, -1, -1).clone()):
        assert torch.equal(_run(q, k, v, B, n, H, mask), dense), f"the all-ones mask {tuple(mask.shape)} at L = {n} differs from the dense launch"


@gpu
def test_a_block_equals_the_dense_kernel_on_its_gathered_keys():
    """L = 640, a random per-head mask: for every (head, query block), flash_attn on the block's 128 query rows and on K / V GATHERED to the
    block's visited tiles, in order (Lq = 128, Lk = 64 cnt < 2048), returns the block-sparse launch's bits for those rows."""
    _lib = L()
    n, H = 640, 2
    q, k, v = _random(1, n, H, 640)
    mask = block_mask("rand0.5", H, n)
    got = _run(q, k, v, 1, n, H, mask)
    counts = set()
    for h in range(H):
        cs = slice(h * D, (h + 1) * D)
        for qb in range(nblocks(n)[0]):
            tiles = mask[h, qb].nonzero().flatten().tolist()
            counts.add(len(tiles))
            keys = torch.cat([torch.arange(t * KB, min(n, (t + 1) * KB)) for t in tiles])
            Lk = len(keys)
            assert Lk == KB * (len(tiles) - 1) + (min(n, (tiles[-1] + 1) * KB) - tiles[-1] * KB) and Lk < 2048
            qs = q[qb * QB:(qb + 1) * QB, cs].contiguous().to(DEV)
            kg, vg = k[keys][:, cs].contiguous().to(DEV), v[keys][:, cs].contiguous()
            one = torch.empty(qs.shape[0], D, dtype=BF16, device=DEV)
            _lib.flash_attn(qs, kg, _vt(vg, 1, Lk, D), one, qs.shape[0], Lk, 1, D, D ** -0.5)
            assert torch.equal(one, got[qb * QB:(qb + 1) * QB, cs]), f"head {h} block {qb} (tiles {tiles}) differs from the dense kernel on its gathered keys"
    assert len(counts) > 1


@gpu
def test_a_blocks_bits_do_not_depend_on_the_launch():
    """L = 640, random operands, a random per-head mask: a query block's rows do not change when the OTHER blocks' lists change, in a stacked
    B = 2 launch, or when a shared mask is given once per head."""
    n, H = 640, 2
    q, k, v = _random(2, n, H, 99)
    mask = block_mask("rand0.5", H, n)
    both = _run(q, k, v, 2, n, H, mask)
    for b in range(2):
        one = _run(q[b * n:(b + 1) * n], k[b * n:(b + 1) * n], v[b * n:(b + 1) * n], 1, n, H, mask)
        assert torch.equal(one, both[b * n:(b + 1) * n]), f"sample {b} of the stacked launch differs from its own launch"
    other = block_mask("checker", H, n)[None].expand(H, -1, -1).clone()
    keep = 2
    other[:, keep] = mask[:, keep]                      # every block's list changes but block 2's
    assert not torch.equal(other, mask)
    alt = _run(q, k, v, 2, n, H, other)
    for b in range(2):
        rows = slice(b * n + keep * QB, b * n + (keep + 1) * QB)
        assert torch.equal(alt[rows], both[rows]), "block 2's rows changed with the other blocks' lists"
    assert not torch.equal(alt, both)
    shared = block_mask("checker", H, n)
    assert torch.equal(_run(q, k, v, 2, n, H, shared), _run(q, k, v, 2, n, H, shared[None].expand(H, -1, -1).clone())), "shared != the same mask per head"


def _masked_truth(q, k, v, B, n, H, emask):
    o = torch.empty(B * n, H * D, dtype=F64)
    for b in range(B):
        for h in range(H):
            rs, cs = slice(b * n, (b + 1) * n), slice(h * D, (h + 1) * D)
            s = (q[rs, cs].double() @ k[rs, cs].double().t() / math.sqrt(D)).masked_fill(~emask[h], -math.inf)
            o[rs, cs] = torch.softmax(s, -1) @ v[rs, cs].double()
    return o


def _sdpa_bf16(q, k, v, B, n, H, emask):
    """bf16 CPU SDPA with the same boolean mask (the oracle's attention_core plus the mask)"""
    import torch.nn.functional as F
    q4, k4, v4 = (t.view(B, n, H, D).transpose(1, 2) for t in (q, k, v))
    return F.scaled_dot_product_attention(q4, k4, v4, attn_mask=emask[None]).transpose(1, 2).reshape(B * n, H * D)


def _seam_gate(got, truth, ref, name):
    """tests/test_attn_window.py's (tests/test_gpu_parity.py's "flash_attention seam") gate"""
    e_hip, e_ora = (got.double().cpu() - truth).abs(), (ref.double() - truth).abs()
    tol = 3 * bf16_ulp(truth.float()) + 2e-3 * truth.abs().float().max()
    m = dict(max_err=float(e_hip.max()), max_err_over_tol=float((e_hip / tol).max()), rms_hip=float(e_hip.pow(2).mean().sqrt()),
             rms_sdpa=float(e_ora.pow(2).mean().sqrt()))
    record_margin("attn_block_sparse random: " + name, **m)
    print("attn_block_sparse random: " + name, json.dumps(m))
    assert (e_hip <= tol).all(), f"{name}: max err {float(e_hip.max()):.3e}"
    assert m["rms_hip"] <= 1.5 * m["rms_sdpa"] + 1e-5, name


@gpu
@pytest.mark.parametrize("B, n, mask", [(2, 200, "checker"), (1, 321, "first+last"), (1, 321, "rand0.5"), (2, 2504, "rand0.3"), (1, 2104, "anti")])
def test_random_operands_against_fp64(B, n, mask):
    H = 2
    q, k, v = _random(B, n, H, 1000 + n + len(mask))
    emask = expand_mask(block_mask(mask, H, n), H, n)
    got = _run(q, k, v, B, n, H, block_mask(mask, H, n))
    _seam_gate(got, _masked_truth(q, k, v, B, n, H, emask), _sdpa_bf16(q, k, v, B, n, H, emask), f"B{B} L{n} mask {mask}")


@gpu
def test_rejections_write_nothing():
    """head_dim 64, mask_heads that is neither 1 nor H, a V^T too narrow for the batch, batch 2 with L % 8 != 0 and a null list: each returns
    non-zero from the C entry point (UnividHipError) before any launch and leaves a sentinel-filled output untouched; the plan entry and the
    wrapper refuse their own."""
    _lib = L()
    n, H = 72, 2
    C = H * D
    qbuf = torch.zeros(2 * n + 8, C, dtype=BF16, device=DEV)
    kbuf = torch.zeros(2 * n + 8, C, dtype=BF16, device=DEV)
    vbuf = torch.zeros(C, n + 128 + 64, dtype=BF16, device=DEV)
    full = torch.full((2 * n + 8, C), SENT, dtype=BF16, device=DEV)
    bm = _lib.prepare_block_mask(torch.ones(1, 2, dtype=torch.bool), n, DEV)
    p = _lib.ptr

    def raw(match, ldvt=vbuf.stride(0), batch=1, n=n, H=H, hd=D, mh=1, idx=bm.tile_idx):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call("uv_flash_attn_bs_bf16", p(qbuf), C, p(kbuf), C, p(vbuf), ldvt, p(full), C, batch, n, H, hd, D ** -0.5, p(idx), p(bm.tile_cnt),
                      mh, _lib.stream_ptr())

    raw("head_dim 64 unsupported", H=4, hd=64)
    raw("mask_heads=3 must be 1", mh=3)
    raw("mask_heads=0 must be 1", mh=0)
    raw("must cover", ldvt=128, batch=2)
    raw("needs L % 8", batch=2, n=68)
    raw("null pointer", idx=None)
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_bs_plan: head_dim 64"):
        _lib.attn_bs_plan(n, 64, 1, 2)
    # the wrapper's own checks (dtype, extent, the mask's L / heads / device) refuse before the C entry point
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_bs\.q: "):
        _lib.flash_attn_bs(qbuf[:n].view(torch.float16), kbuf[:n], vbuf[:, :128], full[:n], n, H, D, 1.0, bm)
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_bs\.vt: "):
        _lib.flash_attn_bs(qbuf[:2 * n], kbuf[:2 * n], torch.zeros(C, 128, dtype=BF16, device=DEV), full[:2 * n], n, H, D, 1.0, bm, batch=2)
    with pytest.raises(_lib.UnividHipError, match=r"prepared for L = 72, the launch has L = 64"):
        _lib.flash_attn_bs(qbuf[:64], kbuf[:64], vbuf[:, :64], full[:64], 64, H, D, 1.0, bm)
    with pytest.raises(_lib.UnividHipError, match=r"the mask has 3 heads, the launch 2"):
        _lib.flash_attn_bs(qbuf[:n], kbuf[:n], vbuf[:, :128], full[:n], n, H, D, 1.0, _lib.prepare_block_mask(torch.ones(3, 1, 2, dtype=torch.bool), n, DEV))
    with pytest.raises(_lib.UnividHipError, match=r"the mask lives on cpu"):
        _lib.flash_attn_bs(qbuf[:n], kbuf[:n], vbuf[:, :128], full[:n], n, H, D, 1.0, _lib.prepare_block_mask(torch.ones(1, 2, dtype=torch.bool), n, "cpu"))
    with pytest.raises(_lib.UnividHipError, match=r"a PreparedBlockMask is required"):
        _lib.flash_attn_bs(qbuf[:n], kbuf[:n], vbuf[:, :128], full[:n], n, H, D, 1.0, torch.ones(1, 2, dtype=torch.bool))
    torch.cuda.synchronize()
    assert bool((full == SENT).all()), "a rejected call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------
# the operator seam
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_seam_block_mask():
    """flash_attention(q, k, v, block_mask=) at B = 2, Lq = Lk = 200 from fp32 inputs (fp32 out on the bf16 grid) and from bf16 inputs, a bool
    tensor and a PreparedBlockMask, shared and per head: the seam test's gate; what is not built raises naming the limit."""
    from univid_amd.wan.attention import attention, flash_attention
    B, n, N = 2, 200, 2
    g = torch.Generator().manual_seed(78)
    q, k, v = (torch.randn(B, n, N, D, generator=g) for _ in range(3))
    v += 0.25
    qb, kb, vb = (t.to(BF16).reshape(B * n, N * D) for t in (q, k, v))
    for mask in (block_mask("checker", N, n), block_mask("rand0.5", N, n)):
        emask = expand_mask(mask, N, n)
        out = flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), block_mask=mask)
        assert out.dtype == F32 and tuple(out.shape) == (B, n, N, D) and torch.equal(out, out.to(BF16).float())
        _seam_gate(out.reshape(B * n, N * D), _masked_truth(qb, kb, vb, B, n, N, emask), _sdpa_bf16(qb, kb, vb, B, n, N, emask), f"seam {tuple(mask.shape)}")
        half = flash_attention(q.to(BF16).to(DEV), k.to(BF16).to(DEV), v.to(BF16).to(DEV), block_mask=L().prepare_block_mask(mask, n, DEV))
        assert half.dtype == BF16 and torch.equal(half.float(), out)
        assert torch.equal(attention(q.to(DEV), k.to(DEV), v.to(DEV), k_lens=torch.tensor([n] * B), block_mask=mask), out)
    assert not torch.equal(out, flash_attention(q.to(DEV), k.to(DEV), v.to(DEV)))
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    mask = block_mask("checker", N, n)
    for match, args in (("fp16", (dq.half(), dk.half(), dv.half(), {})),
                        ("head size 64", (dq[..., :64].contiguous(), dk[..., :64].contiguous(), dv[..., :64].contiguous(), {})),
                        ("Lq != Lk", (dq[:, :100].contiguous(), dk, dv, {})),
                        ("ragged k_lens", (dq, dk, dv, dict(k_lens=torch.tensor([n, 77])))),
                        ("causal / window_size", (dq, dk, dv, dict(causal=True))),
                        ("causal / window_size", (dq, dk, dv, dict(window_size=(8, 8))))):
        a, b, c, kw = args
        with pytest.raises(NotImplementedError, match=match):
            flash_attention(a, b, c, block_mask=mask, dtype=torch.float16 if a.dtype == torch.float16 else BF16, **kw)
    with pytest.raises(TypeError, match="block_mask must be"):
        flash_attention(dq, dk, dv, block_mask=mask.float())
    with pytest.raises(ValueError, match="does not belong to L = 200"):
        flash_attention(dq, dk, dv, block_mask=torch.ones(3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="prepared for L = 136"):
        flash_attention(dq, dk, dv, block_mask=L().prepare_block_mask(torch.ones(2, 3, dtype=torch.bool), 136, DEV))


# ---------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def masked_oracle(emask):
    """The oracle with attention_core - for the self-attention call, the one that passes k_lens - replaced by the same function plus the
    expanded boolean mask [H, L, L] (SDPA in wan_dit.BF16 operands with an attn_mask)."""
    import torch.nn.functional as F
    from oracle import wan_dit
    orig = wan_dit.attention_core

    def core(q, k, v, k_lens=None):
        if k_lens is None:
            return orig(q, k, v)
        assert q.size(1) == k.size(1) and int(k_lens.min()) == k.size(1), "the mask is defined on unpadded self-attention"
        dt = q.dtype
        q, k, v = (t.to(wan_dit.BF16).transpose(1, 2) for t in (q, k, v))
        return F.scaled_dot_product_attention(q, k, v, attn_mask=emask[None]).transpose(1, 2).contiguous().type(dt)

    wan_dit.attention_core = core
    try:
        yield
    finally:
        wan_dit.attention_core = orig


def _rms(a, b):
    return (a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt().item()


@gpu
def test_block_ti2v5b_width_video_mask():
    """One TI2V-5B-width block (3072, 24 heads of 128) on 576 tokens = grid (4, 12, 12) under video_block_mask(frames +-1, rows +-3): HIP
    against the oracle with the expanded mask and its fp32 truth (both on the CPU): rms(hip - truth) <= 1.02 rms(masked oracle - truth). The
    masked output differs from the dense block's, and set_attn_block_mask(None) brings back the dense bits exactly."""
    from oracle import wan_dit
    from univid_amd import detinit
    from univid_amd.wan.attention import video_block_mask
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device
    g = load_golden("dit_block_3072")
    heads, grid, Lt = 24, (4, 12, 12), 576
    mask = video_block_mask(grid, frames=(1, 1), rows=3, cols=-1)
    assert tuple(mask.shape) == nblocks(Lt) and 0.3 < float(mask.double().mean()) < 0.9 and bool(mask.any(-1).all())
    with torch.device(DEV):
        blk = WanAttentionBlock(3072, 14336, heads, (-1, -1), True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, g["seed"])
    blk, sdc = blk.eval(), {k: v.detach().cpu() for k, v in sd.items()}
    x = detinit.uniform_pm1("attn_block_sparse.block.x", Lt * 3072, g["seed"]).reshape(1, Lt, 3072).float() * 2
    tid = (torch.arange(Lt) * 7 // Lt % 2).to(g["tid"].dtype)
    e_rows, ctx = g["e_rows"], g["ctx"]
    fr = _freqs_device(wan_dit.rope_table(D), torch.device(DEV))
    assert L().attn_bs_plan(Lt, D, 1, heads) == expected_plan(1, heads, Lt)

    def run(b):
        xx = x[0].to(DEV).clone()
        with torch.no_grad():
            b._run(xx, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), grid, fr, ctx[0].to(DEV), first_block=False)
        return xx

    base = run(blk)
    blk.set_attn_block_mask(mask)
    got = run(blk)
    assert torch.isfinite(got).all() and torch.equal(run(blk), got) and not torch.equal(got, base), "the masked block equals the dense one"
    blk.set_attn_block_mask(None)
    assert blk.self_attn.attn_block_mask is None and torch.equal(run(blk), base)
    blk.set_attn_block_mask(lambda F, H, W, nh: video_block_mask((F, H, W), frames=(1, 1), rows=3, cols=-1, num_heads=nh))
    assert torch.equal(run(blk), got), "the callable spec (per head, the same mask) must equal the tensor spec"
    args = (sdc, "blocks.0.", x, e_rows[tid].unsqueeze(0), torch.tensor([Lt]), torch.tensor([grid]), wan_dit.rope_table(D))
    t0 = time.time()
    with torch.no_grad(), masked_oracle(expand_mask(mask, 1, Lt)):
        ora = wan_dit.block_forward(*args, ctx, heads, 1e-6)[0]
        old, wan_dit.BF16 = wan_dit.BF16, torch.float32
        try:
            truth = wan_dit.block_forward(*args, ctx.float(), heads, 1e-6)[0]
        finally:
            wan_dit.BF16 = old
    e_hip, e_ora = _rms(got, truth), _rms(ora, truth)
    m = dict(truth_ratio=e_hip / e_ora, rms_vs_truth_hip=e_hip, rms_vs_truth_masked_oracle=e_ora, rms_masked_vs_dense_hip=_rms(got, base),
             density=float(mask.double().mean()), oracle_host_seconds=time.time() - t0)
    record_margin("attn_block_sparse block 3072 L576 video mask", **m)
    print("attn_block_sparse block 3072 L576 video mask", json.dumps(m))
    assert e_hip <= 1.02 * e_ora, f"rms vs truth {e_hip:.4e}, the masked oracle's {e_ora:.4e}"


def _small_model(seed=0, **over):
    """The tiny golden model has head_dim 64: dim 256 with 2 heads instead, weights from detinit."""
    from test_gpu_parity import _tiny_model
    return _tiny_model(seed, num_heads=2, **over)


def frame_mask(F, H, W, num_heads):
    """the callable spec of the small-model tests: every token sees its own frame (grid (4, 8, 8): 64 tokens a frame = one key tile)"""
    from univid_amd.wan.attention import video_block_mask
    frame_mask.calls.append((F, H, W, num_heads))
    return video_block_mask((F, H, W), frames=(0, 0))


frame_mask.calls = []


@gpu
def test_small_model_cfg_pair_setter_and_callable_cache():
    from univid_amd.wan.attention import video_block_mask
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    Lt = 256
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    fixed = video_block_mask((4, 8, 8), frames=(0, 0))
    assert fixed.tolist() == [[True, True, False, False], [False, False, True, True]]
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        gen = m._prep_gen
        m.set_attn_block_mask(fixed)
        assert m._prep_gen > gen and all(b.self_attn.attn_block_mask is m.attn_block_mask and b.cross_attn.attn_block_mask is None for b in m.blocks)
        got = m([x], t, [ctx], Lt)[0]
        ctx2 = (ctx * 0.5).contiguous()
        other = m([x], t, [ctx2], Lt)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], Lt)
        assert torch.equal(pair[0], got) and torch.equal(pair[1], other) and not torch.equal(got, other), "the stacked CFG pair differs from single forwards"
        assert not torch.equal(got, base) and torch.isfinite(got).all()
        with pytest.raises(ValueError, match="does not belong to L = 64"):      # a fixed mask at another L: one frame
            m([x[:, :1].contiguous()], t[:, :64].contiguous(), [ctx], 64)
        m.set_ffn_precision("mxfp8")                                       # independent of the mask: the two combine
        both = m([x], t, [ctx], Lt)[0]
        assert not torch.equal(both, got) and torch.isfinite(both).all()
        m.set_ffn_precision("bf16")
        assert torch.equal(m([x], t, [ctx], Lt)[0], got)
        # a PreparedBlockMask and a callable give the same bits; the callable is evaluated once per grid
        m.set_attn_block_mask(L().prepare_block_mask(fixed, Lt, DEV))
        assert torch.equal(m([x], t, [ctx], Lt)[0], got)
        frame_mask.calls.clear()
        m.set_attn_block_mask(frame_mask)
        assert torch.equal(m([x], t, [ctx], Lt)[0], got) and torch.equal(m([x], t, [ctx], Lt)[0], got)
        assert frame_mask.calls == [(4, 8, 8, 2)], f"the callable ran {frame_mask.calls}: once per distinct grid is expected"
        one = m([x[:, :2].contiguous()], t[:, :128].contiguous(), [ctx], 128)[0]      # another grid: evaluated once more, cached beside the first
        assert frame_mask.calls == [(4, 8, 8, 2), (2, 8, 8, 2)] and torch.isfinite(one).all()
        m([x], t, [ctx], Lt)
        assert len(frame_mask.calls) == 2
        m.set_attn_block_mask(None)
        assert m.attn_block_mask is None and torch.equal(m([x], t, [ctx], Lt)[0], base), "global attention after a round trip must equal the model before"


@gpu
def test_small_model_denoise_graph_and_recapture():
    from univid_amd.wan.attention import video_block_mask
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (2, g["shift"], g["guide_scale"])

    def pipe_in(spec):
        cfg, sd, m = _small_model(g["seed"])
        return WanTI2V(TI2VConfig, model=m, device=DEV, attn_block_mask=spec)

    def gen(pipe, graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    fresh_m, fresh_d = pipe_in(frame_mask), pipe_in(None)
    assert all(b.self_attn.attn_block_mask is fresh_m.model.attn_block_mask for b in fresh_m.model.blocks) and fresh_d.model.attn_block_mask is None
    m_graph = gen(fresh_m, True)
    assert fresh_m._runner is not None
    assert torch.equal(m_graph, gen(fresh_m, False)), "graph != eager with a block mask"
    d_graph = gen(fresh_d, True)
    assert not torch.equal(d_graph, m_graph)
    fresh_d.model.set_attn_block_mask(video_block_mask((4, 8, 8), frames=(0, 0)))
    assert torch.equal(gen(fresh_d, True), m_graph), "after the switch the pipeline does not equal a fresh masked pipeline (no re-capture?)"
    fresh_d.model.set_attn_block_mask(video_block_mask((4, 8, 8), frames=(0, 1)))
    other = gen(fresh_d, True)
    assert not torch.equal(other, m_graph) and not torch.equal(other, d_graph), "another mask replays the old capture"
    fresh_d.model.set_attn_block_mask(None)
    assert torch.equal(gen(fresh_d, True), d_graph), "after the switch back the pipeline does not equal a fresh dense pipeline"
    fresh_m._runner = fresh_d._runner = None


@gpu
def test_a_capture_with_an_unprepared_grid_raises():
    """The callable's mask is built on the CPU and uploaded: inside a capture that cannot happen, so a grid that no eager forward prepared
    raises instead of building the mask there; after AttnBlockMask.prepare the same capture goes through."""
    from univid_amd.wan.model import AttnBlockMask
    r = AttnBlockMask(frame_mask, 2)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    buf = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            buf.add_(1)
            with pytest.raises(RuntimeError, match="was not prepared before this HIP-graph capture"):
                r.resolve((4, 8, 8), 256, torch.device(DEV, 0))
    bm = r.prepare((4, 8, 8), torch.device(DEV, 0))
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph2, stream=side):
            buf.add_(1)
            assert r.resolve((4, 8, 8), 256, torch.device(DEV, 0)) is bm
    torch.cuda.synchronize()


@gpu
def test_unmerged_lora_works_with_a_mask(tmp_path):
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    m.set_attn_block_mask(frame_mask)
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
