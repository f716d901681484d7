"""Sliding-window / causal self-attention: uv_flash_attn_win_bf16 with its two kernels (flash_attn_win12_kernel when the keys one workgroup
streams, min(L, 384 + left + right), are at least 2048; flash_attn_win4_kernel below), the operator seam under `causal` / `window_size`, and
WanModel.set_attn_window - called through `_lib.flash_attn_win` and compared with an fp64 softmax of the same operands under the same
boolean mask: query i of a sample attends key j iff max(0, i - left) <= j <= min(L - 1, i + right), -1 = unbounded.

The kernel part is driven by ONE table (CASES). Every row asserts `attn_win_plan(...)` - the kernel name, and for the 12-wave form the
query-block cut and the grid under the row's OPT_ATTN_CUT - before it launches (-m gpu); the operand builders' own conditions are asserted
for every row without a GPU (tests/test_attn_window_host.py).

Operand families (tests/test_attn_kernels.py's, restated, with the window mask applied in the fp64 reference):
  A        softmax_scale = float32(ln 2): scale * log2(e) is exactly 1 in f32 (asserted), k dense +-1, q rows four +-1 whose columns rotate with
           the row, v integers in -2 .. 2: every P is a power of two and every partial sum of P v and of P is exact in f32 in ANY order (span
           max sum_j 2^(s_ij - min s) |v_jd| < 2^24 over the VISIBLE keys, asserted). Gate: bit-identical to the fp64 softmax rounded to bf16,
           except the elements whose fp64 value lies within relative 2^-18 of a rounding boundary; at most 0.5 % of a case's elements may be
           excepted (a condition of the operands: a seed that misses it is replaced, the cap is never raised).
  spike10  scores in {0, 1} and one key 10 above them for two queries of three, under a window that contains the spike for some queries
  spike6   and not for others: the rescale branch (10 > UV_ATT_DEFER) / P up to 2^7 without a move (6), after skipped and masked tiles.
  Family A under window (0, 0): the result must EQUAL v[i] as a bit pattern (checked against v itself).
Poison INSIDE the sample: a key row j holding +-64 patterns wins the softmax of every query that wrongly sees it. Key j is legitimately
visible to the queries j - right .. j + left, so the rows with a bounded window replace a pair of adjacent key rows (the second the negative
of the first) where those queries are few (at most a quarter of the sample) and give THOSE queries an all-zero q row (score 0 with every key,
the poison included: uniform attention over their window, still exact) - every other query of the sample must not see the pair.
Around every launch, as in tests/test_attn_kernels.py: 8 slack rows (and slack columns where ldo > C) filled with SENT that must come back
unchanged, 8 poison rows behind q and k, 1000 in the V^T columns behind the last sample, poison around column slices."""
import contextlib
import json
import math
import os
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
SENT = -7.25
KNAME = {"win12": "flash_attn_win12_kernel", "win4": "flash_attn_win4_kernel"}


@pytest.fixture(scope="module")
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


@pytest.fixture(autouse=True)
def _default_options():
    from univid_amd import _lib
    _lib.reset_options()
    yield
    _lib.reset_options()


def gpu(f):
    return pytest.mark.gpu(pytest.mark.usefixtures("_init")(f))


def L():
    from univid_amd import _lib
    return _lib


def _up(x, m):
    return (x + m - 1) // m * m


def window_mask(n, win):
    """[n, n] bool: query i (row) sees key j (column) - flash-attn's window_size for Lq == Lk, -1 = unbounded"""
    left, right = win
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    m = torch.ones(n, n, dtype=torch.bool)
    if left >= 0:
        m &= j >= i - left
    if right >= 0:
        m &= j <= i + right
    return m


def span_of(n, win):
    """keys one 12-wave workgroup streams at most (plan_attn_win's measure): min(L, 384 + left + right), an unbounded side counted as L"""
    return min(n, 384 + (n if win[0] < 0 else win[0]) + (n if win[1] < 0 else win[1]))


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
# win: (left, right); fam: operand family; cut: OPT_ATTN_CUT; ld: "dense", "slice" (q and k column slices of one [rows, 3 C + 16] buffer),
# "vt+64" / "vt+8" (ldvt wider than required), "ldo+8" (the store through LDS into a wider row) / "ldo+4" (the direct store)
Case = namedtuple("Case", "B H L win fam cut ld")
CASES = []


def _c(n, win, B=1, H=2, fam="A", cut=0, ld="dense"):
    c = Case(B, H, n, tuple(win), fam, cut, ld)
    if c not in CASES:
        CASES.append(c)


# ---- the 4-wave form: one query, windows of one key, edges one key into / short of the next tile, the hazard row (left = 100: a wave's last
# query sees nothing of the first tile its first query needs), causal at a ragged length, a window wider than the sample, stacked samples
# whose V^T columns start off a tile boundary
for _n, _w in ((1, (0, 0)), (33, (1, 0)), (65, (0, 1)), (150, (31, 0)), (200, (32, 32)), (200, (63, 64)), (321, (100, -1)), (321, (-1, 0)),
               (321, (100, 0)), (321, (400, 400)), (2504, (70, 5)), (2504, (100, 0)), (200, (0, 0)), (321, (64, 63)), (321, (63, 64)),
               (321, (-1, -1)), (321, (0, -1))):
    _c(_n, _w)
for _n in (64, 128):                    # window edges exactly on tile edges
    _c(_n, (63, 0))
    _c(_n, (0, 63))
_c(200, (5, 70), B=2)
_c(200, (64, 63), B=3)
_c(2104, (1663, 0))                     # span 2047: the last one of the 4-wave form
# ---- the 12-wave form: every kind of cut (66 units per head) with 8 (sample, head)s - the XCD-aware order - and with 3 - the plain one
for _w in ((-1, -1), (-1, 0)):
    for _cut in (0, 1, 2, 3):
        _c(2104, _w, B=2, H=4, cut=_cut)
        _c(2104, _w, H=3, cut=_cut)
# forced cuts whose last eight-unit block lies behind the head's last unit (66 units; cut 3: 5 x 12 + 2 x 8, cut 9: 1 x 12 + 8 x 8 - the last block starts at unit 68)
# under a bounded left: the empty block's window would start behind the sample - it must leave without a fetch
for _w in ((0, 2047), (32, -1), (64, 1700)):
    _c(2104, _w, cut=3)
    _c(2104, _w, B=2, H=4, cut=9)
_c(2104, (1664, 0))                     # span 2048: the first one of the 12-wave form
_c(2104, (2047, 0))
_c(2104, (0, 2047), B=2)
_c(2104, (0, 2047), B=3, H=1)
_c(2504, (1100, 1100), B=2, H=4)
_c(2504, (-1, 0))
_c(2504, (100, -1))                     # the hazard row on the 12-wave form
# ---- leading dimensions, one row per layout and form
for _ld in ("slice", "vt+64", "vt+8", "ldo+8", "ldo+4"):
    _c(200, (32, 32), B=2, ld=_ld)
    _c(2104, (2047, 0), B=2, ld=_ld)
# ---- the late spike (key 64 + (L - 64) 2 // 3) under a window that holds it for some queries only
for _fam in ("spike10", "spike6"):
    _c(200, (40, 30), fam=_fam)         # spike at 154: queries 124 .. 194 see it
    _c(321, (100, 60), fam=_fam)        # spike at 235: queries 175 .. 320
    _c(2504, (1000, 700), fam=_fam)     # spike at 1690, span 2084: the 12-wave form; queries 990 .. 2503


def kern_of(c):
    return "win12" if span_of(c.L, c.win) >= 2048 else "win4"


def _id(i, c):
    return (f"{i:03d}-{kern_of(c)}-{c.fam}-B{c.B}H{c.H}-L{c.L}-w{c.win[0]}_{c.win[1]}" + (f"-cut{c.cut}" if kern_of(c) == "win12" else "")
            + ("" if c.ld == "dense" else "-" + c.ld)).replace("-1", "inf")


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


# ---------------------------------------------------------------------------------------------------------------
# the plan every row expects (plan_attn_win, restated from its comment)
# ---------------------------------------------------------------------------------------------------------------
def _auto_cut(nwu, nbh, ncus):
    """plan_attn's automatic cut: a 12-unit workgroup takes time 1, an 8-unit one 0.76, each kind is dealt in id order to the least loaded of
    ncus CUs (12-unit blocks first); the cut with the smallest makespan wins, ties go to fewer 8-unit blocks."""
    best, cut = 1e30, ((nwu + 11) // 12, 0)
    n8 = 0
    while n8 * 8 < nwu + 8:
        n12 = (nwu - 8 * n8 + 11) // 12 if nwu > 8 * n8 else 0
        if n12 == 0 and n8 * 8 - nwu >= 8:
            break
        load = np.zeros(min(ncus, 1024))
        for count, t in ((n12 * nbh, 1.0), (n8 * nbh, 0.76)):
            for _ in range(count):
                load[int(np.argmin(load))] += t
        if load.max() < best - 1e-9:
            best, cut = float(load.max()), (n12, n8)
        n8 += 1
    return cut


def expected_plan(c, ncus):
    nbh = c.H * c.B
    if kern_of(c) == "win4":
        qb = (c.L + 127) // 128
        return dict(kernel=KNAME["win4"], q_blocks=qb, n12=0, grid=qb * nbh)
    nwu = (c.L + 31) // 32
    if c.cut > 0:
        n8 = c.cut - 1
        n12 = (nwu - 8 * n8 + 11) // 12 if nwu > 8 * n8 else 0
    else:
        n12, n8 = _auto_cut(nwu, nbh, ncus)
    return dict(kernel=KNAME["win12"], q_blocks=n12 + n8, n12=n12, grid=(n12 + n8) * nbh)


def assert_plan(c, ncus):
    """Under the row's OPT_ATTN_CUT (left set for the launch; the autouse fixture resets it)."""
    _lib = L()
    _lib.set_option(_lib.OPT_ATTN_CUT, c.cut)
    plan = _lib.attn_win_plan(c.L, D, c.B, c.H, c.win)
    want = expected_plan(c, ncus)
    assert plan == want, f"planned {plan}, the row expects {want}"
    if kern_of(c) == "win12":       # the cut and the grid are the dense plan's for the same (L, batch, H)
        dense = _lib.attn_plan(c.L, c.L, D, c.B, c.H)
        assert (plan["q_blocks"], plan["n12"], plan["grid"]) == (dense["q_blocks"], dense["n12"], dense["grid"])
    return plan


# ---------------------------------------------------------------------------------------------------------------
# operands and references (CPU; shared by the rows that differ in the cut or the layout only)
# ---------------------------------------------------------------------------------------------------------------
Ops = namedtuple("Ops", "q k v scale ref near strict stats poison")


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


def poison_rows(n, win):
    """-> (j, queries) or None: the pair of key rows (j, j + 1) to poison and the queries that legitimately see one of them (their q rows are
    zeroed), where those are at most a quarter of the sample; only for windows bounded on both sides that leave some query outside."""
    left, right = win
    if left < 0 or right < 0 or n < 16:
        return None
    best = None
    for j in (0, n // 2, n - 2):
        lo, hi = max(0, j - right), min(n - 1, j + 1 + left)
        if best is None or hi - lo < best[1][1] - best[1][0]:
            best = (j, (lo, hi))
    j, (lo, hi) = best
    if hi - lo + 1 > n // 4:
        return None
    return j, (lo, hi)


class _OtherSeed(Exception):
    """the operands of this seed miss a condition that depends on the seed alone: the next one is tried"""


@lru_cache(maxsize=None)
def _operands(fam, B, H, n, win):
    base = 7919 * n + 5 * B + H + 104729 * (win[0] + 2) + 1299709 * (win[1] + 2) + {"A": 0, "spike10": 1, "spike6": 2}[fam]
    why = []
    for attempt in range(64):
        g = torch.Generator().manual_seed(base + 15485863 * attempt)
        try:
            return _integer_exponents(g, fam, B, H, n, win)
        except _OtherSeed as ex:
            why.append(str(ex))
    raise AssertionError(f"no seed holds the conditions: {why[-1]}")


def _integer_exponents(g, fam, B, H, n, win):
    C = H * D
    rq = torch.arange(B * n) % n
    scale = np.float32(math.log(2.0))
    sl2 = float(np.float32(scale) * np.float32(1.4426950408889634))       # the f32 product the entry point hands to the kernels
    assert sl2 == 1.0, "scale * log2(e) is not exactly 2^0 in f32"
    mask = window_mask(n, win)
    assert bool(mask.diagonal().all()), "every query sees its own key: no empty rows"
    q = torch.zeros(B * n, C, dtype=F64)
    poison = None
    js = 64 + (n - 64) * 2 // 3
    if fam == "A":
        k = _rint(g, (B * n, C), 0, 1) * 2 - 1
        v = _rint(g, (B * n, C), -2, 2)
        for h in range(H):
            for j in range(4):
                q[torch.arange(B * n), h * D + (rq + 7 * h + D // 4 * j) % D] = _rint(g, (B * n,), 0, 1) * 2 - 1
        poison = poison_rows(n, win)
        if poison is not None:
            j, (lo, hi) = poison
            assert not bool(mask[:lo, j:j + 2].any()) and not bool(mask[hi + 1:, j:j + 2].any()), "a query outside the zeroed range sees the poison"
            assert lo > 0 or hi < n - 1
            pat = _rint(g, (B, C), 0, 1) * 128 - 64
            for b in range(B):
                k[b * n + j], k[b * n + j + 1] = pat[b], -pat[b]
                q[b * n + lo:b * n + hi + 1] = 0
    else:
        gap = 10.0 if fam == "spike10" else 6.0
        assert 64 <= js < n, "the spike belongs into the second or a later tile"
        k = _rint(g, (B * n, C), 0, 1)
        v = _rint(g, (B * n, C), -1, 1)
        for h in range(H):
            k[:, h * D + D - 1] = 0
            k[torch.arange(B) * n + js, h * D + D - 1] = gap
            q[torch.arange(B * n), h * D + (rq + 5 * h) % (D - 1)] = 1
            q[:, h * D + D - 1] = (rq % 3 != 0).double()          # two queries of three see the spike - where their window holds it
        inside = mask[:, js]
        assert bool(inside.any()) and bool((~inside).any()), "the window must hold the spike for some queries and not for others"
        assert bool((inside & (torch.arange(n) % 3 != 0)).any()) and bool((inside & (torch.arange(n) % 3 == 0)).any())
    ref = torch.empty(B * n, C, dtype=F64)
    strict = torch.empty(B * n, C, dtype=BF16)
    span = 0.0
    for b in range(B):
        for h in range(H):
            rs, cs = slice(b * n, (b + 1) * n), slice(h * D, (h + 1) * D)
            S = q[rs, cs] @ k[rs, cs].t()                        # exact integers
            if poison is not None:      # the poison keys' scores: 0 for the zeroed queries, hidden from all others
                assert float(S[:, poison[0]:poison[0] + 2][mask[:, poison[0]:poison[0] + 2]].abs().max()) == 0
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
            E = torch.exp2(X - X.max(-1, keepdim=True).values)
            O, l = E @ v[rs, cs], E.sum(-1)
            assert torch.equal(O.float().double(), O) and torch.equal(l.float().double(), l)
            strict[rs, cs] = (O.float() * (1.0 / l.float())[:, None]).to(BF16)
    assert span < 2 ** 24, f"span 2^{math.log2(span):.2f}: a partial sum could round in fp32"
    near = _near_boundary(ref, 2.0 ** -18)
    share = float(near.double().mean())
    if share > 0.005:
        raise _OtherSeed(f"{share:.4%} of the elements lie at a rounding boundary (at most 0.5 % may be excepted)")
    for t in (q, k, v):
        assert torch.equal(t.to(BF16).double(), t)
    if win == (0, 0):
        assert torch.equal(ref, v), "window (0, 0): the reference is v itself"
    return Ops(q.to(BF16), k.to(BF16), v.to(BF16), float(scale), ref.to(BF16), near, strict, dict(excluded_share=share, span_log2=math.log2(max(span, 1.0))),
               poison)


def ops_of(c):
    return _operands(c.fam, c.B, c.H, c.L, c.win)


# ---------------------------------------------------------------------------------------------------------------
# the launch: operands in the row's memory layout, poison around them, sentinels around the output
# ---------------------------------------------------------------------------------------------------------------
def _poison(rows, cols, g):
    p = (torch.randint(0, 2, (rows, cols), generator=g, device=DEV) * 128 - 64).to(BF16)
    p[1::2] = -p[0:rows - rows % 2:2]
    return p


def _launch(c, o):
    """One flash_attn_win call of the row -> the dense result [B L, C] on the CPU; the sentinels are asserted here."""
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
    _lib.flash_attn_win(q, k, vt, out, c.L, c.H, D, o.scale, c.win, batch=c.B)
    torch.cuda.synchronize()
    host = full.cpu()
    stray = int((host != SENT).sum()) - int((host[:rows, :C] != SENT).sum())
    assert stray == 0, f"{stray} elements outside the [{rows}, {C}] result were written (buffer {tuple(host.shape)})"
    assert not bool((host[:rows, :C] == SENT).any()), "part of the result was not written"
    return host[:rows, :C].contiguous()


def _where(c, i, j):
    return f"(row {i} = sample {i // c.L} query {i % c.L}: unit {i % c.L // 32} lane {i % 32}; column {j} = head {j // D} d {j % D})"


def _compare(o, got):
    diff = (got.view(torch.int16) != o.ref.view(torch.int16)) & ~((got == 0) & (o.ref == 0))
    strict = (got.view(torch.int16) != o.strict.view(torch.int16)) & ~((got == 0) & (o.strict == 0))
    return diff & ~o.near, int((diff & o.near).sum()), int(strict.sum())


@gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_window_kernel_is_bit_exact_on_designed_operands(c):
    """The planned kernel (asserted), launched once on the row's designed operands: bit-identical to the masked fp64 softmax rounded to bf16
    outside the excepted elements (at most 0.5 %: asserted by the builder); window (0, 0) EQUAL to v as a bit pattern; sentinels and
    poison as the file's docstring says."""
    ncus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = assert_plan(c, ncus)
    o = ops_of(c)
    got = _launch(c, o)
    bad, in_band, strict = _compare(o, got)
    name = IDS[CASES.index(c)]
    print(f"{name}: {plan}; {o.stats}; poison {o.poison}; mismatches in the excepted band {in_band}, against the strict prediction {strict}")
    record_margin(f"attn_window/{name}", kernel=plan["kernel"], band_mismatches=in_band, strict_mismatches=strict, **o.stats)
    if c.win == (0, 0):
        same = (got.view(torch.int16) == o.v.view(torch.int16)) | ((got == 0) & (o.v == 0))
        assert bool(same.all()), f"{name}: window (0, 0) must return v itself; {int((~same).sum())} elements differ"
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


def _run(q, k, v, B, n, H, win, dense=False):
    _lib = L()
    C = H * D
    vt = torch.zeros(C, _lib.vt_cols(B, n), dtype=BF16, device=DEV)
    vt[:, :B * n] = v.to(DEV).t()
    out = torch.empty(B * n, C, dtype=BF16, device=DEV)
    if dense:
        _lib.flash_attn(q.to(DEV), k.to(DEV), vt, out, n, n, H, D, D ** -0.5, batch=B)
    else:
        _lib.flash_attn_win(q.to(DEV), k.to(DEV), vt, out, n, H, D, D ** -0.5, win, batch=B)
    return out


@gpu
@pytest.mark.parametrize("n, kern", [(200, "win4"), (2104, "win12")])
def test_full_window_equals_the_dense_kernels_bit_for_bit(n, kern):
    """A window that covers every key - (-1, -1) and (L - 1, L - 1) - through the win entry is torch.equal to flash_attn on random operands."""
    B, H = 2, 2
    q, k, v = _random(B, n, H, 5 + n)
    dense = _run(q, k, v, B, n, H, None, dense=True)
    for win in ((-1, -1), (n - 1, n - 1)):
        assert L().attn_win_plan(n, D, B, H, win)["kernel"] == KNAME[kern]
        assert torch.equal(_run(q, k, v, B, n, H, win), dense), f"window {win} at L = {n} differs from the dense launch"


@gpu
def test_a_querys_bits_do_not_depend_on_the_launch():
    """L = 2504, random operands, window (300, 200) - the 4-wave form - and (1000, 700) - span 2084, the 12-wave form, where OPT_ATTN_CUT
    acts: cuts 0-3 give equal outputs and a stacked B = 2 launch equals the two single launches. The two forms agree as well: each window
    forced onto the other form (OPT_ATTN_WIN_FORM) gives the same bits."""
    _lib = L()
    n, H = 2504, 2
    q, k, v = _random(2, n, H, 99)
    for win, kern in (((300, 200), "win4"), ((1000, 700), "win12")):
        assert _lib.attn_win_plan(n, D, 2, H, win)["kernel"] == KNAME[kern]
        outs = []
        for cut in (0, 1, 2, 3):
            _lib.set_option(_lib.OPT_ATTN_CUT, cut)
            outs.append(_run(q, k, v, 2, n, H, win))
        _lib.set_option(_lib.OPT_ATTN_CUT, 0)
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), f"{win}: the cut changes the bits"
        for b in range(2):
            one = _run(q[b * n:(b + 1) * n], k[b * n:(b + 1) * n], v[b * n:(b + 1) * n], 1, n, H, win)
            assert torch.equal(one, outs[0][b * n:(b + 1) * n]), f"{win}: sample {b} of the stacked launch differs from its own launch"
        for form, other in ((1, "win12"), (2, "win4")):
            _lib.set_option(_lib.OPT_ATTN_WIN_FORM, form)
            assert _lib.attn_win_plan(n, D, 2, H, win)["kernel"] == KNAME[other]
            assert torch.equal(_run(q, k, v, 2, n, H, win), outs[0]), f"{win}: the {other} form gives other bits"
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, 0)


def _masked_truth(q, k, v, B, n, H, win):
    mask = window_mask(n, win)
    o = torch.empty(B * n, H * D, dtype=F64)
    for b in range(B):
        for h in range(H):
            rs, cs = slice(b * n, (b + 1) * n), slice(h * D, (h + 1) * D)
            s = (q[rs, cs].double() @ k[rs, cs].double().t() / math.sqrt(D)).masked_fill(~mask, -math.inf)
            o[rs, cs] = torch.softmax(s, -1) @ v[rs, cs].double()
    return o, mask


def _sdpa_bf16(q, k, v, B, n, H, mask):
    """bf16 CPU SDPA with the same boolean mask (the oracle's attention_core plus the window)"""
    import torch.nn.functional as F
    q4, k4, v4 = (t.view(B, n, H, D).transpose(1, 2) for t in (q, k, v))
    return F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask.view(1, 1, n, n)).transpose(1, 2).reshape(B * n, H * D)


def _seam_gate(got, truth, ref, name):
    """tests/test_gpu_parity.py's "flash_attention seam" gate"""
    e_hip, e_ora = (got.double().cpu() - truth).abs(), (ref.double() - truth).abs()
    tol = 3 * bf16_ulp(truth.float()) + 2e-3 * truth.abs().float().max()
    m = dict(max_err=float(e_hip.max()), max_err_over_tol=float((e_hip / tol).max()), rms_hip=float(e_hip.pow(2).mean().sqrt()),
             rms_sdpa=float(e_ora.pow(2).mean().sqrt()))
    record_margin("attn_window random: " + name, **m)
    print("attn_window random: " + name, json.dumps(m))
    assert (e_hip <= tol).all(), f"{name}: max err {float(e_hip.max()):.3e}"
    assert m["rms_hip"] <= 1.5 * m["rms_sdpa"] + 1e-5, name


@gpu
@pytest.mark.parametrize("B, n, win", [(2, 200, (40, 25)), (1, 321, (100, 0)), (1, 321, (-1, 0)), (2, 2504, (300, 200)), (1, 2504, (1000, 700)),
                                       (1, 2104, (-1, 0))])
def test_random_operands_against_fp64(B, n, win):
    H = 2
    q, k, v = _random(B, n, H, 1000 + n + win[0])
    truth, mask = _masked_truth(q, k, v, B, n, H, win)
    got = _run(q, k, v, B, n, H, win)
    _seam_gate(got, truth, _sdpa_bf16(q, k, v, B, n, H, mask), f"B{B} L{n} window {win} {L().attn_win_plan(n, D, B, H, win)['kernel']}")


@gpu
def test_rejections_write_nothing():
    """head_dim 64, a window side of -2, a V^T too narrow for the batch and batch 2 with L % 8 != 0: each returns non-zero from the C entry
    point (UnividHipError) before any launch and leaves a sentinel-filled output untouched; the plan entry refuses the same."""
    _lib = L()
    n, H = 72, 2
    C = H * D
    qbuf = torch.zeros(2 * n + 8, C, dtype=BF16, device=DEV)
    kbuf = torch.zeros(2 * n + 8, C, dtype=BF16, device=DEV)
    vbuf = torch.zeros(C, n + 128 + 64, dtype=BF16, device=DEV)
    full = torch.full((2 * n + 8, C), SENT, dtype=BF16, device=DEV)
    p = _lib.ptr

    def raw(match, ldvt=vbuf.stride(0), batch=1, n=n, H=H, hd=D, win=(8, 8)):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call("uv_flash_attn_win_bf16", p(qbuf), C, p(kbuf), C, p(vbuf), ldvt, p(full), C, batch, n, H, hd, D ** -0.5, win[0], win[1],
                      _lib.stream_ptr())

    raw("head_dim 64 unsupported", H=4, hd=64)
    raw(r"window \(-2, 8\)", win=(-2, 8))
    raw(r"window \(8, -2\)", win=(8, -2))
    raw("must cover", ldvt=128, batch=2)
    raw("needs L % 8", batch=2, n=68)
    for match, kw in (("head_dim 64", dict(D=64)), (r"window \(-2, 0\)", dict(window=(-2, 0)))):
        with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_win_plan: " + match):
            _lib.attn_win_plan(n, **{"D": D, "window": (4, 4), **kw})
    # the wrapper's own checks (dtype, extent) refuse before the C entry point
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_win\.q: "):
        _lib.flash_attn_win(qbuf[:n].view(torch.float16), kbuf[:n], vbuf[:, :128], full[:n], n, H, D, 1.0, (4, 4))
    with pytest.raises(_lib.UnividHipError, match=r"flash_attn_win\.vt: "):
        _lib.flash_attn_win(qbuf[:2 * n], kbuf[:2 * n], torch.zeros(C, 128, dtype=BF16, device=DEV), full[:2 * n], n, H, D, 1.0, (4, 4), batch=2)
    torch.cuda.synchronize()
    assert bool((full == SENT).all()), "a rejected call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------
# the operator seam
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_seam_window_and_causal():
    """flash_attention(q, k, v, window_size=(40, 25)) and causal=True at B = 2, Lq = Lk = 136, fp32 inputs: fp32 out on the bf16 grid, the
    seam test's gate; what is not built raises NotImplementedError naming the limit."""
    from univid_amd.wan.attention import attention, flash_attention
    B, n, N = 2, 136, 2
    g = torch.Generator().manual_seed(78)
    q, k, v = (torch.randn(B, n, N, D, generator=g) for _ in range(3))
    v += 0.25
    qb, kb, vb = (t.to(BF16).reshape(B * n, N * D) for t in (q, k, v))
    for kw, win in ((dict(window_size=(40, 25)), (40, 25)), (dict(causal=True), (-1, 0)), (dict(causal=True, window_size=(30, 7)), (30, 0))):
        out = flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), **kw)
        assert out.dtype == F32 and tuple(out.shape) == (B, n, N, D) and torch.equal(out, out.to(BF16).float())
        truth, mask = _masked_truth(qb, kb, vb, B, n, N, win)
        _seam_gate(out.reshape(B * n, N * D), truth, _sdpa_bf16(qb, kb, vb, B, n, N, mask), f"seam {kw}")
        assert torch.equal(attention(q.to(DEV), k.to(DEV), v.to(DEV), k_lens=torch.tensor([n] * B), **kw), out)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    for match, args in (("fp16", (dq.half(), dk.half(), dv.half(), {})),
                        ("head size 64", (dq[..., :64].contiguous(), dk[..., :64].contiguous(), dv[..., :64].contiguous(), {})),
                        ("Lq != Lk", (dq[:, :100].contiguous(), dk, dv, {})),
                        ("ragged k_lens", (dq, dk, dv, dict(k_lens=torch.tensor([n, 77]))))):
        a, b, c, kw = args
        with pytest.raises(NotImplementedError, match=match):
            flash_attention(a, b, c, window_size=(40, 25), dtype=torch.float16 if a.dtype == torch.float16 else BF16, **kw)
    with pytest.raises(ValueError, match="window_size"):
        flash_attention(dq, dk, dv, window_size=(-2, 3))


# ---------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def windowed_oracle(win):
    """The oracle with attention_core - for the self-attention call, the one that passes k_lens - replaced by the same function plus the
    boolean window mask (SDPA in wan_dit.BF16 operands with an attn_mask)."""
    import torch.nn.functional as F
    from oracle import wan_dit
    orig = wan_dit.attention_core

    def core(q, k, v, k_lens=None):
        if k_lens is None:
            return orig(q, k, v)
        assert q.size(1) == k.size(1) and int(k_lens.min()) == k.size(1), "the window is defined on unpadded self-attention"
        dt = q.dtype
        q, k, v = (t.to(wan_dit.BF16).transpose(1, 2) for t in (q, k, v))
        mask = window_mask(q.size(2), win).view(1, 1, q.size(2), q.size(2))
        return F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).contiguous().type(dt)

    wan_dit.attention_core = core
    try:
        yield
    finally:
        wan_dit.attention_core = orig


def _rms(a, b):
    return (a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt().item()


def _block_3072(seed, win):
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock
    with torch.device(DEV):
        blk = WanAttentionBlock(3072, 14336, 24, win, True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, seed)
    return blk.eval(), {k: v.detach().cpu() for k, v in sd.items()}


def _block_case(name, x, e_rows, tid, grid, ctx, blk, sdc, win):
    """One block built with window_size=win, HIP against the windowed oracle and its fp32 truth (both on the CPU): rms(hip - truth) <= 1.02
    rms(windowed oracle - truth) - the gate of every block-level mode test. The windowed output differs from the dense block's, and
    set_attn_window(None) brings back the dense bits exactly (those of a block built dense)."""
    from oracle import wan_dit
    from univid_amd.wan.model import _freqs_device
    heads = 24
    Lt = x.shape[1]
    fr = _freqs_device(wan_dit.rope_table(D), torch.device(DEV))

    def run(b):
        xx = x[0].to(DEV).clone()
        with torch.no_grad():
            b._run(xx, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), tuple(grid[0].tolist()), fr, ctx[0].to(DEV), first_block=False)
        return xx

    assert blk.self_attn.attn_window == win and blk.window_size == win
    got = run(blk)
    assert torch.isfinite(got).all() and torch.equal(run(blk), got)
    blk.set_attn_window(None)
    base = run(blk)
    assert blk.self_attn.attn_window is None and not torch.equal(got, base), "the windowed block equals the dense one"
    blk.set_attn_window((-1, -1))
    assert torch.equal(run(blk), base)
    blk.set_attn_window(win)
    assert torch.equal(run(blk), got), "the window after a round trip through global attention must equal the block before it"
    args = (sdc, "blocks.0.", x, e_rows[tid].unsqueeze(0), torch.tensor([Lt]), grid, wan_dit.rope_table(D))
    t0 = time.time()
    with torch.no_grad(), windowed_oracle(win):
        ora = wan_dit.block_forward(*args, ctx, heads, 1e-6)[0]
        old, wan_dit.BF16 = wan_dit.BF16, torch.float32
        try:
            truth = wan_dit.block_forward(*args, ctx.float(), heads, 1e-6)[0]
        finally:
            wan_dit.BF16 = old
    e_hip, e_ora = _rms(got, truth), _rms(ora, truth)
    m = dict(truth_ratio=e_hip / e_ora, rms_vs_truth_hip=e_hip, rms_vs_truth_windowed_oracle=e_ora, rms_windowed_vs_dense_hip=_rms(got, base),
             oracle_host_seconds=time.time() - t0)
    record_margin("attn_window " + name, **m)
    print("attn_window " + name, json.dumps(m))
    assert e_hip <= 1.02 * e_ora, f"{name}: rms vs truth {e_hip:.4e}, the windowed oracle's {e_ora:.4e}"


@gpu
def test_block_ti2v5b_width_short_kernel():
    g = load_golden("dit_block_3072")
    win = (16, 8)
    blk, sdc = _block_3072(g["seed"], win)
    assert g["x"].shape[1] == 48 and L().attn_win_plan(48, D, 1, 24, win)["kernel"] == KNAME["win4"]
    _block_case("block 3072 L48 window (16, 8)", g["x"], g["e_rows"], g["tid"], g["grid"], g["ctx"], blk, sdc, win)


def _long_block(win, kern):
    from univid_amd import detinit
    g = load_golden("dit_block_3072")
    Lt = 2304
    x = detinit.uniform_pm1("attn_window.block.x", Lt * 3072, g["seed"]).reshape(1, Lt, 3072).float() * 2
    tid = (torch.arange(Lt) * 7 // Lt % 2).to(g["tid"].dtype)
    blk, sdc = _block_3072(g["seed"], win)
    assert span_of(Lt, win) == min(Lt, 384 + sum(win)) and L().attn_win_plan(Lt, D, 1, 24, win)["kernel"] == KNAME[kern]
    _block_case(f"block 3072 L2304 window {win}", x, g["e_rows"], tid, torch.tensor([[4, 24, 24]]), g["ctx"], blk, sdc, win)


@gpu
def test_block_ti2v5b_width_one_frame_each_way():
    """2 304 tokens (grid 4 x 24 x 24) with window (576, 576), one frame each way. A workgroup streams at most 384 + 1152 = 1536 keys of it:
    by plan_attn_win's rule (span >= 2048) that is the 4-WAVE form, which is what is asserted; the 12-wave form under the block is the
    next test's."""
    _long_block((576, 576), "win4")


@gpu
def test_block_ti2v5b_width_long_kernel():
    """The same block and inputs with window (1152, 1152), two frames each way: span 2304, the 12-wave form under the model."""
    _long_block((1152, 1152), "win12")


def _small_model(seed=0, **over):
    """The tiny golden model has head_dim 64: dim 256 with 2 heads instead, weights from detinit."""
    from test_gpu_parity import _tiny_model
    return _tiny_model(seed, num_heads=2, **over)


WIN = (64, 64)


@gpu
def test_small_model_cfg_pair_setter_and_ffn_mode():
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    Lt = 256
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        gen = m._prep_gen
        m.set_attn_window(WIN)
        assert m._prep_gen > gen and m.window_size == WIN and m.config["window_size"] == WIN
        assert all(b.self_attn.attn_window == WIN and b.cross_attn.attn_window is None for b in m.blocks)
        got = m([x], t, [ctx], Lt)[0]
        ctx2 = (ctx * 0.5).contiguous()
        other = m([x], t, [ctx2], Lt)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], Lt)
        assert torch.equal(pair[0], got) and torch.equal(pair[1], other) and not torch.equal(got, other), "the stacked CFG pair differs from single forwards"
        assert not torch.equal(got, base) and torch.isfinite(got).all()
        m.set_ffn_precision("mxfp8")                                       # independent of the window: the two combine
        both = m([x], t, [ctx], Lt)[0]
        assert not torch.equal(both, got) and torch.isfinite(both).all()
        m.set_ffn_precision("bf16")
        assert torch.equal(m([x], t, [ctx], Lt)[0], got)
        m.set_attn_window(None)
        assert torch.equal(m([x], t, [ctx], Lt)[0], base), "global attention after a round trip must equal the model before the switch"
        # a model CONSTRUCTED with the window lands in the same state
        cfg2, sd2, m2 = _small_model(g["seed"], window_size=WIN)
        assert m2.window_size == WIN and all(b.self_attn.attn_window == WIN for b in m2.blocks)
        assert torch.equal(m2([x], t, [ctx], Lt)[0], got)


@gpu
def test_small_model_denoise_graph_and_recapture():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (2, g["shift"], g["guide_scale"])

    def pipe_in(win):
        cfg, sd, m = _small_model(g["seed"])
        return WanTI2V(TI2VConfig, model=m, device=DEV, attn_window=win)

    def gen(pipe, graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    fresh_w, fresh_d = pipe_in(WIN), pipe_in(None)
    assert fresh_w.model.window_size == WIN and all(b.self_attn.attn_window == WIN for b in fresh_w.model.blocks)
    assert fresh_d.model.window_size == (-1, -1)
    w_graph = gen(fresh_w, True)
    assert fresh_w._runner is not None
    assert torch.equal(w_graph, gen(fresh_w, False)), "graph != eager with a window"
    d_graph = gen(fresh_d, True)
    assert not torch.equal(d_graph, w_graph)
    fresh_d.model.set_attn_window(WIN)
    assert torch.equal(gen(fresh_d, True), w_graph), "after the switch the pipeline does not equal a fresh windowed pipeline (no re-capture?)"
    fresh_d.model.set_attn_window(None)
    assert torch.equal(gen(fresh_d, True), d_graph), "after the switch back the pipeline does not equal a fresh dense pipeline"
    fresh_w._runner = fresh_d._runner = None


@gpu
def test_checkpoint_with_a_window_loads(tmp_path):
    """A diffusers-layout directory whose config.json says "window_size": [64, 64] loads and equals the setter on a (-1, -1) model."""
    from safetensors.torch import save_file
    from univid_amd.wan.model import WanModel
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    conf = {k: (list(v) if isinstance(v, tuple) else v) for k, v in dict(cfg, model_type="ti2v", window_size=list(WIN)).items()}
    with open(os.path.join(tmp_path, "config.json"), "w") as f:
        json.dump(conf, f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(tmp_path, "diffusion_pytorch_model.safetensors"))
    loaded = WanModel.from_pretrained(str(tmp_path)).to(DEV)
    assert loaded.window_size == WIN and all(b.self_attn.attn_window == WIN for b in loaded.blocks)
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        m.set_attn_window(WIN)
        assert torch.equal(loaded([x], t, [ctx], 256)[0], m([x], t, [ctx], 256)[0])


@gpu
def test_unmerged_lora_works_with_a_window(tmp_path):
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    m.set_attn_window(WIN)
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
