"""Every flash-attention kernel instance plan_attn (csrc/attn_args.h) can select and launch_attn (csrc/attention.hip) names - the 12-wave
long-key kernel, the three-workgroups-per-CU short-key kernel and the generic kernel at head_dim 128 and 64, with bf16 / fp16 operands and
with the fused q-norm prologue: ten instances - called through `_lib.flash_attn` and compared with an fp64 softmax of the same operands.

The whole file is driven by ONE table (CASES). Every case names the kernel it expects and asserts `attn_plan(...)` - for the 12-wave
kernel also the query-block cut and the grid under the case's OPT_ATTN_CUT - before it launches (-m gpu); the operand builders' own
conditions are asserted for every table row without a GPU (test_operand_builders_hold_their_conditions).

Operand families:
  A       "integer exponents". softmax_scale = float32(ln 2): scale * log2(e) is exactly 1 in f32 (asserted), k dense +-1, q rows four +-1
          whose columns rotate with the row, v integers in -2 .. 2. Scores are even integers in [-4, 4], every P is a power of two (exact in
          bf16 / fp16), every partial sum of P v and of P is a multiple of one power of two and - the builder asserts the span
          max sum_j 2^(s_ij - min s) |v_jd| < 2^24 - exact in fp32 in ANY order and wherever the deferred maximum sits. The kernel's only
          inexact steps are the reciprocal of the row sum and the final product (and a 1-ulp error of the hardware exp2 on an integer, if it
          has one). Gate: bit-identical to the fp64 softmax rounded to the 16-bit type, except the elements whose fp64 value lies within
          relative 2^-18 (fp16: 2^-21) of a rounding boundary; at most 0.5 % of a case's elements may be excepted (asserted).
          The fp64 softmax is taken in base 2 with the exponent scale the entry point documents, float32(scale) * float32(log2 e) = 1:
          float32(ln 2) itself is 2e-8 away from ln 2, and with exp(s * float32(ln 2)) the sums that cancel to exactly 0 (dozens of
          elements per case) come out as 1e-10 - no relative band covers that.
  spike10 family A with scores in {0, 1} (v in -1 .. 1) and one late key 10 above them for two queries of three: more than UV_ATT_DEFER = 8,
          so the reference maximum moves and O and l are rescaled by a power of two;
  spike6  the same with the key 6 above: P up to 2^7 against the old maximum, no move.
  B       "selector", at the production scale D^-0.5: k distinct +-1 rows, q_i = c k_t(i) (c = 40 at D = 128, 96 at D = 64), t walking over
          all keys. The runner-up exponent is at least 300 below the winner (asserted), so every other P is exactly 0 in f32 and
          out[i] must EQUAL v[t(i)] as a bit pattern - v being random finite bit patterns of the type, subnormals included. Two things the
          arithmetic itself fixes: an accumulator that starts at +0 returns +0 for v = -0 (the signs of zeros are not compared), and the sums
          a row carries BEFORE its winner arrives (up to Lk keys at weights up to 2^8) must stay finite in f32, so bf16 exponent fields from
          224 on are folded down (|v| < 2^97).
Every case: the output has 8 slack rows (and slack columns where ldo > C) filled with SENT that must come back unchanged, the V^T columns
behind the last sample hold 1000, q and k have 8 more rows of +-64 patterns that would win every softmax, and where q / k are column
slices of one wider buffer the columns around the slices hold the same."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import record_margin

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
F64 = torch.float64
DEV = "cuda"
SENT = -7.25            # exact in bf16 and fp16; no designed result equals it
KNAME = {"fwd12": "flash_attn_fwd12_kernel", "fwd3": "flash_attn_fwd3_kernel", "d128": "flash_attn_fwd_kernel<128>", "d64": "flash_attn_fwd_kernel<64>"}
# the ten instances launch_attn names: (kernel, fp16 operands, q-norm prologue)
INSTANCES = {("fwd12", False, False), ("fwd12", False, True), ("fwd3", False, False), ("fwd3", False, True), ("d128", False, False),
             ("d128", False, True), ("d128", True, False), ("d64", False, False), ("d64", False, True), ("d64", True, False)}


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


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
# kern: the kernel the plan must name (KNAME); dt: operand / output type; qn: q is the raw projection, the Q prologue applies the norm;
# fam: operand family; cut: OPT_ATTN_CUT; ld: "dense", "slice" (q and k are the column slices [:, :C] and [:, C + 8:2 C + 8] of one
# [rows, 3 C + 16] buffer), "ldk24" (ldk = 2^24: the only way to flash_attn_fwd_kernel<128> with bf16 operands), "vt+64" / "vt+8" (ldvt
# that much wider than required), "ldo+8" (the transpose through LDS into a wider row) / "ldo+4" (the direct store)
Case = namedtuple("Case", "kern dt qn fam B H D Lq Lk cut ld")
CASES = []


def _c(kern, Lq, Lk, dt=BF16, qn=False, fam="A", B=1, H=2, cut=0, ld=None):
    D = 64 if kern == "d64" else 128
    if kern == "d128" and dt == BF16:
        ld, H = "ldk24", 1
    CASES.append(Case(kern, dt, qn, fam, B, H, D, Lq, Lk, cut, ld or "dense"))


# flash_attn_fwd3_kernel: the lone short tile, the paired main loop at even and odd tile counts, the ragged tile on either buffer, the last
# Lk before flash_attn_fwd12_kernel; one query, a second wave with one query, a last wave without any
for _lk in (5, 63, 64, 65, 128, 129, 192, 200, 256, 321, 2040):
    for _lq in (1, 33, 150):
        _c("fwd3", _lq, _lk)
# flash_attn_fwd12_kernel: even / odd tile counts with and without a ragged tile, under every kind of cut (16 units per head: 1 = 12 + 4 with
# 8 loader-only waves, 2 = 12 + 8, 3 = 8 + 8); 8 (sample, head)s: the XCD-aware block order
for _lk in (2048, 2104, 2112, 2184):
    for _cut in (0, 1, 2, 3):
        _c("fwd12", 500, _lk, B=2, H=4, cut=_cut)
for _cut in (0, 1, 2, 3):
    _c("fwd12", 500, 2104, H=3, cut=_cut)              # 3 (sample, head)s: block totals no multiple of 8, plain id order
_c("fwd12", 500, 2104, B=2, H=2, cut=2)                # 4 + 4 blocks: plain id order with both kinds
_c("fwd12", 1, 2048)
_c("fwd12", 1, 2104)
# flash_attn_fwd_kernel: head_dim 64 in both types, head_dim 128 with fp16 operands
for _kern, _dt in (("d64", BF16), ("d64", F16), ("d128", F16)):
    for _lk in (5, 64, 65, 128, 200, 256):
        for _lq in (1, 150, 260):
            _c(_kern, _lq, _lk, dt=_dt)
# flash_attn_fwd_kernel<128> with bf16 operands: 64 ldk >= 2^30
_c("d128", 150, 5)
_c("d128", 150, 70)
# the q-norm prologue of each of the four kernels: a short and a ragged key sequence
for _kern, _lks in (("fwd12", (2048, 2104)), ("fwd3", (5, 200)), ("d128", (5, 70)), ("d64", (5, 200))):
    for _lk in _lks:
        _c(_kern, 150, _lk, qn=True)
# stacked samples whose V^T columns start off a tile boundary (Lk a multiple of 8, none of 64); the ranker head: one query per sample
for _b in (2, 3):
    for _lk in (72, 200):
        _c("fwd3", 150, _lk, B=_b)
        _c("d64", 150, _lk, B=_b)
    _c("fwd12", 150, 2104, B=_b)
_c("d128", 150, 200, dt=F16, B=3)
_c("d64", 150, 72, dt=F16, B=3)
_c("d64", 1, 72, dt=F16, B=16)
_c("d64", 1, 200, B=16)
_c("fwd3", 1, 200, B=16)
_c("fwd12", 1, 2104, B=16, H=1)
# leading dimensions
for _ld in ("slice", "vt+64", "vt+8", "ldo+8", "ldo+4"):
    _c("fwd3", 150, 200, B=2, ld=_ld)
    _c("fwd12", 150, 2104, B=2, ld=_ld)
    _c("d64", 150, 200, B=2, ld=_ld)
# the late spike: the rescale branch, and P > 1 without a move
for _fam in ("spike10", "spike6"):
    _c("fwd3", 150, 200, fam=_fam)
    _c("d64", 150, 200, fam=_fam)
    _c("d64", 150, 256, dt=F16, fam=_fam)
    _c("d128", 150, 200, dt=F16, fam=_fam)
    _c("d128", 150, 70, fam=_fam)
    _c("fwd12", 150, 2104, fam=_fam)                   # (the 12-wave kernel has no Lk <= 256; the span is asserted all the same)
# the selector: one case per kernel and type, a ragged last tile, two samples
_c("fwd12", 500, 2104, fam="B", B=2)
_c("fwd3", 260, 200, fam="B", B=2)
_c("d128", 150, 72, fam="B", B=2)
_c("d128", 260, 200, dt=F16, fam="B", B=2)
_c("d64", 260, 200, fam="B", B=2)
_c("d64", 260, 200, dt=F16, fam="B", B=2)


def _id(i, c):
    return (f"{i:03d}-{c.kern}-{'f16' if c.dt == F16 else 'bf16'}{'-qnorm' if c.qn else ''}-{c.fam}-B{c.B}H{c.H}-Lq{c.Lq}-Lk{c.Lk}"
            + (f"-cut{c.cut}" if c.kern == "fwd12" else "") + ("" if c.ld == "dense" else "-" + c.ld))


IDS = [_id(i, c) for i, c in enumerate(CASES)]


def _layout(c):
    """(ldq, ldk, ldvt, ldo) of the case"""
    C = c.H * c.D
    ldq = ldk = ldo = C
    ldvt = (c.B - 1) * c.Lk + _up(c.Lk, 64)
    if c.ld == "slice":
        ldq = ldk = 3 * C + 16
    elif c.ld == "ldk24":
        ldk = 1 << 24
    elif c.ld in ("vt+64", "vt+8"):
        ldvt += int(c.ld[3:])
    elif c.ld in ("ldo+8", "ldo+4"):
        ldo += int(c.ld[4:])
    return ldq, ldk, ldvt, ldo


# ---------------------------------------------------------------------------------------------------------------
# the plan every case expects
# ---------------------------------------------------------------------------------------------------------------
def _auto_cut(nwu, nbh, ncus):
    """plan_attn's automatic cut, restated from its comment: a 12-unit workgroup takes time 1, an 8-unit one 0.76, each kind is dealt in id
    order to the least loaded of ncus CUs (12-unit blocks first); the cut with the smallest makespan wins, ties go to fewer 8-unit blocks."""
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


def _expected_plan(c, ncus):
    nbh = c.H * c.B
    if c.kern != "fwd12":
        qb = (c.Lq + 127) // 128
        return dict(kernel=KNAME[c.kern], q_blocks=qb, n12=0, grid=qb * nbh)
    nwu = (c.Lq + 31) // 32
    if c.cut > 0:
        n8 = c.cut - 1
        n12 = (nwu - 8 * n8 + 11) // 12 if nwu > 8 * n8 else 0
    else:
        n12, n8 = _auto_cut(nwu, nbh, ncus)
    return dict(kernel=KNAME[c.kern], q_blocks=n12 + n8, n12=n12, grid=(n12 + n8) * nbh)


def _assert_plan(c, ncus):
    """Under the case's OPT_ATTN_CUT (left set for the launch; the autouse fixture resets it)."""
    _lib = L()
    _lib.set_option(_lib.OPT_ATTN_CUT, c.cut)
    _, ldk, ldvt, _ = _layout(c)
    plan = _lib.attn_plan(c.Lq, c.Lk, c.D, c.B, c.H, c.dt == F16, ldk=ldk, ldvt=ldvt)
    want = _expected_plan(c, ncus)
    assert plan == want, f"planned {plan}, the case expects {want}"
    assert _lib.attn_kernel_name(c.Lq, c.Lk, c.D, c.B, H=c.H, f16=c.dt == F16, ldk=ldk, ldvt=ldvt) == want["kernel"]
    if c.kern == "fwd12" and c.cut and c.Lq == 500:
        assert (plan["n12"], plan["q_blocks"] - plan["n12"]) == {1: (2, 0), 2: (1, 1), 3: (0, 2)}[c.cut]
    return plan


# ---------------------------------------------------------------------------------------------------------------
# operands and references (CPU; shared by the cases that differ in the cut or the layout only)
# ---------------------------------------------------------------------------------------------------------------
# q k v: dense [B Lq, C] / [B Lk, C] / [B Lk, C] in the 16-bit type (q: the DESIGNED q); q_raw rs w: what a q-norm case passes;
# ref: the gate's expectation as 16-bit values; near: the elements excepted from the bit-exact gate (family A); strict: family A's result
# if exp2 is exact on integers and the reciprocal is correctly rounded (measured, not gated); stats: excluded share, span
Ops = namedtuple("Ops", "q k v scale q_raw rs w ref near strict stats")


def _near_boundary(x, dt, rel):
    """fp64 x -> which elements lie within rel |x| of a rounding boundary of the 16-bit format (the midpoint of two neighbours), ties included"""
    bits, emin = (8, -126) if dt == BF16 else (11, -14)
    m, e = torch.frexp(x.abs())                               # |x| = m 2^e, m in [0.5, 1)
    e = e.clamp_min(emin + 1)
    scaled = torch.ldexp(x.abs(), bits - e)                   # |x| in units of the format's spacing at x
    frac = scaled - scaled.floor()
    return (frac - 0.5).abs() <= rel * scaled


def _rint(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _qnorm_parts(g, q, dt):
    """rs a power of two per row, w in {+-1, +-2} per column, q_raw = q / (rs w): the prologue's bf16(bf16(q_raw rs) w) is the designed q"""
    rows, C = q.shape
    rs = torch.ldexp(torch.ones(rows, dtype=F64), torch.randint(-3, 4, (rows,), generator=g))
    w = (_rint(g, (C,), 0, 1) * 2 - 1) * (_rint(g, (C,), 1, 2))
    q_raw = q / (rs[:, None] * w)
    assert torch.equal(((q_raw.to(dt).float() * rs.float()[:, None]).to(dt).float() * w.float()).to(dt).double(), q)
    return q_raw.to(dt), rs.float(), w.float()


class _OtherSeed(Exception):
    """the operands of this seed miss a condition that depends on the seed alone: the next one is tried"""


@lru_cache(maxsize=None)
def _operands(fam, f16, qn, B, H, D, Lq, Lk):
    """The operands of a case, from the first of 64 seeds whose operands hold the seed-dependent conditions (family A: at most 0.5 % of the
    elements at a rounding boundary - one element is 0.4 % of a one-query case; family B: distinct key rows, the gap of 300). The choice
    looks at the operands and the fp64 reference only. Every other condition is asserted outright."""
    base = 1000003 * (f16 + 2 * qn) + 7919 * Lk + 31 * Lq + 5 * B + H + D + {"A": 0, "spike10": 1, "spike6": 2, "B": 3}[fam]
    why = []
    for attempt in range(64):
        g = torch.Generator().manual_seed(base + 15485863 * attempt)
        try:
            return (_selector if fam == "B" else _integer_exponents)(g, fam, F16 if f16 else BF16, qn, B, H, D, Lq, Lk)
        except _OtherSeed as ex:
            why.append(str(ex))
    raise AssertionError(f"no seed holds the conditions: {why[-1]}")


def _integer_exponents(g, fam, dt, qn, B, H, D, Lq, Lk):
    f16 = dt == F16
    C = H * D
    rq = torch.arange(B * Lq) % Lq
    # ---- family A and its spikes
    scale = np.float32(math.log(2.0))                          # s = 0
    sl2 = float(np.float32(scale) * np.float32(1.4426950408889634))       # the f32 product the entry point hands to the kernels
    assert sl2 == 1.0, "scale * log2(e) is not exactly 2^0 in f32"
    q = torch.zeros(B * Lq, C, dtype=F64)
    if fam == "A":
        k = _rint(g, (B * Lk, C), 0, 1) * 2 - 1
        v = _rint(g, (B * Lk, C), -2, 2)
        for h in range(H):
            for j in range(4):          # 32 consecutive rows touch every column of the head
                q[torch.arange(B * Lq), h * D + (rq + 7 * h + D // 4 * j) % D] = _rint(g, (B * Lq,), 0, 1) * 2 - 1
    else:
        gap, js = (10.0 if fam == "spike10" else 6.0), 64 + (Lk - 64) * 2 // 3
        assert 64 <= js < Lk, "the spike belongs into the second or a later tile"
        k = _rint(g, (B * Lk, C), 0, 1)
        v = _rint(g, (B * Lk, C), -1, 1)
        for h in range(H):
            k[:, h * D + D - 1] = 0
            k[torch.arange(B) * Lk + js, h * D + D - 1] = gap
            q[torch.arange(B * Lq), h * D + (rq + 5 * h) % (D - 1)] = 1
            q[:, h * D + D - 1] = (rq % 3 != 0).double()          # two queries of three see the spike
    ref = torch.empty(B * Lq, C, dtype=F64)
    strict = torch.empty(B * Lq, C, dtype=dt)
    span = 0.0
    for b in range(B):
        for h in range(H):
            qs, ks, cs = slice(b * Lq, (b + 1) * Lq), slice(b * Lk, (b + 1) * Lk), slice(h * D, (h + 1) * D)
            S = q[qs, cs] @ k[ks, cs].t()                       # exact integers
            X = S * sl2
            P = torch.exp2(X - X.max(-1, keepdim=True).values)
            ref[qs, cs] = (P @ v[ks, cs]) / P.sum(-1, keepdim=True)
            E = torch.exp2(S - S.min())                         # every P in units of the smallest one: exact powers of two
            span = max(span, float((E @ v[ks, cs].abs()).max()), float(E.sum(-1).max()))
            if fam != "A":
                spike, rest = S[:, js], torch.cat((S[:, :js], S[:, js + 1:]), 1)
                sees = q[qs, h * D + D - 1] == 1
                assert float(rest.max()) == 1 and float(rest.min()) == 0 and bool((spike[~sees] <= 1).all())
                assert bool((spike[sees] - rest.max(-1).values[sees] >= gap - 1).all()) and bool((spike[sees] >= gap).all())
            E = torch.exp2(S - S.max(-1, keepdim=True).values)
            O, l = E @ v[ks, cs], E.sum(-1)
            assert torch.equal(O.float().double(), O) and torch.equal(l.float().double(), l)
            strict[qs, cs] = (O.float() * (1.0 / l.float())[:, None]).to(dt)
    assert span < 2 ** 24, f"span 2^{math.log2(span):.2f}: a partial sum could round in fp32"
    near = _near_boundary(ref, dt, 2.0 ** (-21 if f16 else -18))
    share = float(near.double().mean())
    if share > 0.005:
        raise _OtherSeed(f"{share:.4%} of the elements lie at a rounding boundary (at most 0.5 % may be excepted)")
    for t in (q, k, v):
        assert torch.equal(t.to(dt).double(), t)
    q_raw, rs, w = _qnorm_parts(g, q, dt) if qn else (None, None, None)
    return Ops(q.to(dt), k.to(dt), v.to(dt), float(scale), q_raw, rs, w, ref.to(dt), near, strict, dict(excluded_share=share, span_log2=math.log2(span)))


def _selector(g, fam, dt, qn, B, H, D, Lq, Lk):
    C = H * D
    scale = np.float32(D ** -0.5)
    coef = 40.0 if D == 128 else 96.0
    k = _rint(g, (B * Lk, C), 0, 1) * 2 - 1
    # t: the first and the last key of the sample, the last key of the last whole tile and the first of the ragged one, then a walk over
    # all keys (Lq >= Lk: every key is some query's) or a stride through them; head h is shifted by 17 h
    fixed = [0, Lk - 1, Lk // 64 * 64 - 1, Lk // 64 * 64, Lk - 2]
    walk = torch.arange(Lq - len(fixed))
    t0 = torch.cat((torch.tensor(fixed), walk % Lk if len(walk) >= Lk else walk * 97 % Lk))
    bits = torch.randint(0, 1 << 16, (B * Lk, C), generator=g, dtype=torch.int32)
    if dt == BF16:
        ex = (bits >> 7) & 0xFF
        bits = (bits & ~(0xFF << 7)) | ((ex % 224) << 7)        # finite, |v| < 2^97 (see the file's docstring); subnormals and zeros stay
    else:
        ex = (bits >> 10) & 0x1F
        bits = (bits & ~(0x1F << 10)) | ((ex % 31) << 10)       # every finite fp16 pattern
    v = (bits - ((bits >> 15) << 16)).to(torch.int16).view(dt)
    mag, tiny = v.float().abs(), 2.0 ** (-14 if dt == F16 else -126)
    assert bool(torch.isfinite(mag).all()) and bool(((mag > 0) & (mag < tiny)).any()) and bool((mag == 0).any()), "no subnormals / zeros among v"
    q = torch.empty(B * Lq, C, dtype=F64)
    ref = torch.empty(B * Lq, C, dtype=dt)
    gap = math.inf
    seen = torch.zeros(Lk, dtype=torch.bool)
    for b in range(B):
        for h in range(H):
            qs, ks, cs = slice(b * Lq, (b + 1) * Lq), slice(b * Lk, (b + 1) * Lk), slice(h * D, (h + 1) * D)
            t = (t0 + 17 * h) % Lk
            seen[t] = True
            q[qs, cs] = coef * k[ks, cs][t]
            ref[qs, cs] = v[ks, cs][t]
            e = (q[qs, cs] @ k[ks, cs].t()) * float(np.float32(scale) * np.float32(1.4426950408889634))      # the exponents, exact to 1e-13
            top = e.topk(2, -1)
            if not torch.equal(top.indices[:, 0], t):
                raise _OtherSeed("a query's winner is not its own key (two equal key rows)")
            gap = min(gap, float((top.values[:, 0] - top.values[:, 1]).min()))
    if gap < 300:
        raise _OtherSeed(f"a runner-up exponent is only {gap:.1f} below the winner")
    assert bool(seen[[0, Lk - 1, Lk // 64 * 64 - 1, Lk // 64 * 64]].all()) and (len(walk) < Lk or bool(seen.all()))
    assert torch.equal(q.to(dt).double(), q)
    q_raw, rs, w = _qnorm_parts(g, q, dt) if qn else (None, None, None)
    return Ops(q.to(dt), k.to(dt), v, float(scale), q_raw, rs, w, ref, None, None, dict(selector_gap=gap))


def _ops(c):
    return _operands(c.fam, c.dt == F16, c.qn, c.B, c.H, c.D, c.Lq, c.Lk)


# ---------------------------------------------------------------------------------------------------------------
# the launch: operands in the case's memory layout, poison around them, sentinels around the output
# ---------------------------------------------------------------------------------------------------------------
def _poison(rows, cols, dt, g):
    """+-64 patterns, every second row the negative of the one before: attended as a key, one of each pair wins the softmax of any query
    it is not orthogonal to"""
    p = (torch.randint(0, 2, (rows, cols), generator=g, device=DEV) * 128 - 64).to(dt)
    p[1::2] = -p[0:rows - rows % 2:2]
    return p


def _launch(c, o):
    """One flash_attn call of the case -> the dense result [B Lq, C] on the CPU; the sentinels are asserted here."""
    _lib = L()
    C, rq, rk = c.H * c.D, c.B * c.Lq, c.B * c.Lk
    ldq, ldk, ldvt, ldo = _layout(c)
    g = torch.Generator(device=DEV).manual_seed(CASES.index(c))
    qv = (o.q_raw if c.qn else o.q).to(DEV)
    big = None
    if c.ld == "slice":
        buf = _poison(max(rq, rk) + 8, ldq, c.dt, g)
        q, k = buf[:rq, :C], buf[:rk, C + 8:2 * C + 8]
        q.copy_(qv)
        k.copy_(o.k.to(DEV))
    else:
        qb = _poison(rq + 8, C, c.dt, g)
        qb[:rq] = qv
        q = qb[:rq]
        if c.ld == "ldk24":         # only the addressed rows are written
            big = torch.empty((rk - 1) * ldk + C, dtype=c.dt, device=DEV)
            k = torch.as_strided(big, (rk, C), (ldk, 1))
            k.copy_(o.k.to(DEV))
        else:
            kb = _poison(rk + 8, C, c.dt, g)
            kb[:rk] = o.k.to(DEV)
            k = kb[:rk]
    vt = torch.full((C, ldvt), 1000.0, dtype=c.dt, device=DEV)
    vt[:, :rk] = o.v.to(DEV).t()
    full = torch.full((rq + 8, ldo), SENT, dtype=c.dt, device=DEV)
    out = full[:rq, :C]
    assert (q.stride(0), k.stride(0), vt.stride(0), out.stride(0)) == (ldq, ldk, ldvt, ldo)
    kw = dict(q_rs=o.rs.to(DEV), q_weight=o.w.to(DEV)) if c.qn else {}
    _lib.flash_attn(q, k, vt, out, c.Lq, c.Lk, c.H, c.D, o.scale, batch=c.B, **kw)
    torch.cuda.synchronize()
    host = full.cpu()
    del big, k
    if c.ld == "ldk24":
        torch.cuda.empty_cache()
    stray = int((host != SENT).sum()) - int((host[:rq, :C] != SENT).sum())
    assert stray == 0, f"{stray} elements outside the [{rq}, {C}] result were written (buffer {tuple(host.shape)})"
    if c.fam != "B":          # (a selected v may be any bit pattern, SENT's too; there the equality with v is the proof)
        assert not bool((host[:rq, :C] == SENT).any()), "part of the result was not written"
    return host[:rq, :C].contiguous()


def _where(c, i, j):
    return f"(row {i} = sample {i // c.Lq} query {i % c.Lq}: unit {i % c.Lq // 32} lane {i % 32}; column {j} = head {j // c.D} d {j % c.D})"


def _compare(c, o, got):
    """-> (mismatches outside the excepted elements, inside them, against the strict prediction); zeros compare equal whatever their sign"""
    diff = (got.view(torch.int16) != o.ref.view(torch.int16)) & ~((got == 0) & (o.ref == 0))
    if o.near is None:
        return diff, 0, 0
    strict = (got.view(torch.int16) != o.strict.view(torch.int16)) & ~((got == 0) & (o.strict == 0))
    return diff & ~o.near, int((diff & o.near).sum()), int(strict.sum())


@gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_attn_kernel_is_bit_exact_on_designed_operands(c):
    """The planned kernel (asserted), launched once on the case's designed operands: family A and the spikes bit-identical to the fp64
    softmax rounded to the 16-bit type outside the excepted elements (at most 0.5 %: asserted by the builder), family B equal to the selected
    V rows bit for bit; sentinels and poison as the file's docstring says. Recorded per case: the excepted share, the span, the mismatches
    INSIDE the excepted band (33 elements over 18 cases on an MI355X) and against the strict prediction (exact exp2, correctly rounded
    reciprocal: 0 in every case, so the hardware exp2 is exact on integers)."""
    ncus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = _assert_plan(c, ncus)
    o = _ops(c)
    got = _launch(c, o)
    bad, in_band, strict = _compare(c, o, got)
    name = IDS[CASES.index(c)]
    print(f"{name}: {plan}; {o.stats}; mismatches in the excepted band {in_band}, against the strict prediction {strict}")
    record_margin(f"attn_kernels/{name}", kernel=plan["kernel"], band_mismatches=in_band, strict_mismatches=strict, **o.stats)
    if bad.any():
        i, j = (int(x) for x in bad.nonzero()[0])
        rows = sorted({int(x) for x in bad.nonzero()[:, 0]})
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the reference, in {len(rows)} rows (first rows {rows[:8]}); "
                             f"first at {_where(c, i, j)}: got {got[i, j].item()!r}, expected {o.ref[i, j].item()!r}")


# ---------------------------------------------------------------------------------------------------------------
# without a GPU: the builders' conditions and the plans (256 CUs) of every table row; the table itself
# ---------------------------------------------------------------------------------------------------------------
def test_operand_builders_hold_their_conditions():
    """Every table row, on the CPU: the scale equality, the span below 2^24, the excepted share at or below 0.5 %, the spikes' score
    pattern, the selector's gap of at least 300 and its walk over the keys (all asserted inside the builders), and the row's plan as the
    library gives it for 256 CUs."""
    worst = dict(excluded_share=0.0, span_log2=0.0, selector_gap=math.inf)
    for c in CASES:
        o = _ops(c)
        _assert_plan(c, 256)
        assert o.ref.shape == (c.B * c.Lq, c.H * c.D) and o.ref.dtype == c.dt
        for key, val in o.stats.items():
            worst[key] = min(worst[key], val) if key == "selector_gap" else max(worst[key], val)
    print(f"{len(CASES)} cases, {_operands.cache_info().currsize} operand sets: largest excepted share {worst['excluded_share']:.4%}, largest span "
          f"2^{worst['span_log2']:.2f}, smallest selector gap {worst['selector_gap']:.1f}")
    assert worst["excluded_share"] <= 0.005 and worst["span_log2"] < 24 and worst["selector_gap"] >= 300


def test_boundary_band_is_what_it_says():
    """_near_boundary on hand-made values: exact ties and values 2^-19 (relative) off a boundary are excepted, values 2^-17 off are not;
    representable values never are."""
    for dt, bits, rel in ((BF16, 8, 2.0 ** -18), (F16, 11, 2.0 ** -21)):
        ulp = 2.0 ** (1 - bits)                                  # spacing in [1, 2)
        tie = 1.0 + 2.5 * ulp
        x = torch.tensor([tie, tie * (1 + rel / 2), tie * (1 - rel / 2), tie * (1 + 2 * rel), tie * (1 - 2 * rel), 1.0 + 3 * ulp, -tie, 0.0, tie * 2.0 ** -9], dtype=F64)
        assert _near_boundary(x, dt, rel).tolist() == [True, True, True, False, False, False, True, False, True]


def test_case_table_covers_the_ten_instances():
    """The table reaches exactly the ten kernel instances launch_attn names, each family B kernel / type pair, and for every kernel the
    layouts, cuts and batch shapes the file's docstring promises."""
    assert {(c.kern, c.dt == F16, c.qn) for c in CASES} == INSTANCES and len(INSTANCES) == 10
    assert {(c.kern, c.dt == F16) for c in CASES if c.fam == "B"} == {(k, f) for k, f, _ in INSTANCES}
    assert all(c.B == 2 and c.Lk % 64 for c in CASES if c.fam == "B")
    for kern in ("fwd3", "fwd12", "d64"):
        assert {c.ld for c in CASES if c.kern == kern} == {"dense", "slice", "vt+64", "vt+8", "ldo+8", "ldo+4"}, kern
        assert {2, 3, 16} <= {c.B for c in CASES if c.kern == kern and c.Lk % 64}, kern
    assert all(c.ld == "ldk24" and c.H == 1 for c in CASES if c.kern == "d128" and c.dt == BF16)
    assert {c.cut for c in CASES if c.kern == "fwd12" and c.Lq == 500 and c.H * c.B == 8} == {0, 1, 2, 3}
    assert {c.cut for c in CASES if c.kern == "fwd12" and c.Lq == 500 and c.H * c.B % 8} == {0, 1, 2, 3}
    for kern, dt in (("fwd3", BF16), ("fwd12", BF16), ("d64", BF16), ("d64", F16), ("d128", F16), ("d128", BF16)):
        assert {"A", "spike10", "spike6", "B"} == {c.fam for c in CASES if c.kern == kern and c.dt == dt}, (kern, dt)
    assert all(c.B == 1 or c.Lk % 8 == 0 for c in CASES) and all(c.H <= 4 and c.Lq <= 500 for c in CASES)
    assert len(set(IDS)) == len(IDS)


# ---------------------------------------------------------------------------------------------------------------
# what the host refuses
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_attn_rejections():
    """Each argument check of attn_entry returns non-zero (UnividHipError through the wrapper) before any launch and leaves a
    sentinel-filled output untouched. Which layer refuses: the C entry point for ldq % 8, Lk % 8 with batch > 1, a misaligned pointer
    and head_dim 96 (the Python check passes them: it verifies dtype, layout and extent); for a V^T too narrow for the batch and for q_rs
    without q_weight the Python check refuses first, so the C check is also driven directly through `_lib.call`; q-norm with fp16 operands
    has no C entry point at all (attn_entry<true> is never given a q_rs) - `_lib.flash_attn` refuses it."""
    _lib = L()
    Lq, Lk, H, D = 40, 72, 2, 128
    C = H * D
    scale = D ** -0.5
    qbuf = torch.zeros(2 * Lq + 8, C + 8, dtype=BF16, device=DEV)
    kbuf = torch.zeros(2 * Lk + 8, C, dtype=BF16, device=DEV)
    vbuf = torch.zeros(C, Lk + 128 + 64, dtype=BF16, device=DEV)
    full = torch.full((2 * Lq + 8, C), SENT, dtype=BF16, device=DEV)
    rs, w = torch.ones(2 * Lq, device=DEV), torch.ones(C, device=DEV)
    q, k, vt, out = qbuf[:Lq, :C], kbuf[:Lk], vbuf[:, :128], full[:Lq]

    def refused(match, q=q, k=k, vt=vt, out=out, Lq=Lq, Lk=Lk, H=H, D=D, batch=1, **kw):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.flash_attn(q, k, vt, out, Lq, Lk, H, D, scale, batch=batch, **kw)

    def refused_in_c(match, entry, *args):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call(entry, *args)

    p = _lib.ptr
    # ---- the C entry point refuses
    refused("multiples of 8", q=torch.as_strided(qbuf, (Lq, C), (C + 4, 1)))                      # ldq % 8
    refused("16-byte aligned", q=torch.as_strided(qbuf, (Lq, C), (C + 8, 1), 4))                  # q 8 bytes off
    refused("16-byte aligned", vt=torch.as_strided(vbuf, (C, 128), (vbuf.stride(0), 1), 4))
    refused("needs Lk % 8", Lk=68, batch=2, k=kbuf[:2 * 68], vt=vbuf[:, :68 + 128], q=qbuf[:2 * Lq, :C], out=full[:2 * Lq])
    refused("head_dim 96 unsupported", H=1, D=96, q=qbuf[:Lq, :96], k=kbuf[:Lk, :96], vt=vbuf[:96, :128], out=full[:Lq, :96])
    # ---- the Python check refuses first; the C check driven directly
    refused("addresses", batch=2, vt=torch.zeros(C, 128, dtype=BF16, device=DEV), k=kbuf[:2 * Lk], q=qbuf[:2 * Lq, :C], out=full[:2 * Lq])
    refused_in_c("must cover", "uv_flash_attn_bf16", p(qbuf), C + 8, p(kbuf), C, p(vbuf), 128, p(full), C, 2, Lq, Lk, H, D, scale, _lib.stream_ptr())
    refused("a tensor is required", q_rs=rs)
    refused_in_c("q_rs / q_weight missing", "uv_flash_attn_bf16_qnorm", p(qbuf), C + 8, p(kbuf), C, p(vbuf), 128, p(full), C, 1, Lq, Lk, H, D, scale,
                 p(rs), None, _lib.stream_ptr())
    refused_in_c("16-byte aligned", "uv_flash_attn_bf16_qnorm", p(qbuf), C + 8, p(kbuf), C, p(vbuf), 128, p(full), C, 1, Lq, Lk, H, D, scale,
                 p(rs[1:]), p(w), _lib.stream_ptr())
    # ---- only the wrapper can refuse
    refused("bf16 only", q=qbuf.view(F16)[:Lq, :C], k=kbuf.view(F16)[:Lk], vt=vbuf.view(F16)[:, :128], out=full.view(F16)[:Lq], q_rs=rs, q_weight=w)
    torch.cuda.synchronize()
    assert bool((full == SENT).all()), "a rejected call wrote to its output"
