"""GPU (-m gpu): every bf16 / fp16 "NT" GEMM kernel the launch planner (plan_gemm, csrc/gemm_bf16.hip) can select, with every epilogue its
family is built for, called directly through the C ABI and compared with an fp64 product of the same operands.

The whole file is driven by ONE table (CASES). Every case names the plan it expects - a list of (kernel, first row, rows) - and asserts
`gemm_plan(...)` equals it before every launch; cases whose plan depends on the CU count skip on a device that does not report 256. The
names in the table are exactly the reachable ones of the library's name table (test_case_table_names_every_kernel).

Gates:
  (a) bit-exact on designed operands (test_gemm_kernel_is_bit_exact_on_designed_operands): small integers times a power of two, so every
      product and every partial sum - in any order, split over K slices or not - is exact in fp32 and the result must EQUAL the fp64
      reference rounded once to the 16-bit format, ties included (at least 1 % of every case's results are exact ties);
  (b) random normal operands through the existing assert_bf16_kernel (test_gemm_kernel_on_random_operands);
  (c) sentinels: every output (and ssq) has 8 slack rows and, where the case is `wide`, slack columns, pre-filled with SENT, and all of them
      are SENT afterwards; slack columns of A, W and the gate table hold a huge finite value, rows behind M / N hold NaN;
  (d) kernels that serve the same (M, N, K) give identical designed-operand outputs (asserted pairwise so that a failure names the pair);
  (e) what the host refuses raises UnividHipError and leaves the output untouched (test_gemm_rejections).
"""
import os
import re
from collections import namedtuple

import pytest
import torch

from conftest import bf16_ulp, record_margin
from test_gpu_parity import assert_bf16_kernel

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
F64 = torch.float64
DEV = "cuda"
SENT = -7.25            # exact in fp32, bf16 and fp16
E_BF16, E_GELU, E_F32, E_RESID, E_GATE, E_T, E_SSQ = range(7)      # include/univid_hip.h: UV_EPI_*
EPI_NAME = ["BF16", "GELU_BF16", "F32_FROM_BF16", "RESID_F32", "GATE_RESID_F32", "BF16_T", "BF16_SSQ"]
ALL7 = frozenset(range(7))


@pytest.fixture(scope="module", autouse=True)
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


def L():
    from univid_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
# plan: what uv_gemm_plan must report, ((kernel, m0, rows), ...); cfg: tile_cfg; dt: operand / 16-bit output type; wide: lda = K + 8,
# ldw = K + 16, ldo = N + 8 (16-bit outputs) / N + 4 (f32 outputs; N + 8 where the plan needs ldo % 8 == 0), gate_stride = N + 4,
# ld_ssq = N / 32 + 3, transposed output: 8 more columns; epis: None = every epilogue all kernels of the plan are built for
Case = namedtuple("Case", "plan cfg dt M N K wide epis")

# the gemm_bf16_nt_kernel forms: tile_cfg -> (name, BM, BN, stages, columns per wave)
NT_FORMS = {1: ("T128", 128, 128, 2, 64), 12: ("RING128", 128, 128, 4, 64), 5: ("T256", 256, 256, 2, 64), 6: ("T256x192", 256, 192, 2, 48),
            2: ("DIAG2", 256, 256, 2, 64), 3: ("DIAG3", 256, 128, 2, 64), 4: ("DIAG4", 256, 192, 2, 48), 10: ("DIAG10", 128, 128, 4, 64),
            11: ("DIAG11", 128, 128, 4, 32), 13: ("DIAG13", 128, 128, 2, 32)}
# the epilogues each kernel is built for (the host decides: launch_cfg / launch_8ph_splitk). UV_EPI_BF16_SSQ needs whole 32-column groups
# per wave (not the 192-column tiles: 48 columns per wave); the split-K strip has the bf16 and the residual epilogues
BUILT = {"PERSIST": ALL7, "PINGPONG": ALL7, "DIAG14": ALL7, "SPLITK4": frozenset((E_BF16, E_RESID, E_GATE)), "SPLITK2": frozenset((E_BF16, E_RESID, E_GATE))}
BUILT.update({name: ALL7 if cols % 32 == 0 else ALL7 - {E_SSQ} for name, _, _, _, cols in NT_FORMS.values()})
F16_KERNELS = {"PERSIST", "PINGPONG", "RING128", "T128", "T256"}      # what tile_cfg 0 can return for fp16 operands

CASES = []


def _c(plan, cfg, M, N, K, dt=BF16, epis=None):
    if isinstance(plan, str):
        plan = ((plan, 0, M),)
    CASES.append(Case(tuple(plan), cfg, dt, M, N, K, len(CASES) % 2 == 1, epis))


for _cfg, (_name, _bm, _bn, _ns, _cols) in NT_FORMS.items():
    # one row / one row short of a tile / a second, almost empty row tile; the narrowest N / 16 columns short / a second, narrow column
    # tile; fewer K tiles than stages / exactly as many / one more. A Latin square: every value of each axis against every value of the
    # other two axes' pairs at least once
    _Ms, _Ns, _Ks = (1, _bm - 1, _bm + 1), (16, _bn - 16, _bn + 16), (64, 64 * _ns, 64 * (_ns + 1))
    for _i, _m in enumerate(_Ms):
        for _j, _n in enumerate(_Ns):
            _c(_name, _cfg, _m, _n, _Ks[(_i + _j) % 3])
    if _cols % 32 == 0:       # N % 32 == 0, which the sums of squares need: the same edges in whole 32-column groups
        _c(_name, _cfg, _bm + 1, _bn + 32, _Ks[2])
        _c(_name, _cfg, _bm - 1, _bn - 32, _Ks[1])
        _c(_name, _cfg, 1, 32, _Ks[0])
# the one-tile ping-pong kernel (VAR 5 = tile_cfg 7, the 4-phase reference schedule = 14): K = its minimum (2 K-tile pairs: no steady-state
# iteration), 3 pairs, 5 pairs
for _cfg, _name in ((7, "PINGPONG"), (14, "DIAG14")):
    for _k in (256, 384, 640):
        for _m, _n in ((255, 240), (257, 272), (512, 512)):
            _c(_name, _cfg, _m, _n, _k)
# the persistent kernel alone: 8 tiles (one per workgroup), 12 (8 workgroups with unequal lists), 272 (more than one per workgroup at 256
# CUs; 17 row tiles: no multiple of any gm)
for _k in (384, 512):
    for _m, _n in ((512, 1024), (768, 1024), (4352, 4096)):
        _c("PERSIST", 17, _m, _n, _k)
# split-K through the workspace: 4 slices of 256 / 384, 2 slices of 256 / 384; one ragged tile and 2 x 3 ragged tiles
for _cfg, _name, _Ks in ((19, "SPLITK4", (1024, 1536)), (20, "SPLITK2", (512, 768))):
    for _k in _Ks:
        for _m, _n in ((100, 256), (300, 528)):
            _c(_name, _cfg, _m, _n, _k)
N_DIRECT = len(CASES)         # from here on: plans that depend on the CU count (256)
# two-step plans: 17 x 16 tiles = one round of 256 and 16 tiles -> 4 096 rows and a 60-row strip
_c((("PINGPONG", 0, 4096), ("RING128", 4096, 60)), 8, 4156, 4096, 256)
_c((("T256", 0, 4096), ("RING128", 4096, 60)), 9, 4156, 4096, 256)
_c((("PERSIST", 0, 4096), ("RING128", 4096, 60)), 18, 4156, 4096, 384)
_c((("PERSIST", 0, 8192), ("RING128", 8192, 100)), 0, 8292, 4096, 384)
_c((("PINGPONG", 0, 4096), ("RING128", 4096, 60)), 0, 4156, 4096, 384)
# tile_cfg 0, one step, each kernel it can reach (PINGPONG by both rules: under two rounds of whole tiles; tall and narrow)
_c("T256", 0, 4156, 4096, 256)             # K < 384: not the large path (the 16-wave kernel at the shape of the tile_cfg 8 / 9 cases)
_c("PERSIST", 0, 8192, 4096, 384)
_c("PINGPONG", 0, 2048, 1024, 384)
_c("PINGPONG", 0, 11008, 768, 256)
_c("RING128", 0, 300, 512, 64)
_c("T128", 0, 2000, 4240, 64)
_c("T256", 0, 2048, 1024, 64)
_c("T256x192", 0, 2048, 1152, 64)
_c("T256", 0, 2048, 1152, 64, epis=(E_SSQ,))                  # the sums of squares cannot take the 192-column tiles
# fp16 operands: the five kernels tile_cfg 0 can return, and the shape where bf16 takes T256x192
_c((("PERSIST", 0, 8192), ("RING128", 8192, 100)), 0, 8292, 4096, 384, dt=F16)
_c("PINGPONG", 0, 2048, 1024, 384, dt=F16)
_c("RING128", 0, 300, 512, 64, dt=F16)
_c("T128", 0, 2000, 4240, 64, dt=F16)
_c("T256", 0, 2048, 1024, 64, dt=F16)
_c("T256", 0, 2048, 1152, 64, dt=F16)

IDS = [f"{i:03d}-cfg{c.cfg}-{'+'.join(s[0] for s in c.plan)}-{'f16' if c.dt == F16 else 'bf16'}-{c.M}x{c.N}x{c.K}" + ("-wide" if c.wide else "")
       for i, c in enumerate(CASES)]


def _cu_dependent(c):
    return CASES.index(c) >= N_DIRECT


def _epis(c):
    if c.epis is not None:
        return tuple(c.epis)
    e = set(ALL7)
    for name, _, _ in c.plan:
        e &= BUILT[name]
    if c.dt == F16 or c.N % 32:       # uv_gemm_bf16_nt_ssq: bf16 only, whole 32-column groups
        e.discard(E_SSQ)
    return tuple(sorted(e))


def _variant(c):
    """0: bias and gate_tid given; 1: bias = None; 2: gate_tid = None. A function of the shape, so kernels that share a shape share operands."""
    return (c.M + c.N // 16 + c.K // 128) % 3


def _need_cus(c):
    if _cu_dependent(c):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != 256:
            pytest.skip(f"the expected plan is the 256-CU one ({cus} CUs here)")


# ---------------------------------------------------------------------------------------------------------------
# operands in the kernels' memory layout
# ---------------------------------------------------------------------------------------------------------------
Ops = namedtuple("Ops", "a w bias x0 gate tid A W B G")       # a / w / bias / gate: views into padded buffers; A W B G: the dense values


def _up(x, m):
    return (x + m - 1) // m * m


def _huge(dt):
    """a huge finite value of the type: 2^111 (bf16), 28 672 (fp16), 2.6e33 (f32) - a kernel that reads slack columns cannot stay inside any gate"""
    return {BF16: 2.0 ** 111, F16: 28672.0, F32: 2.6e33}[dt]


def _padded(t, ld, dt):
    """t [R, C] -> the first R rows / C columns of a [R + 8, ld] buffer: slack columns huge, the 8 rows behind NaN"""
    R, C = t.shape
    buf = torch.full((R + 8, ld), _huge(dt), dtype=dt, device=DEV)
    buf[R:] = float("nan")
    buf[:R, :C] = t.to(dt)
    return buf[:R, :C]


def _operands(c, A, W, B, gen):
    """A [M, K], W [N, K], B [N] f32 values on the device that the 16-bit type holds exactly -> Ops. x0 / gate: random f32; tid: random gate
    rows 0 .. 2 (repeated from row to row); per _variant the bias or tid is None."""
    M, N, K = c.M, c.N, c.K
    v = _variant(c)
    a = _padded(A, K + 8 if c.wide else K, c.dt)
    w = _padded(W, K + 16 if c.wide else K, c.dt)
    bias = None
    if v != 1:
        bb = torch.full((N + 8,), float("nan"), dtype=c.dt, device=DEV)
        bb[:N] = B.to(c.dt)
        bias = bb[:N]
    x0 = torch.randn(M, N, device=DEV, generator=gen)
    G = torch.randn(3, N, device=DEV, generator=gen)
    gate = _padded(G, N + 4 if c.wide else N, F32)
    tid = None
    if v != 2:
        tt = torch.full((M + 8,), 3, dtype=torch.int32, device=DEV)         # (row 3 of the gate buffer is NaN)
        tt[:M] = torch.randint(0, 3, (M,), device=DEV, generator=gen, dtype=torch.int32)
        tid = tt[:M]
    return Ops(a, w, bias, x0, gate, tid, A, W, B if v != 1 else torch.zeros_like(B), G)


def _gate_rows(o):
    return o.G[o.tid.long()] if o.tid is not None else o.G[0:1]


def _plan(c, epi, ldo, ws_bytes):
    return [(s["kernel"], s["m0"], s["rows"]) for s in L().gemm_plan(c.M, c.N, c.K, epi, ldo, c.cfg, c.dt == F16, ws_bytes)]


def _workspace(c, cfg=None):
    """split-K: the workspace of the whole problem, slabs and counters pre-filled with NaN"""
    sk = {19: 4, 20: 2}.get(c.cfg if cfg is None else cfg)
    if sk is None:
        return None
    ws = torch.empty(4096 + _up(c.M, 256) // 256 * (_up(c.N, 256) // 256) * sk * 262144, dtype=torch.uint8, device=DEV)
    ws.view(F32).fill_(float("nan"))
    return ws


def _launch(c, epi, o, cfg=None):
    """One call of the case's entry point with epilogue `epi` (cfg: another tile_cfg on the same operands, no plan asserted). Asserts the
    plan before the launch and the sentinels after it (gate c). Returns the dense result [M, N] (BF16_T: transposed back; BF16_SSQ:
    (out, ssq))."""
    _lib = L()
    M, N, K = c.M, c.N, c.K
    f32out = epi in (E_F32, E_RESID, E_GATE)
    ws = _workspace(c, cfg)
    nws = 0 if ws is None else ws.numel()
    if epi == E_T:
        ldo, shape, reg = _up(M, 8) + (8 if c.wide else 0), None, (N, M)
    else:
        ldo, reg = N + ((4 if f32out else 8) if c.wide else 0), (M, N)
        if f32out and c.wide and c.cfg == 0 and cfg is None and _plan(c, epi, ldo, nws) != list(c.plan):
            ldo = N + 8           # this plan needs ldo % 8 == 0 (the tall-and-narrow rule)
    if cfg is None:
        plan = _plan(c, epi, ldo, nws)
        assert plan == list(c.plan), f"planned {plan}, the case expects {list(c.plan)}"
    out = torch.full((reg[0] + 8, ldo), SENT, dtype=F32 if f32out else c.dt, device=DEV)
    if epi in (E_RESID, E_GATE):
        out[:M, :N] = o.x0
    tile_cfg = c.cfg if cfg is None else cfg
    ssq = None
    if epi == E_SSQ:
        ssq = torch.full((M + 8, N // 32 + (3 if c.wide else 0)), SENT, dtype=F32, device=DEV)
        _lib.gemm_bf16_ssq(o.a, o.w, o.bias, out, ssq, M=M, tile_cfg=tile_cfg)
    else:
        kw = dict(gate=o.gate, gate_tid=o.tid) if epi == E_GATE else {}
        _lib.gemm_bf16(o.a, o.w, o.bias, out, epi, M=M, tile_cfg=tile_cfg, ws=ws, **kw)
    torch.cuda.synchronize()
    name = f"{EPI_NAME[epi]} tile_cfg {tile_cfg}"
    for buf, (r, q) in ((out, reg),) + (((ssq, (M, N // 32)),) if ssq is not None else ()):
        stray = int((buf != SENT).sum()) - int((buf[:r, :q] != SENT).sum())
        assert stray == 0, f"{name}: {stray} elements outside the [{r}, {q}] result were written (buffer {tuple(buf.shape)})"
        if epi not in (E_RESID, E_GATE):
            assert not bool((buf[:r, :q] == SENT).all()), f"{name}: nothing was written"
    got = out[:reg[0], :reg[1]]
    if epi == E_T:
        got = got.t()
    return (got, ssq[:M, :N // 32]) if epi == E_SSQ else got


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def _ulp16(x, dt):
    """spacing of the 16-bit format at |x| (f32 tensor): 8 (bf16) / 11 (fp16) significant bits, the subnormal spacing below the smallest normal"""
    bits, emin = (8, -126) if dt == BF16 else (11, -14)
    e = torch.frexp(x.abs().float())[1] - 1                   # |x| = m 2^(e + 1), m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x, dtype=F32), e - (bits - 1))


def _tie_share(v, dt):
    """share of the f32 values v that lie exactly midway between two neighbours of the 16-bit format"""
    y = v.to(dt).float()
    return float(((v - y).abs() == 0.5 * _ulp16(v, dt)).float().mean())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _assert_bits(got, ref, name):
    """got equals ref bit for bit (+0 / -0: a sum that cancels may be either)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = (_bits(got) != _bits(ref)) & ~((got == 0) & (ref == 0))
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the reference; first at (row, column) {i}: "
                             f"got {got[i].item()!r}, expected {ref[i].item()!r}")


def _rand_int(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()


def _exact_product(c, A, W, B):
    """fp64 A W^T + bias of designed operands (A integers, W and bias integers x 2^-4), with the condition under which every kernel must
    reproduce it exactly asserted on the operands: K max|a| max|w| + max|bias|, in units of 2^-4, stays below 2^24 - so every product and
    every partial sum, in any order, is an integer number of units that fp32 holds - and the fp64 result round-trips through fp32."""
    units = c.K * float(A.abs().max()) * float(W.abs().max()) * 16 + float(B.abs().max()) * 16
    assert units < 2 ** 24, f"K max|a| max|w| + max|bias| = {units} units of 2^-4"
    assert torch.equal(A, A.round()) and torch.equal(W * 16, (W * 16).round()) and torch.equal(B * 16, (B * 16).round())
    assert torch.equal(A.to(c.dt).float(), A) and torch.equal(W.to(c.dt).float(), W) and torch.equal(B.to(c.dt).float(), B)
    acc = A.double() @ W.double().t() + B.double()
    assert torch.equal(acc.float().double(), acc), "the fp64 reference is not an fp32 number"
    return acc.float()


def _gelu64(x):
    """tanh-GELU in fp64 as x sigmoid(2 u): 0.5 x (1 + tanh u) cancels to 0 below x = -6.9 even in fp64, where the true value is still a
    normal bf16 number"""
    x = x.double()
    return x / (1.0 + torch.exp(-2.0 * 0.7978845608028654 * (x + 0.044715 * x ** 3)))


_SEEN = {}            # gate (d): (dtype, M, N, K, class, epilogue) -> (case id, dense result)
_GELU = {}            # designed-operand GELU: kernel -> [bit-identical, elements]
_RANDOM = {}          # random operands: kernel -> [bit-identical, elements] over the 16-bit epilogues


def _agree(c, cls, epi, got):
    """Gate (d): the first kernel that served this (M, N, K) with these operands gave the same bits."""
    key = (c.dt, c.M, c.N, c.K, cls, epi)
    me = IDS[CASES.index(c)]
    if key in _SEEN:
        other, ref = _SEEN[key]
        for g, r in zip(got if isinstance(got, tuple) else (got,), ref):
            _assert_bits(g, r, f"{EPI_NAME[epi]} ({cls} operands): {me} against {other}")
    else:
        _SEEN[key] = (me, tuple(g.clone() for g in (got if isinstance(got, tuple) else (got,))))


def _check_gelu(c, got, y, name):
    """GELU of the EXACT pre-activation y (already bit-exact under UV_EPI_BF16): against the fp64 tanh-GELU of y rounded once to the 16-bit
    format, every element within 1 ulp of the format - no allowance for a pre-activation flip, there is none. One absolute term is added:
    |y| 2^-126. The epilogue is specified as f32 arithmetic, y times a sigmoid factor; a factor under f32's smallest normal number 2^-126
    is not an f32 number any more and may become 0, which moves the product by at most |y| 2^-126 = 1e-37 at the y = -10.06 .. -10.25
    where that happens (bf16 has f32's exponent range, so 1 ulp there is 2^-133; fp16 never sees the term). The bit-identical share
    is measured, recorded, and gated at the project's 0.995 (assert_gelu) over the kernel's cases."""
    ref = _gelu64(y).to(c.dt)
    d = (got.float() - ref.float()).abs()
    ulp = _ulp16(torch.maximum(got.float().abs(), ref.float().abs()), c.dt)
    assert bool(torch.isfinite(got.float()).all()), name
    over = d > ulp + y.float().abs() * 2.0 ** -126
    if over.any():
        i = tuple(int(v) for v in over.nonzero()[0])
        raise AssertionError(f"{name}: {int(over.sum())} of {d.numel()} elements further than 1 ulp from the fp64 GELU; first at {i}: pre-activation "
                             f"{y[i].item()!r}, got {got[i].item()!r}, expected {ref[i].item()!r}")
    same = int((d == 0).sum())
    for k in {s[0] for s in c.plan}:
        cur = _GELU.setdefault(k, [0, 0])
        cur[0] += same
        cur[1] += d.numel()
    print(f"{name}: {same} of {d.numel()} bit-identical to the rounded fp64 GELU")
    if d.numel() >= 20000:
        assert same >= 0.995 * d.numel(), f"{name}: only {same / d.numel():.5f} bit-identical"


# ---------------------------------------------------------------------------------------------------------------
# (a) bit-exact on designed operands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gemm_kernel_is_bit_exact_on_designed_operands(c):
    """Gates (a), (c), (d). Operands whose every product and partial sum is exact in fp32:
      wide    A integers in [lo, 15], W integers in [lo, 15] x 2^-4, bias integers in [-15, 15] x 2^-4. lo = -15; where fewer than 1 % of the
              results would be exact ties of the 16-bit rounding (fp16's 11 bits at K = 64: the sums are too small to need rounding), the
              magnitudes are raised: lo = -7, then 0 (all-positive operands: every sum is large);
      narrow  A and W x 2^4 in {-1, 0, 1}, bias integers in [-3, 3] x 2^-4: every result under 256 units of 2^-4, so no 16-bit output needs
              rounding and every 32-column sum of squares is exact in fp32 (asserted on the reference) - UV_EPI_BF16_SSQ's class; GELU
              runs on it too, because its pre-activations fall where GELU is not the identity.
    _exact_product asserts K max|a| max|w| + max|bias| < 2^24 units on the operands. Then bf16(acc + bias) must EQUAL the fp64 result rounded
    once, bit for bit - ties to even included -, and so must the f32 epilogues computed from it with the kernel's rounding points:
    float(y), x0 + float(y), x0 + (float(y) * g) as two f32 operations, the transposed y; out and ssq of UV_EPI_BF16_SSQ; split-K is
    bit-identical to the unsplit ping-pong kernel (tile_cfg 7) because its partial sums are exact too."""
    _need_cus(c)
    ci = CASES.index(c)
    epis = _epis(c)
    name = IDS[ci]
    M, N, K = c.M, c.N, c.K
    splitk = c.cfg in (19, 20)
    # ---- the wide class
    if set(epis) - {E_SSQ}:
        for lo in (-15, -7, 0):
            gen = torch.Generator(device=DEV).manual_seed(100000 * (c.dt == F16) + M * 31 + N * 7 + K + lo)
            A, W, B = _rand_int(gen, (M, K), lo, 15), _rand_int(gen, (N, K), lo, 15) / 16, _rand_int(gen, (N,), -15, 15) / 16
            if _variant(c) == 1:
                B = torch.zeros_like(B)
            acc = _exact_product(c, A, W, B)
            ties = _tie_share(acc, c.dt)
            if ties >= 0.01:
                break
        assert ties >= 0.01, f"only {ties:.4f} of the results are rounding ties"
        o = _operands(c, A, W, B, gen)
        y = acc.to(c.dt)
        yf = y.float()
        print(f"{name}: lo = {lo}, ties {ties:.4f}, max |y| {float(yf.abs().max())}")
        refs = {E_BF16: y, E_F32: yf, E_RESID: o.x0 + yf, E_T: y, E_GATE: o.x0 + (yf * _gate_rows(o))}
        for epi in epis:
            if epi == E_SSQ:
                continue
            got = _launch(c, epi, o)
            if epi == E_GELU:
                _check_gelu(c, got, y, f"{name} GELU (wide operands)")
            else:
                _assert_bits(got, refs[epi], f"{name} {EPI_NAME[epi]}")
            _agree(c, "wide", epi, got)
            if splitk:
                _assert_bits(got, _launch(c, epi, o, cfg=7), f"{name} {EPI_NAME[epi]}: split-K against tile_cfg 7")
    # ---- the narrow class
    if E_SSQ in epis or E_GELU in epis:
        gen = torch.Generator(device=DEV).manual_seed(7000000 + M * 31 + N * 7 + K)
        A, W, B = _rand_int(gen, (M, K), -1, 1), _rand_int(gen, (N, K), -1, 1) / 16, _rand_int(gen, (N,), -3, 3) / 16
        if _variant(c) == 1:
            B = torch.zeros_like(B)
        acc = _exact_product(c, A, W, B)
        units = float(acc.abs().max()) * 16
        assert units < 256, f"max |result| = {units} units of 2^-4: a 16-bit output would need rounding"
        assert 32 * units * units < 2 ** 24, "a 32-column sum of squares would not be exact in fp32"
        o = _operands(c, A, W, B, gen)
        y = acc.to(c.dt)
        assert torch.equal(y.float(), acc)
        if E_SSQ in epis:
            got, ssq = _launch(c, E_SSQ, o)
            _assert_bits(got, y, f"{name} BF16_SSQ out")
            _assert_bits(ssq, (acc.double() ** 2).view(M, N // 32, 32).sum(-1).float(), f"{name} BF16_SSQ ssq")
            _agree(c, "narrow", E_SSQ, (got, ssq))
        if E_GELU in epis:
            got = _launch(c, E_GELU, o)
            _check_gelu(c, got, y, f"{name} GELU (narrow operands)")
            _agree(c, "narrow", E_GELU, got)
    record_margin("gemm_kernels/designed_gelu_bit_identical_share", **{k: v[0] / v[1] for k, v in sorted(_GELU.items())})


@pytest.mark.parametrize("K", [384, 512])
def test_persistent_tile_walk_does_not_depend_on_gm(K):
    """The persistent kernel at 272 tiles (4 352 x 4 096: 17 row tiles, no multiple of any gm; more than one tile per workgroup at 256 CUs)
    under UV_OPT_GEMM_GM = 1, 2, 4, 8: every epilogue bit-identical to the automatic walk (which gate (a) ties to the fp64 reference)."""
    _lib = L()
    c = next(c for c in CASES if c.cfg == 17 and c.M == 4352 and c.K == K)
    gen = torch.Generator(device=DEV).manual_seed(K)
    A, W, B = _rand_int(gen, (c.M, K), -15, 15), _rand_int(gen, (c.N, K), -15, 15) / 16, _rand_int(gen, (c.N,), -15, 15) / 16
    o = _operands(c, A, W, B, gen)
    auto = {epi: _launch(c, epi, o) for epi in _epis(c)}
    try:
        for gm in (1, 2, 4, 8):
            _lib.set_option(_lib.OPT_GEMM_GM, gm)
            for epi, ref in auto.items():
                got = _launch(c, epi, o)
                for g, r in zip(got if epi == E_SSQ else (got,), ref if epi == E_SSQ else (ref,)):
                    _assert_bits(g, r, f"UV_OPT_GEMM_GM = {gm}, {EPI_NAME[epi]}")
    finally:
        _lib.reset_options()


# ---------------------------------------------------------------------------------------------------------------
# (b) random operands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gemm_kernel_on_random_operands(c):
    """Gates (b), (c): the normal operands of test_gemm_bf16_epilogues (a = randn / 2, w = randn / 20, bias = randn / 10) against the fp64
    product rounded to the 16-bit type, through assert_bf16_kernel: every element within 1 ulp (+ 2e-5 max|ref|); the residual epilogues
    within the same bound (x gate). The bit-identical share (0.999 for the plain epilogues and the residual ones, GELU 0.995) is asserted
    per case where the case has at least 20 000 results - below that one legitimate rounding flip is more than 0.001 of the case - and
    per kernel over all its cases in test_random_operand_shares_per_kernel."""
    _need_cus(c)
    ci = CASES.index(c)
    name = IDS[ci]
    M, N, K = c.M, c.N, c.K
    gen = torch.Generator(device=DEV).manual_seed(55000 + ci)
    A = (torch.randn(M, K, device=DEV, generator=gen) * 0.5).to(c.dt).float()
    W = (torch.randn(N, K, device=DEV, generator=gen) * 0.05).to(c.dt).float()
    B = (torch.randn(N, device=DEV, generator=gen) * 0.1).to(c.dt).float()
    o = _operands(c, A, W, B, gen)
    yb = (A.double() @ W.double().t() + o.B.double()).to(c.dt)
    yf = yb.float()
    big = M * N >= 20000
    floor = 2e-5 * yf.abs().max()
    ulp = bf16_ulp(yf) + floor
    tally = [0, 0]

    def count(same):
        tally[0] += int(same.sum())
        tally[1] += same.numel()

    for epi in _epis(c):
        res = _launch(c, epi, o)
        got = res[0] if epi == E_SSQ else res
        nm = f"{name} {EPI_NAME[epi]}"
        if epi in (E_BF16, E_F32, E_T, E_SSQ):
            assert_bf16_kernel(got, yb, min_exact=0.999 if big else 0.0, name=nm)
            count(got.float() == yf)
            if epi == E_SSQ:
                # the sums of squares are those of the kernel's OWN outputs, in fp32: 32 squares and 31 additions, each within 2^-24 relative
                want = (got.double() ** 2).view(M, N // 32, 32).sum(-1)
                assert bool(((res[1].double() - want).abs() <= 33 * 2.0 ** -24 * want).all()), f"{nm}: ssq"
        elif epi == E_GELU:
            ref = torch.nn.functional.gelu(yb, approximate="tanh")
            assert_bf16_kernel(got, ref, max_ulp=1.0, min_exact=0.995 if big else 0.0, name=nm, extra=1.2 * bf16_ulp(yf.cpu()))
        else:
            g = _gate_rows(o) if epi == E_GATE else None
            ref = o.x0 + yf * g if epi == E_GATE else o.x0 + yf
            d = (got - ref).abs()
            tol = ulp * g.abs() + 1e-6 if epi == E_GATE else ulp
            assert bool((d <= tol).all()), f"{nm}: max err {float(d.max()):.3e}"
            assert not big or float((d == 0).float().mean()) > 0.999, f"{nm}: only {float((d == 0).float().mean()):.5f} bit-identical"
            count(d == 0)
    for k in {s[0] for s in c.plan}:
        cur = _RANDOM.setdefault((k, c.dt == F16), [0, 0])
        cur[0] += tally[0]
        cur[1] += tally[1]
    print(f"{name}: {tally[0]} of {tally[1]} bit-identical")


def test_random_operand_shares_per_kernel():
    """The bit-identical share of gate (b) per kernel, over all the cases of this session that ran it (0.999, the bound of the per-case
    gate, at a sample size where it means something), recorded under gemm_kernels/."""
    shares = {f"{k}{'/f16' if f16 else ''}": v[0] / v[1] for (k, f16), v in sorted(_RANDOM.items())}
    record_margin("gemm_kernels/random_bit_identical_share", **shares)
    for k, s in shares.items():
        assert s >= 0.999, f"{k}: only {s:.5f} of the random-operand results are bit-identical to the rounded fp64 product"
    gelu = {k: v[0] / v[1] for k, v in sorted(_GELU.items())}
    for k, s in gelu.items():
        assert s >= 0.995, f"{k}: only {s:.5f} of the designed-operand GELU results are bit-identical to the rounded fp64 GELU"


# ---------------------------------------------------------------------------------------------------------------
# the table itself, the reference's rounding, the rejections
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_names_every_kernel():
    """The kernels the cases expect are exactly the reachable names of the library's table (kGemmKernelName next to enum GemmKernel): every
    GemmKernel, GK_DIAG once per tile_cfg of gemm_bf16_diag.hip, and for fp16 the five tile_cfg 0 can return. Every epilogue a kernel is
    built for runs on it; every kernel sees dense and wide buffers, a null bias, a null gate_tid and a gate_tid with repeated rows."""
    csrc = os.path.join(os.path.dirname(L().LIB_PATH), "csrc")
    src = open(os.path.join(csrc, "gemm_bf16.hip")).read()
    names = re.findall(r'"([^"]+)"', re.search(r"kGemmKernelName\[[^\]]*\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1))
    kinds = re.findall(r"\b(GK_\w+)\b", re.search(r"enum GemmKernel\s*\{(.*?)\};", src, flags=re.S).group(1))
    assert len(names) == len(kinds) == 9 and names[-1] == "DIAG" and kinds[-1] == "GK_DIAG"
    diag = re.findall(r"case (\d+):", open(os.path.join(csrc, "gemm_bf16_diag.hip")).read())
    reachable = set(names[:-1]) | {"DIAG" + d for d in diag}
    assert len(diag) == 7 and reachable == set(BUILT)
    assert {s[0] for c in CASES if c.dt == BF16 for s in c.plan} == reachable
    assert {s[0] for c in CASES if c.dt == F16 for s in c.plan} == F16_KERNELS
    assert any(c.dt == F16 and c.plan[0][0] == "T256" and (c.M, c.N, c.K) == (b.M, b.N, b.K) for c in CASES for b in CASES if b.plan[0][0] == "T256x192")
    for k in reachable:
        mine = [c for c in CASES if c.dt == BF16 and k in {s[0] for s in c.plan}]
        assert {e for c in mine for e in _epis(c)} == set(BUILT[k]), k
        assert {c.wide for c in mine} == {False, True}, k
        assert {_variant(c) for c in mine} == {0, 1, 2}, k
    for k in F16_KERNELS:
        mine = [c for c in CASES if c.dt == F16 and k in {s[0] for s in c.plan}]
        assert {e for c in mine for e in _epis(c)} == set(ALL7 - {E_SSQ}), k
    assert {c.wide for c in CASES if c.dt == F16} == {False, True}
    two = [c for c in CASES if len(c.plan) == 2]
    assert {c.cfg for c in two} == {0, 8, 9, 18} and all(_cu_dependent(c) for c in two)
    assert all(c.plan[0][2] + c.plan[1][2] == c.M and c.plan[1][1] == c.plan[0][2] for c in two)


def test_reference_rounding_is_nearest_even():
    """The reference's own rounding (f32 -> 16-bit through Tensor.to) is round-to-nearest-even on the device and on the CPU: exact ties of
    both formats, checked against hand-computed neighbours."""
    for dev in ("cpu", DEV):
        v = torch.tensor([257.0, 259.0, -257.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 258.5, 2.0 ** -7 * 257], device=dev)
        assert v.to(BF16).float().tolist() == [256.0, 260.0, -256.0, 1.0, 1 + 2.0 ** -6, 258.0, 2.0]
        assert _tie_share(v, BF16) == pytest.approx(6 / 7)
        v = torch.tensor([2049.0, 2051.0, -2049.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.5], device=dev)
        assert v.to(F16).float().tolist() == [2048.0, 2052.0, -2048.0, 1.0, 1 + 2.0 ** -9, 2050.0]
        assert _tie_share(v, F16) == pytest.approx(5 / 6)


def test_gemm_rejections():
    """Gate (e): what gemm_entry and the kernel families' own argument checks refuse raises UnividHipError before any launch and leaves a
    sentinel-filled output (and ssq) untouched."""
    _lib = L()
    M, N, K = 512, 512, 256
    a = torch.zeros(M + 8, 1024 + 16, dtype=BF16, device=DEV)
    w = torch.zeros(N + 8, 1024 + 16, dtype=BF16, device=DEV)
    out = torch.full((M + 8, N + 8), SENT, dtype=BF16, device=DEV)
    o32 = torch.full((M + 8, N + 8), SENT, dtype=F32, device=DEV)
    ssq = torch.full((M + 8, N // 32), SENT, dtype=F32, device=DEV)
    ws = torch.empty(4096 + 4 * 4 * 262144, dtype=torch.uint8, device=DEV)

    def refused(match, M=M, N=N, K=K, lda=K + 16, ldw=K + 16, ldo=N + 8, epi=E_BF16, cfg=0, o=out, aoff=0, gate=None, ws=None, f16=False):
        A = torch.as_strided(a.view(F16) if f16 else a, (M, K), (lda, 1), aoff)
        W = torch.as_strided(w.view(F16) if f16 else w, (N, K), (ldw, 1))
        O = torch.as_strided(o.view(F16) if f16 else o, (M, N), (ldo, 1))
        with pytest.raises(_lib.UnividHipError, match=match):
            if epi == E_SSQ:
                _lib.gemm_bf16_ssq(A, W, None, O, ssq, M=M, tile_cfg=cfg)
            else:
                _lib.gemm_bf16(A, W, None, O, epi, M=M, gate=gate, tile_cfg=cfg, ws=ws)

    refused("multiple of 64", K=224)
    refused("multiple of 16", N=504)
    refused("lda/ldw", lda=K + 4)
    refused("lda/ldw", ldw=K + 12)
    refused("16-byte aligned", aoff=4)
    refused("ldo must be", ldo=N + 2)
    refused("gate table", epi=E_GATE, o=o32)
    refused("gate table", epi=E_GATE, o=o32, gate=torch.zeros(1, N + 2, device=DEV)[:, :N])
    refused("needs N % 32", epi=E_SSQ, N=496)
    refused("needs N % 32", epi=E_SSQ, ldo=N + 4)
    refused("32-column groups", epi=E_SSQ, cfg=6)
    refused("32-column groups", epi=E_SSQ, cfg=4)
    refused("unknown tile_cfg 15", cfg=15)
    refused("unknown epilogue 9", epi=9)
    refused("tile_cfg 7 needs", cfg=7, K=192)
    refused("tile_cfg 14 needs", cfg=14, K=192)
    refused("tile_cfg 14 needs", cfg=14, K=128)
    refused("tile_cfg 17 needs", cfg=17, K=256)
    refused("whole 256x256 tiles", cfg=17, M=500, K=384)
    refused("whole 256x256 tiles", cfg=17, N=496, K=384)
    refused("16 bytes per lane", cfg=17, K=384, ldo=N + 4)
    refused("16 bytes per lane", cfg=17, K=384, ldo=N + 4, epi=E_T)
    refused("too few tiles", cfg=17, M=256, N=256, K=384)
    refused("split-K 4 needs", cfg=19, K=512, ws=ws)
    refused("split-K 2 needs", cfg=20, K=256, ws=ws)
    refused("workspace of", cfg=19, K=1024)
    refused("workspace of", cfg=19, K=1024, ws=ws[:4096 + 15 * 262144])
    refused("not 1", cfg=19, K=1024, epi=E_GELU, ws=ws)
    refused("not 5", cfg=20, K=1024, epi=E_T, ws=ws)
    refused("only tile_cfg 0", cfg=7, f16=True)
    torch.cuda.synchronize()
    for buf in (out, o32, ssq):
        assert bool((buf == SENT).all()), "a rejected call wrote to its output"
