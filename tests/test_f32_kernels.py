"""GPU (-m gpu): the fp32 pieces of the hot path that had only coarse gates - the f32 MFMA GEMM uv_gemm_f32_nt (csrc/gemm_f32.hip: the DiT
head, every 1x1 convolution of the VAE, the three products of the VAE attention block), _Engine.attention (wan/vae2_2.py) with its
n4 = round_up(H W, 4) padding, and the four sampler kernels (csrc/sampler.hip) past one pass of their 2048 x 256 grid.

1. uv_gemm_f32_nt, ONE case table (CASES), called through the C ABI with raw pointers:
  (a) designed operands (A integers in [-8, 8] x 2^-3, W integers in [-8, 8] x 2^-2, bias / residual multiples of 2^-5 below 64): every
      product and every partial sum in any order is exact in fp32, so the output must EQUAL the fp64 reference;
  (b) random normal operands: |err| <= (K + 2) eps (|a| |w|^T + |bias| + |resid|), eps = 2^-24, per element - K products and K + 1
      additions in any order;
  (c) random operands, K >= 64 and M N >= 4096: the rms error against fp64 is at most 1.25 x that of a sequential fp32 emulation on the
      CPU (seq_emulation), which performs at least as many roundings as the kernel; both and their ratio are recorded;
  (d) sentinels: the output has 8 slack rows (and slack columns where wide), pre-filled with SENT, all intact afterwards; slack columns
      of A, W and the residual hold 3e38, rows of A behind M and of W behind N hold NaN; the written region is finite;
  (e) the first 17 rows of an M = 129 result equal an M = 17 call on the same rows bit for bit;
  (f) what the entry refuses raises UnividHipError with its message and leaves the output untouched.
2. _Engine.attention against the same block in fp64 on the CPU (attention_reference, written from oracle.wan_vae), at n = H W with
   n4 - n = 2, 3, 1, 0, 0, 1: elementwise rtol 1e-3 / atol 1e-4, rms error <= 2 x the fp32 block with seq_emulation products, and a
   frame submitted alone (T = 1) gives the bits it has inside a T = 2 call.
3. The sampler kernels at n = 1 ... 1 048 653 (one lane, partial blocks, exactly the grid, one element into the second pass, a third
   partial pass), bit-exact against the reference's fp32 torch expressions, 64 sentinels behind n.

The CPU-side helpers (the case table's coverage, seq_emulation, the designed-operand generator with its exactness for every K of the
table under a random summation order, attention_reference against oracle.wan_vae.WanVAE._attn, the sampler expressions against
oracle.unipc / oracle.dpmpp) are checked without a GPU by `python tests/test_f32_kernels.py`.
"""
import math
from collections import namedtuple

import pytest
import torch

from conftest import record_margin
from test_glue_kernels import _assert_bits, _call, _gen, _reject, _sent
from test_gpu_parity import _small_vae, assert_f32_close

pytestmark = pytest.mark.gpu

F32 = torch.float32
F64 = torch.float64
DEV = "cuda"
EPS = 2.0 ** -24
SENT = -7.25
HUGE = 3e38
NAN = float("nan")


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


# ---------------------------------------------------------------------------------------------------------------
# 1. uv_gemm_f32_nt: the case table
# ---------------------------------------------------------------------------------------------------------------
# kind: "table" (own buffers; wide: lda = K + 4, ldw = K + 8, ldo = N + 4), "score" (A and W are column slices of one [n4, 3C] buffer,
# M = n rows of A, N = n4, ldo = n4), "pv" (A [n, n4], W [C, n4], tight), "head" (33 x 192 x 3072, tight). resid: ldr = N + 8
Case = namedtuple("Case", "kind M N K bias resid wide")

MS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)           # around the 16-row fragment, the 64-row wave, the 128-row tile
NS = (4, 12, 16, 60, 64, 68, 124, 128, 132, 260, 388)
KS = (4, 28, 32, 36, 60, 64, 68, 100, 3072)                    # below / at / above one 32-float stage; 1, 2, 3 stages; the head's depth
EDGE_M, EDGE_N = (127, 128, 129), (124, 128, 132)
CASES = []


def _c(M, N, K, kind="table", **over):
    """Options by position in the table: wide on alternate cases, bias absent on every third, a residual on two of every five - periods
    2, 3 and 5, so that every option meets every K-tail class (test_case_table_covers_the_axes)."""
    i = len(CASES)
    if K == 3072 and (M > 129 or N > 192):                     # the head's depth only at the head's size
        K = 100
    o = dict(bias=i % 3 != 1, resid=i % 5 in (0, 3), wide=kind == "table" and i % 2 == 1)
    o.update(over)
    CASES.append(Case(kind, M, N, K, **o))


# a Latin-square selection: M_i with N_(i + 4t) and K_(i + 3t), t = 0, 1, 2 - every value of each axis at least three times
for _i, _m in enumerate(MS):
    for _t in range(3):
        _c(_m, NS[(_i + 4 * _t) % 11], KS[(_i + 3 * _t) % 9])
# every (M edge, N edge) pair of the tile boundary the selection left out, each with another K
for _a, _m in enumerate(EDGE_M):
    for _b, _n in enumerate(EDGE_N):
        if not any((c.M, c.N) == (_m, _n) for c in CASES):
            _c(_m, _n, KS[(3 * _a + _b + 1) % 9])
_c(129, 388, 64)                                               # tiles_m = 2, tiles_n = 4
_c(300, 132, 36)                                               # tiles_m = 3, tiles_n = 2
# the production layouts: the attention block's score and P V products at n = 143 (n4 = 144) and n = 6 (n4 = 8), C = 128; the DiT head
for _n in (143, 6):
    _n4 = (_n + 3) // 4 * 4
    _c(_n, _n4, 128, kind="score", bias=False, resid=False)
    _c(_n, 128, _n4, kind="pv", bias=False, resid=False)
_c(33, 192, 3072, kind="head", bias=True, resid=False)

IDS = [f"{i:02d}-{c.kind}-{c.M}x{c.N}x{c.K}" + ("-bias" if c.bias else "") + ("-resid" if c.resid else "") + ("-wide" if c.wide else "")
       for i, c in enumerate(CASES)]


def _ktail(K):
    """K-tail class: the live 4-float chunks of the last 32-float stage - all 8 (K % 32 = 0), one (4), all but one (28)."""
    return K % 32


def check_case_table():
    table = [c for c in CASES if c.kind == "table"]
    assert {c.M for c in table} == set(MS) and {c.N for c in table} == set(NS) and {c.K for c in table} == set(KS)
    assert {(c.M, c.N) for c in table} >= {(m, n) for m in EDGE_M for n in EDGE_N}
    assert {(129, 388, 64), (300, 132, 36)} <= {(c.M, c.N, c.K) for c in table}
    assert all(c.M <= 129 and c.N <= 192 for c in CASES if c.K == 3072)
    assert {c.kind for c in CASES} == {"table", "score", "pv", "head"}
    assert {_ktail(c.K) for c in table} == {0, 4, 28}
    for opt in ("bias", "resid", "wide"):
        for val in (False, True):
            seen = {_ktail(c.K) for c in table if getattr(c, opt) == val}
            assert seen == {0, 4, 28}, f"{opt} = {val} meets only the K-tail classes {sorted(seen)}"
    assert {(c.bias, c.resid) for c in table} == {(False, False), (False, True), (True, False), (True, True)}
    assert len(CASES) <= 60


def test_case_table_covers_the_axes():
    """Every M, N and K of the axes MS, NS and KS, every pair of {127, 128, 129} x {124, 128, 132}, both tiles_m != tiles_n cases, K = 3072
    only at M <= 129 and N <= 192, the production layouts, and every option (bias, residual, wide) present and absent at every K-tail
    class (K % 32 = 0, 4, 28)."""
    check_case_table()


# ---------------------------------------------------------------------------------------------------------------
# CPU-side helpers: operands and references
# ---------------------------------------------------------------------------------------------------------------
def seq_emulation(a, w, bias=None, resid=None):
    """a w^T (+ bias) (+ resid) in fp32 on the CPU, one k at a time in order: acc = acc + a[:, k] * w[:, k], every product and every
    addition rounded to fp32 on its own (no FMA), bias and residual added last."""
    a, wt = a.float(), w.float().t().contiguous()
    acc = torch.zeros(a.shape[0], wt.shape[1], dtype=F32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * wt[k]
    if bias is not None:
        acc = acc + bias.float()
    if resid is not None:
        acc = acc + resid.float()
    return acc


def exact_mm(a, w, bias=None, resid=None):
    """The same product in the operands' own precision through torch.matmul (fp64 operands: the reference)."""
    y = a @ w.t()
    if bias is not None:
        y = y + bias
    if resid is not None:
        y = y + resid
    return y


def designed_operands(M, N, K, gen):
    """A [M, K] integers in [-8, 8] x 2^-3, W [N, K] integers in [-8, 8] x 2^-2, bias [N] and residual [M, N] integers in [-2047, 2047] x
    2^-5, drawn per element: a dropped, duplicated or misplaced k-slot changes the sum."""
    A = torch.randint(-8, 9, (M, K), generator=gen).float() / 8
    W = torch.randint(-8, 9, (N, K), generator=gen).float() / 4
    B = torch.randint(-2047, 2048, (N,), generator=gen).float() / 32
    R = torch.randint(-2047, 2048, (M, N), generator=gen).float() / 32
    return A, W, B, R


def exact_reference(A, W, B=None, R=None):
    """fp64 A W^T + B + R of designed operands as an fp32 tensor, with the condition under which any summation order reproduces it
    asserted: in units of 2^-5 every product is an integer, and K max|a| max|w| + max|B| + max|R| stays below 2^24."""
    units = A.shape[1] * float(A.abs().max()) * float(W.abs().max()) * 32
    for t in (B, R):
        if t is not None:
            units += float(t.abs().max()) * 32
            assert torch.equal(t * 32, (t * 32).round())
    assert torch.equal(A * 8, (A * 8).round()) and torch.equal(W * 4, (W * 4).round())
    assert units < 2 ** 24, f"{units} units of 2^-5"
    ref = exact_mm(A.double(), W.double(), None if B is None else B.double(), None if R is None else R.double())
    assert torch.equal(ref.float().double(), ref), "the fp64 reference is not an fp32 number"
    return ref.float()


def random_order_sum(A, W, B, R, gen):
    """fp32 sum of the K products, the bias and the residual of every output in ONE random order (the same for all outputs)."""
    K = A.shape[1]
    terms = [("k", k) for k in range(K)] + [("b", 0), ("r", 0)]
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=F32)
    for i in torch.randperm(len(terms), generator=gen).tolist():
        kind, k = terms[i]
        acc = acc + (A[:, k:k + 1] * W[:, k] if kind == "k" else B if kind == "b" else R)
    return acc


def attention_reference(x, gamma, wqkv, bqkv, wproj, bproj, mm=exact_mm):
    """AttentionBlock.forward (oracle.wan_vae.WanVAE._attn) on channels-last frames x [T, H, W, C] in x's dtype: rms_norm, the 1x1 to_qkv,
    softmax(q k^T / sqrt(C)) v, proj, + x. mm(a, w, bias, resid) = a w^T + bias + resid: torch.matmul (fp64: the reference) or
    seq_emulation (fp32: the yardstick of the rms gate)."""
    from oracle import wan_vae
    T, H, W, C = x.shape
    out = torch.empty_like(x)
    for t in range(T):
        rows = x[t].reshape(H * W, C)
        y = wan_vae.rms_norm(rows, gamma.view(1, C))
        qkv = mm(y, wqkv, bqkv)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        p = torch.softmax(mm(q, k) * (1.0 / math.sqrt(C)), dim=-1)
        o = mm(p, v.t().contiguous())
        out[t] = mm(o, wproj, bproj, rows).reshape(H, W, C)
    return out


def attention_weights(C, seed):
    """gamma, to_qkv, proj of one block: q and k entries ~ N(0, 1.5^2), so the logits q k / sqrt(C) have a spread of about 2 and the
    softmax is not flat (asserted where it is used)."""
    g = _gen(seed)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    wqkv = torch.randn(3 * C, C, generator=g) * (1.5 / math.sqrt(C))
    bqkv = torch.randn(3 * C, generator=g) * 0.3
    wproj = torch.randn(C, C, generator=g) / math.sqrt(C)
    bproj = torch.randn(C, generator=g) * 0.3
    return gamma, wqkv, bqkv, wproj, bproj


def _s(v):
    """a coefficient as the reference holds it: a 0-dim fp32 CPU tensor"""
    return torch.tensor(float(v), dtype=F32)


def ref_cfg_convert(cond, uncond, sample, gs, sigma):
    """textimage2video.py:385-386 and convert_model_output (oracle.unipc.FlowUniPC.step): (noise_pred, x0)."""
    noise_pred = uncond + _s(gs) * (cond - uncond)
    return noise_pred, sample - _s(sigma) * noise_pred


def ref_unipc_predictor(x, m0, m_prev, r, c1, c2, rk, order):
    """oracle.unipc.FlowUniPC._predict with the coefficients given (r = sigma_t / sigma_s0, c1 = alpha_t h_phi_1, c2 = alpha_t B_h)."""
    from oracle import unipc as ou
    x_t_ = _s(r) * x - _s(c1) * m0
    if order == 2:
        d1s = torch.stack([(m_prev - m0) / _s(rk)], dim=1)
        pred_res = ou._einsum_ac(torch.tensor([0.5], dtype=x.dtype), d1s)
    else:
        return x_t_            # pred_res = 0: x_t_ - c2 * 0 is x_t_ (an x_t_ of -0.0 aside)
    return x_t_ - _s(c2) * pred_res


def ref_unipc_corrector(x_last, m0, m_prev, model_t, r, c1, c2, rho0, rho_last, rk, order):
    """oracle.unipc.FlowUniPC._correct with the coefficients given."""
    from oracle import unipc as ou
    x_t_ = _s(r) * x_last - _s(c1) * m0
    if order == 2:
        d1s = torch.stack([(m_prev - m0) / _s(rk)], dim=1)
        corr_res = ou._einsum_ac(_s(rho0).view(1), d1s)
    else:
        corr_res = 0
    return x_t_ - _s(c2) * (corr_res + _s(rho_last) * (model_t - m0))


def ref_dpmpp_update(x, m0, m1, r, c, inv_r0, order):
    """oracle.dpmpp.FlowDPMpp._first / _second with the coefficients given (r = sigma_t / sigma_s0, c = alpha_t (exp(-h) - 1),
    inv_r0 = 1 / r0)."""
    if order == 1:
        return _s(r) * x - _s(c) * m0
    d1 = _s(inv_r0) * (m0 - m1)
    return _s(r) * x - _s(c) * m0 - 0.5 * _s(c) * d1


def unipc_real_coefficients(si, which, order):
    """The coefficients FlowUniPCMultistepScheduler (10 steps, shift 5) hands to the kernels at step index si, as python floats:
    which = 'p' -> (r, c1, c2, rk), 'c' -> (r, c1, c2, rho0, rho_last, rk), 's' -> sigma."""
    from univid_amd.wan.fm_solvers_unipc import FlowUniPCMultistepScheduler
    s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
    s.set_timesteps(10, device="cpu", shift=5.0)
    if which == "s":
        return s.sigmas[si].item()
    if which == "p":
        c = s._coeffs(si + 1, si, order, [si - i for i in range(1, order)])
        return c["r"], c["c1"], c["c2"], c["rk"]
    c = s._coeffs(si, si - 1, order, [si - (i + 1) for i in range(1, order)])
    if order == 1:
        rho0, rho_last = 0.0, 0.5
    else:
        rhos = torch.linalg.solve(c["R"], c["b"]).to(F32)
        rho0, rho_last = rhos[0].item(), rhos[-1].item()
    return c["r"], c["c1"], c["c2"], rho0, rho_last, c["rk"]


def _oracle_unipc(si, m_prev, m0):
    from oracle import unipc as ou
    o = ou.FlowUniPC(1000, shift=1)
    o.set_timesteps(10, shift=5.0)
    o.step_index, o.model_outputs = si, [m_prev, m0]
    return o


# ---------------------------------------------------------------------------------------------------------------
# uv_gemm_f32_nt: buffers and the launch
# ---------------------------------------------------------------------------------------------------------------
def _padded(t, ld):
    """t [R, C] (CPU) -> the first R rows / C columns of a [R + 8, ld] device buffer: slack columns 3e38, the 8 rows behind NaN"""
    R, C = t.shape
    buf = torch.full((R + 8, ld), HUGE, dtype=F32)
    buf[R:] = NAN
    buf[:R, :C] = t
    return buf.to(DEV)[:R, :C]


def _launch(c, A, W, B, R, M=None, name=""):
    """One uv_gemm_f32_nt call in the case's memory layout on the first M rows of A (default all). Asserts gate (d). Returns the dense
    [M, N] result on the CPU."""
    N, K = c.N, c.K
    M = c.M if M is None else M
    if c.kind == "score":             # one [n4, 3C] buffer: q columns | k columns | v columns (never read: huge)
        n, n4, C = c.M, c.N, c.K
        buf = torch.full((n4 + 8, 3 * C), HUGE, dtype=F32)
        buf[n4:] = NAN
        buf[n:n4, :C] = NAN
        buf[:n, :C] = A
        buf[:n4, C:2 * C] = W
        buf = buf.to(DEV)
        a, w = buf[:, :C], buf[:, C:2 * C]
    else:
        a, w = _padded(A, K + 4 if c.wide else K), _padded(W, K + 8 if c.wide else K)
    ldo = N + 4 if c.wide else N
    out = _sent(c.M + 8, ldo)
    bias = resid = None
    if c.bias:
        bias = torch.cat([B, torch.full((8,), NAN)]).to(DEV)
    if c.resid:
        resid = _padded(R, N + 8)
    _call("uv_gemm_f32_nt", a, a.stride(0), w, w.stride(0), bias, M, N, K, out, ldo, resid, 0 if resid is None else resid.stride(0))
    torch.cuda.synchronize()
    out = out.cpu()
    stray = int((out != SENT).sum()) - int((out[:M, :N] != SENT).sum())
    assert stray == 0, f"{name}: {stray} elements outside the [{M}, {N}] result were written (buffer {tuple(out.shape)})"
    got = out[:M, :N]
    assert not bool((got == SENT).all()), f"{name}: nothing was written"
    assert bool(torch.isfinite(got).all()), f"{name}: NaN or inf in the result (a slack column or a row behind M / N was read)"
    return got


def _opts(c, B, R):
    return (B if c.bias else None), (R if c.resid else None)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gemm_f32_is_bit_exact_on_designed_operands(c):
    """Gates (a), (d). A integers in [-8, 8] x 2^-3, W integers in [-8, 8] x 2^-2, bias and residual integers in [-2047, 2047] x 2^-5: in
    units of 2^-5 every product is an integer of magnitude <= 64 and every partial sum in any order stays below K 64 + 4094 <= 200 702 <
    2^24 (exact_reference asserts it on the operands), so the kernel's permuted summation, its zero-page K tail and its epilogue must
    reproduce the fp64 result exactly - torch.equal, no tolerance."""
    name = IDS[CASES.index(c)]
    A, W, B, R = designed_operands(c.M, c.N, c.K, _gen(1000 + CASES.index(c)))
    B, R = _opts(c, B, R)
    ref = exact_reference(A, W, B, R)
    got = _launch(c, A, W, B, R, name=name)
    if not torch.equal(got, ref):
        bad = got != ref
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact product; first at (row, column) {i}: "
                             f"got {got[i].item()!r}, expected {ref[i].item()!r}")


_WORST = {"ratio": 0.0, "err_over_bound": 0.0}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gemm_f32_on_random_operands(c):
    """Gates (b), (c), (d). a ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias and residual ~ N(0, 1).
    (b) per element |err| <= (K + 2) eps (|a| |w|^T + |bias| + |resid|) against fp64: K products and K + 1 additions in any order.
    (c) K >= 64 and M N >= 4096: rms error <= 1.25 x the rms error of seq_emulation (the sequential fp32 sum on the CPU: at least as many
    roundings as the kernel, whose exact products are summed in a permuted order; the rms over >= 4096 outputs spreads by about 1 %).
    Recorded under f32/gemm_rms/<case>."""
    ci = CASES.index(c)
    name = IDS[ci]
    M, N, K = c.M, c.N, c.K
    g = _gen(5000 + ci)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    B, R = _opts(c, torch.randn(N, generator=g), torch.randn(M, N, generator=g))
    got = _launch(c, A, W, B, R, name=name)
    dB, dR = (None if B is None else B.double()), (None if R is None else R.double())
    ref = exact_mm(A.double(), W.double(), dB, dR)
    mag = exact_mm(A.double().abs(), W.double().abs(), None if B is None else dB.abs(), None if R is None else dR.abs())
    err = (got.double() - ref).abs()
    worst = float((err / ((K + 2) * EPS * mag)).max())
    _WORST["err_over_bound"] = max(_WORST["err_over_bound"], worst)
    print(f"{name}: max |err| / bound = {worst:.4f}")
    assert bool((err <= (K + 2) * EPS * mag).all()), f"{name}: max |err| / ((K + 2) eps (|a||w|^T + |bias| + |resid|)) = {worst:.3f}"
    if K >= 64 and M * N >= 4096:
        rms = float(err.pow(2).mean().sqrt())
        emu = float((seq_emulation(A, W, B, R).double() - ref).pow(2).mean().sqrt())
        _WORST["ratio"] = max(_WORST["ratio"], rms / emu)
        print(f"{name}: rms error {rms:.4e}, sequential fp32 emulation {emu:.4e}, ratio {rms / emu:.4f}")
        record_margin(f"f32/gemm_rms/{name}", kernel_rms_err=rms, emulation_rms_err=emu, ratio=rms / emu)
        assert rms <= 1.25 * emu, f"{name}: rms error {rms:.4e} > 1.25 x {emu:.4e} (the sequential fp32 emulation)"
    record_margin("f32/gemm_random", max_err_over_bound=_WORST["err_over_bound"], max_rms_ratio=_WORST["ratio"])


def test_gemm_f32_rows_do_not_depend_on_the_launch():
    """Gate (e): the first 17 rows of the M = 129 result of (129, 388, 64) equal, bit for bit, an M = 17 call on the same rows (random
    operands, bias and residual given): a row's value depends neither on the row tiles beside it nor on the clamped loads behind M."""
    c = Case("table", 129, 388, 64, True, True, True)
    g = _gen(77)
    A, W = torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g) / 8
    B, R = torch.randn(c.N, generator=g), torch.randn(c.M, c.N, generator=g)
    full = _launch(c, A, W, B, R, name="M = 129")
    part = _launch(c, A, W, B, R, M=17, name="M = 17")
    _assert_bits(part, full[:17], "M = 17 against the first 17 rows of M = 129")


def test_gemm_f32_rejections():
    """Gate (f): K % 4, N % 4, any ld % 4, a pointer one float off (A, W, out, bias, residual), M = 0 and a null A are refused by the C
    entry with its message, and the sentinel-filled output is untouched."""
    M, N, K = 16, 16, 32
    a, w = torch.zeros(M + 1, K + 8, device=DEV), torch.zeros(N + 1, K + 8, device=DEV)
    bias, resid = torch.zeros(N + 8, device=DEV), torch.zeros(M + 1, N + 8, device=DEV)
    out = _sent(M + 8, N + 8)

    def refused(match, M=M, N=N, K=K, lda=K + 8, ldw=K + 8, ldo=N + 8, ldr=N + 8, A=a, W=w, O=out, B=bias, R=resid):
        _reject(match, "uv_gemm_f32_nt", A, lda, W, ldw, B, M, N, K, O, ldo, R, ldr)

    refused("K and N must be multiples of 4", K=30)
    refused("K and N must be multiples of 4", N=14)
    refused("must be multiples of 4", lda=K + 2)
    refused("must be multiples of 4", ldw=K + 6)
    refused("must be multiples of 4", ldo=N + 2)
    refused("must be multiples of 4", ldr=N + 1)
    refused("16-byte aligned", A=a.view(-1)[1:])
    refused("16-byte aligned", W=w.view(-1)[1:])
    refused("16-byte aligned", O=out.view(-1)[1:])
    refused("16-byte aligned", B=bias[1:])
    refused("16-byte aligned", R=resid.view(-1)[1:])
    refused("bad shape", M=0)
    refused("null pointer", A=None)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a rejected call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------
# 2. the VAE attention block
# ---------------------------------------------------------------------------------------------------------------
# (H, W, C): n = 6, 9, 15, 16, 132, 143 -> n4 - n = 2, 3, 1, 0, 0, 1 (132 and 143 cross the 128-row tile) at the small model's width;
# C = 1024 (the production decoder's) at (13, 11)
ATTN_CASES = [(2, 3, 128), (3, 3, 128), (5, 3, 128), (4, 4, 128), (12, 11, 128), (13, 11, 128), (13, 11, 1024)]
_ENGINES = {}


def _attention_engine(C):
    """(engine in precision 'fp32', AttentionBlock of width C with attention_weights(C)). C = the small model's width: the mid-block of
    the small WanVAE_'s decoder, through WanVAE_.prepare. C = 1024: a whole WanVAE_ of that width is hundreds of millions of
    parameters, so the engine is built over a bare AttentionBlock(1024) - _Engine collects the convolutions of whatever module it is
    given."""
    if C not in _ENGINES:
        from univid_amd.wan import vae2_2
        wts = attention_weights(C, 40 + C)
        if C == 128:
            m, _ = _small_vae(0)
            blk = m.decoder.middle[1]
            assert isinstance(blk, vae2_2.AttentionBlock) and blk.dim == C
        else:
            m = blk = vae2_2.AttentionBlock(C).to(DEV).eval()
        with torch.no_grad():
            for p, v in zip((blk.norm.gamma, blk.to_qkv.weight, blk.to_qkv.bias, blk.proj.weight, blk.proj.bias), wts):
                p.copy_(v.view(p.shape))
        eng = m.prepare("fp32")._engine if C == 128 else vae2_2._Engine(m, "fp32")
        assert eng.precision == "fp32"
        _ENGINES[C] = (eng, blk, wts)
    return _ENGINES[C]


@pytest.mark.parametrize("H,W,C", ATTN_CASES, ids=[f"{h}x{w}-C{c}" for h, w, c in ATTN_CASES])
def test_vae_attention_block(H, W, C):
    """_Engine.attention(blk, x [2, H, W, C]), x ~ 3 N(0, 1), against attention_reference in fp64:
      * every element within the fp32 path's contract rtol 1e-3 / atol 1e-4;
      * rms error <= 2 x the rms error of the same block in fp32 on the CPU with its three products by seq_emulation (the margin of 2
        covers three chained stages and the softmax between them); both recorded under f32/attention/<case>;
      * each frame submitted alone (T = 1) gives, bit for bit, what it has inside the T = 2 call: the reused pad rows of xn and the
        per-frame buffers carry nothing over.
    The softmax is not flat: the largest probability of a row averages more than 2 / n (asserted on the reference's logits)."""
    eng, blk, wts = _attention_engine(C)
    n = H * W
    x = 3.0 * torch.randn(2, H, W, C, generator=_gen(100 * n + C))
    ref = attention_reference(x.double(), *[t.double() for t in wts])
    with torch.no_grad():
        xd = x.to(DEV)
        got = eng.attention(blk, xd)
        alone = [eng.attention(blk, xd[t:t + 1].contiguous()) for t in range(2)]
    torch.cuda.synchronize()
    got = got.cpu()
    # the reference's own softmax, to show the case is not a flat average
    rows = x[0].reshape(n, C).double()
    from oracle import wan_vae
    qkv = exact_mm(wan_vae.rms_norm(rows, wts[0].double().view(1, C)), wts[1].double(), wts[2].double())
    peak = float(torch.softmax(qkv[:, :C] @ qkv[:, C:2 * C].t() / math.sqrt(C), -1).max(-1).values.mean())
    assert peak > min(0.9, 2.0 / n), f"flat softmax: mean row maximum {peak:.4f} at n = {n}"
    assert_f32_close(got, ref, rtol=1e-3, atol=1e-4, name=f"attention {H}x{W} C{C}")
    emu = attention_reference(x, *wts, mm=seq_emulation)
    rms = float((got.double() - ref).pow(2).mean().sqrt())
    rms_emu = float((emu.double() - ref).pow(2).mean().sqrt())
    print(f"attention {H}x{W} C{C}: rms error {rms:.4e}, fp32 CPU block {rms_emu:.4e}, ratio {rms / rms_emu:.4f}, softmax peak {peak:.3f}")
    record_margin(f"f32/attention/{H}x{W}-C{C}", kernel_rms_err=rms, emulation_rms_err=rms_emu, ratio=rms / rms_emu,
                  max_abs_err=float((got.double() - ref).abs().max()), softmax_mean_row_max=peak)
    assert rms <= 2.0 * rms_emu, f"rms error {rms:.4e} > 2 x {rms_emu:.4e} (the fp32 block on the CPU)"
    for t in range(2):
        _assert_bits(alone[t][0], got[t], f"frame {t} alone against frame {t} of the T = 2 call")


# ---------------------------------------------------------------------------------------------------------------
# 3. the sampler kernels past one grid pass
# ---------------------------------------------------------------------------------------------------------------
# one lane; a partial block; a whole block and one lane; exactly the 2048 x 256 grid; one element into the second pass; a third, partial pass
SAMPLER_N = [1, 255, 257, 524288, 524289, 1048653]
SLACK = 64


def _latents(n, k, seed):
    """k random fp32 latents of n elements (CPU), shaped [1, n] as the reference's expressions expect a batch axis"""
    g = _gen(seed)
    return [torch.randn(1, n, generator=g) for _ in range(k)]


def _coefs(k, seed):
    """k random fp32 coefficients of magnitude about 1 (0.5 ... 1.5, either sign), as python floats: every product rounds"""
    g = _gen(seed)
    v = (0.5 + torch.rand(k, generator=g)) * (torch.randint(0, 2, (k,), generator=g).float() * 2 - 1)
    return [x.item() for x in v]


def _dev(t):
    return t.reshape(-1).to(DEV)


def _check_out(buf, n, ref, name):
    buf = buf.cpu()
    assert bool((buf[n:] == SENT).all()), f"{name}: the {SLACK} elements behind n = {n} were written"
    _assert_bits(buf[:n], ref.reshape(-1), name)


@pytest.mark.parametrize("with_np", [False, True], ids=["x0", "x0+noise_pred"])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_cfg_convert_past_one_grid_pass(n, with_np):
    """uv_cfg_convert at random guide_scale / sigma, noise_pred None and present, bit-exact against ref_cfg_convert; then the
    guide_scale = 0, cond is uncond form that step() uses: x0 equals sample - sigma * model_output bit for bit. (On a -0.0 / -0.0 pair
    u + 0 * (c - u) is +0.0 by construction, where model_output itself is -0.0: the sign of a zero x0 term may then differ. The inputs
    here are random normals without signed zeros; that pair is not gated.)"""
    cond, uncond, sample = _latents(n, 3, n)
    gs, sigma = _coefs(2, n + 1)
    ref_np, ref_x0 = ref_cfg_convert(cond, uncond, sample, gs, sigma)
    x0 = _sent(n + SLACK)
    npred = _sent(n + SLACK) if with_np else None
    _call("uv_cfg_convert", _dev(cond), _dev(uncond), _dev(sample), gs, sigma, npred, x0, n)
    torch.cuda.synchronize()
    _check_out(x0, n, ref_x0, f"cfg_convert x0, n = {n}")
    if with_np:
        _check_out(npred, n, ref_np, f"cfg_convert noise_pred, n = {n}")
    assert not bool((cond == 0).any() | (sample == 0).any())
    x0 = _sent(n + SLACK)
    c = _dev(cond)
    _call("uv_cfg_convert", c, c, _dev(sample), 0.0, sigma, None, x0, n)
    torch.cuda.synchronize()
    _check_out(x0, n, sample - _s(sigma) * cond, f"cfg_convert as step() calls it, n = {n}")


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_unipc_corrector_past_one_grid_pass(n, order):
    """uv_unipc_corrector at six random coefficients of magnitude about 1 (every product rounds), order 1 (no history pointer) and 2,
    bit-exact against ref_unipc_corrector (oracle.unipc.FlowUniPC._correct's expression); the 64 elements behind n stay SENT."""
    x_last, m0, m_prev, model_t = _latents(n, 4, 2 * n + order)
    co = _coefs(6, n + order)
    out = _sent(n + SLACK)
    _call("uv_unipc_corrector", _dev(x_last), _dev(m0), _dev(m_prev) if order == 2 else None, _dev(model_t), out, *co, order, n)
    torch.cuda.synchronize()
    _check_out(out, n, ref_unipc_corrector(x_last, m0, m_prev, model_t, *co, order), f"unipc_corrector order {order}, n = {n}")


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_unipc_predictor_past_one_grid_pass(n, order):
    """uv_unipc_predictor, as above, against ref_unipc_predictor (oracle.unipc.FlowUniPC._predict's expression)."""
    x, m0, m_prev = _latents(n, 3, 3 * n + order)
    co = _coefs(4, n + 10 + order)
    out = _sent(n + SLACK)
    _call("uv_unipc_predictor", _dev(x), _dev(m0), _dev(m_prev) if order == 2 else None, out, *co, order, n)
    torch.cuda.synchronize()
    _check_out(out, n, ref_unipc_predictor(x, m0, m_prev, *co, order), f"unipc_predictor order {order}, n = {n}")


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", SAMPLER_N)
def test_dpmpp_update_past_one_grid_pass(n, order):
    """uv_dpmpp_update, as above, against ref_dpmpp_update (oracle.dpmpp.FlowDPMpp._first / _second's expressions)."""
    x, m0, m1 = _latents(n, 3, 5 * n + order)
    co = _coefs(3, n + 20 + order)
    out = _sent(n + SLACK)
    _call("uv_dpmpp_update", _dev(x), _dev(m0), _dev(m1) if order == 2 else None, out, *co, order, n)
    torch.cuda.synchronize()
    _check_out(out, n, ref_dpmpp_update(x, m0, m1, *co, order), f"dpmpp_update order {order}, n = {n}")


# step index -> (corrector order | None, predictor order) of the 10-step schedule: warm-up, a middle step, the last step (lower_order_final;
# sigma_t = 0, so lambda_t = +inf and r = 0, c1 = c2 = -1)
UNIPC_REAL = {0: (None, 1), 5: (2, 2), 9: (2, 1)}


@pytest.mark.parametrize("si", sorted(UNIPC_REAL))
def test_unipc_kernels_with_the_schedulers_coefficients(si):
    """The coefficient sets FlowUniPCMultistepScheduler (10 steps, shift 5) computes at step 0, step 5 and the last step, at n = 524 289
    (one element into the second grid pass): cfg_convert at the step's sigma, the corrector and the predictor against
    oracle.unipc.FlowUniPC's own _correct / _predict at the same step index, bit-exact."""
    n = 524289
    corr_order, pred_order = UNIPC_REAL[si]
    x, m0, m_prev, model_t = _latents(n, 4, 900 + si)
    sigma = unipc_real_coefficients(si, "s", 0)
    out = _sent(n + SLACK)
    _call("uv_cfg_convert", _dev(model_t), _dev(m0), _dev(x), 5.0, sigma, None, out, n)
    torch.cuda.synchronize()
    _check_out(out, n, ref_cfg_convert(model_t, m0, x, 5.0, sigma)[1], f"cfg_convert at step {si}")
    o = _oracle_unipc(si, m_prev, m0)
    if corr_order is not None:
        co = unipc_real_coefficients(si, "c", corr_order)
        out = _sent(n + SLACK)
        _call("uv_unipc_corrector", _dev(x), _dev(m0), _dev(m_prev), _dev(model_t), out, *co, corr_order, n)
        torch.cuda.synchronize()
        _check_out(out, n, o._correct(model_t, x, corr_order), f"unipc_corrector at step {si}")
    co = unipc_real_coefficients(si, "p", pred_order)
    out = _sent(n + SLACK)
    _call("uv_unipc_predictor", _dev(x), _dev(m0), _dev(m_prev) if pred_order == 2 else None, out, *co, pred_order, n)
    torch.cuda.synchronize()
    _check_out(out, n, o._predict(x, pred_order), f"unipc_predictor at step {si}")


# ---------------------------------------------------------------------------------------------------------------
# the CPU-side helpers, checked without a GPU: python tests/test_f32_kernels.py
# ---------------------------------------------------------------------------------------------------------------
def cpu_selfcheck():
    from oracle import dpmpp as od
    from oracle import wan_vae
    check_case_table()
    print(f"case table: {len(CASES)} cases, coverage asserted")
    # seq_emulation: inside the derived bound of gate (b), and worse than torch's blocked fp32 product (gate (c) is not vacuous)
    for M, N, K in ((129, 192, 3072), (143, 144, 1024)):
        g = _gen(K)
        A, W, B, R = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        ref = exact_mm(A.double(), W.double(), B.double(), R.double())
        mag = exact_mm(A.double().abs(), W.double().abs(), B.double().abs(), R.double().abs())
        err = (seq_emulation(A, W, B, R).double() - ref).abs()
        assert bool((err <= (K + 2) * EPS * mag).all()) and float(err.max()) > 0
        rms, blocked = float(err.pow(2).mean().sqrt()), float((exact_mm(A, W, B, R).double() - ref).pow(2).mean().sqrt())
        print(f"seq_emulation ({M}, {N}, {K}): rms error {rms:.3e}, {rms / blocked:.2f} x torch's fp32 product, max err / bound {float((err / ((K + 2) * EPS * mag)).max()):.4f}")
    # the designed operands are exact for every K of the table: the sequential order and a random one reproduce the fp64 reference
    for K in sorted({c.K for c in CASES}):
        g = _gen(K)
        A, W, B, R = designed_operands(24, 20, K, g)
        ref = exact_reference(A, W, B, R)
        assert torch.equal(seq_emulation(A, W, B, R), ref) and torch.equal(random_order_sum(A, W, B, R, g), ref), K
    for ci, c in enumerate(CASES):
        A, W, B, R = designed_operands(c.M, c.N, c.K, _gen(1000 + ci))
        exact_reference(A, W, *_opts(c, B, R))
    print("designed operands: exact in fp32 under sequential and random summation order for K in", sorted({c.K for c in CASES}))
    # attention_reference against the oracle's own block (channels-first, F.scaled_dot_product_attention) in fp64
    for H, Wd, C in ((2, 3, 128), (13, 11, 128)):
        wts = [t.double() for t in attention_weights(C, 40 + C)]
        x = 3.0 * torch.randn(2, H, Wd, C, generator=_gen(1), dtype=F64)
        sd = {"a.norm.gamma": wts[0].view(C, 1, 1), "a.to_qkv.weight": wts[1].view(3 * C, C, 1, 1), "a.to_qkv.bias": wts[2],
              "a.proj.weight": wts[3].view(C, C, 1, 1), "a.proj.bias": wts[4]}
        want = wan_vae.WanVAE(sd, wan_vae.SMALL_CFG)._attn("a.", x.permute(3, 0, 1, 2).unsqueeze(0))[0].permute(1, 2, 3, 0)
        ref = attention_reference(x, *wts)
        assert float((ref - want).abs().max()) < 1e-12, float((ref - want).abs().max())
        emu = attention_reference(x.float(), *[t.float() for t in wts], mm=seq_emulation)
        assert_f32_close(emu, ref, name="fp32 block")
        print(f"attention_reference {H}x{Wd} C{C}: max |diff| to oracle.wan_vae._attn {float((ref - want).abs().max()):.2e}; "
              f"fp32 block rms error {float((emu.double() - ref).pow(2).mean().sqrt()):.3e}")
    # the sampler expressions: against oracle.unipc at the scheduler's own coefficients, against oracle.dpmpp at its coefficients
    x, m0, m_prev, model_t = _latents(1000, 4, 3)
    for si, (co_order, p_order) in UNIPC_REAL.items():
        o = _oracle_unipc(si, m_prev, m0)
        if co_order is not None:
            assert torch.equal(ref_unipc_corrector(x, m0, m_prev, model_t, *unipc_real_coefficients(si, "c", co_order), co_order), o._correct(model_t, x, co_order))
        assert torch.equal(ref_unipc_predictor(x, m0, m_prev, *unipc_real_coefficients(si, "p", p_order), p_order), o._predict(x, p_order))
    assert torch.equal(ref_unipc_corrector(x, m0, None, model_t, *unipc_real_coefficients(1, "c", 1), 1), _oracle_unipc(1, None, m0)._correct(model_t, x, 1))
    d = od.FlowDPMpp(1000, shift=1)
    d.set_timesteps(sigmas=od.get_sampling_sigmas(10, 5.0))
    d.step_index, d.model_outputs = 5, [m_prev, m0]
    st, s0, s1 = d.sigmas[6], d.sigmas[5], d.sigmas[4]
    h, h0 = d._lambda(st) - d._lambda(s0), d._lambda(s0) - d._lambda(s1)
    r, c, inv = (st / s0).item(), ((1 - st) * (torch.exp(-h) - 1.0)).item(), (1.0 / (h0 / h)).item()
    assert torch.equal(ref_dpmpp_update(x, m0, m_prev, r, c, inv, 2), d._second(x)) and torch.equal(ref_dpmpp_update(x, m0, None, r, c, inv, 1), d._first(m0, x))
    print("sampler expressions: equal to oracle.unipc / oracle.dpmpp bit for bit")


if __name__ == "__main__":
    cpu_selfcheck()
