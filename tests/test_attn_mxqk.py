"""The opt-in MXFP8 q / k mode of the DiT's self-attention (WanModel.set_attn_precision("mxfp8_qk")): the attention entry point
uv_flash_attn_mxqk with its two kernels (flash_attn_mxqk12_kernel for Lk >= 2048, flash_attn_mxqk4_kernel below), the quantising producer
uv_rmsnorm_rope_qk_mx, and the model / pipeline behaviour (-m gpu). tests/test_attn_mxqk_host.py checks the table and the builders without a GPU.

1  lane map       one-hot codes against distinct per-block scale bytes, read back through a selector V: integer-exact
2  designed       the operand families of tests/test_attn_kernels.py (imported, not restated; every one is exact in MXFP8: asserted), the
                  same gate: bit-identical to the fp64 softmax of the dequantised operands rounded to bf16, outside the at most 0.5 % of
                  elements at a rounding boundary (family A, spikes); bit patterns of the selected V rows (family B); its decorations
                  (sentinel slack rows / columns, V^T pad of 1000, eight poison code / scale rows behind q and k, strided ldo, column slices)
3  random         against the bf16 kernel on the dequantised operands (derived gate) and against the fp64 softmax (truth ratio)
4  independence   a query's bits do not depend on the launch, the cut or the batch; run to run
5  producer       rmsnorm_rope_qk_mx == rmsnorm_rope_qk then mx_quant, bit for bit
6  rejections     write nothing
7  model          one TI2V-5B-width block against an oracle whose rope_apply quantises-dequantises (short and long kernel), round trip,
                  CFG pair, HIP-graph denoise, un-merged LoRA"""
import contextlib
import json
import math
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

from conftest import load_golden, record_margin
from test_attn_kernels import SENT, _auto_cut, _operands, _up
from test_mxfp8 import mx_dequant, mx_qdq, mx_quant_ref

BF16 = torch.bfloat16
U8 = torch.uint8
F64 = torch.float64
DEV = "cuda"
D = 128
KNAME = {"mx12": "flash_attn_mxqk12_kernel", "mx4": "flash_attn_mxqk4_kernel"}


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


# ---------------------------------------------------------------------------------------------------------------
# the case table of group 2 (the shapes of tests/test_attn_kernels.py's fwd3 / fwd12 rows: the operand sets are shared through its cache)
# ---------------------------------------------------------------------------------------------------------------
# ld: "dense", "slice" (q / k codes are the byte slices [:, :C] and [:, C + 16:2 C + 16] of one [rows, 3 C + 32] buffer, the scales the slices
# [:, :C / 32] and [:, C / 32 + 4:2 C / 32 + 4] of one [rows, 3 C / 32 + 8] buffer), "vt+64" / "vt+8", "ldo+8" (through LDS) / "ldo+4" (direct store)
Case = namedtuple("Case", "kern fam B H Lq Lk cut ld")
CASES = []


def _c(kern, Lq, Lk, fam="A", B=1, H=2, cut=0, ld="dense"):
    assert (kern == "mx12") == (Lk >= 2048)
    CASES.append(Case(kern, fam, B, H, Lq, Lk, cut, ld))


for _lk in (5, 63, 64, 65, 128, 129, 200, 2040):       # lone short tile, even / odd tile counts, ragged tile on either stage, last Lk of the kernel
    for _lq in (1, 33, 150):
        _c("mx4", _lq, _lk)
for _lk in (2048, 2104, 2112, 2184):                   # 16 units per head: cut 1 = 12 + 4 with 8 loader-only waves, 2 = 12 + 8, 3 = 8 + 8
    for _cut in (0, 1, 2, 3):
        _c("mx12", 500, _lk, B=2, H=4, cut=_cut)
for _cut in (0, 1, 2, 3):
    _c("mx12", 500, 2104, H=3, cut=_cut)               # block totals no multiple of 8: plain id order
_c("mx12", 1, 2048)
_c("mx12", 1, 2104)
for _b in (2, 3):                                      # stacked samples whose V^T columns start off a tile boundary
    _c("mx4", 150, 72, B=_b)
    _c("mx4", 150, 200, B=_b)
    _c("mx12", 150, 2104, B=_b)
for _ld in ("slice", "vt+64", "vt+8", "ldo+8", "ldo+4"):
    _c("mx4", 150, 200, B=2, ld=_ld)
    _c("mx12", 150, 2104, B=2, ld=_ld)
for _fam in ("spike10", "spike6"):                     # the maximum-moves branch, and P > 1 without a move
    _c("mx4", 150, 200, fam=_fam)
    _c("mx12", 150, 2104, fam=_fam)
_c("mx12", 500, 2104, fam="B", B=2)                    # the selector at the production scale, a ragged last tile, two samples
_c("mx4", 260, 200, fam="B", B=2)


def _id(i, c):
    return (f"{i:03d}-{c.kern}-{c.fam}-B{c.B}H{c.H}-Lq{c.Lq}-Lk{c.Lk}" + (f"-cut{c.cut}" if c.kern == "mx12" else "")
            + ("" if c.ld == "dense" else "-" + c.ld))


IDS = [_id(i, c) for i, c in enumerate(CASES)]


def _ops(c):
    return _operands(c.fam, False, False, c.B, c.H, D, c.Lq, c.Lk)


def _layout(c):
    """(ldq = ldk in bytes, ld_s, ldvt, ldo) of the case"""
    C = c.H * D
    ldq, ld_s, ldo = C, C // 32, C
    ldvt = (c.B - 1) * c.Lk + _up(c.Lk, 64)
    if c.ld == "slice":
        ldq, ld_s = 3 * C + 32, 3 * C // 32 + 8
    elif c.ld in ("vt+64", "vt+8"):
        ldvt += int(c.ld[3:])
    elif c.ld in ("ldo+8", "ldo+4"):
        ldo += int(c.ld[4:])
    return ldq, ld_s, ldvt, ldo


def expected_plan(kern, B, H, Lq, cut, ncus):
    nbh = H * B
    if kern != "mx12":
        qb = (Lq + 127) // 128
        return dict(kernel=KNAME[kern], q_blocks=qb, n12=0, grid=qb * nbh)
    nwu = (Lq + 31) // 32
    if cut > 0:
        n8 = cut - 1
        n12 = (nwu - 8 * n8 + 11) // 12 if nwu > 8 * n8 else 0
    else:
        n12, n8 = _auto_cut(nwu, nbh, ncus)
    return dict(kernel=KNAME[kern], q_blocks=n12 + n8, n12=n12, grid=(n12 + n8) * nbh)


def assert_plan(c, ncus):
    """Under the case's OPT_ATTN_CUT (left set for the launch; the autouse fixture resets it)."""
    _lib = L()
    _lib.set_option(_lib.OPT_ATTN_CUT, c.cut)
    plan = _lib.attn_mxqk_plan(c.Lq, c.Lk, D, c.B, c.H)
    want = expected_plan(c.kern, c.B, c.H, c.Lq, c.cut, ncus)
    assert plan == want, f"planned {plan}, the case expects {want}"
    if c.kern == "mx12" and c.cut and c.Lq == 500:
        assert (plan["n12"], plan["q_blocks"] - plan["n12"]) == {1: (2, 0), 2: (1, 1), 3: (0, 2)}[c.cut]
    return plan


def mx_exact(x):
    """bf16 [rows, C] -> (codes, scales) under the format's rule; asserts that the operand survives it exactly"""
    codes, scales = mx_quant_ref(x)
    assert torch.equal(mx_dequant(codes, scales), x.double()), "a designed operand is not exact in MXFP8"
    return codes, scales


def _poison_codes(rows, cols, g):
    """+-448 codes, every second row the negative of the one before; with a scale byte of 131 (x16) one of each pair wins any softmax"""
    p = (torch.randint(0, 2, (rows, cols), generator=g, device=DEV) * 0x80 + 0x7E).to(U8)
    p[1::2] = p[0:rows - rows % 2:2] ^ 0x80
    return p


def _launch(c, o):
    """One flash_attn_mxqk call of the case -> the dense result [B Lq, C] on the CPU; sentinels asserted here."""
    _lib = L()
    C, rq, rk = c.H * D, c.B * c.Lq, c.B * c.Lk
    ldq, ld_s, ldvt, ldo = _layout(c)
    g = torch.Generator(device=DEV).manual_seed(CASES.index(c))
    (qc0, qs0), (kc0, ks0) = mx_exact(o.q), mx_exact(o.k)
    if c.ld == "slice":
        buf = _poison_codes(max(rq, rk) + 8, ldq, g)
        sbuf = torch.full((max(rq, rk) + 8, ld_s), 131, dtype=U8, device=DEV)
        qc, kc = buf[:rq, :C], buf[:rk, C + 16:2 * C + 16]
        qs, ks = sbuf[:rq, :C // 32], sbuf[:rk, C // 32 + 4:2 * C // 32 + 4]
    else:
        qb, kb = _poison_codes(rq + 8, C, g), _poison_codes(rk + 8, C, g)
        qsb, ksb = torch.full((rq + 8, ld_s), 131, dtype=U8, device=DEV), torch.full((rk + 8, ld_s), 131, dtype=U8, device=DEV)
        qc, kc, qs, ks = qb[:rq], kb[:rk], qsb[:rq], ksb[:rk]
    qc.copy_(qc0.to(DEV)), kc.copy_(kc0.to(DEV)), qs.copy_(qs0.to(DEV)), ks.copy_(ks0.to(DEV))
    vt = torch.full((C, ldvt), 1000.0, dtype=BF16, device=DEV)
    vt[:, :rk] = o.v.to(DEV).t()
    full = torch.full((rq + 8, ldo), SENT, dtype=BF16, device=DEV)
    out = full[:rq, :C]
    assert (qc.stride(0), kc.stride(0), qs.stride(0), ks.stride(0), vt.stride(0), out.stride(0)) == (ldq, ldq, ld_s, ld_s, ldvt, ldo)
    _lib.flash_attn_mxqk(qc, qs, kc, ks, vt, out, c.Lq, c.Lk, c.H, D, o.scale, batch=c.B)
    torch.cuda.synchronize()
    host = full.cpu()
    stray = int((host != SENT).sum()) - int((host[:rq, :C] != SENT).sum())
    assert stray == 0, f"{stray} elements outside the [{rq}, {C}] result were written (buffer {tuple(host.shape)})"
    if c.fam != "B":
        assert not bool((host[:rq, :C] == SENT).any()), "part of the result was not written"
    return host[:rq, :C].contiguous()


def _where(c, i, j):
    return f"(row {i} = sample {i // c.Lq} query {i % c.Lq}: unit {i % c.Lq // 32} lane {i % 32}; column {j} = head {j // D} d {j % D})"


# ---------------------------------------------------------------------------------------------------------------
# 1. lane map
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Lk", [128, 2048])
@pytest.mark.parametrize("side", ["q", "k"])
def test_lane_map_exact(side, Lk):
    """Query i is the one-hot code 1.0 at head-dim position i, key j < 128 the one-hot code 1.0 at position j (the keys behind them are
    zero), V selects: v[j][d] = (d == j). One side's scale bytes are 127 + (b + row) % 4 for block b - four different bytes per row -,
    the other side's 127. With scale * log2(e) = 1 exactly, S[i][i] = 2^a, a = (i / 32 + i) % 4, every other S is 0, every P a power of two:
    out[i][i] / out[i][d] must be EXACTLY 2^(2^a) for every d != i (both are one rounding of a power of two times the same f32 reciprocal), and
    out[i][i] the bf16 of 1 / (1 + (Lk - 1) 2^-S) to 2 ulp. A code byte that met another byte position lights up a second column; a scale byte
    taken from another block, lane or op_sel changes a."""
    _lib = L()
    n = 128
    scale = np.float32(math.log(2.0))
    assert float(np.float32(scale) * np.float32(1.4426950408889634)) == 1.0
    kern = "mx12" if Lk >= 2048 else "mx4"
    assert _lib.attn_mxqk_plan(n, Lk, D, 1, 1)["kernel"] == KNAME[kern]
    idx = torch.arange(n)
    qc, kc = torch.zeros(n, D, dtype=U8), torch.zeros(Lk, D, dtype=U8)
    qc[idx, idx] = 0x38
    kc[idx, idx] = 0x38
    qs, ks = torch.full((n, 4), 127, dtype=U8), torch.full((Lk, 4), 127, dtype=U8)
    var = (127 + (torch.arange(4)[None, :] + idx[:, None]) % 4).to(U8)
    if side == "q":
        qs[:] = var
    else:
        ks[:n] = var
    a = (idx // 32 + idx) % 4
    S = torch.exp2(a.double())
    assert torch.equal((mx_dequant(qc, qs) @ mx_dequant(kc, ks).t())[idx, idx], S) and set(a.tolist()) == {0, 1, 2, 3}
    v = torch.zeros(Lk, D, dtype=BF16)
    v[idx, idx] = 1.0
    vt = torch.zeros(D, _up(Lk, 64), dtype=BF16, device=DEV)
    vt[:, :Lk] = v.t().to(DEV)
    out = torch.full((n, D), SENT, dtype=BF16, device=DEV)
    _lib.flash_attn_mxqk(qc.to(DEV), qs.to(DEV), kc.to(DEV), ks.to(DEV), vt, out, n, Lk, 1, D, float(scale))
    got = out.cpu().double()
    diag = got[idx, idx]
    want = 1.0 / (1.0 + (Lk - 1) * torch.exp2(-S))
    assert bool(((diag - want).abs() <= 2 * want * 2.0 ** -8).all()), "the winner's weight is off: a scale byte from the wrong block?"
    ratio = diag[:, None] / got
    off = ~torch.eye(n, dtype=torch.bool)
    bad = (ratio != torch.exp2(S)[:, None]) & off
    if bad.any():
        i, j = (int(t) for t in bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} elements; first: query {i} (block {i // 32}) column {j}: ratio {ratio[i, j].item()}, expected 2^{S[i].item()}")


# ---------------------------------------------------------------------------------------------------------------
# 2. designed families, bit-exact
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_mxqk_kernel_is_bit_exact_on_designed_operands(c):
    ncus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = assert_plan(c, ncus)
    o = _ops(c)
    got = _launch(c, o)
    diff = (got.view(torch.int16) != o.ref.view(torch.int16)) & ~((got == 0) & (o.ref == 0))
    in_band = 0
    if o.near is not None:
        in_band = int((diff & o.near).sum())
        diff = diff & ~o.near
    name = IDS[CASES.index(c)]
    print(f"{name}: {plan}; {o.stats}; mismatches in the excepted band {in_band}")
    record_margin(f"attn_mxqk/{name}", kernel=plan["kernel"], band_mismatches=in_band, **o.stats)
    if diff.any():
        i, j = (int(x) for x in diff.nonzero()[0])
        rows = sorted({int(x) for x in diff.nonzero()[:, 0]})
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.numel()} elements differ from the reference, in {len(rows)} rows (first rows {rows[:8]}); "
                             f"first at {_where(c, i, j)}: got {got[i, j].item()!r}, expected {o.ref[i, j].item()!r}")


# ---------------------------------------------------------------------------------------------------------------
# 3. random operands: against the bf16 kernel on the dequantised operands, and against fp64
# ---------------------------------------------------------------------------------------------------------------
def _random_problem(B, H, Lq, Lk, seed):
    g = torch.Generator().manual_seed(seed)
    C = H * D
    q, k = torch.randn(B * Lq, C, generator=g).to(BF16), torch.randn(B * Lk, C, generator=g).to(BF16)
    k[:, 5::37] *= 6                                                    # outlier channels: blocks whose scale is set by one element
    v = torch.rand(B * Lk, C, generator=g).to(BF16)                     # >= 0: P.V cannot cancel
    (qc, qs), (kc, ks) = mx_quant_ref(q), mx_quant_ref(k)
    qd, kd = mx_dequant(qc, qs), mx_dequant(kc, ks)
    assert torch.equal(qd.to(BF16).double(), qd) and torch.equal(kd.to(BF16).double(), kd), "e4m3 x 2^e is not exact in bf16 here"
    scale = D ** -0.5
    ref = torch.empty(B * Lq, C, dtype=F64)
    for b in range(B):
        for h in range(H):
            qr, kr, cs = slice(b * Lq, (b + 1) * Lq), slice(b * Lk, (b + 1) * Lk), slice(h * D, (h + 1) * D)
            P = torch.softmax(qd[qr, cs] @ kd[kr, cs].t() * float(np.float32(scale)), -1)
            ref[qr, cs] = P @ v[kr, cs].double()
    return (qc, qs, kc, ks), (qd.to(BF16), kd.to(BF16)), v, scale, ref


@gpu
@pytest.mark.parametrize("B,H,Lq,Lk", [(1, 2, 150, 321), (2, 4, 500, 2104)])
def test_random_operands_against_the_bf16_kernel(B, H, Lq, Lk):
    """flash_attn on the dequantised q / k multiplies the SAME numbers (e4m3 x 2^e is exact in bf16: asserted) and runs the same softmax and
    P.V code with the same deferred maximum per 32-key half. What differs: the f32 summation order of S (one block-scaled instruction sums
    64 products where the bf16 kernel chains four 16-element steps), hence a few P entries whose bf16 rounding flips, hence the rounding of
    the output. Gate (derived, v >= 0 so P.V does not cancel): a flipped P entry changes its term by 2^-8 relative, so the output moves by at
    most 2^-8 out before its own rounding adds one ulp: |delta| <= ulp_bf16(out) + 2^-8 out elementwise, and at least 90 % of the elements
    identical (a relative perturbation of S of ~2^-22 flips a bf16 rounding with probability ~2^-14 per P entry). Against the fp64 softmax
    of the same operands the mode may be no further than 1.02 x the bf16 kernel's distance (the project's truth-ratio margin)."""
    _lib = L()
    C = H * D
    codes, deq, v, scale, ref = _random_problem(B, H, Lq, Lk, 7 * Lk + Lq)
    assert _lib.attn_mxqk_plan(Lq, Lk, D, B, H)["kernel"] == KNAME["mx12" if Lk >= 2048 else "mx4"]
    vt = torch.zeros(C, (B - 1) * Lk + _up(Lk, 64), dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.to(DEV).t()
    out_mx, out_bf = (torch.full((B * Lq, C), SENT, dtype=BF16, device=DEV) for _ in range(2))
    qc, qs, kc, ks = (t.to(DEV) for t in codes)
    _lib.flash_attn_mxqk(qc, qs, kc, ks, vt, out_mx, Lq, Lk, H, D, scale, batch=B)
    _lib.flash_attn(deq[0].to(DEV), deq[1].to(DEV), vt, out_bf, Lq, Lk, H, D, scale, batch=B)
    mx, bf = out_mx.cpu().double(), out_bf.cpu().double()
    same = float((mx == bf).double().mean())
    ulp = torch.exp2(torch.floor(torch.log2(bf.abs().clamp_min(2.0 ** -126))) - 7)
    excess = ((mx - bf).abs() - (ulp + 2.0 ** -8 * bf.abs())).max().item()
    e_mx, e_bf = (mx - ref).pow(2).mean().sqrt().item(), (bf - ref).pow(2).mean().sqrt().item()
    m = dict(identical_share=same, worst_excess_over_gate=excess, rms_vs_fp64_mxqk=e_mx, rms_vs_fp64_bf16_kernel=e_bf, truth_ratio=e_mx / e_bf)
    print(f"random B{B} H{H} Lq{Lq} Lk{Lk}", json.dumps(m))
    record_margin(f"attn_mxqk/random-B{B}H{H}-Lq{Lq}-Lk{Lk}", **m)
    assert excess <= 0, f"an element is {excess:.3e} beyond ulp + 2^-8 out of the bf16 kernel's"
    assert same >= 0.90, f"only {same:.2%} of the elements equal the bf16 kernel's"
    assert e_mx <= 1.02 * e_bf, f"rms against fp64 {e_mx:.4e}, the bf16 kernel's {e_bf:.4e}"


# ---------------------------------------------------------------------------------------------------------------
# 4. row independence
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Lk", [200, 2104])
def test_a_querys_bits_do_not_depend_on_the_launch(Lk):
    _lib = L()
    B, H, Lq = 2, 4, 500
    C = H * D
    codes, _, v, scale, _ = _random_problem(B, H, Lq, Lk, 11 + Lk)
    qc, qs, kc, ks = (t.to(DEV) for t in codes)
    vt = torch.zeros(C, (B - 1) * Lk + _up(Lk, 64), dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.to(DEV).t()

    def run(qc_, qs_, kc_, ks_, vt_, lq, batch):
        out = torch.full((batch * lq, C), SENT, dtype=BF16, device=DEV)
        _lib.flash_attn_mxqk(qc_, qs_, kc_, ks_, vt_, out, lq, Lk, H, D, scale, batch=batch)
        return out

    base = run(qc, qs, kc, ks, vt, Lq, B)
    assert torch.equal(run(qc, qs, kc, ks, vt, Lq, B), base), "two runs of one launch differ"
    for cut in (1, 2, 3):                                       # (Lk < 2048: the option does not reach the 4-wave kernel; same bits all the same)
        _lib.set_option(_lib.OPT_ATTN_CUT, cut)
        assert torch.equal(run(qc, qs, kc, ks, vt, Lq, B), base), f"cut {cut} changes bits"
    _lib.set_option(_lib.OPT_ATTN_CUT, 0)
    vt1 = torch.zeros(C, _up(Lk, 64), dtype=BF16, device=DEV)
    for b in range(B):                                          # batch 2 == two batch-1 launches
        vt1[:, :Lk] = vt[:, b * Lk:(b + 1) * Lk]
        one = run(qc[b * Lq:(b + 1) * Lq], qs[b * Lq:(b + 1) * Lq], kc[b * Lk:(b + 1) * Lk], ks[b * Lk:(b + 1) * Lk], vt1, Lq, 1)
        assert torch.equal(one, base[b * Lq:(b + 1) * Lq]), f"sample {b} alone differs from the stacked launch"
        if b == 0:                                              # queries 100 .. 132 alone: another unit, another lane, another block
            few = run(qc[100:133], qs[100:133], kc[:Lk], ks[:Lk], vt1, 33, 1)
            assert torch.equal(few, base[100:133]), "33 queries alone differ from the same queries inside 500"


# ---------------------------------------------------------------------------------------------------------------
# 5. producer
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Ls,nsamp,C,grid,row0", [(1, 1, 128, (1, 1, 1), 0), (63, 1, 256, (3, 4, 5), 0), (257, 2, 3072, (4, 8, 8), 0),
                                                  (257, 2, 3072, (5, 8, 8), 37), (4100, 1, 256, (4, 32, 32), 0)])
def test_producer_equals_norm_rope_then_quantise(Ls, nsamp, C, grid, row0):
    """uv_rmsnorm_rope_qk_mx against its definition, uv_rmsnorm_rope_qk followed by uv_mx_quant_bf16 on q and on k: codes and scales bit for
    bit. (L 4100: the four-rows-per-wave launch of the kernel; C 3072: its predicate-free instantiation.) Inputs carry whole-zero blocks
    and one large element in some blocks; they come back unchanged, and so do the slack bytes behind the codes and the scales."""
    from univid_amd.wan.model import _freqs_device, rope_params
    _lib = L()
    Lr = Ls * nsamp
    g = torch.Generator().manual_seed(Lr + C)
    d = D
    fr = _freqs_device(torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1), torch.device(DEV))
    xs = []
    for _ in range(2):
        x = torch.randn(Lr, C + 8, generator=g)
        x[:, 3::64] *= 30                                          # one large element per second block
        x[0, 32:64] = 0                                            # whole-zero blocks
        x[Lr // 2, 96:128] = 0
        xs.append(x.to(BF16).to(DEV))
    wq, wk = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) * 2 - 1).to(DEV)
    q, k = xs[0][:, :C], xs[1][:, :C]
    keep = [t.clone() for t in xs]
    ldc, ld_s = C + 16, C // 32 + 4
    bufs = [torch.full((Lr, ldc if i < 2 else ld_s), 0xA5, dtype=U8, device=DEV) for i in range(4)]
    qc, kc, qs, ks = bufs[0][:, :C], bufs[1][:, :C], bufs[2][:, :C // 32], bufs[3][:, :C // 32]
    _lib.rmsnorm_rope_qk_mx(q, k, wq, wk, qc, qs, kc, ks, Lr, Ls, C, D, 1e-6, fr, grid, row0=row0)
    torch.cuda.synchronize()
    assert torch.equal(xs[0], keep[0]) and torch.equal(xs[1], keep[1]), "the producer changed its inputs"
    for b, w in zip(bufs, (C, C, C // 32, C // 32)):
        assert bool((b[:, w:] == 0xA5).all()), "slack bytes behind the codes / scales were written"
    q2, k2 = q.clone(), k.clone()                                  # (same row stride as the views: contiguous copies)
    _lib.rmsnorm_rope_qk(q2, k2, wq, wk, Lr, Ls, C, D, 1e-6, fr, grid, row0=row0)
    for name, x2, codes, scales in (("q", q2, qc, qs), ("k", k2, kc, ks)):
        c2, s2 = torch.empty(Lr, C, dtype=U8, device=DEV), torch.empty(Lr, C // 32, dtype=U8, device=DEV)
        _lib.mx_quant(x2, c2, s2)
        assert torch.equal(scales, s2), f"{name}: {int((scales != s2).sum())} scale bytes differ from the two-pass form"
        assert torch.equal(codes, c2), f"{name}: {int((codes != c2).sum())} codes differ from the two-pass form"
        assert int(s2[0, 1]) == 0 and int((c2[0, 32:64] & 0x7F).sum()) == 0, "the all-zero block: scale byte 0, codes +-0"
        cr, sr = mx_quant_ref(x2.cpu())                            # and the two-pass form is the format's rule
        assert torch.equal(c2.cpu(), cr) and torch.equal(s2.cpu(), sr)


# ---------------------------------------------------------------------------------------------------------------
# 6. rejections write nothing
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_rejections_write_nothing():
    _lib = L()
    Lq, Lk, H = 40, 72, 2
    C = H * D
    scale = D ** -0.5
    qcb = torch.zeros(2 * Lq + 8, C + 32, dtype=U8, device=DEV)
    kcb = torch.zeros(2 * Lk + 8, C + 32, dtype=U8, device=DEV)
    qsb = torch.full((2 * Lq + 8, C // 32 + 8), 127, dtype=U8, device=DEV)
    ksb = torch.full((2 * Lk + 8, C // 32 + 8), 127, dtype=U8, device=DEV)
    vbuf = torch.zeros(C, Lk + 128 + 64, dtype=BF16, device=DEV)
    full = torch.full((2 * Lq + 8, C), SENT, dtype=BF16, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr

    def raw(match, entry="uv_flash_attn_mxqk", qc=qcb, ldq=C + 32, qs=qsb, ld_qs=C // 32 + 8, kc=kcb, ldk=C + 32, ks=ksb, ld_ks=C // 32 + 8, vt=vbuf,
            ldvt=vbuf.stride(0), batch=1, Lk=Lk, H=H, hd=D):
        with pytest.raises(_lib.UnividHipError, match=match) as ei:
            _lib.call(entry, p(qc) if qc is not None else None, ldq, p(qs) if qs is not None else None, ld_qs, p(kc), ldk, p(ks) if ks is not None else None,
                      ld_ks, p(vt), ldvt, p(full), C, batch, Lq, Lk, H, hd, scale, st())
        assert entry in str(ei.value)

    raw("head_dim 64 unsupported", H=4, hd=64)
    raw("null scale pointer", qs=None)
    raw("null scale pointer", ks=None)
    raw("ld_qs/ld_ks must be", ld_qs=4)                                     # too small for H = 2
    raw("ld_qs/ld_ks must be", ld_ks=C // 32 + 2)                           # no multiple of 4
    raw("multiples of 16 bytes", ldq=C + 8)
    raw("16-byte aligned", qc=qcb.view(-1)[8:])                             # misaligned codes
    raw("4-byte aligned", ks=ksb.view(-1)[2:])
    raw("needs Lk % 8", batch=2, Lk=68)
    raw("must cover", batch=2, ldvt=128)
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_mxqk_plan"):
        _lib.attn_mxqk_plan(Lq, Lk, 64, 1, 4)
    # the wrapper's own check (dtype / extent) and the producer's entry point
    with pytest.raises(_lib.UnividHipError, match="flash_attn_mxqk.q_scales"):
        _lib.flash_attn_mxqk(qcb[:Lq, :C], qsb.view(torch.int8)[:Lq, :C // 32], kcb[:Lk, :C], ksb[:Lk, :C // 32], vbuf[:, :128], full[:Lq], Lq, Lk, H, D, scale)
    x = torch.ones(Lq, C, dtype=BF16, device=DEV)
    w = torch.ones(C, device=DEV)
    codes, scales = torch.full((Lq, C), 0xA5, dtype=U8, device=DEV), torch.full((Lq, C // 32), 0xA5, dtype=U8, device=DEV)
    for match, kw in (("head_dim 64 unsupported", dict(hd=64)), ("ld_s must be", dict(ld_s=6)), ("null scale pointer", dict(sc=None))):
        hd, ld_s, sc = kw.get("hd", D), kw.get("ld_s", C // 32), kw.get("sc", scales)
        with pytest.raises(_lib.UnividHipError, match=match) as ei:
            _lib.call("uv_rmsnorm_rope_qk_mx", p(x), p(w), p(codes), p(sc) if sc is not None else None, p(x), p(w), p(codes),
                      p(sc) if sc is not None else None, C, C, ld_s, Lq, Lq, C, hd, 1e-6, None, 0, 0, 0, 0, st())
        assert "uv_rmsnorm_rope_qk_mx" in str(ei.value)
    torch.cuda.synchronize()
    assert bool((full == SENT).all()) and bool((codes == 0xA5).all()) and bool((scales == 0xA5).all()), "a rejected call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------
# 7. model level
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def emulated_mxqk():
    """The oracle with rope_apply - called for the self-attention's q and k only - returning the quantise-dequantise of its bf16 result
    (blocks of 32 along the head dimension): the operands uv_flash_attn_mxqk multiplies."""
    from oracle import wan_dit
    orig = wan_dit.rope_apply
    wan_dit.rope_apply = lambda x, grid_sizes, freqs: mx_qdq(orig(x, grid_sizes, freqs).to(BF16))
    try:
        yield
    finally:
        wan_dit.rope_apply = orig


def _rms(a, b):
    return (a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt().item()


def _block_3072(seed):
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock
    dim, ffn, heads = 3072, 14336, 24
    with torch.device(DEV):
        blk = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, seed)
    return blk.eval(), {k: v.detach().cpu() for k, v in sd.items()}


def _block_case(name, x, e_rows, tid, grid, ctx, blk, sdc, with_ffn=True):
    """One block, HIP in the mode against the emulated oracle and the fp32 truth (both on the CPU). Gate (a): rms(hip - truth) <= 1.02
    rms(emulated oracle - truth). Recorded, not gated: the relative rms against the emulated oracle, the mode's distance from the truth
    over the bf16 mode's, the same with ffn_precision "mxfp8" on as well; the host seconds of the two oracle runs."""
    from oracle import wan_dit
    from univid_amd.wan.model import _freqs_device
    heads, d = 24, 128
    Lt = x.shape[1]
    fr = _freqs_device(wan_dit.rope_table(d), torch.device(DEV))

    def run():
        xx = x[0].to(DEV).clone()
        with torch.no_grad():
            blk._run(xx, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), tuple(grid[0].tolist()), fr, ctx[0].to(DEV), first_block=False)
        return xx

    base = run()
    blk.set_attn_precision("mxfp8_qk")
    got = run()
    assert not torch.equal(got, base) and torch.isfinite(got).all()
    assert torch.equal(run(), got)
    both = None
    if with_ffn:
        blk.set_ffn_precision("mxfp8")
        both = run()
        blk.set_ffn_precision("bf16")
    blk.set_attn_precision("bf16")
    assert torch.equal(run(), base), "bf16 after a round trip through mxfp8_qk must equal the block before the switch"
    args = (sdc, "blocks.0.", x, e_rows[tid].unsqueeze(0), torch.tensor([Lt]), grid, wan_dit.rope_table(d))
    t0 = time.time()
    with torch.no_grad(), emulated_mxqk():
        emu = wan_dit.block_forward(*args, ctx, heads, 1e-6)[0]
    old, wan_dit.BF16 = wan_dit.BF16, torch.float32
    try:
        with torch.no_grad():
            truth = wan_dit.block_forward(*args, ctx.float(), heads, 1e-6)[0]
    finally:
        wan_dit.BF16 = old
    host_s = time.time() - t0
    e_hip, e_emu, e_bf = _rms(got, truth), _rms(emu, truth), _rms(base, truth)
    m = dict(rel_rms_vs_emulated_oracle=_rms(got, emu) / emu.float().pow(2).mean().sqrt().item(), truth_ratio=e_hip / e_emu,
             rms_vs_truth_mxqk=e_hip, rms_vs_truth_emulated_oracle=e_emu, rms_vs_truth_bf16_mode=e_bf, mxqk_over_bf16_distance_from_truth=e_hip / e_bf,
             oracle_host_seconds=host_s)
    if both is not None:
        m["mxqk_and_mxfp8_ffn_over_bf16_distance_from_truth"] = _rms(both, truth) / e_bf
    record_margin("mxqk " + name, **m)
    print("mxqk " + name, json.dumps(m))
    assert e_hip <= 1.02 * e_emu, f"{name}: rms vs truth {e_hip:.4e}, the emulated oracle's {e_emu:.4e}"


@gpu
def test_block_ti2v5b_width_short_kernel():
    g = load_golden("dit_block_3072")
    blk, sdc = _block_3072(g["seed"])
    assert L().attn_mxqk_plan(48, 48, D, 1, 24)["kernel"] == KNAME["mx4"]
    _block_case("block 3072 L48", g["x"], g["e_rows"], g["tid"], g["grid"], g["ctx"], blk, sdc)


@gpu
def test_block_ti2v5b_width_long_kernel():
    """2 304 tokens (grid 4 x 24 x 24): the 12-wave kernel under the model; inputs from detinit. The oracle and its fp32 truth run on the CPU."""
    from univid_amd import detinit
    g = load_golden("dit_block_3072")
    blk, sdc = _block_3072(g["seed"])
    Lt = 2304
    assert L().attn_mxqk_plan(Lt, Lt, D, 1, 24)["kernel"] == KNAME["mx12"]
    x = detinit.uniform_pm1("mxqk.block.x", Lt * 3072, g["seed"]).reshape(1, Lt, 3072).float() * 2
    tid = (torch.arange(Lt) * 7 // Lt % 2).to(g["tid"].dtype)
    _block_case("block 3072 L2304", x, g["e_rows"], tid, torch.tensor([[4, 24, 24]]), g["ctx"], blk, sdc, with_ffn=False)


def _small_model(seed=0):
    """The tiny golden model has head_dim 64: dim 256 with 2 heads instead, weights from detinit."""
    from test_gpu_parity import _tiny_model
    return _tiny_model(seed, num_heads=2)


@gpu
def test_small_model_cfg_pair_and_round_trip():
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    Lt = 256
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        gen = m._prep_gen
        m.set_attn_precision("mxfp8_qk")
        assert m._prep_gen > gen
        got = m([x], t, [ctx], Lt)[0]
        ctx2 = (ctx * 0.5).contiguous()
        other = m([x], t, [ctx2], Lt)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], Lt)
        assert torch.equal(pair[0], got) and torch.equal(pair[1], other) and not torch.equal(got, other), "the stacked CFG pair differs from single forwards"
        assert not torch.equal(got, base) and torch.isfinite(got).all()
        m.set_ffn_precision("mxfp8")                                       # the two modes are independent and combine
        assert not torch.equal(m([x], t, [ctx], Lt)[0], got)
        m.set_ffn_precision("bf16")
        assert torch.equal(m([x], t, [ctx], Lt)[0], got)
        m.set_attn_precision("bf16")
        assert torch.equal(m([x], t, [ctx], Lt)[0], base), "bf16 after a round trip must equal the model before the switch"


@gpu
def test_small_model_denoise_graph_and_mode_switch():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (2, g["shift"], g["guide_scale"])

    def pipe_in(mode):
        cfg, sd, m = _small_model(g["seed"])
        return WanTI2V(TI2VConfig, model=m, device=DEV, attn_precision=mode)

    def gen(pipe, graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    fresh_mx, fresh_bf = pipe_in("mxfp8_qk"), pipe_in("bf16")
    assert fresh_mx.model.attn_precision == "mxfp8_qk" and all(b.self_attn.attn_precision == "mxfp8_qk" for b in fresh_mx.model.blocks)
    mx_graph = gen(fresh_mx, True)
    assert fresh_mx._runner is not None
    assert torch.equal(mx_graph, gen(fresh_mx, False)), "graph != eager in mxfp8_qk mode"
    bf_graph = gen(fresh_bf, True)
    assert not torch.equal(bf_graph, mx_graph)
    fresh_bf.model.set_attn_precision("mxfp8_qk")
    assert torch.equal(gen(fresh_bf, True), mx_graph), "after the switch the pipeline does not equal a fresh mxfp8_qk pipeline"
    fresh_bf.model.set_attn_precision("bf16")
    assert torch.equal(gen(fresh_bf, True), bf_graph), "after the switch back the pipeline does not equal a fresh bf16 pipeline"
    fresh_mx._runner = fresh_bf._runner = None


@gpu
def test_unmerged_lora_on_q_and_k_works_in_the_mode(tmp_path):
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    m.set_attn_precision("mxfp8_qk")
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    attn = [f"blocks.{i}.self_attn.{p}" for i in range(cfg["num_layers"]) for p in ("q", "k")]
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, attn, 8, 6, b_std=0.2), 8, 16)
    mgr = LoRAManager()
    with torch.no_grad():
        base = m([x], t, [ctx], 256)[0]
        mgr.load_lora_weights(str(tmp_path / "A"), m, merge=False, name="A")
        with_a = m([x], t, [ctx], 256)[0]
        assert not torch.equal(with_a, base) and torch.isfinite(with_a).all()
        mgr.unload("A")
        assert torch.equal(m([x], t, [ctx], 256)[0], base), "unload does not restore the bits"
