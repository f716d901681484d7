"""The opt-in MXFP8 q / k + P.V mode of the DiT's self-attention (WanModel.set_attn_precision("mxfp8_qk_pv")): the V^T quantiser
uv_vt_mx_quant, the attention entry point uv_flash_attn_mxpv with its two kernels (flash_attn_mxpv12_kernel for Lk >= 2048,
flash_attn_mxpv4_kernel below) and the model / pipeline behaviour (-m gpu). tests/test_attn_mxpv_host.py checks the table and the builders
without a GPU. Builders, the case table and the MXFP8 reference come from test_attn_kernels, test_attn_mxqk and test_mxfp8.

1  quantiser      uv_vt_mx_quant against mx_quant_ref of each sample's zero-padded V^T rows after undoing the stated key permutation and scale
                  arrangement, bit for bit; pads; sentinels around both outputs
2  lane map       one-hot P against V codes / scale bytes that encode (channel, key): integer-exact, every key of two tiles, every d block
3  P format       the smallest subnormal code, the tie below it, code 256 without a move, the move just beyond it
4  designed       test_attn_mxqk's table (families A, spike10, spike6, B with a V that is exact along the keys) plus the family `tail`:
                  bit-identical to the fp64 softmax of the dequantised operands rounded to bf16 (A / spikes: outside the excepted band)
5  random         against the fp64 truth and an fp64 emulation of the format; the same distance for uv_flash_attn_mxqk
6  independence   a query's bits do not depend on the launch, the cut, the batch or its neighbours; run to run
7  rejections     write nothing
8  model          one TI2V-5B-width block against an oracle with the format emulated (short and long kernel), round trip, CFG pair, HIP-graph
                  denoise, mode switch, un-merged LoRA"""
import contextlib
import json
import math
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

from conftest import load_golden, record_margin
from test_attn_kernels import SENT, _near_boundary, _up
from test_attn_mxqk import CASES as QK_CASES, Case, _block_3072, _ops as _qk_ops, _poison_codes, _random_problem, _rms, _small_model, _where, \
    emulated_mxqk, expected_plan, mx_exact
from test_mxfp8 import mx_dequant, mx_quant_ref

DEFER_PV, PSHIFT = 1, 7          # include/univid_hip.h: UV_ATT_MXPV_DEFER, UV_ATT_MXPV_PSHIFT (their sum is 8)

BF16 = torch.bfloat16
U8 = torch.uint8
F64 = torch.float64
F8 = torch.float8_e4m3fn
DEV = "cuda"
D = 128
KNAME = {"mx12": "flash_attn_mxpv12_kernel", "mx4": "flash_attn_mxpv4_kernel"}
LOG2E_F32 = np.float32(1.4426950408889634)

# Gates of the measured kind (the project's rule: measured on the GPU x 1.2; profiles/mxpv_parity_margins.json holds the measurements).
# GATE_RANDOM: rms(hip - truth) / rms(fp64 emulation of the format - truth), with the emulation left in fp64 and with it rounded to bf16 as
# the kernel's output is. GATE_BLOCK: rms(hip - truth) / rms(emulated oracle - truth) of one block.
GATE_RANDOM = {(1, 2, 150, 200): (1.2 * 1.1014, 1.2 * 0.9965), (2, 4, 500, 2104): (1.2 * 1.4170, 1.2 * 1.0147)}
GATE_BLOCK = {"block 3072 L48": 1.2 * 1.0000, "block 3072 L2304": 1.2 * 1.0018}


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
# the V^T format on the host: reference, the stated permutation / arrangement and its inverse
# ---------------------------------------------------------------------------------------------------------------
_K = torch.arange(32)
PERM34 = (_K & 7) | ((_K & 8) << 1) | ((_K & 16) >> 1)      # byte p of a stored 32-key block holds key perm34(p) (an involution)


def vt_ref(v, B, Lk):
    """bf16 v [B Lk, C] -> (codes uint8 [C, B Lkp], scale bytes uint8 [C, B Lkp / 32]) in NATURAL key order: mx_quant_ref of each sample's
    V^T rows zero-padded to Lkp = roundup(Lk, 64); a block without any key has the scale byte 127."""
    C, Lkp = v.shape[1], _up(Lk, 64)
    pad = torch.zeros(C, B * Lkp, dtype=BF16)
    for b in range(B):
        pad[:, b * Lkp:b * Lkp + Lk] = v[b * Lk:(b + 1) * Lk].t()
    codes, sc = mx_quant_ref(pad)
    start = torch.arange(B * Lkp // 32) % (Lkp // 32) * 32
    sc[:, start >= Lk] = 127
    return codes, sc


def vt_dequant(codes, sc, B, Lk):
    """natural-order codes / scales -> fp64 v [B Lk, C]"""
    Lkp = codes.shape[1] // B
    full = mx_dequant(codes, sc)
    return torch.cat([full[:, b * Lkp:b * Lkp + Lk].t() for b in range(B)]).contiguous()


def vt_pack(codes, sc, H):
    """natural order -> the layout of include/univid_hip.h: codes permuted inside each 32-key block, scales tile-major [H, tiles, 2, 32, 4]"""
    C, W = codes.shape
    pc = codes.reshape(C, W // 32, 32)[:, :, PERM34].reshape(C, W).contiguous()
    ps = sc.reshape(H, 4, 32, W // 64, 2).permute(0, 3, 4, 2, 1).reshape(H, 4 * W).contiguous()
    return pc, ps


def vt_unpack(pc, ps, H):
    C, W = pc.shape
    codes = pc.reshape(C, W // 32, 32)[:, :, PERM34].reshape(C, W).contiguous()
    sc = ps.reshape(H, W // 64, 2, 32, 4).permute(0, 4, 3, 1, 2).reshape(C, W // 32).contiguous()
    return codes, sc


def vt_exact(v, B, Lk):
    """bf16 v -> natural codes / scales; asserts that v survives the format along the keys exactly"""
    codes, sc = vt_ref(v, B, Lk)
    assert torch.equal(vt_dequant(codes, sc, B, Lk), v.double()), "a designed V is not exact in MXFP8 along the keys"
    return codes, sc


def softmax_ref(q, k, v, scale, B, H, Lq, Lk):
    """fp64 softmax(q k^T scale) v per (sample, head) of fp64 operands -> fp64 [B Lq, C]"""
    out = torch.empty(B * Lq, H * D, dtype=F64)
    for b in range(B):
        for h in range(H):
            qr, kr, cs = slice(b * Lq, (b + 1) * Lq), slice(b * Lk, (b + 1) * Lk), slice(h * D, (h + 1) * D)
            P = torch.softmax(q[qr, cs] @ k[kr, cs].t() * float(np.float32(scale)), -1)
            out[qr, cs] = P @ v[kr, cs]
    return out


def emulated_ref(q, k, v, scale, B, H, Lq, Lk):
    """The format in fp64: P = exp2((s - rowmax) scale log2 e), numerator from e4m3_RNE(P 2^PSHIFT) 2^-PSHIFT, denominator from the unrounded P"""
    sl2 = float(np.float32(scale) * LOG2E_F32)
    out = torch.empty(B * Lq, H * D, dtype=F64)
    for b in range(B):
        for h in range(H):
            qr, kr, cs = slice(b * Lq, (b + 1) * Lq), slice(b * Lk, (b + 1) * Lk), slice(h * D, (h + 1) * D)
            S = q[qr, cs] @ k[kr, cs].t()
            P = torch.exp2((S - S.max(-1, keepdim=True).values) * sl2)
            Pq = (P * 2.0 ** PSHIFT).float().to(F8).double() * 2.0 ** -PSHIFT
            out[qr, cs] = (Pq @ v[kr, cs]) / P.sum(-1, keepdim=True)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the case table of group 4: test_attn_mxqk's own (shapes, cuts, batches, decorations, families) plus the family `tail`
# ---------------------------------------------------------------------------------------------------------------
# ld (decorations as there; the V^T ones act on the codes and scales): "slice", "vt+64" (ldvc + 64, ld_vs + 256), "vt+8" (ldvc + 16, ld_vs + 8:
# the smallest slack the alignment rules allow), "ldo+8" (through LDS) / "ldo+4" (direct store)
CASES = list(QK_CASES)
for _kern, _lk, _b in (("mx4", 200, 1), ("mx12", 2104, 1), ("mx12", 2104, 2)):
    CASES.append(Case(_kern, "tail", _b, 2, 150, _lk, 0, "dense"))


def _id(i, c):
    return (f"{i:03d}-{c.kern}-{c.fam}-B{c.B}H{c.H}-Lq{c.Lq}-Lk{c.Lk}" + (f"-cut{c.cut}" if c.kern == "mx12" else "")
            + ("" if c.ld == "dense" else "-" + c.ld))


IDS = [_id(i, c) for i, c in enumerate(CASES)]
PvOps = namedtuple("PvOps", "q k v scale ref near stats")
_CACHE = {}


def tail_gap(Lk):
    """G of the family `tail`: the largest G with Lk 2^-G >= 1 (11 at 2104, 7 at 200); 2^-G 2^PSHIFT is a normal e4m3 code"""
    G = int(math.floor(math.log2(Lk)))
    assert Lk * 2.0 ** -G >= 1 and PSHIFT - G >= -6
    return G


def _tail(B, H, Lq, Lk):
    """One early key (key 3 + head) G above all the others, which are all equal: scores G and 0 at scale log2(e) = 1. V is one row w at the
    early key and one row u at every other key, both in {-1, 0, 1} per channel: O = w + (Lk - 1) 2^-G u, l = 1 + (Lk - 1) 2^-G - the tail
    carries (Lk - 1) 2^-G >= 0.97 of the peak's mass. Nine values per head, none within 2^-18 of a bf16 rounding boundary (asserted): the
    kernel's f32 O * (1 / l) rounds as the fp64 quotient does."""
    G, C = tail_gap(Lk), H * D
    g = torch.Generator().manual_seed(4242 + Lk)
    q, k = torch.zeros(B * Lq, C, dtype=F64), torch.zeros(B * Lk, C, dtype=F64)
    w = torch.randint(-1, 2, (C,), generator=g).double()
    u = torch.randint(-1, 2, (C,), generator=g).double()
    v = u.repeat(B * Lk, 1)
    for h in range(H):
        q[:, h * D + D - 1] = 1
        rows = torch.arange(B) * Lk + 3 + h
        k[rows, h * D + D - 1] = G
        v[rows, h * D:(h + 1) * D] = w[h * D:(h + 1) * D]
    scale = np.float32(math.log(2.0))
    assert float(scale * LOG2E_F32) == 1.0
    ref = softmax_ref(q, k, v, scale, B, H, Lq, Lk)
    assert not bool(_near_boundary(ref, BF16, 2.0 ** -18).any()), "a tail value lies at a bf16 rounding boundary"
    flushed = w / (1 + (Lk - 1) * 2.0 ** -G)                  # what a kernel that drops the tail from the numerator would give
    assert float((flushed - ref[0]).abs().max()) > 0.25
    return PvOps(q.to(BF16), k.to(BF16), v.to(BF16), float(scale), ref.to(BF16), None, dict(tail_gap=G, tail_mass=(Lk - 1) * 2.0 ** -G))


def _selector_v(c, o):
    """Family B with a V that survives the format along the keys: random values over 24 binades, quantised-dequantised per sample in blocks
    of 32 keys (idempotent: asserted by vt_exact). The selector's q and k stay; the reference is the fp64 softmax, which IS the selected row."""
    g = torch.Generator().manual_seed(977 + c.Lk + c.Lq)
    v0 = (torch.randn(c.B * c.Lk, c.H * D, generator=g) * torch.exp2(torch.randint(-12, 13, (c.B * c.Lk, c.H * D), generator=g).float())).to(BF16)
    v = vt_dequant(*vt_ref(v0, c.B, c.Lk), c.B, c.Lk).to(BF16)
    ref = softmax_ref(o.q.double(), o.k.double(), v.double(), o.scale, c.B, c.H, c.Lq, c.Lk).to(BF16)
    return PvOps(o.q, o.k, v, o.scale, ref, None, dict(o.stats))


def _ops(c):
    if c not in _CACHE:
        if c.fam == "tail":
            _CACHE[c] = _tail(c.B, c.H, c.Lq, c.Lk)
        else:
            o = _qk_ops(c)
            _CACHE[c] = _selector_v(c, o) if c.fam == "B" else PvOps(o.q, o.k, o.v, o.scale, o.ref, o.near, dict(o.stats))
    return _CACHE[c]


def check_exactness(c, o):
    """The conditions under which the kernel must be bit-exact: q, k exact in MXFP8 along the head dimension, V along the keys, and every P a
    power of two inside the NORMAL e4m3 range under PSHIFT for any admissible reference maximum: with integer scores at scale log2(e) = 1 the
    reference is a score of the row (an integer) between max - DEFER_PV and max, so codes lie in [2^(PSHIFT - span), 2^(PSHIFT + DEFER_PV)] and
    need span <= PSHIFT + 6. Family B: the runner-up is >= 300 below the winner (P = 0 exactly in f32, code 0; the winner's code is 128 or 256)."""
    mx_exact(o.q), mx_exact(o.k), vt_exact(o.v, c.B, c.Lk)
    if c.fam == "B":
        assert o.stats["selector_gap"] >= 300
        return dict(span=0.0)
    assert float(np.float32(o.scale) * LOG2E_F32) == 1.0
    span = 0.0
    for b in range(c.B):
        for h in range(c.H):
            qr, kr, cs = slice(b * c.Lq, (b + 1) * c.Lq), slice(b * c.Lk, (b + 1) * c.Lk), slice(h * D, (h + 1) * D)
            S = o.q[qr, cs].double() @ o.k[kr, cs].double().t()
            assert torch.equal(S, S.round())
            span = max(span, float((S.max(-1).values - S.min(-1).values).max()))
    assert span <= PSHIFT + 6, f"score span {span}: a P would be a subnormal code"
    return dict(span=span)


def _layout(c):
    """(ldq = ldk in bytes, ld_s, ldvc, ld_vs, ldo) of the case"""
    C = c.H * D
    ldq, ld_s, ldo = C, C // 32, C
    ldvc = c.B * _up(c.Lk, 64)
    ld_vs = 4 * ldvc
    if c.ld == "slice":
        ldq, ld_s = 3 * C + 32, 3 * C // 32 + 8
    elif c.ld == "vt+64":
        ldvc, ld_vs = ldvc + 64, ld_vs + 256
    elif c.ld == "vt+8":
        ldvc, ld_vs = ldvc + 16, ld_vs + 8
    elif c.ld in ("ldo+8", "ldo+4"):
        ldo += int(c.ld[4:])
    return ldq, ld_s, ldvc, ld_vs, ldo


def assert_plan(c, ncus):
    """Under the case's OPT_ATTN_CUT (left set for the launch; the autouse fixture resets it): the mxqk plan's geometry, the mxpv kernel."""
    _lib = L()
    _lib.set_option(_lib.OPT_ATTN_CUT, c.cut)
    plan = _lib.attn_mxpv_plan(c.Lq, c.Lk, D, c.B, c.H)
    want = dict(expected_plan(c.kern, c.B, c.H, c.Lq, c.cut, ncus), kernel=KNAME[c.kern])
    assert plan == want, f"planned {plan}, the case expects {want}"
    qk = _lib.attn_mxqk_plan(c.Lq, c.Lk, D, c.B, c.H)
    assert (plan["q_blocks"], plan["n12"], plan["grid"]) == (qk["q_blocks"], qk["n12"], qk["grid"])
    return plan


def _launch(c, o):
    """One flash_attn_mxpv call of the case -> the dense result [B Lq, C] on the CPU; sentinels asserted here. V^T codes and scales come from
    the host reference (vt_ref + vt_pack), not from the GPU quantiser; slack columns hold +-448 codes and the scale byte 254."""
    _lib = L()
    C, rq, rk = c.H * D, c.B * c.Lq, c.B * c.Lk
    ldq, ld_s, ldvc, ld_vs, ldo = _layout(c)
    g = torch.Generator(device=DEV).manual_seed(CASES.index(c))
    (qc0, qs0), (kc0, ks0) = mx_exact(o.q), mx_exact(o.k)
    vc0, vs0 = vt_pack(*vt_exact(o.v, c.B, c.Lk), c.H)
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
    vcb, vsb = _poison_codes(C, ldvc, g), torch.full((c.H, ld_vs), 254, dtype=U8, device=DEV)
    vc, vs = vcb[:, :vc0.shape[1]], vsb[:, :vs0.shape[1]]
    vc.copy_(vc0.to(DEV)), vs.copy_(vs0.to(DEV))
    full = torch.full((rq + 8, ldo), SENT, dtype=BF16, device=DEV)
    out = full[:rq, :C]
    assert (qc.stride(0), kc.stride(0), qs.stride(0), ks.stride(0), vc.stride(0), vs.stride(0), out.stride(0)) == (ldq, ldq, ld_s, ld_s, ldvc, ld_vs, ldo)
    _lib.flash_attn_mxpv(qc, qs, kc, ks, vc, vs, out, c.Lq, c.Lk, c.H, D, o.scale, batch=c.B)
    torch.cuda.synchronize()
    host = full.cpu()
    stray = int((host != SENT).sum()) - int((host[:rq, :C] != SENT).sum())
    assert stray == 0, f"{stray} elements outside the [{rq}, {C}] result were written (buffer {tuple(host.shape)})"
    return host[:rq, :C].contiguous()


# ---------------------------------------------------------------------------------------------------------------
# 1. the quantiser
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,Lk,H", [(1, 5, 1), (1, 63, 2), (1, 64, 1), (1, 65, 2), (1, 200, 1), (1, 2104, 1), (2, 72, 2), (3, 72, 1), (2, 200, 1),
                                    (2, 2104, 1), (3, 2104, 1)])
def test_vt_mx_quant_is_the_reference_bit_for_bit(B, Lk, H):
    """Lk 72 and 2104: sample 1 starts at a column that is no multiple of 32 (72, 2104 = 24 mod 32) - blocks count from the sample's first
    key. Inputs carry whole-zero blocks, one large element in some blocks, values behind every sample's last key (the next sample's, or
    1000 in the slack) that must not leak; ldvt, ldvc and ld_vs have slack; 0xA5 sentinels around both outputs stay."""
    _lib = L()
    C, Lkp = H * D, _up(Lk, 64)
    g = torch.Generator().manual_seed(31 * Lk + B)
    v = torch.randn(B * Lk, C, generator=g) * torch.exp2(torch.randint(-6, 7, (B * Lk, 1), generator=g).float())
    v[::7, 3::16] *= 40
    v[:min(40, Lk), 5] = 0
    v = v.to(BF16)
    ldvt = (B - 1) * Lk + _up(Lk, 64) + 24
    vt = torch.full((C, ldvt), 1000.0, dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.to(DEV).t()
    keep = vt.clone()
    cbuf = torch.full((C + 2, B * Lkp + 32), 0xA5, dtype=U8, device=DEV)
    sbuf = torch.full((H + 2, 4 * B * Lkp + 8), 0xA5, dtype=U8, device=DEV)
    codes, scales = cbuf[1:C + 1, :B * Lkp], sbuf[1:H + 1, :4 * B * Lkp]
    _lib.vt_mx_quant(vt, codes, scales, Lk, H, D, batch=B)
    torch.cuda.synchronize()
    assert torch.equal(vt, keep), "the quantiser changed its input"
    ch, sh = cbuf.cpu(), sbuf.cpu()
    got_c, got_s = ch[1:C + 1, :B * Lkp].clone(), sh[1:H + 1, :4 * B * Lkp].clone()
    ch[1:C + 1, :B * Lkp] = 0xA5
    sh[1:H + 1, :4 * B * Lkp] = 0xA5
    assert bool((ch == 0xA5).all()) and bool((sh == 0xA5).all()), "bytes around the codes / scales were written"
    want_c, want_s = vt_ref(v, B, Lk)
    nat_c, nat_s = vt_unpack(got_c, got_s, H)
    assert torch.equal(nat_s, want_s), f"{int((nat_s != want_s).sum())} scale bytes differ from mx_quant_ref"
    assert torch.equal(nat_c, want_c), f"{int((nat_c != want_c).sum())} codes differ from mx_quant_ref"
    for b in range(B):                                             # pads: zero codes, scale 127 where a block holds no key
        assert int(nat_c[:, b * Lkp + Lk:(b + 1) * Lkp].sum()) == 0
        first_pad_block = (b * Lkp + _up(Lk, 32)) // 32
        assert bool((nat_s[:, first_pad_block:(b + 1) * Lkp // 32] == 127).all())
    assert not bool(((nat_c & 0x7F) == 0x7F).any()), "a NaN code"
    assert torch.equal(vt_pack(want_c, want_s, H)[0], got_c) and torch.equal(vt_pack(want_c, want_s, H)[1], got_s)


# ---------------------------------------------------------------------------------------------------------------
# 2. lane map of the P.V instruction
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Lk", [128, 2048])
@pytest.mark.parametrize("digit", [0, 1, 2])
def test_pv_lane_map_exact(digit, Lk):
    """Query i < 128 selects key i: one-hot q / k codes with scale bytes 132 / 131 give S[i][i] = 512 at scale log2(e) = 1, every other S is
    0, so P is one-hot exactly (2^-512 = 0 in f32), its code 128, l = 1, and out[i][c] = V[i][c] exactly. V^T is given as codes and scale
    bytes that together encode (channel, key): the code byte 0x08 + (key % 64) - 64 distinct positive normal codes, one per key position of a
    tile - and the scale byte 32 + 8 sigma, sigma = ((digit_c * 2 + key half) * 2 + tile parity), digit_c = (c / 6^digit) % 6: the value's
    exponent separates sigma from the code's own exponent, and the three digits together identify the channel. A key that met another byte
    position, a block that took the other register half, a scale byte from another channel, key half, tile or op_sel: a different value."""
    _lib = L()
    n = 128
    scale = np.float32(math.log(2.0))
    assert float(scale * LOG2E_F32) == 1.0
    assert _lib.attn_mxpv_plan(n, Lk, D, 1, 1)["kernel"] == KNAME["mx12" if Lk >= 2048 else "mx4"]
    idx = torch.arange(n)
    qc, kc = torch.zeros(n, D, dtype=U8), torch.zeros(Lk, D, dtype=U8)
    qc[idx, idx] = 0x38
    kc[idx, idx] = 0x38
    qs, ks = torch.full((n, 4), 132, dtype=U8), torch.full((Lk, 4), 131, dtype=U8)
    assert torch.equal((mx_dequant(qc, qs) @ mx_dequant(kc, ks).t())[idx, idx], torch.full((n,), 512.0, dtype=F64))
    key, ch = torch.arange(Lk)[None, :], torch.arange(D)[:, None]
    codes = (0x08 + key % 64).to(U8).expand(D, Lk).contiguous()                   # natural order [channel, key]
    blk = torch.arange(Lk // 32)[None, :]
    sigma = ((ch // 6 ** digit % 6) * 2 + blk % 2) * 2 + blk // 2 % 2
    sc = (32 + 8 * sigma).to(U8)
    pairs = codes[:, :128].long() * 256 + sc[:, :4].long().repeat_interleave(32, 1)
    assert len(torch.unique(mx_dequant(codes, sc)[:, :128])) == len(torch.unique(pairs)) >= 64 * 4 and int(sigma.max()) <= 23, "a value names its (code, scale)"
    vc, vs = vt_pack(codes, sc, 1)
    out = torch.full((n, D), SENT, dtype=BF16, device=DEV)
    _lib.flash_attn_mxpv(qc.to(DEV), qs.to(DEV), kc.to(DEV), ks.to(DEV), vc.to(DEV), vs.to(DEV), out, n, Lk, 1, D, float(scale))
    got = out.cpu().double()
    want = mx_dequant(codes, sc)[:, :n].t()                                       # [query = key, channel]
    assert torch.equal(want.to(BF16).double(), want)
    bad = got != want
    if bad.any():
        i, j = (int(t) for t in bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} elements; first: query / key {i} (tile {i // 64} half {i // 32 % 2} position {i % 32}) channel {j} "
                             f"(block {j // 32}): got {got[i, j].item()!r}, expected {want[i, j].item()!r}")


# ---------------------------------------------------------------------------------------------------------------
# 3. the P format from both sides
# ---------------------------------------------------------------------------------------------------------------
def _two_keys(Lk, s_first, s_last, v_first, v_last):
    """One query (1 at head-dim 0 and 1); key 0 scores s_first, the last key - the first of a new tile - s_last, every key between -512
    (P = 0 exactly). -> the launch's result [D] and the fp64 value rounded to bf16"""
    _lib = L()
    assert (Lk - 1) % 64 == 0
    q = torch.zeros(1, D, dtype=F64)
    q[0, :2] = 1
    k = torch.zeros(Lk, D, dtype=F64)
    k[1:Lk - 1, 0] = -512
    for row, s in ((0, s_first), (Lk - 1, s_last)):
        k[row, 0], k[row, 1] = s - s % 2, s % 2                       # 17 = 16 + 1: both exact e4m3 under the block's scale
    v = torch.zeros(Lk, D, dtype=F64)
    v[0], v[Lk - 1] = v_first, v_last
    scale = np.float32(math.log(2.0))
    (qc, qs), (kc, ks) = mx_exact(q.to(BF16)), mx_exact(k.to(BF16))
    vc, vs = vt_pack(*vt_exact(v.to(BF16), 1, Lk), 1)
    out = torch.full((1, D), SENT, dtype=BF16, device=DEV)
    _lib.flash_attn_mxpv(qc.to(DEV), qs.to(DEV), kc.to(DEV), ks.to(DEV), vc.to(DEV), vs.to(DEV), out, 1, Lk, 1, D, float(scale))
    return out.cpu()[0], softmax_ref(q, k, v, scale, 1, 1, 1, Lk)[0]


@gpu
@pytest.mark.parametrize("Lk", [65, 2049])
def test_p_format_from_both_sides(Lk):
    """(a) gap PSHIFT + 9: P 2^PSHIFT = 2^-9, the smallest subnormal e4m3 code - the output is 8 x 2^-(PSHIFT + 9) / (1 + 2^-(PSHIFT + 9)) rounded
    to bf16, not zero. (b) gap PSHIFT + 10: the tie between 0 and 2^-9 rounds to even, the output is exactly 0 (l still counts the P).
    (c) the late key DEFER_PV above the reference: P = 2^DEFER_PV, code 256, no move; (d) DEFER_PV + 1 above: the reference moves. (c) and
    (d) equal the fp64 value rounded to bf16 (13 / 3 and 4.6: not at a rounding boundary)."""
    got, ref = _two_keys(Lk, PSHIFT + 9, 0, 0.0, 8.0)
    want = ref.to(BF16)
    assert float(want[0]) == 8 * 2.0 ** -(PSHIFT + 9) and torch.equal(got, want), f"smallest subnormal code: got {got[0].item()!r}, expected {want[0].item()!r}"
    got, ref = _two_keys(Lk, PSHIFT + 10, 0, 0.0, 8.0)
    assert float(ref[0]) > 0 and bool((got == 0).all()), f"a P of 2^-(PSHIFT + 10) must round to the code 0: got {got[0].item()!r}"
    for s_last in (DEFER_PV, DEFER_PV + 1):
        got, ref = _two_keys(Lk, 0, s_last, 3.0, 5.0)
        assert not bool(_near_boundary(ref, BF16, 2.0 ** -18).any())
        assert torch.equal(got, ref.to(BF16)), f"late key {s_last} above the reference: got {got[0].item()!r}, expected {ref[0].item()!r}"


# ---------------------------------------------------------------------------------------------------------------
# 4. designed families, bit-exact
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_mxpv_kernel_is_bit_exact_on_designed_operands(c):
    ncus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = assert_plan(c, ncus)
    o = _ops(c)
    cond = check_exactness(c, o)
    got = _launch(c, o)
    assert not bool((got == SENT).any()), "part of the result was not written"
    diff = (got.view(torch.int16) != o.ref.view(torch.int16)) & ~((got == 0) & (o.ref == 0))
    in_band = 0
    if o.near is not None:
        assert c.fam in ("A", "spike10", "spike6") and o.stats["excluded_share"] <= 0.005
        in_band = int((diff & o.near).sum())
        diff = diff & ~o.near
    name = IDS[CASES.index(c)]
    print(f"{name}: {plan}; {o.stats}; {cond}; mismatches in the excepted band {in_band}")
    record_margin(f"attn_mxpv/{name}", kernel=plan["kernel"], band_mismatches=in_band, **cond, **o.stats)
    if diff.any():
        i, j = (int(x) for x in diff.nonzero()[0])
        rows = sorted({int(x) for x in diff.nonzero()[:, 0]})
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.numel()} elements differ from the reference, in {len(rows)} rows (first rows {rows[:8]}); "
                             f"first at {_where(c, i, j)}: got {got[i, j].item()!r}, expected {o.ref[i, j].item()!r}")


# ---------------------------------------------------------------------------------------------------------------
# 5. random operands
# ---------------------------------------------------------------------------------------------------------------
def _random_pv(B, H, Lq, Lk, seed):
    """test_attn_mxqk's random problem with V quantised along the keys -> device operands and the fp64 dequantised ones"""
    codes, deq, v, scale, _ = _random_problem(B, H, Lq, Lk, seed)
    vq = vt_ref(v, B, Lk)
    vd = vt_dequant(*vq, B, Lk)
    assert torch.equal(vd.to(BF16).double(), vd)
    return codes, vt_pack(*vq, H), (deq[0].double(), deq[1].double(), vd), scale


@gpu
@pytest.mark.parametrize("B,H,Lq,Lk", [(1, 2, 150, 200), (2, 4, 500, 2104)])
def test_random_operands_against_truth_and_emulation(B, H, Lq, Lk):
    """truth = the fp64 softmax of the dequantised q, k, V; emulation = the format in fp64 (e4m3 P against the TRUE row maximum, unrounded
    denominator). The kernel differs from the emulation in the reference maximum only (it may lag the true one by up to DEFER_PV, which moves
    the e4m3 grid under P) and in v_exp_f32's last bits: the ratio of the two distances from the truth is measured, not derivable, and gated
    at measured x 1.2. First measurement: 1.101 (Lk 200) and 1.417 (Lk 2104) - above 1.05 because the fp64 emulation does not round its
    OUTPUT: over 2 104 keys the P rounding averages out (emulation 8.1e-4) and the bf16 rounding of the output, which the kernel has and
    uv_flash_attn_mxqk has alone (7.9e-4), is what remains (1.15e-3 ~ sqrt(8.1^2 + 7.9^2) e-4). With the emulation rounded to bf16 the ratios
    are 0.9965 and 1.0147; both forms are gated. Recorded beside them: the distance of uv_flash_attn_mxqk (bf16 V and P) on the same
    operands - the price of this half."""
    _lib = L()
    C = H * D
    codes, (vc, vs), (qd, kd, vd), scale = _random_pv(B, H, Lq, Lk, 7 * Lk + Lq)
    assert _lib.attn_mxpv_plan(Lq, Lk, D, B, H)["kernel"] == KNAME["mx12" if Lk >= 2048 else "mx4"]
    qc, qs, kc, ks = (t.to(DEV) for t in codes)
    out_pv, out_qk = (torch.full((B * Lq, C), SENT, dtype=BF16, device=DEV) for _ in range(2))
    _lib.flash_attn_mxpv(qc, qs, kc, ks, vc.to(DEV), vs.to(DEV), out_pv, Lq, Lk, H, D, scale, batch=B)
    vt = torch.zeros(C, (B - 1) * Lk + _up(Lk, 64), dtype=BF16, device=DEV)
    vt[:, :B * Lk] = vd.to(BF16).to(DEV).t()
    _lib.flash_attn_mxqk(qc, qs, kc, ks, vt, out_qk, Lq, Lk, H, D, scale, batch=B)
    truth = softmax_ref(qd, kd, vd, scale, B, H, Lq, Lk)
    emu = emulated_ref(qd, kd, vd, scale, B, H, Lq, Lk)
    pv, qk = out_pv.cpu().double(), out_qk.cpu().double()
    assert bool(torch.isfinite(pv).all())
    rms = lambda a: (a - truth).pow(2).mean().sqrt().item()
    e_pv, e_emu, e_emu16, e_qk = rms(pv), rms(emu), rms(emu.to(BF16).double()), rms(qk)
    m = dict(rms_vs_truth_mxpv=e_pv, rms_vs_truth_emulation=e_emu, rms_vs_truth_emulation_rounded_to_bf16=e_emu16, rms_vs_truth_mxqk=e_qk,
             ratio_mxpv_over_emulation=e_pv / e_emu, ratio_mxpv_over_emulation_rounded_to_bf16=e_pv / e_emu16, ratio_mxpv_over_mxqk=e_pv / e_qk, rel_rms_mxpv_vs_truth=e_pv / truth.pow(2).mean().sqrt().item())
    print(f"random B{B} H{H} Lq{Lq} Lk{Lk}", json.dumps(m))
    record_margin(f"attn_mxpv/random-B{B}H{H}-Lq{Lq}-Lk{Lk}", **m)
    gate, gate16 = GATE_RANDOM[(B, H, Lq, Lk)]
    assert e_pv <= gate * e_emu, f"rms against the truth {e_pv:.4e}, the emulation's {e_emu:.4e}: ratio {e_pv / e_emu:.4f} > {gate:.4f}"
    assert e_pv <= gate16 * e_emu16, f"rms against the truth {e_pv:.4e}, the bf16-rounded emulation's {e_emu16:.4e}: ratio {e_pv / e_emu16:.4f} > {gate16:.4f}"


# ---------------------------------------------------------------------------------------------------------------
# 6. independence and determinism
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Lk", [200, 2104])
def test_a_querys_bits_do_not_depend_on_the_launch(Lk):
    """test_attn_mxqk's method: one launch twice, every cut, each sample alone, 33 queries alone (another unit, another lane, other
    neighbours in the wave: the reference maximum is a query's own decision). The two kernel sizes cannot see the same keys (Lk decides);
    both run the same body on the same per-wave arithmetic and both are covered here."""
    _lib = L()
    B, H, Lq = 2, 4, 500
    C, Lkp = H * D, _up(Lk, 64)
    codes, (vc, vs), _, scale = _random_pv(B, H, Lq, Lk, 11 + Lk)
    qc, qs, kc, ks = (t.to(DEV) for t in codes)
    vc, vs = vc.to(DEV), vs.to(DEV)

    def run(qc_, qs_, kc_, ks_, vc_, vs_, lq, batch):
        out = torch.full((batch * lq, C), SENT, dtype=BF16, device=DEV)
        _lib.flash_attn_mxpv(qc_, qs_, kc_, ks_, vc_, vs_, out, lq, Lk, H, D, scale, batch=batch)
        return out

    base = run(qc, qs, kc, ks, vc, vs, Lq, B)
    assert torch.equal(run(qc, qs, kc, ks, vc, vs, Lq, B), base), "two runs of one launch differ"
    for cut in (1, 2, 3):
        _lib.set_option(_lib.OPT_ATTN_CUT, cut)
        assert torch.equal(run(qc, qs, kc, ks, vc, vs, Lq, B), base), f"cut {cut} changes bits"
    _lib.set_option(_lib.OPT_ATTN_CUT, 0)
    for b in range(B):                                          # batch 2 == two batch-1 launches
        vc1, vs1 = vc[:, b * Lkp:(b + 1) * Lkp].contiguous(), vs[:, 4 * b * Lkp:4 * (b + 1) * Lkp].contiguous()
        one = run(qc[b * Lq:(b + 1) * Lq], qs[b * Lq:(b + 1) * Lq], kc[b * Lk:(b + 1) * Lk], ks[b * Lk:(b + 1) * Lk], vc1, vs1, Lq, 1)
        assert torch.equal(one, base[b * Lq:(b + 1) * Lq]), f"sample {b} alone differs from the stacked launch"
        if b == 0:
            few = run(qc[100:133], qs[100:133], kc[:Lk], ks[:Lk], vc1, vs1, 33, 1)
            assert torch.equal(few, base[100:133]), "33 queries alone differ from the same queries inside 500"


# ---------------------------------------------------------------------------------------------------------------
# 7. rejections write nothing
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_rejections_write_nothing():
    _lib = L()
    Lq, Lk, H = 40, 72, 2
    C, Lkp = H * D, 128
    scale = D ** -0.5
    qcb = torch.zeros(2 * Lq + 8, C + 32, dtype=U8, device=DEV)
    kcb = torch.zeros(2 * Lk + 8, C + 32, dtype=U8, device=DEV)
    qsb = torch.full((2 * Lq + 8, C // 32 + 8), 127, dtype=U8, device=DEV)
    ksb = torch.full((2 * Lk + 8, C // 32 + 8), 127, dtype=U8, device=DEV)
    vcb = torch.full((C + 1, 2 * Lkp + 32), 0xA5, dtype=U8, device=DEV)
    vsb = torch.full((H + 1, 8 * Lkp + 16), 0xA5, dtype=U8, device=DEV)
    vtb = torch.ones(C, 2 * Lk + 64, dtype=BF16, device=DEV)
    full = torch.full((2 * Lq + 8, C), SENT, dtype=BF16, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr
    count = _lib.CALL_COUNT

    def raw(match, vc=vcb, ldvc=vcb.stride(0), vs=vsb, ld_vs=vsb.stride(0), batch=1, H=H, hd=D, ldq=C + 32):
        with pytest.raises(_lib.UnividHipError, match=match) as ei:
            _lib.call("uv_flash_attn_mxpv", p(qcb), ldq, p(qsb), C // 32 + 8, p(kcb), C + 32, p(ksb), C // 32 + 8, p(vc) if vc is not None else None, ldvc,
                      p(vs) if vs is not None else None, ld_vs, p(full), C, batch, Lq, Lk, H, hd, scale, st())
        assert "uv_flash_attn_mxpv" in str(ei.value)

    def rawq(match, vt=vtb, ldvt=vtb.stride(0), vc=vcb, ldvc=vcb.stride(0), vs=vsb, ld_vs=vsb.stride(0), batch=1, Lk=Lk, hd=D):
        with pytest.raises(_lib.UnividHipError, match=match) as ei:
            _lib.call("uv_vt_mx_quant", p(vt), ldvt, p(vc), ldvc, p(vs) if vs is not None else None, ld_vs, batch, Lk, H, hd, st())
        assert "uv_vt_mx_quant" in str(ei.value)

    raw("head_dim 64 unsupported", H=4, hd=64)
    raw("null scale pointer", vs=None)
    raw("null pointer", vc=None)
    raw("ldvc=.* must be", batch=2, ldvc=Lkp)                                # short: two samples need 2 Lkp columns
    raw("ldvc=.* must be", ldvc=Lkp + 8)                                     # no multiple of 16
    raw("ld_vs=.* must be", ld_vs=4 * Lkp - 4)
    raw("16-byte aligned", vc=vcb.view(-1)[8:])
    raw("4-byte aligned", vs=vsb.view(-1)[2:])
    raw("multiples of 16 bytes", ldq=C + 8)
    rawq("head_dim 64 unsupported", hd=64)
    rawq("needs Lk % 8", batch=2, Lk=68)
    rawq("ldvt=.* must be", batch=2, ldvt=Lk + 64)                           # does not cover the second sample
    rawq("ldvc=.* must be", batch=2, ldvc=Lkp)
    rawq("ld_vs=.* must be", ld_vs=4 * Lkp - 4)
    rawq("16-byte aligned", vt=vtb.view(-1)[4:])
    rawq("4-byte aligned", vs=vsb.view(-1)[1:])
    assert _lib.CALL_COUNT == count + 16, "every raw call above reached the library once and was refused there"
    with pytest.raises(_lib.UnividHipError, match="uv_flash_attn_mxpv_plan"):
        _lib.attn_mxpv_plan(Lq, Lk, 64, 1, 4)
    # the wrappers' own checks (dtype / extent): the library is not reached, CALL_COUNT does not move
    count = _lib.CALL_COUNT
    qc, qs, kc, ks = qcb[:Lq, :C], qsb[:Lq, :C // 32], kcb[:Lk, :C], ksb[:Lk, :C // 32]
    with pytest.raises(_lib.UnividHipError, match="flash_attn_mxpv.vt_codes"):
        _lib.flash_attn_mxpv(qc, qs, kc, ks, vcb.view(torch.int8)[:C, :Lkp], vsb[:H, :4 * Lkp], full[:Lq], Lq, Lk, H, D, scale)
    with pytest.raises(_lib.UnividHipError, match="flash_attn_mxpv.vt_scales"):
        _lib.flash_attn_mxpv(qc, qs, kc, ks, vcb[:C, :Lkp], torch.zeros(H, 2 * Lkp, dtype=U8, device=DEV), full[:Lq], Lq, Lk, H, D, scale)
    with pytest.raises(_lib.UnividHipError, match="vt_mx_quant.vt"):
        _lib.vt_mx_quant(vtb.float(), vcb[:C, :Lkp], vsb[:H, :4 * Lkp], Lk, H, D)
    with pytest.raises(_lib.UnividHipError, match="vt_mx_quant.vt_codes"):
        _lib.vt_mx_quant(vtb, torch.zeros(C, Lkp, dtype=U8, device=DEV), vsb[:H, :8 * Lkp], Lk, H, D, batch=2)
    assert _lib.CALL_COUNT == count
    torch.cuda.synchronize()
    assert bool((full == SENT).all()) and bool((vcb == 0xA5).all()) and bool((vsb == 0xA5).all()), "a rejected call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------
# 8. model level
# ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def emulated_mxpv():
    """The oracle in the format, patched at run time: rope_apply quantises-dequantises q and k (emulated_mxqk), and the SELF-attention's core
    (the call that carries k_lens) runs emulated_ref's arithmetic per head on V quantised-dequantised along the keys, rounded to bf16."""
    from oracle import wan_dit
    orig = wan_dit.attention_core

    def core(q, k, v, k_lens=None):
        if k_lens is None:
            return orig(q, k, v)
        b, lq, n, d = q.shape
        lk = k.shape[1]
        assert b == 1 and int(k_lens.min()) == lk and d == D
        qd, kd = q.to(BF16).double().reshape(lq, n * d), k.to(BF16).double().reshape(lk, n * d)
        vb = v.to(BF16).reshape(lk, n * d)
        vd = vt_dequant(*vt_ref(vb, 1, lk), 1, lk)
        out = emulated_ref(qd, kd, vd, d ** -0.5, 1, n, lq, lk)
        return out.to(BF16).reshape(1, lq, n, d).type(q.dtype)

    wan_dit.attention_core = core
    try:
        with emulated_mxqk():
            yield
    finally:
        wan_dit.attention_core = orig


def _block_case(name, x, e_rows, tid, grid, ctx, blk, sdc):
    """One block in the mode against the emulated oracle and the fp32 truth (both on the CPU). Gate: rms(hip - truth) <= GATE_BLOCK x
    rms(emulated oracle - truth) (measured x 1.2). Recorded: the distances from the truth of hip, the emulated oracle, mxfp8_qk and bf16."""
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
    qk = run()
    blk.set_attn_precision("mxfp8_qk_pv")
    got = run()
    assert not torch.equal(got, base) and not torch.equal(got, qk) and torch.isfinite(got).all()
    assert torch.equal(run(), got)
    blk.set_attn_precision("bf16")
    assert torch.equal(run(), base), "bf16 after a round trip through mxfp8_qk_pv must equal the block before the switch"
    args = (sdc, "blocks.0.", x, e_rows[tid].unsqueeze(0), torch.tensor([Lt]), grid, wan_dit.rope_table(d))
    t0 = time.time()
    with torch.no_grad(), emulated_mxpv():
        emu = wan_dit.block_forward(*args, ctx, heads, 1e-6)[0]
    old, wan_dit.BF16 = wan_dit.BF16, torch.float32
    try:
        with torch.no_grad():
            truth = wan_dit.block_forward(*args, ctx.float(), heads, 1e-6)[0]
    finally:
        wan_dit.BF16 = old
    host_s = time.time() - t0
    e_hip, e_emu, e_qk, e_bf = _rms(got, truth), _rms(emu, truth), _rms(qk, truth), _rms(base, truth)
    m = dict(rel_rms_vs_emulated_oracle=_rms(got, emu) / emu.float().pow(2).mean().sqrt().item(), truth_ratio=e_hip / e_emu, rms_vs_truth_mxpv=e_hip,
             rms_vs_truth_emulated_oracle=e_emu, rms_vs_truth_mxqk_mode=e_qk, rms_vs_truth_bf16_mode=e_bf, mxpv_over_bf16_distance_from_truth=e_hip / e_bf,
             mxpv_over_mxqk_distance_from_truth=e_hip / e_qk, oracle_host_seconds=host_s)
    record_margin("mxpv " + name, **m)
    print("mxpv " + name, json.dumps(m))
    assert e_hip <= GATE_BLOCK[name] * e_emu, f"{name}: rms vs truth {e_hip:.4e}, the emulated oracle's {e_emu:.4e}"


@gpu
def test_block_ti2v5b_width_short_kernel():
    g = load_golden("dit_block_3072")
    blk, sdc = _block_3072(g["seed"])
    assert L().attn_mxpv_plan(48, 48, D, 1, 24)["kernel"] == KNAME["mx4"]
    _block_case("block 3072 L48", g["x"], g["e_rows"], g["tid"], g["grid"], g["ctx"], blk, sdc)


@gpu
def test_block_ti2v5b_width_long_kernel():
    """2 304 tokens (grid 4 x 24 x 24): the 12-wave kernel under the model; inputs from detinit. The oracle and its fp32 truth run on the CPU."""
    from univid_amd import detinit
    g = load_golden("dit_block_3072")
    blk, sdc = _block_3072(g["seed"])
    Lt = 2304
    assert L().attn_mxpv_plan(Lt, Lt, D, 1, 24)["kernel"] == KNAME["mx12"]
    x = detinit.uniform_pm1("mxqk.block.x", Lt * 3072, g["seed"]).reshape(1, Lt, 3072).float() * 2
    tid = (torch.arange(Lt) * 7 // Lt % 2).to(g["tid"].dtype)
    _block_case("block 3072 L2304", x, g["e_rows"], tid, torch.tensor([[4, 24, 24]]), g["ctx"], blk, sdc)


@gpu
def test_small_model_cfg_pair_and_round_trip():
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    Lt = 256
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        m.set_attn_precision("mxfp8_qk")
        qk = m([x], t, [ctx], Lt)[0]
        gen = m._prep_gen
        m.set_attn_precision("mxfp8_qk_pv")
        assert m._prep_gen > gen
        got = m([x], t, [ctx], Lt)[0]
        ctx2 = (ctx * 0.5).contiguous()
        other = m([x], t, [ctx2], Lt)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], Lt)
        assert torch.equal(pair[0], got) and torch.equal(pair[1], other) and not torch.equal(got, other), "the stacked CFG pair differs from single forwards"
        assert not torch.equal(got, base) and not torch.equal(got, qk) and torch.isfinite(got).all()
        m.set_ffn_precision("mxfp8")                                       # the modes are independent and combine
        assert not torch.equal(m([x], t, [ctx], Lt)[0], got)
        m.set_ffn_precision("bf16")
        assert torch.equal(m([x], t, [ctx], Lt)[0], got)
        m.set_attn_precision("mxfp8_qk")
        assert torch.equal(m([x], t, [ctx], Lt)[0], qk)
        m.set_attn_precision("bf16")
        assert torch.equal(m([x], t, [ctx], Lt)[0], base), "bf16 after a round trip must equal the model before the switch"


@gpu
def test_small_model_denoise_graph_and_mode_switch():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (2, g["shift"], g["guide_scale"])
    mode = "mxfp8_qk_pv"

    def pipe_in(mode_):
        cfg, sd, m = _small_model(g["seed"])
        return WanTI2V(TI2VConfig, model=m, device=DEV, attn_precision=mode_)

    def gen(pipe, graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    fresh_pv, fresh_qk = pipe_in(mode), pipe_in("mxfp8_qk")
    assert fresh_pv.model.attn_precision == mode and all(b.self_attn.attn_precision == mode for b in fresh_pv.model.blocks)
    pv_graph = gen(fresh_pv, True)
    assert fresh_pv._runner is not None
    assert torch.equal(pv_graph, gen(fresh_pv, False)), "graph != eager in mxfp8_qk_pv mode"
    assert torch.equal(pv_graph, gen(fresh_pv, True)), "a second replay differs"
    qk_graph = gen(fresh_qk, True)
    assert not torch.equal(qk_graph, pv_graph)
    fresh_qk.model.set_attn_precision(mode)                                # a capture made in another mode is not replayed
    assert torch.equal(gen(fresh_qk, True), pv_graph), "after the switch the pipeline does not equal a fresh mxfp8_qk_pv pipeline"
    fresh_qk.model.set_attn_precision("mxfp8_qk")
    assert torch.equal(gen(fresh_qk, True), qk_graph), "after the switch back the pipeline does not equal a fresh mxfp8_qk pipeline"
    fresh_pv._runner = fresh_qk._runner = None


@gpu
def test_unmerged_lora_on_q_k_v_works_in_the_mode(tmp_path):
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    m.set_attn_precision("mxfp8_qk_pv")
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
