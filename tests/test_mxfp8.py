"""The opt-in MXFP8 mode of the DiT's FFN projections (WanModel.set_ffn_precision("mxfp8")): the quantiser uv_mx_quant_bf16, the GEMM
uv_gemm_mxfp8_nt on the block-scaled matrix instruction, and the model / pipeline behaviour. The format's rule (include/univid_hip.h) is
restated here as a CPU emulation (mx_quant_ref / mx_dequant); the model tests put that emulation inside the oracle's two FFN linears."""
import contextlib
import json
import os

import pytest
import torch

from conftest import ROOT, bf16_ulp, load_golden, record_margin
from test_gpu_parity import _rel_rms, _tiny_model, _truth_forward

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
U8 = torch.uint8
DEV = "cuda"
MARGINS = os.path.join(ROOT, "profiles", "mxfp8_parity_margins.json")


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


def L():
    from univid_amd import _lib
    return _lib


# ---- the format, on the CPU -------------------------------------------------------------------------------------------------------
def mx_quant_ref(x):
    """bf16 [M, K] -> (e4m3fn codes uint8 [M, K], e8m0 scales uint8 [M, K / 32]): per block of 32 consecutive K elements
    e = clamp(biased_fp32_exponent(amax) - 8, 0, 254), element = RNE(clamp(x / 2^(e - 127), -448, 448)) to e4m3fn."""
    M, K = x.shape
    xf = x.float().reshape(M, K // 32, 32)
    amax = xf.abs().amax(-1)
    e = (((amax.view(torch.int32) >> 23) & 0xff) - 8).clamp(0, 254)
    scaled = xf.double() / torch.exp2(e.double() - 127).unsqueeze(-1)           # exact: a power of two, in double
    codes = scaled.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(U8).reshape(M, K)
    return codes, e.to(U8)


def mx_dequant(codes, scales):
    M, K = codes.shape
    v = codes.contiguous().view(torch.float8_e4m3fn).double().reshape(M, K // 32, 32) * torch.exp2(scales.double() - 127).unsqueeze(-1)
    return v.reshape(M, K)


def mx_qdq(x):
    """bf16 -> the values the MXFP8 GEMM multiplies, as f32."""
    shp = x.shape
    return mx_dequant(*mx_quant_ref(x.reshape(-1, shp[-1]))).float().reshape(shp)


def gemm_mx(a, a_s, w, w_s, bias, out, epi, **kw):
    return L().gemm_mxfp8(a, a_s, w, w_s, bias, out, epi, **kw)


# ---- 1. lane map, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(16, 256, 128), (257, 256, 384), (1, 512, 256)])
@pytest.mark.parametrize("sparse", ["w", "a"])
def test_lane_map_exact_integers(M, N, K, sparse):
    """Integer codes (exact in e4m3), asymmetric in both operands, scale bytes varying per row and block over powers of two; one operand
    dense and the other with 8 non-zero k per row at positions that move with the row, so every result is an integer below 256 - exact
    in fp32 at every partial sum and in the epilogue's bf16 - while every k position and every row / column is told apart."""
    from univid_amd._lib import EPI_F32_FROM_BF16
    m, n, k = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    a_val = ((m * 3 + k * 5 + (m * k) % 4) % 7 - 3).float()                  # -3 .. 3
    w_val = ((n * 5 + k * 3 + (n + 2 * k) % 3) % 2 + 1).float()              # 1 .. 2
    a_pos = ((k - m * 11) % (K // 8) == 0)
    w_pos = ((k - n * 7) % (K // 8) == 0)
    if sparse == "w":
        w_val = w_val * w_pos
    else:
        a_val = a_val * a_pos
    a_sc = (127 + (m + k[:, ::32] // 32) % 2).to(U8)                          # x1, x2
    w_sc = (127 + (n * 3 + k[:, ::32] // 32) % 2).to(U8)
    a_codes, w_codes = a_val.to(torch.float8_e4m3fn).view(U8), w_val.to(torch.float8_e4m3fn).view(U8)
    assert torch.equal(a_codes.view(torch.float8_e4m3fn).float(), a_val) and torch.equal(w_codes.view(torch.float8_e4m3fn).float(), w_val)
    ref = mx_dequant(a_codes, a_sc) @ mx_dequant(w_codes, w_sc).t()           # fp64
    assert 8 < float(ref.abs().max()) <= 256 and torch.equal(ref, ref.round()) and float(ref.std()) > 2
    assert M == 1 or not torch.equal(ref[0], ref[1]) and not torch.equal(ref[:, 0], ref[:, 1])
    out = torch.full((M, N), -7.0, device=DEV)
    gemm_mx(a_codes.to(DEV), a_sc.to(DEV), w_codes.to(DEV), w_sc.to(DEV), None, out, EPI_F32_FROM_BF16)
    assert torch.equal(out.cpu().double(), ref), f"{int((out.cpu().double() != ref).sum())} of {ref.numel()} elements differ"


# ---- 2. quantiser -----------------------------------------------------------------------------------------------------------------
def _quant_input(M, K, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, ld, generator=g)
    x[:, 7::61] *= 20                                                           # outlier channels
    x = x.to(BF16)
    r = min(3, M - 1)
    x[0, 32:64] = 0                                                             # an all-zero block
    x[r, 64:96] = (torch.rand(32, generator=g) * 3).to(BF16)
    x[r, 70] = 4.0                                                              # amax an exact power of two
    x[0, 96:128] = (torch.rand(32, generator=g) * 1.7).to(BF16)
    x[0, 100], x[0, 101], x[0, 102] = 1.9, -1.99, 1.76                          # scale into (448, 512): clamped to +-448
    sub = torch.arange(1, 33, dtype=torch.int16) * 3                            # bf16 subnormals: a block of them, and some beside normal values
    x[min(1, M - 1), 0:32] = sub.view(BF16)
    x[min(2, M - 1), 0:8] = (sub[:8] | torch.tensor(-32768, dtype=torch.int16)).view(BF16)
    x[min(2, M - 1), 8] = 2.0 ** -120
    return x


@pytest.mark.parametrize("M,K,ld", [(1, 128, 128), (63, 384, 384), (257, 3072, 3072), (300, 14336, 14336 + 64)])
def test_quantiser_bit_exact(M, K, ld):
    x = _quant_input(M, K, ld, M + K)
    codes_ref, scales_ref = mx_quant_ref(x[:, :K])
    assert int(scales_ref[0, 1]) == 0 and int(codes_ref[0, 32:64].sum()) == 0
    assert int(codes_ref[0, 100]) == 0x7E and int(codes_ref[0, 101]) == 0xFE
    xd = x.to(DEV)
    codes = torch.full((M, ld), 0xA5, dtype=U8, device=DEV)
    scales = torch.full((M, K // 32 + 4), 0xA5, dtype=U8, device=DEV)
    L().mx_quant(xd, codes, scales, K=K)
    c, s = codes.cpu(), scales.cpu()
    assert torch.equal(s[:, :K // 32], scales_ref), f"{int((s[:, :K // 32] != scales_ref).sum())} scale bytes differ"
    assert torch.equal(c[:, :K], codes_ref), f"{int((c[:, :K] != codes_ref).sum())} codes differ"
    assert not ((c[:, :K] & 0x7F) == 0x7F).any(), "a NaN code"
    assert (c[:, K:] == 0xA5).all() and (s[:, K // 32:] == 0xA5).all(), "bytes beyond K / K / 32 were written"
    if M == 257:                                                                # launch-independence: rows 5 .. 200 on their own
        c2 = torch.zeros(196, K, dtype=U8, device=DEV)
        s2 = torch.zeros(196, K // 32, dtype=U8, device=DEV)
        L().mx_quant(xd[5:201], c2, s2)
        assert torch.equal(c2, codes[5:201, :K]) and torch.equal(s2, scales[5:201, :K // 32])


# ---- 3. GEMM against the bf16 GEMM on the dequantised operands ----------------------------------------------------------------------
def _gemm_problem(M, N, K, seed):
    """Operands with BOTH signs whose products are all positive (one sign pattern along k for both): the sums do not cancel, so the fp32
    summation-order difference between the two kernels stays far below the 16-bit rounding of the result (a cancelling sum would put the
    f32 error of the partial sums against the spacing of a tiny result, which is a property of the data, not of either kernel)."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
    a = (torch.randn(M, K, generator=g).abs() * 0.5 * sign).to(BF16)
    w = (torch.randn(N, K, generator=g).abs() * (2.0 / K) * sign).to(BF16)
    a[:, 5::97] *= 8
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16)
    return a, w, bias


def _plan_crossing_shape():
    """The planner takes 256x256 tiles once they fill a round of the chip (the ragged last row tile included), 128x128 tiles below that:
    the smallest such problem with 16 column tiles and 40 rows in its last row tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_tiles = 16
    return ((-(-cus // n_tiles) - 1) * 256 + 40, n_tiles * 256, 256)


@pytest.mark.parametrize("shape", [(257, 512, 256), (1014, 3072, 3072), (300, 256, 14336), "plan"])
def test_gemm_vs_bf16_gemm_on_dequantised_operands(shape):
    """e4m3 x 2^e is exact in bf16 here, so uv_gemm_bf16_nt on the dequantised operands multiplies the same numbers exactly and differs
    by the f32 summation order only: every element within 1 ulp of the epilogue's 16-bit rounding. For UV_EPI_BF16 / F32_FROM_BF16 that
    rounding is the output. For the residual epilogues it is the added term y: 1 bf16 ulp of y, times |gate|, plus the f32 roundings of
    the multiply and the add, which the two runs perform on different values (2^-23 of each). For UV_EPI_GELU_BF16 it is the
    pre-activation: two pre-activations 1 ulp apart give exact GELU values at most max|gelu'| = 1.129 ulp(pre) apart, each then rounded
    to the output's grid (half an output ulp each): 1.129 ulp(pre) + 1 ulp(out)."""
    from univid_amd._lib import EPI_BF16, EPI_F32_FROM_BF16, EPI_GATE_RESID_F32, EPI_GELU_BF16, EPI_RESID_F32
    M, N, K = _plan_crossing_shape() if shape == "plan" else shape
    a, w, bias = _gemm_problem(M, N, K, M + N + K)
    (ac, a_s), (wc, w_s) = mx_quant_ref(a), mx_quant_ref(w)
    ad, wd = mx_dequant(ac, a_s), mx_dequant(wc, w_s)
    assert torch.equal(ad.to(BF16).double(), ad) and torch.equal(wd.to(BF16).double(), wd), "dequantised operands must be exact in bf16"
    ad, wd, bias = ad.to(BF16).to(DEV), wd.to(BF16).to(DEV), bias.to(DEV)
    ac, a_s, wc, w_s = ac.to(DEV), a_s.to(DEV), wc.to(DEV), w_s.to(DEV)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(M, N, generator=g).to(DEV)
    gate = torch.randn(3, N, generator=g).to(DEV)
    tid = torch.randint(0, 3, (M,), generator=g, dtype=torch.int32).to(DEV)
    pre = torch.zeros(M, N, dtype=BF16, device=DEV)
    L().gemm_bf16(ad, wd, bias, pre, EPI_BF16)
    for epi, name in ((EPI_BF16, "BF16"), (EPI_GELU_BF16, "GELU_BF16"), (EPI_F32_FROM_BF16, "F32_FROM_BF16"), (EPI_RESID_F32, "RESID_F32"),
                      (EPI_GATE_RESID_F32, "GATE_RESID_F32")):
        f32 = epi in (EPI_F32_FROM_BF16, EPI_RESID_F32, EPI_GATE_RESID_F32)
        rmw = epi in (EPI_RESID_F32, EPI_GATE_RESID_F32)
        kw = dict(gate=gate, gate_tid=tid) if epi == EPI_GATE_RESID_F32 else {}
        outs = []
        for run in (lambda o: L().gemm_bf16(ad, wd, bias, o, epi, **kw), lambda o: gemm_mx(ac, a_s, wc, w_s, bias, o, epi, **kw)):
            o = x0.clone() if rmw else torch.full((M, N), -3.0, device=DEV, dtype=torch.float32 if f32 else BF16)
            run(o)
            outs.append(o.float())
        ref, got = outs
        d = (got - ref).abs()
        if rmw:
            scale = gate[tid.long()].abs() if epi == EPI_GATE_RESID_F32 else 1.0
            tol = bf16_ulp(pre.float()) * scale + (torch.maximum(ref.abs(), got.abs()) + pre.float().abs() * scale) * 2.0 ** -23
        elif epi == EPI_GELU_BF16:
            tol = bf16_ulp(torch.maximum(ref.abs(), got.abs())) + 1.129 * bf16_ulp(pre.float())
        else:
            tol = bf16_ulp(torch.maximum(ref.abs(), got.abs()))
        same = (d == 0).float().mean().item()
        print(f"mxfp8 gemm {M}x{N}x{K} {name}: {same:.5f} identical, max err / tol {float((d / tol).max()):.3f}")
        assert torch.isfinite(got).all() and (d <= tol).all(), f"{name}: {int((d > tol).sum())} elements beyond 1 ulp (max ratio {float((d / tol).max()):.3f})"
        assert same > 0.9, f"{name}: only {same:.4f} identical"
        if shape == "plan" and epi == EPI_BF16:
            # the last 140 rows as a launch of their own (under a round of tiles: the other kernel of the plan): the same bits
            alone = torch.zeros(140, N, dtype=BF16, device=DEV)
            gemm_mx(ac[M - 140:], a_s[M - 140:], wc, w_s, bias, alone, epi)
            assert torch.equal(alone.float(), got[M - 140:]), "a row's bits depend on which kernel of the plan computed it"


# ---- 4. row independence ------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_launch():
    from univid_amd._lib import EPI_BF16
    M, N, K = 600, 512, 512
    g = torch.Generator().manual_seed(4)
    (ac, a_s), (wc, w_s) = mx_quant_ref(torch.randn(M, K, generator=g).to(BF16)), mx_quant_ref((torch.randn(N, K, generator=g) * 0.05).to(BF16))
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16).to(DEV)
    ac, a_s, wc, w_s = ac.to(DEV), a_s.to(DEV), wc.to(DEV), w_s.to(DEV)

    def run(codes, scales):
        out = torch.zeros(codes.shape[0], N, dtype=BF16, device=DEV)
        gemm_mx(codes, scales, wc, w_s, bias, out, EPI_BF16)
        return out

    full = run(ac, a_s)
    assert torch.equal(run(ac, a_s), full), "two identical launches differ"
    assert torch.equal(run(ac[128:385], a_s[128:385]), full[128:385]), "rows [128, 385) depend on the launch they run in"
    poisoned = ac.clone()
    poisoned[300] = 0x7F                                                        # a row of NaN codes
    out = run(poisoned, a_s)
    keep = torch.arange(M, device=DEV) != 300
    assert torch.equal(out[keep], full[keep]) and torch.isnan(out[300].float()).all()


# ---- 5. rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing():
    from univid_amd._lib import EPI_BF16, EPI_BF16_T, UnividHipError, call, ptr, stream_ptr
    M, N, K = 64, 256, 256
    a, a_s = torch.zeros(M, K, dtype=U8, device=DEV), torch.full((M, K // 32), 127, dtype=U8, device=DEV)
    w, w_s = torch.zeros(N + 16, K, dtype=U8, device=DEV), torch.full((N + 16, K // 32), 127, dtype=U8, device=DEV)
    out = torch.full((M, N), 5.0, dtype=BF16, device=DEV)
    keep = out.clone()

    def go(a_=a, as_=a_s, w_=w, ws_=w_s, N_=N, K_=K, epi=EPI_BF16, ld_as=K // 32, out_=out):
        call("uv_gemm_mxfp8_nt", ptr(a_), K, ptr(as_), ld_as, ptr(w_), K, ptr(ws_), K // 32, None, M, N_, K_, epi, ptr(out_), N, None, None, 0,
             stream_ptr())

    for bad in (dict(K_=192), dict(N_=100), dict(as_=None), dict(ws_=None), dict(ld_as=4), dict(a_=a.view(-1)[8:]), dict(epi=EPI_BF16_T),
                dict(epi=6), dict(epi=-1)):
        with pytest.raises(UnividHipError) as ei:
            go(**bad)
        assert "uv_gemm_mxfp8_nt:" in str(ei.value) and len(str(ei.value)) > 40
    x = torch.zeros(M, K, dtype=BF16, device=DEV)
    codes, scales = torch.full((M, K), 9, dtype=U8, device=DEV), torch.full((M, K // 32), 9, dtype=U8, device=DEV)
    for args in ((x, K, codes, K, scales, K // 32, M, 192), (x, K, codes, K, scales, 4, M, K), (x, K, codes, K, None, K // 32, M, K),
                 (x.view(-1)[4:], K, codes, K, scales, K // 32, M - 1, K)):
        with pytest.raises(UnividHipError) as ei:
            call("uv_mx_quant_bf16", ptr(args[0]), args[1], ptr(args[2]), args[3], ptr(args[4]), args[5], args[6], args[7], stream_ptr())
        assert "uv_mx_quant_bf16:" in str(ei.value)
    torch.cuda.synchronize()
    assert torch.equal(out, keep) and (codes == 9).all() and (scales == 9).all(), "a rejected call wrote something"
    go()
    torch.cuda.synchronize()
    assert not torch.equal(out, keep)


# ---- the emulated oracle ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def emulated_mxfp8_ffn():
    """The oracle with its two FFN linears computing on quantise-dequantise operands (activations and the bf16 weight copy alike), fp32
    accumulate, bf16(acc + bias): the arithmetic of uv_gemm_mxfp8_nt up to the summation order."""
    from oracle import wan_dit
    orig, cache = wan_dit.lin, {}

    def lin(sd, key, x):
        if not (key.endswith("ffn.0") or key.endswith("ffn.2")):
            return orig(sd, key, x)
        if key not in cache:
            cache[key] = mx_qdq(sd[key + ".weight"].to(BF16))
        y = torch.nn.functional.linear(mx_qdq(x.to(BF16)), cache[key]) + sd[key + ".bias"].to(BF16).float()
        return y.to(BF16)

    wan_dit.lin = lin
    try:
        yield
    finally:
        wan_dit.lin = orig


def _gate(name):
    """(b): rel_rms(hip_mxfp8, emulated oracle) <= measured x 1.2 (profiles/mxfp8_parity_margins.json, measured on MI355X)."""
    with open(MARGINS) as f:
        return 1.2 * float(json.load(f)[name]["rel_rms_vs_emulated_oracle"])


def _rms(a, b):
    return (a.float().cpu() - b.float().cpu()).pow(2).mean().sqrt().item()


def _check_mode(name, hip_mx, hip_bf16, emu, truth, ref_bf16):
    """Gates (a) truth ratio <= 1.02 and (b) the margin against the emulated oracle; records the mode's distance from the truth
    relative to the bf16 mode's."""
    e_hip, e_emu, e_bf = _rms(hip_mx, truth), _rms(emu, truth), _rms(hip_bf16, truth)
    rel = _rel_rms(hip_mx, emu)
    m = dict(rel_rms_vs_emulated_oracle=rel, truth_ratio=e_hip / e_emu, rms_vs_truth_mxfp8=e_hip, rms_vs_truth_emulated_oracle=e_emu,
             rms_vs_truth_bf16_mode=e_bf, mxfp8_over_bf16_distance_from_truth=e_hip / e_bf,
             rel_rms_bf16_mode_vs_bf16_oracle=_rel_rms(hip_bf16, ref_bf16), truth_rms=truth.float().pow(2).mean().sqrt().item())
    record_margin("mxfp8 " + name, **m)
    print("mxfp8 " + name, json.dumps(m))
    assert torch.isfinite(hip_mx).all()
    assert e_hip <= 1.02 * e_emu, f"{name}: rms vs truth {e_hip:.4e}, the emulated oracle's {e_emu:.4e}"
    assert rel <= _gate(name), f"{name}: rel rms vs the emulated oracle {rel:.4e} > gate {_gate(name):.4e}"


# ---- 7. one block at production width -----------------------------------------------------------------------------------------------
def test_block_ti2v5b_width():
    from oracle import wan_dit
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device, rope_params
    g = load_golden("dit_block_3072")
    dim, ffn, heads, Lt = 3072, 14336, 24, 48
    with torch.device(DEV):
        blk = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
        never = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, g["seed"])
    never.load_state_dict(blk.state_dict())
    blk.eval(), never.eval()
    d = dim // heads
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    fr = _freqs_device(freqs, torch.device(DEV))
    e0 = g["e_rows"][g["tid"]].unsqueeze(0)
    seq_lens = torch.tensor([Lt])

    def run(b):
        x = g["x"][0].to(DEV).clone()
        with torch.no_grad():
            b._run(x, Lt, g["e_rows"].reshape(2, -1).to(DEV), g["tid"].to(torch.int32).to(DEV), (2, 4, 6), fr, g["ctx"][0].to(DEV), first_block=False)
        return x

    base = run(never)
    blk.set_ffn_precision("mxfp8")
    got = run(blk)
    assert blk._prep["ffn0"].w.dtype == U8 and not torch.equal(got, base)
    blk.set_ffn_precision("bf16")
    assert torch.equal(run(blk), base), "bf16 after a round trip through mxfp8 must equal a block that never switched"
    sdc = {k: v.detach().cpu() for k, v in sd.items()}
    args = (sdc, "blocks.0.", g["x"], e0, seq_lens, g["grid"], wan_dit.rope_table(d))
    with torch.no_grad(), emulated_mxfp8_ffn():
        emu = wan_dit.block_forward(*args, g["ctx"], heads, 1e-6)[0]
    old, wan_dit.BF16 = wan_dit.BF16, torch.float32
    try:
        with torch.no_grad():
            truth = wan_dit.block_forward(*args, g["ctx"].float(), heads, 1e-6)[0]
    finally:
        wan_dit.BF16 = old
    _check_mode("block 3072", got, base, emu, truth, g["out_f32"][0])


# ---- 8. tiny model end to end -------------------------------------------------------------------------------------------------------
def test_tiny_forward_and_cfg_pair():
    from oracle import wan_dit
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    Lt = 256
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        m.set_ffn_precision("mxfp8")
        got = m([x], t, [ctx], Lt)[0]
        ctx2 = (ctx * 0.5).contiguous()
        other = m([x], t, [ctx2], Lt)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], Lt)
        truth = _truth_forward(sd, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
        with emulated_mxfp8_ffn():
            emu = wan_dit.dit_forward(sd, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
    assert torch.equal(pair[0], got) and torch.equal(pair[1], other) and not torch.equal(got, other), "the stacked CFG pair differs from single forwards"
    assert not torch.equal(got, base)
    _check_mode("tiny forward", got, base, emu, truth, g["out_one"])


def test_tiny_denoise_graph_and_mode_switch():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (4, g["shift"], g["guide_scale"])

    def pipe_in(mode):
        cfg, sd, m = _tiny_model(g["seed"])
        return WanTI2V(TI2VConfig, model=m, device=DEV, ffn_precision=mode)

    def gen(pipe, graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    fresh_mx, fresh_bf = pipe_in("mxfp8"), pipe_in("bf16")
    assert fresh_mx.model.ffn_precision == "mxfp8" and all(b.ffn_precision == "mxfp8" for b in fresh_mx.model.blocks)
    mx_graph = gen(fresh_mx, True)
    assert fresh_mx._runner is not None
    assert torch.equal(mx_graph, gen(fresh_mx, False)), "graph != eager in mxfp8 mode"
    bf_graph = gen(fresh_bf, True)
    assert not torch.equal(bf_graph, mx_graph)
    # one pipeline, the mode switched between two generations: the captured graph of the other mode must not be replayed
    fresh_bf.model.set_ffn_precision("mxfp8")
    assert torch.equal(gen(fresh_bf, True), mx_graph), "after the switch to mxfp8 the pipeline does not equal a fresh mxfp8 pipeline"
    fresh_bf.model.set_ffn_precision("bf16")
    assert torch.equal(gen(fresh_bf, True), bf_graph), "after the switch back the pipeline does not equal a fresh bf16 pipeline"
    fresh_mx._runner = fresh_bf._runner = None


def test_merged_lora_is_requantised_and_attention_adapters_stay_unmerged(tmp_path):
    """Merged adapters on the FFN are re-quantised; an un-merged adapter on the attention projections keeps working in mxfp8 mode."""
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    m.set_ffn_precision("mxfp8")
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    names = [f"blocks.{i}.{p}" for i in range(cfg["num_layers"]) for p in ("ffn.0", "ffn.2")]
    attn = [f"blocks.{i}.self_attn.{p}" for i in range(cfg["num_layers"]) for p in ("q", "o")]
    _write_adapter(str(tmp_path / "F"), _lora_factors(cfg, names, 8, 5, b_std=0.2), 8, 16)
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, attn, 8, 6, b_std=0.2), 8, 16)
    mgr = LoRAManager()
    with torch.no_grad():
        base = m([x], t, [ctx], 256)[0]
        with pytest.raises(NotImplementedError):
            mgr.load_lora_weights(str(tmp_path / "F"), m, merge=False, name="F")
        assert torch.equal(m([x], t, [ctx], 256)[0], base)
        mgr.load_lora_weights(str(tmp_path / "A"), m, merge=False, name="A")
        with_a = m([x], t, [ctx], 256)[0]
        assert not torch.equal(with_a, base)
        mgr.unload("A")
        assert torch.equal(m([x], t, [ctx], 256)[0], base)
        mgr.load_lora_weights(str(tmp_path / "F"), m)                           # merged: the FFN weights change and are re-quantised
        assert not torch.equal(m([x], t, [ctx], 256)[0], base)
