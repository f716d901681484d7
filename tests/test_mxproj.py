"""The opt-in MXFP8 mode of the DiT's attention projections (WanModel.set_proj_precision("mxfp8")): the LayerNorm + modulation producer
that stores MXFP8 (uv_layernorm_mod_mx), the two epilogues the attention projections need on MXFP8 operands (uv_gemm_mxfp8_nt_t,
uv_gemm_mxfp8_nt_ssq), and the model / pipeline behaviour. Every kernel here is DEFINED by bytes another entry point writes, so the kernel
tests are byte comparisons; the model tests put the format's CPU emulation (tests/test_mxfp8.py) inside the oracle's six projections."""
import contextlib
import json
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden, record_margin
from test_gpu_parity import _rel_rms, _tiny_model, _truth_forward
from test_mxfp8 import _gemm_problem, _plan_crossing_shape, _rms, mx_qdq, mx_quant_ref

pytestmark = pytest.mark.gpu

BF16, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
DEV = "cuda"
MARGINS = os.path.join(ROOT, "profiles", "mxproj_parity_margins.json")


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


def L():
    from univid_amd import _lib
    return _lib


# ---- 1. uv_layernorm_mod_mx is its definition ---------------------------------------------------------------------------------------
LN_TABLE = [(1, 256, 1, 0, "none"), (5, 256, 2, 0, "-"), (63, 1024, 1, 1, "mixed"), (257, 3072, 1, 0, "mixed"), (257, 3072, 2, 0, "-"),
            (9, 3072, 1, 1, "none"), (6, 4096, 1, 0, "none"), (3, 8192, 2, 0, "-")]


@pytest.mark.parametrize("rows,C,mode,round_ln,tids", LN_TABLE, ids=[f"L{c[0]}-C{c[1]}-m{c[2]}-r{c[3]}-{c[4]}" for c in LN_TABLE])
def test_layernorm_mod_mx_is_layernorm_mod_then_mx_quant(rows, C, mode, round_ln, tids):
    """Codes and scales byte-equal to _lib.layernorm_mod (bf16) followed by _lib.mx_quant, and to the format rule restated on the CPU applied
    to that bf16 output; pad columns (ldc = C + 64, ld_s = C / 32 + 4) keep their sentinel bytes."""
    g = torch.Generator().manual_seed(rows * 7 + C + mode)
    x = torch.randn(rows, C, generator=g) * torch.exp2(torch.linspace(-6, 6, rows)).unsqueeze(1)      # rows span 2^-6 .. 2^6
    x[rows // 2] = 3.25                                                                                  # one constant row
    n_t = 3
    # parameters whose magnitude moves along the columns, so that the blocks of a row take different scale bytes
    col = torch.exp2(torch.linspace(-5, 5, C))
    tab = torch.randn(n_t, 2 * C, generator=g) * torch.cat([col, col.flip(0)])
    w, b = torch.randn(C, generator=g) * col, torch.randn(C, generator=g) * col.flip(0)
    if mode == 2:
        w[64:96] = 0                                                                                     # an all-zero block: w = b = 0
        b[64:96] = 0
    tid = None
    if tids == "mixed":
        tid = torch.randint(0, n_t, (rows,), generator=g, dtype=torch.int32)
        if rows > 8:
            tid[4], tid[5], tid[6] = 0, 1, 2                                                            # differ from their 4-row group's first row
            assert len(set(tid[4:8].tolist())) > 1
    kw = dict(mode=mode, round_ln=bool(round_ln))
    if mode == 1:
        kw.update(tab=tab.to(DEV), shift_off=0, scale_off=C, tid=None if tid is None else tid.to(DEV))
    else:
        kw.update(w=w.to(DEV), b=b.to(DEV))
    xd = x.to(DEV)
    ref = torch.zeros(rows, C, dtype=BF16, device=DEV)
    L().layernorm_mod(xd, ref, rows, C, 1e-6, **kw)
    ldc, ld_s = C + 64, C // 32 + 4
    c2, s2 = torch.full((rows, ldc), 0xA5, dtype=U8, device=DEV), torch.full((rows, ld_s), 0xA5, dtype=U8, device=DEV)
    L().mx_quant(ref, c2, s2, K=C)
    codes, scales = torch.full((rows, ldc), 0xA5, dtype=U8, device=DEV), torch.full((rows, ld_s), 0xA5, dtype=U8, device=DEV)
    L().layernorm_mod_mx(xd, codes, scales, rows, C, 1e-6, **kw)
    c, s = codes.cpu(), scales.cpu()
    assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 1
    assert torch.equal(s, s2.cpu()), f"{int((s != s2.cpu()).sum())} scale bytes differ from layernorm_mod + mx_quant"
    assert torch.equal(c, c2.cpu()), f"{int((c != c2.cpu()).sum())} codes differ from layernorm_mod + mx_quant"
    codes_ref, scales_ref = mx_quant_ref(ref.cpu())
    assert torch.equal(s[:, :C // 32], scales_ref) and torch.equal(c[:, :C], codes_ref), "the bytes differ from the format rule on the bf16 output"
    assert (c[:, C:] == 0xA5).all() and (s[:, C // 32:] == 0xA5).all(), "bytes beyond C / C / 32 were written"
    assert not ((c[:, :C] & 0x7F) == 0x7F).any(), "a NaN code"
    assert len(set(scales_ref.flatten().tolist())) > 4, "the case must exercise several scale bytes"
    if mode == 2:
        assert (s[:, 2] == 0).all() and (c[:, 64:96] == 0).all(), "an all-zero block: scale byte 0, codes 0"


# ---- 2. / 3. the two epilogues --------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(257, 512, 256), (1014, 3072, 3072), "plan", (6, 256, 128)]
_problems = {}


def _problem(shape):
    """Quantised operands, bias and the UV_EPI_BF16 output of uv_gemm_mxfp8_nt for one shape: computed once, shared, never written."""
    if shape not in _problems:
        from univid_amd._lib import EPI_BF16
        M, N, K = _plan_crossing_shape() if shape == "plan" else shape
        a, w, bias = _gemm_problem(M, N, K, M + N + K)
        (ac, a_s), (wc, w_s) = mx_quant_ref(a), mx_quant_ref(w)
        ops = tuple(t.to(DEV) for t in (ac, a_s, wc, w_s, bias))
        out = torch.zeros(M, N, dtype=BF16, device=DEV)
        L().gemm_mxfp8(*ops[:4], ops[4], out, EPI_BF16)
        _problems[shape] = (M, N, K, ops, out)
    return _problems[shape]


def ssq_ref(out):
    """The header's one summation order, in separate fp32 multiplies and adds: quad sums ((x0^2 + x1^2) + x2^2) + x3^2 over the 8 quads of
    a 32-column group, u_f = s_f + s_(4+f), G = (u0 + u1) + (u2 + u3)."""
    M, N = out.shape
    x = out.float().cpu().reshape(M, N // 32, 8, 4)
    sq = x * x
    s = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    u = s[..., :4] + s[..., 4:]
    return (u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=str)
def test_gemm_mxfp8_t_is_the_transposed_bf16_epilogue(shape):
    M, N, K, (ac, a_s, wc, w_s, bias), out = _problem(shape)
    ldo = (M + 7) // 8 * 8 + 8
    out_t = torch.full((N, ldo), -7.0, dtype=BF16, device=DEV)
    L().gemm_mxfp8_t(ac, a_s, wc, w_s, bias, out_t, M=M)
    assert torch.equal(out_t[:, :M].view(torch.int16), out.t().view(torch.int16)), \
        f"{int((out_t[:, :M].view(torch.int16) != out.t().view(torch.int16)).sum())} of {M * N} elements differ from UV_EPI_BF16"
    assert (out_t[:, M:] == -7.0).all(), "the pad columns were written"
    assert float(out.float().abs().max()) > 0.5


def test_gemm_mxfp8_t_and_ssq_rejections_write_nothing():
    from univid_amd._lib import UnividHipError, call, ptr, stream_ptr
    M, N, K = 64, 256, 256
    a, a_s = torch.zeros(M, K, dtype=U8, device=DEV), torch.full((M, K // 32), 127, dtype=U8, device=DEV)
    w, w_s = torch.zeros(N, K, dtype=U8, device=DEV), torch.full((N, K // 32), 127, dtype=U8, device=DEV)
    out_t, out = torch.full((N, M), 5.0, dtype=BF16, device=DEV), torch.full((M, N), 5.0, dtype=BF16, device=DEV)
    ssq = torch.full((M, N // 32), 5.0, device=DEV)
    for bad in (dict(K=192), dict(N=100), dict(ld_as=4)):
        k = dict(dict(K=K, N=N, ld_as=K // 32), **bad)
        with pytest.raises(UnividHipError, match="uv_gemm_mxfp8_nt_t:"):
            call("uv_gemm_mxfp8_nt_t", ptr(a), K, ptr(a_s), k["ld_as"], ptr(w), K, ptr(w_s), K // 32, None, M, k["N"], k["K"], ptr(out_t), M, stream_ptr())
        with pytest.raises(UnividHipError, match="uv_gemm_mxfp8_nt_ssq:"):
            call("uv_gemm_mxfp8_nt_ssq", ptr(a), K, ptr(a_s), k["ld_as"], ptr(w), K, ptr(w_s), K // 32, None, M, k["N"], k["K"], ptr(out), N, ptr(ssq),
                 N // 32, stream_ptr())
    with pytest.raises(UnividHipError, match="uv_gemm_mxfp8_nt_ssq:"):
        call("uv_gemm_mxfp8_nt_ssq", ptr(a), K, ptr(a_s), K // 32, ptr(w), K, ptr(w_s), K // 32, None, M, N, K, ptr(out), N, None, N // 32, stream_ptr())
    torch.cuda.synchronize()
    assert (out_t == 5.0).all() and (out == 5.0).all() and (ssq == 5.0).all(), "a rejected call wrote something"


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=str)
def test_gemm_mxfp8_ssq_output_and_sums_of_squares(shape):
    M, N, K, (ac, a_s, wc, w_s, bias), out = _problem(shape)
    got = torch.full((M, N), -7.0, dtype=BF16, device=DEV)
    ssq = torch.full((M, N // 32 + 3), -7.0, device=DEV)
    L().gemm_mxfp8_ssq(ac, a_s, wc, w_s, bias, got, ssq, M=M)
    assert torch.equal(got.view(torch.int16), out.view(torch.int16)), "out differs from UV_EPI_BF16's bits"
    ref = ssq_ref(got)
    s = ssq.cpu()
    assert torch.equal(s[:, :N // 32].view(torch.int32), ref.view(torch.int32)), \
        f"{int((s[:, :N // 32] != ref).sum())} of {ref.numel()} sums differ from the stated order"
    assert (s[:, N // 32:] == -7.0).all(), "columns beyond N / 32 of ssq were written"


# ---- 4. rows do not depend on the launch --------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_launch():
    M, N, K = 600, 512, 512
    g = torch.Generator().manual_seed(4)
    (ac, a_s), (wc, w_s) = mx_quant_ref(torch.randn(M, K, generator=g).to(BF16)), mx_quant_ref((torch.randn(N, K, generator=g) * 0.05).to(BF16))
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16).to(DEV)
    ac, a_s, wc, w_s = ac.to(DEV), a_s.to(DEV), wc.to(DEV), w_s.to(DEV)

    def run_t(codes, scales):
        m = codes.shape[0]
        o = torch.zeros(N, (m + 7) // 8 * 8, dtype=BF16, device=DEV)
        L().gemm_mxfp8_t(codes, scales, wc, w_s, bias, o, M=m)
        return o[:, :m]

    def run_ssq(codes, scales):
        m = codes.shape[0]
        o, q = torch.zeros(m, N, dtype=BF16, device=DEV), torch.zeros(m, N // 32, device=DEV)
        L().gemm_mxfp8_ssq(codes, scales, wc, w_s, bias, o, q)
        return o, q

    full_t = run_t(ac, a_s)
    assert torch.equal(run_t(ac[128:385], a_s[128:385]), full_t[:, 128:385]), "V^T: rows [128, 385) depend on the launch they run in"
    full_o, full_q = run_ssq(ac, a_s)
    o, q = run_ssq(ac[128:385], a_s[128:385])
    assert torch.equal(o, full_o[128:385]) and torch.equal(q, full_q[128:385]), "ssq: rows [128, 385) depend on the launch they run in"
    assert torch.equal(full_t, full_o.t())


# ---- the emulated oracle ------------------------------------------------------------------------------------------------------------
_PROJ = re.compile(r"(self_attn\.[qkvo]|cross_attn\.[qo])$")


@contextlib.contextmanager
def emulated_mxfp8_proj():
    """The oracle with its six covered projections computing on quantise-dequantise operands (activations and the bf16 weight copy alike),
    fp32 accumulate, bf16(acc + bias): the arithmetic of the MXFP8 GEMMs up to the summation order. Patched from here: oracle/ is untouched."""
    from oracle import wan_dit
    orig, cache = wan_dit.lin, {}

    def lin(sd, key, x):
        if not _PROJ.search(key):
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
    """(b): rel_rms(hip mode, emulated oracle) <= measured x 1.2 (profiles/mxproj_parity_margins.json, measured on MI355X)."""
    with open(MARGINS) as f:
        return 1.2 * float(json.load(f)[name]["rel_rms_vs_emulated_oracle"])


def _check_mode(name, hip_mx, hip_bf16, emu, truth, ref_bf16):
    """Gates (a) truth ratio <= 1.02 and (b) the margin against the emulated oracle; records the mode's distance from the truth relative to
    the bf16 mode's (the price README quotes)."""
    e_hip, e_emu, e_bf = _rms(hip_mx, truth), _rms(emu, truth), _rms(hip_bf16, truth)
    rel = _rel_rms(hip_mx, emu)
    m = dict(rel_rms_vs_emulated_oracle=rel, truth_ratio=e_hip / e_emu, rms_vs_truth_mxfp8=e_hip, rms_vs_truth_emulated_oracle=e_emu,
             rms_vs_truth_bf16_mode=e_bf, mxfp8_over_bf16_distance_from_truth=e_hip / e_bf,
             rel_rms_bf16_mode_vs_bf16_oracle=_rel_rms(hip_bf16, ref_bf16), truth_rms=truth.float().pow(2).mean().sqrt().item())
    record_margin("mxproj " + name, **m)
    print("mxproj " + name, json.dumps(m))
    assert torch.isfinite(hip_mx).all()
    assert e_hip <= 1.02 * e_emu, f"{name}: rms vs truth {e_hip:.4e}, the emulated oracle's {e_emu:.4e}"
    assert rel <= _gate(name), f"{name}: rel rms vs the emulated oracle {rel:.4e} > gate {_gate(name):.4e}"


# ---- 5. one block at production width -----------------------------------------------------------------------------------------------
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
    blk.set_proj_precision("mxfp8")
    got = run(blk)
    sa, ca = blk.self_attn._prep, blk.cross_attn._prep
    assert all(sa[n].w.dtype == U8 for n in "qkvo") and ca["q"].w.dtype == U8 and ca["o"].w.dtype == U8 and ca["k"].w.dtype == BF16
    assert not torch.equal(got, base)
    blk.set_proj_precision("bf16")
    assert torch.equal(run(blk), base), "bf16 after a round trip through mxfp8 must equal a block that never switched"
    sdc = {k: v.detach().cpu() for k, v in sd.items()}
    args = (sdc, "blocks.0.", g["x"], e0, seq_lens, g["grid"], wan_dit.rope_table(d))
    with torch.no_grad(), emulated_mxfp8_proj():
        emu = wan_dit.block_forward(*args, g["ctx"], heads, 1e-6)[0]
    old, wan_dit.BF16 = wan_dit.BF16, torch.float32
    try:
        with torch.no_grad():
            truth = wan_dit.block_forward(*args, g["ctx"].float(), heads, 1e-6)[0]
    finally:
        wan_dit.BF16 = old
    _check_mode("block 3072", got, base, emu, truth, g["out_f32"][0])


# ---- 6. tiny model end to end -------------------------------------------------------------------------------------------------------
def test_tiny_forward_and_cfg_pair():
    from oracle import wan_dit
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    Lt = 256
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    with torch.no_grad():
        base = m([x], t, [ctx], Lt)[0]
        m.set_proj_precision("mxfp8")
        got = m([x], t, [ctx], Lt)[0]
        ctx2 = (ctx * 0.5).contiguous()
        other = m([x], t, [ctx2], Lt)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], Lt)
        truth = _truth_forward(sd, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
        with emulated_mxfp8_proj():
            emu = wan_dit.dit_forward(sd, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
    assert torch.equal(pair[0], got) and torch.equal(pair[1], other) and not torch.equal(got, other), "the stacked CFG pair differs from single forwards"
    assert not torch.equal(got, base)
    _check_mode("tiny forward", got, base, emu, truth, g["out_one"])


def test_all_three_mxfp8_modes_together_graph_equals_eager():
    """proj + ffn + attention ("mxfp8_qk_pv") on one model (two heads of 128: the attention mode's geometry): finite, graph == eager."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    cfg, sd, m = _tiny_model(g["seed"], num_heads=2)
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV, ffn_precision="mxfp8", attn_precision="mxfp8_qk_pv", proj_precision="mxfp8")

    def gen(graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], 2, g["shift"], g["guide_scale"],
                                graph=graph).clone()

    a = gen(True)
    assert pipe._runner is not None and torch.isfinite(a).all()
    assert torch.equal(a, gen(False)), "graph != eager with the three MXFP8 modes on"
    pipe._runner = None


# ---- 7. denoise ---------------------------------------------------------------------------------------------------------------------
def test_tiny_denoise_graph_mode_switch_and_closure_path():
    import logging
    from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    args = (4, g["shift"], g["guide_scale"])

    def pipe_in(mode):
        cfg, sd, m = _tiny_model(g["seed"])
        return WanTI2V(TI2VConfig, model=m, device=DEV, proj_precision=mode)

    def gen(pipe, graph):
        with torch.no_grad():
            return pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()], *args, graph=graph).clone()

    fresh_mx, fresh_bf = pipe_in("mxfp8"), pipe_in("bf16")
    assert fresh_mx.model.proj_precision == "mxfp8" and all(b.self_attn.proj_precision == "mxfp8" for b in fresh_mx.model.blocks)
    mx_graph = gen(fresh_mx, True)
    assert fresh_mx._runner is not None
    assert torch.equal(mx_graph, gen(fresh_mx, False)), "graph != eager in the mode"
    bf_graph = gen(fresh_bf, True)
    assert not torch.equal(bf_graph, mx_graph)
    # one pipeline, the mode switched between two generations: neither the captured graph nor the cached K / V^T of the other mode comes back
    fresh_bf.model.set_proj_precision("mxfp8")
    assert torch.equal(gen(fresh_bf, True), mx_graph), "after the switch the pipeline does not equal a fresh pipeline of the mode"
    fresh_bf.model.set_proj_precision("bf16")
    assert torch.equal(gen(fresh_bf, True), bf_graph), "after the switch back the pipeline does not equal a fresh bf16 pipeline"
    # the reference's closures (native=False: `forward` re-assigned on every cross-attention) against the native text weight, in the mode
    res = {}
    for native in (False, True):
        ccfg = CrossAttentionConfig(use_dynamic_text_weight=True, total_sampling_steps=8, text_weight_transition_ratio=0.5)
        wr = Wan22ContextWrapper(fresh_mx, None, logging.getLogger("test_mxproj"), ccfg, native=native)
        wr.set_bagel_context(torch.zeros(1, 4, 8))
        assert native or all("forward" in b.cross_attn.__dict__ for b in fresh_mx.model.blocks)
        with torch.no_grad(), wr.scheduled():
            res[native] = fresh_mx.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], *args).clone()
        wr.restore_original_methods()
    assert torch.equal(res[True], res[False]), "the closure path differs from the native path in the mode"
    assert not torch.equal(res[True], mx_graph), "the text weight must change the result"
    fresh_mx._runner = fresh_bf._runner = None


# ---- 8. LoRA ------------------------------------------------------------------------------------------------------------------------
def test_merged_lora_is_requantised_and_unload_restores(tmp_path):
    from test_gpu_parity import _lora_factors, _write_adapter
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    m.set_proj_precision("mxfp8")
    x, t, ctx = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    attn = [f"blocks.{i}.self_attn.{p}" for i in range(cfg["num_layers"]) for p in ("q", "o")]
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, attn, 8, 6, b_std=0.2), 8, 16)
    mgr = LoRAManager()
    with torch.no_grad():
        base = m([x], t, [ctx], 256)[0]
        with pytest.raises(NotImplementedError):
            mgr.load_lora_weights(str(tmp_path / "A"), m, merge=False, name="A")
        assert torch.equal(m([x], t, [ctx], 256)[0], base)
        codes = m.blocks[0].self_attn._prep["q"].w.clone()
        mgr.load_lora_weights(str(tmp_path / "A"), m)                           # merged: the weights change and are re-quantised
        assert not torch.equal(m([x], t, [ctx], 256)[0], base)
        assert m.blocks[0].self_attn._prep["q"].w.dtype == U8 and not torch.equal(m.blocks[0].self_attn._prep["q"].w, codes)
        mgr.unload()
        assert torch.equal(m([x], t, [ctx], 256)[0], base), "unload must restore the base bits"
        assert torch.equal(m.blocks[0].self_attn._prep["q"].w, codes)


# ---- 9. the FFN mode's new producer -------------------------------------------------------------------------------------------------
def test_ffn_mode_producer_equals_the_two_pass_producer(monkeypatch):
    """ffn_precision "mxfp8" alone: ffn.0's input now comes from uv_layernorm_mod_mx. One block's output must be bit-equal to the same block
    run with the two-pass producer - _lib.layernorm_mod into a bf16 buffer, then _lib.mx_quant - in front of the same GEMMs."""
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device, rope_params
    dim, ffn, heads, Lt, Lc = 256, 512, 2, 96, 16
    with torch.device(DEV):
        blk = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
    detinit.init_state_dict_({"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}, 3)
    blk.eval()
    blk.set_ffn_precision("mxfp8")
    d = dim // heads
    fr = _freqs_device(torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1),
                       torch.device(DEV))
    gen = torch.Generator().manual_seed(9)
    x0 = torch.randn(Lt, dim, generator=gen).to(DEV)
    e_rows = (torch.randn(2, 6 * dim, generator=gen) * 0.3).to(DEV)
    tid = (torch.arange(Lt) % 2).to(torch.int32).to(DEV)
    ctx = torch.randn(Lc, dim, generator=gen).to(BF16).to(DEV)

    def run():
        x = x0.clone()
        with torch.no_grad():
            blk._run(x, Lt, e_rows, tid, (2, 6, 8), fr, ctx, first_block=False)
        return x

    calls = []
    real = L().layernorm_mod_mx

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(L(), "layernorm_mod_mx", counted)
    fused = run()
    assert len(calls) == 1, "with proj_precision 'bf16' only ffn.0's input is produced as MXFP8"

    def two_pass(x, codes, scales, rows, C, eps, **kw):
        h = torch.empty(rows, C, dtype=BF16, device=x.device)
        L().layernorm_mod(x, h, rows, C, eps, **kw)
        return L().mx_quant(h, codes, scales, M=rows, K=C)

    monkeypatch.setattr(L(), "layernorm_mod_mx", two_pass)
    assert torch.equal(run(), fused) and torch.isfinite(fused).all()
