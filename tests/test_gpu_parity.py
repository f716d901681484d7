"""GPU (-m gpu): the HIP path, called through the C ABI, against the CPU oracle and the golden vectors.

Tolerances (written here on purpose, see DESIGN.md "Parity"):
  * integer-free, everything is floating point; the north star's bar is rtol 1e-3 / atol 1e-4 "bf16".
  * fp32 paths (LayerNorm/modulation in f32, head, sampler updates, the whole VAE): rtol 1e-3 / atol 1e-4 on EVERY element
    (they come out 100-1000x tighter); the UniPC/CFG updates are BIT-EXACT given identical model outputs.
  * single bf16-output kernels (GEMM epilogues, RMSNorm+RoPE, attention): every element within a few bf16 ulp of the
    oracle and almost all bit-identical - a bf16 result can only differ from the oracle's by a rounding flip, because
    accumulation order differs (the reference's own FA2/cuBLAS kernels differ from the CPU oracle in the same way).
  * whole DiT forwards / sampler trajectories: bf16 rounding flips (2^-9 relative each) propagate, so elementwise
    rtol 1e-3 / atol 1e-4 cannot hold on every element for ANY second implementation (including the reference on its
    own GPU kernels). The gate is: (a) a stated fraction of the elements inside rtol 1e-3 / atol 1e-4 (>= 90 % for the
    tiny DiT, >= 70 % for one TI2V-5B-width block, where the reference's own roundings already put the ORACLE 1e-3 rms
    from the unrounded result) and max error <= 1 % of the output range, (b) rms error against a no-bf16-rounding
    "truth" run of the oracle not larger than 1.3x the oracle's own (measured: equal to 3 digits).
"""
import math
import os

import pytest
import torch

from conftest import bf16_ulp, load_golden, record_margin

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()                      # raises (fails the suite loudly) if the extension or the gfx950 device is missing
    yield


@pytest.fixture(autouse=True)
def _default_options():
    """Developer switches (uv_set_option) are process-wide: every test starts from and leaves the production defaults."""
    from univid_amd import _lib
    _lib.reset_options()
    yield
    _lib.reset_options()


def L():
    from univid_amd import _lib
    return _lib


def assert_bf16_kernel(got, ref, max_ulp=1.0, min_exact=0.999, name="", extra=None, rare=None):
    """Every element within `max_ulp` bf16 ulps of the oracle (+ an absolute floor of 2e-5 * max|ref| for results that
    are small only through cancellation, where fp32 accumulation-order noise is many ulps OF THE RESULT), and at least
    `min_exact` of the elements bit-identical. rare = (fraction, slack): at most `fraction` of the elements may exceed that
    bound, by at most `slack` (a tensor or a number) - for kernels with an INTERMEDIATE bf16 rounding point, where an fp32
    summation-order difference flips that rounding on about one element per million."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all(), name
    d = (got - ref).abs()
    ulp = bf16_ulp(torch.maximum(ref.abs(), got.abs()))
    tol = max_ulp * ulp + 2e-5 * ref.abs().max() + (0 if extra is None else extra)
    if rare is not None:
        over = d > tol
        assert over.float().mean().item() <= rare[0], f"{name}: {int(over.sum())} of {d.numel()} elements beyond {max_ulp} ulp"
        tol = tol + rare[1]
    assert (d <= tol).all(), f"{name}: max excess {float((d - tol).max()):.3e} (max err {float(d.max()):.3e})"
    exact = (d == 0).float().mean().item()
    assert exact >= min_exact, f"{name}: only {exact:.5f} bit-identical"


def assert_gelu(got, pre, name="GELU"):
    """GELU-tanh epilogue against torch's on the bf16 pre-activation `pre`: every element within 1 bf16 ulp (+ the effect of
    a pre-activation rounding flip); >= 99.9 % bit-identical where the reference formula 0.5*x*(1+tanh(u)) is
    well-conditioned (x > -1.5). Below that 1+tanh(u) cancels and torch's fp32 result carries a relative error of up to
    1e-4 that depends on its tanh implementation (CPU and GPU torch differ there too); the kernel evaluates the same
    function as x/(1+exp(-2u)) without the cancellation, so there only 1-ulp agreement is required."""
    pre = pre.cpu()
    ref = torch.nn.functional.gelu(pre, approximate="tanh")
    assert_bf16_kernel(got, ref, max_ulp=1.0, min_exact=0.995, name=name, extra=1.2 * bf16_ulp(pre.float()))
    well = pre.float() > -1.5
    exact = (got.cpu().float()[well] == ref.float()[well]).float().mean().item()
    assert exact >= 0.999, f"{name}: only {exact:.5f} bit-identical for x > -1.5"


def assert_f32_close(got, ref, rtol=1e-3, atol=1e-4, name=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all(), name
    bad = ((got - ref).abs() > atol + rtol * ref.abs()).sum().item()
    assert bad == 0, f"{name}: {bad}/{ref.numel()} outside rtol={rtol} atol={atol}; max abs {float((got - ref).abs().max()):.3e}"


def assert_model_close(got, ref, truth=None, frac=0.946, name="", max_rel=4.6e-4, truth_ratio=1.02):
    """Composite-path gate: fraction of elements inside rtol 1e-3 / atol 1e-4, max |err| / range, and rms error against the
    no-rounding truth run relative to the oracle's own. Every gate is what MI355X measured over rounds 2 and 3
    (profiles/r02_parity_margins.json, r03_parity_margins.json: the two agree to the fourth digit on the fractions) x 1.2 - for the
    maximum error: 1.2 x the larger of the two rounds; for a fraction: the tighter of 1 - 1.2 x the measured OUTSIDE fraction and the
    measured inside fraction / 1.2 (round 4; x 1.5 before). The defaults are the tiny-DiT forwards (measured 95.6-96.1 %
    inside, max 3.8e-4 of the range, truth ratio 0.999-1.001); wider models pass their own numbers. The measured values are
    written to the margins file again on every run (conftest.record_margin)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert torch.isfinite(got).all(), name
    d = (got - ref).abs()
    inside = (d <= 1e-4 + 1e-3 * ref.abs()).float().mean().item()
    m = dict(inside_frac=inside, max_abs_err=d.max().item(), ref_absmax=ref.abs().max().item(),
             max_err_over_range=(d.max() / ref.abs().max()).item(),
             rel_rms_vs_oracle=(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item(),
             gate_frac=frac, gate_max_rel=max_rel)
    if truth is not None:
        truth = truth.float().cpu()
        e_hip = (got - truth).pow(2).mean().sqrt().item()
        e_ora = (ref - truth).pow(2).mean().sqrt().item()
        m.update(rms_vs_truth_hip=e_hip, rms_vs_truth_oracle=e_ora, truth_ratio=e_hip / max(e_ora, 1e-30), gate_truth_ratio=truth_ratio)
    record_margin(name or "unnamed", **m)
    assert inside >= frac, f"{name}: only {inside:.3f} of elements inside rtol 1e-3 / atol 1e-4"
    assert d.max() <= max_rel * ref.abs().max(), f"{name}: max abs err {float(d.max()):.3e} vs range {float(ref.abs().max()):.3e}"
    if truth is not None:
        assert e_hip <= truth_ratio * e_ora + 1e-6, f"{name}: rms error vs truth {e_hip:.3e} (oracle's own {e_ora:.3e})"


# ---------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(300, 512, 256), (1000, 768, 192), (257, 3072, 3072), (5, 16, 64)])
def test_gemm_bf16_epilogues(M, N, K):
    from univid_amd._lib import (EPI_BF16, EPI_BF16_T, EPI_F32_FROM_BF16, EPI_GATE_RESID_F32, EPI_GELU_BF16, EPI_RESID_F32)
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(BF16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16)
    acc = a.double() @ w.double().t() + bias.double()
    yb = acc.to(BF16)                                  # what F.linear under autocast returns (fp32 acc, one rounding)
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    for cfg in (0, 1, 2, 3):
        out = torch.zeros(M, N, dtype=BF16, device=DEV)
        L().gemm_bf16(ad, wd, bd, out, EPI_BF16, tile_cfg=cfg)
        assert_bf16_kernel(out, yb, name=f"EPI_BF16 cfg{cfg}")
    out = torch.zeros(M, N, dtype=BF16, device=DEV)
    L().gemm_bf16(ad, wd, bd, out, EPI_GELU_BF16)
    # a rounding flip of the pre-activation moves GELU's output by up to |gelu'| <= 1.13 input ulps
    assert_gelu(out, yb)
    out = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    L().gemm_bf16(ad, wd, bd, out, EPI_F32_FROM_BF16)
    assert_bf16_kernel(out, yb, name="F32_FROM_BF16")
    x0 = torch.randn(M, N, generator=g)
    gate = torch.randn(3, N, generator=g)
    tid = torch.randint(0, 3, (M,), generator=g, dtype=torch.int32)
    x = x0.to(DEV)
    L().gemm_bf16(ad, wd, bd, x, EPI_RESID_F32)
    d = (x.cpu() - (x0 + yb.float())).abs()
    assert (d <= bf16_ulp(yb) + 2e-5 * yb.float().abs().max()).all() and (d == 0).float().mean() > 0.999
    x = x0.to(DEV)
    L().gemm_bf16(ad, wd, bd, x, EPI_GATE_RESID_F32, gate=gate.to(DEV), gate_tid=tid.to(DEV))
    ref = x0 + yb.float() * gate[tid.long()]
    d = (x.cpu() - ref).abs()
    assert (d <= (bf16_ulp(yb) + 2e-5 * yb.float().abs().max()) * gate[tid.long()].abs() + 1e-6).all()
    assert (d == 0).float().mean() > 0.999
    Mp = (M + 63) // 64 * 64
    outT = torch.zeros(N, Mp, dtype=BF16, device=DEV)
    L().gemm_bf16(ad, wd, bd, outT, EPI_BF16_T)
    assert_bf16_kernel(outT[:, :M], yb.t(), name="BF16_T")
    assert (outT[:, M:] == 0).all()


@pytest.mark.parametrize("M,N,K,cfgs", [(300, 512, 256, (7, 10)), (1100, 768, 384, (7, 10)), (70000, 256, 256, (7, 8, 9, 0)),
                                        (66000 + 5, 512, 128 * 5, (8, 0))])
def test_gemm_bf16_pingpong_ring_split(M, N, K, cfgs):
    """The 8-wave ping-pong kernel (cfg 7), the 4-stage ring kernel (cfg 10) and the leftover-row split (cfg 8/9, and what
    cfg 0 picks for big shapes) give the same results as the reference product for every epilogue, ragged M included."""
    from univid_amd._lib import (EPI_BF16, EPI_BF16_T, EPI_F32_FROM_BF16, EPI_GATE_RESID_F32, EPI_GELU_BF16, EPI_RESID_F32)
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g, device=DEV) * 0.5).to(BF16)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(BF16)
    bias = (torch.randn(N, generator=g, device=DEV) * 0.1).to(BF16)
    yb = (a.double() @ w.double().t() + bias.double()).to(BF16)
    x0 = torch.randn(M, N, generator=g, device=DEV)
    gate = torch.randn(3, N, generator=g, device=DEV)
    tid = torch.randint(0, 3, (M,), generator=g, device=DEV, dtype=torch.int32)
    floor = 2e-5 * yb.float().abs().max()
    for cfg in cfgs:
        out = torch.zeros(M, N, dtype=BF16, device=DEV)
        L().gemm_bf16(a, w, bias, out, EPI_BF16, tile_cfg=cfg)
        assert_bf16_kernel(out, yb, name=f"EPI_BF16 cfg{cfg}")
        out.zero_()
        L().gemm_bf16(a, w, bias, out, EPI_GELU_BF16, tile_cfg=cfg)
        assert_gelu(out, yb, name=f"GELU cfg{cfg}")
        o32 = torch.zeros(M, N, dtype=torch.float32, device=DEV)
        L().gemm_bf16(a, w, bias, o32, EPI_F32_FROM_BF16, tile_cfg=cfg)
        assert_bf16_kernel(o32, yb, name=f"F32_FROM_BF16 cfg{cfg}")
        x = x0.clone()
        L().gemm_bf16(a, w, bias, x, EPI_RESID_F32, tile_cfg=cfg)
        d = (x - (x0 + yb.float())).abs()
        assert (d <= bf16_ulp(yb.cpu()).to(DEV) + floor).all() and (d == 0).float().mean() > 0.999, f"RESID cfg{cfg}"
        x = x0.clone()
        L().gemm_bf16(a, w, bias, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid, tile_cfg=cfg)
        gr = gate[tid.long()]
        d = (x - (x0 + yb.float() * gr)).abs()
        assert (d <= (bf16_ulp(yb.cpu()).to(DEV) + floor) * gr.abs() + 1e-6).all() and (d == 0).float().mean() > 0.999, f"GATE cfg{cfg}"
        Mp = (M + 63) // 64 * 64
        outT = torch.zeros(N, Mp, dtype=BF16, device=DEV)
        L().gemm_bf16(a, w, bias, outT, EPI_BF16_T, tile_cfg=cfg)
        assert_bf16_kernel(outT[:, :M], yb.t(), name=f"BF16_T cfg{cfg}")
        assert (outT[:, M:] == 0).all()


@pytest.mark.parametrize("M,N,K", [(22880, 3072, 3072), (2300, 2048, 640), (22880, 3072, 14336)])
def test_gemm_schedules_bit_identical(M, N, K):
    """Race screen at full size: the persistent ping-pong kernel (17 / 18 = with the ragged rows split off; what the automatic
    choice 0 takes for large projections), the one-tile-per-workgroup ping-pong schedule (7), the 4-phase reference schedule
    (14), the leftover-row split (8) and the 16-wave kernel (5) accumulate in the same K order, so their FULL outputs must
    agree bit for bit; an LDS hazard (fragment read before its DMA landed, half-tile restaged too early, a next-tile prefetch
    landing in a buffer still being read) would show as a mismatching tile. Also the fp32 read-modify-write epilogue staged
    through LDS (7, 8, 0) against the fragment-wise one of the reference schedule (14)."""
    from univid_amd._lib import EPI_BF16, EPI_BF16_T, EPI_GATE_RESID_F32, EPI_GELU_BF16
    g = torch.Generator(device=DEV).manual_seed(3)
    a = (torch.rand(M, K, device=DEV, generator=g) * 2 - 1).to(BF16)
    w = ((torch.rand(N, K, device=DEV, generator=g) * 2 - 1) * 0.05).to(BF16)
    bias = (torch.rand(N, device=DEV, generator=g) - 0.5).to(BF16)
    big = M >= 4096
    ref = torch.zeros(M, N, device=DEV, dtype=BF16)
    L().gemm_bf16(a, w, None, ref, EPI_BF16, tile_cfg=5)
    for rep in range(3):
        for cfg in (7, 14, 8, 0) + ((18,) if big else ()):
            out = torch.zeros(M, N, device=DEV, dtype=BF16)
            L().gemm_bf16(a, w, None, out, EPI_BF16, tile_cfg=cfg)
            assert torch.equal(out, ref), f"cfg {cfg} rep {rep}: {int((out != ref).sum())} elements differ"
    if not big:
        return
    # the other epilogues of the persistent kernel against the one-tile-per-workgroup launch (8) / the fragment-wise RMW epilogue (14)
    for epi in (EPI_GELU_BF16, EPI_BF16_T):
        shape = (N, (M + 63) // 64 * 64) if epi == EPI_BF16_T else (M, N)
        r, o = torch.zeros(shape, device=DEV, dtype=BF16), torch.zeros(shape, device=DEV, dtype=BF16)
        L().gemm_bf16(a, w, bias, r, epi, tile_cfg=8)
        L().gemm_bf16(a, w, bias, o, epi, tile_cfg=0)
        assert torch.equal(o, r), f"epilogue {epi}: persistent != one tile per workgroup"
    x0 = torch.rand(M, N, device=DEV, generator=g)
    gate = torch.rand(2, N, device=DEV, generator=g)
    tid = (torch.arange(M, device=DEV) * 2 // M).to(torch.int32)
    outs = []
    for cfg in (14, 8, 0):
        x = x0.clone()
        L().gemm_bf16(a, w, bias, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid, tile_cfg=cfg)
        outs.append(x)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "row-coalesced RMW epilogue != fragment-wise"


@pytest.mark.parametrize("M,N,K,sk", [(1120, 3072, 14336, 4), (1120, 3072, 3072, 4), (1120, 3072, 3072, 2), (300, 512, 1024, 4), (2000, 256, 512, 2)])
def test_gemm_splitk_strip_deterministic_and_within_one_ulp(M, N, K, sk):
    """The split-K form of the one-tile-per-workgroup ping-pong kernel (tile_cfg 19 / 20: tiles x split workgroups, f32 partial tiles
    published through the caller's workspace, summed in slice order by the last arriver, then the ordinary epilogue) - what the ffn.2
    leftover strip runs as. Not bit-identical to the unsplit accumulation (four f32 partial sums instead of one chain), so: the SAME
    bits run after run while the chip is busy (arrival order must not matter; a publish / acquire hole would show as a stale tile),
    >= 99.9 % of the elements identical to the unsplit kernel and none further than one ulp of the epilogue's 16-bit rounding; a
    poisoned workspace (NaN slabs, garbage counters) changes nothing; the read-modify-write epilogues likewise."""
    from univid_amd._lib import EPI_BF16, EPI_GATE_RESID_F32, EPI_RESID_F32, UnividHipError
    g = torch.Generator(device=DEV).manual_seed(M + K + sk)
    a = (torch.rand(M, K, device=DEV, generator=g) * 2 - 1).to(BF16)
    w = ((torch.rand(N, K, device=DEV, generator=g) * 2 - 1) * 0.05).to(BF16)
    bias = (torch.rand(N, device=DEV, generator=g) - 0.5).to(BF16)
    cfg = {4: 19, 2: 20}[sk]
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    need = 4096 + tiles * sk * 262144
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ws.view(torch.float32).fill_(float("nan"))                 # slabs AND counters start as garbage
    ref = torch.zeros(M, N, device=DEV, dtype=BF16)
    L().gemm_bf16(a, w, bias, ref, EPI_BF16, tile_cfg=7)
    first = None
    busy = torch.empty(64 << 20, device=DEV)
    for rep in range(6):
        if rep % 2:
            busy.normal_()                                      # other work in flight: the arrival order of the slices varies
        out = torch.zeros(M, N, device=DEV, dtype=BF16)
        L().gemm_bf16(a, w, bias, out, EPI_BF16, tile_cfg=cfg, ws=ws)
        if first is None:
            first = out
        assert torch.equal(out, first), f"rep {rep}: {int((out != first).sum())} elements differ from the first run"
    same = (first == ref).float().mean().item()
    d = (first.float() - ref.float()).abs()
    # (+ an absolute floor: where the partial sums cancel to ~0 the f32 error of the SUMS exceeds the spacing of the tiny RESULT)
    ulp = bf16_ulp(torch.maximum(ref.float().abs(), first.float().abs())) + 2e-5 * ref.float().abs().max()
    assert same >= 0.999 and (d <= ulp).all(), (same, float(d.max()))
    yb = (a.double() @ w.double().t() + bias.double()).to(BF16)
    assert_bf16_kernel(first, yb, name=f"split-K {sk}")
    x0 = torch.rand(M, N, device=DEV, generator=g)
    gate = torch.rand(2, N, device=DEV, generator=g)
    tid = (torch.arange(M, device=DEV) * 2 // M).to(torch.int32)
    for epi, kw in ((EPI_RESID_F32, {}), (EPI_GATE_RESID_F32, dict(gate=gate, gate_tid=tid))):
        xr, xs, xs2 = x0.clone(), x0.clone(), x0.clone()
        L().gemm_bf16(a, w, bias, xr, epi, tile_cfg=7, **kw)
        L().gemm_bf16(a, w, bias, xs, epi, tile_cfg=cfg, ws=ws, **kw)
        L().gemm_bf16(a, w, bias, xs2, epi, tile_cfg=cfg, ws=ws, **kw)
        assert torch.equal(xs, xs2)
        scale = gate[tid.long()].abs() if epi == EPI_GATE_RESID_F32 else 1.0
        dd = (xs - xr).abs()
        assert (xs == xr).float().mean() >= 0.999 and (dd <= ulp * scale + 1e-6).all(), (epi, float(dd.max()))
    with pytest.raises(UnividHipError, match="workspace"):
        L().gemm_bf16(a, w, bias, torch.zeros(M, N, device=DEV, dtype=BF16), EPI_BF16, tile_cfg=cfg, ws=ws[:need - 256])


def test_gemm_ffn2_strip_takes_splitk_with_a_workspace():
    """tile_cfg 0 at the CFG pair's ffn.2 shape (22 880 x 3 072 x 14 336, gated residual): with the workspace uv_gemm_splitk_ws_bytes
    names, the rows of the whole 256-row rounds are bit-identical to the workspace-free launch and the 1 120 leftover rows are the
    split-K strip's (= tile_cfg 19 on those rows alone, bit for bit; within one ulp of the 128x128 ring's); without a workspace, or with
    one that is too small, the call IS the old launch. K = 3 072 projections report no split-K strip."""
    from univid_amd._lib import EPI_GATE_RESID_F32
    M, N, K = 22880, 3072, 14336
    assert L().gemm_splitk_ws_bytes(M, N, 3072) == 0 and L().gemm_splitk_ws_bytes(1024, N, K) == 0
    need = L().gemm_splitk_ws_bytes(M, N, K)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the strip geometry below is the 256-CU one ({cus} CUs here)")
    m_main = 21760
    assert need == 4096 + 5 * 12 * 4 * 262144
    g = torch.Generator(device=DEV).manual_seed(11)
    a = (torch.rand(M, K, device=DEV, generator=g) * 2 - 1).to(BF16)
    w = ((torch.rand(N, K, device=DEV, generator=g) * 2 - 1) * 0.05).to(BF16)
    bias = (torch.rand(N, device=DEV, generator=g) - 0.5).to(BF16)
    x0 = torch.rand(M, N, device=DEV, generator=g)
    gate = torch.rand(2, N, device=DEV, generator=g)
    tid = (torch.arange(M, device=DEV) * 2 // M).to(torch.int32)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    kw = dict(gate=gate, gate_tid=tid)
    plain, with_ws, small_ws, strip = x0.clone(), x0.clone(), x0.clone(), x0[m_main:].clone()
    L().gemm_bf16(a, w, bias, plain, EPI_GATE_RESID_F32, **kw)
    L().gemm_bf16(a, w, bias, with_ws, EPI_GATE_RESID_F32, ws=ws, **kw)
    L().gemm_bf16(a, w, bias, small_ws, EPI_GATE_RESID_F32, ws=ws[:need - 256], **kw)
    L().gemm_bf16(a[m_main:], w, bias, strip, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid[m_main:], tile_cfg=19, ws=ws)
    assert torch.equal(small_ws, plain)
    assert torch.equal(with_ws[:m_main], plain[:m_main])
    assert torch.equal(with_ws[m_main:], strip)
    d = (with_ws[m_main:] - plain[m_main:]).abs()
    assert not torch.equal(with_ws[m_main:], plain[m_main:]) and (d == 0).float().mean() >= 0.999 and float(d.max()) < 0.04


def test_host_blocking_sync_policy_can_be_set_and_reset():
    """uv_host_blocking_sync: hipDeviceScheduleBlockingSync for the current device and back to the runtime's default, while the device is in
    use (bench.py toggles it between two generations of one process); results of a launch in between are unaffected."""
    from univid_amd import parallel
    from univid_amd._lib import EPI_BF16
    a = torch.randn(256, 128, device=DEV).to(BF16)
    w = torch.randn(64, 128, device=DEV).to(BF16)
    ref = torch.zeros(256, 64, dtype=BF16, device=DEV)
    L().gemm_bf16(a, w, None, ref, EPI_BF16)
    for on in (True, False, True):
        L().host_blocking_sync(on)
        out = torch.zeros(256, 64, dtype=BF16, device=DEV)
        L().gemm_bf16(a, w, None, out, EPI_BF16)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    parallel.host_policy(torch.device(DEV if ":" in DEV else DEV + ":0"))
    L().host_blocking_sync(False)
    parallel._blocking_set.clear()


def test_gemm_rejects_bad_shapes():
    from univid_amd._lib import EPI_BF16, UnividHipError
    a = torch.zeros(8, 48, dtype=BF16, device=DEV)
    w = torch.zeros(16, 48, dtype=BF16, device=DEV)
    out = torch.zeros(8, 16, dtype=BF16, device=DEV)
    with pytest.raises(UnividHipError, match="multiple of 64"):
        L().gemm_bf16(a, w, None, out, EPI_BF16)
    with pytest.raises(UnividHipError):
        L().gemm_bf16(a.cpu(), w, None, out, EPI_BF16)


@pytest.mark.parametrize("M,N,K", [(300, 192, 256), (1000, 48, 48), (513, 192, 3072), (7, 4, 12)])
def test_gemm_f32(M, N, K):
    g = torch.Generator().manual_seed(1)
    a, w, b, r = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    out = torch.zeros(M, N, device=DEV)
    L().gemm_f32(a.to(DEV), w.to(DEV), b.to(DEV), out, resid=r.to(DEV))
    assert_f32_close(out, (a.double() @ w.double().t() + b.double() + r.double()).float(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("Lq,Lk,H,D", [(300, 300, 2, 128), (256, 512, 3, 128), (1000, 77, 2, 128), (260, 260, 4, 64), (33, 1, 1, 128),
                                       (1200, 1200, 2, 128)])
def test_flash_attention_vs_oracle(Lq, Lk, H, D):
    from oracle import wan_dit
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    C = H * D
    q, k, v = (torch.randn(n, C, generator=g).to(BF16) for n in (Lq, Lk, Lk))
    ref = wan_dit.attention_core(q.view(1, Lq, H, D), k.view(1, Lk, H, D), v.view(1, Lk, H, D)).view(Lq, C)
    qf, kf, vf = (t.double().view(-1, H, D).transpose(0, 1) for t in (q, k, v))
    truth = (torch.softmax(qf @ kf.transpose(1, 2) / math.sqrt(D), -1) @ vf).transpose(0, 1).reshape(Lq, C)
    vt = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
    vt[:, :Lk] = v.t().to(DEV)
    out = torch.zeros(Lq, C, dtype=BF16, device=DEV)
    L().flash_attn(q.to(DEV), k.to(DEV), vt, out, Lq, Lk, H, D, 1.0 / math.sqrt(D))
    got = out.float().cpu()
    # both are bf16-P flash kernels with different tilings: compare each against the fp64 truth
    e_hip, e_ora = (got - truth).abs(), (ref.float() - truth).abs()
    tol = 3 * bf16_ulp(truth.float()) + 2e-3 * truth.abs().float().max()
    assert (e_hip <= tol).all(), f"max err {float(e_hip.max()):.3e}"
    assert e_hip.pow(2).mean().sqrt() <= 1.5 * e_ora.pow(2).mean().sqrt() + 1e-5


@pytest.mark.parametrize("Lk", [5, 63, 64, 65, 128, 129, 192, 200, 256, 321])
def test_flash_attention_key_tile_edges(Lk):
    """Every path of the key-tile loop of the head_dim-128 kernel (two-tile unrolled main loop with compile-time buffer parity, one or two
    peeled full tiles, the ragged tile on either buffer, a lone short tile): against the fp64 softmax, with ragged query rows (Lq = 150:
    the second workgroup's last wave owns no query) and V = 1 giving exactly 1."""
    Lq, H, D = 150, 2, 128
    C = H * D
    g = torch.Generator().manual_seed(100 + Lk)
    q, k, v = (torch.randn(n, C, generator=g).to(BF16) for n in (Lq, Lk, Lk))
    qf, kf, vf = (t.double().view(-1, H, D).transpose(0, 1) for t in (q, k, v))
    truth = (torch.softmax(qf @ kf.transpose(1, 2) / math.sqrt(D), -1) @ vf).transpose(0, 1).reshape(Lq, C)
    vt = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
    vt[:, :Lk] = v.t().to(DEV)
    out = torch.full((Lq + 8, C), 7.0, dtype=BF16, device=DEV)      # guard rows: nothing may be written past Lq
    L().flash_attn(q.to(DEV), k.to(DEV), vt, out, Lq, Lk, H, D, 1.0 / math.sqrt(D))
    assert (out[Lq:] == 7.0).all()
    err = (out[:Lq].double().cpu() - truth).abs()
    assert (err <= 3 * bf16_ulp(truth.float()) + 2e-3 * float(truth.abs().max())).all(), f"Lk={Lk}: max err {float(err.max()):.3e}"
    vt[:, :Lk] = 1.0
    vt[:, Lk:] = 1000.0                                              # padding columns must never be attended
    L().flash_attn(q.to(DEV), k.to(DEV), vt, out, Lq, Lk, H, D, 1.0 / math.sqrt(D))
    assert (out[:Lq].float() - 1).abs().max() <= 2 ** -7


@pytest.mark.parametrize("Lq,Lk", [(300, 300), (2200, 2200), (1000, 77), (2304, 2304)])
def test_flash_attention_nan_and_masked_tile_behaviour_is_pinned(Lq, Lk):
    """attention.hip is built with -fno-honor-nans (univid_amd/build.py: removes the canonicalising v_max in front of every fmaxf on MFMA
    outputs). Round-4 advisor: a promise about NaNs under that flag holds for one compiler's codegen only - so it is pinned HERE, for all
    three kernels (short-key fwd3, generic, long-key fwd12): (a) a NaN in ONE query row poisons exactly that row (all heads it touches) and
    leaves every other row bit-identical to the clean run; (b) a NaN in ONE key poisons every row of that head and leaves the other head
    bit-identical; (c) the masked tail of a ragged last key tile (scores at -inf, possibly a whole 32-key half) yields finite rows - also when
    the padding columns of V^T hold huge values; (d) +-inf-free inputs never produce a NaN. A compiler that folds these paths fails here."""
    H, D = 2, 128
    C = H * D
    g = torch.Generator().manual_seed(Lq + Lk)
    q, k, v = (torch.randn(n, C, generator=g).to(BF16).to(DEV) for n in (Lq, Lk, Lk))
    vt = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
    vt[:, :Lk] = v.t()
    vt[:, Lk:] = 3.0e38                                                      # (c): finite garbage in the padding columns

    def run(q_, k_):
        out = torch.empty(Lq, C, dtype=BF16, device=DEV)
        L().flash_attn(q_, k_, vt, out, Lq, Lk, H, D, 1.0 / math.sqrt(D))
        return out.float()

    clean = run(q, k)
    assert torch.isfinite(clean).all()                                       # (c), (d)
    qn = q.clone()
    qn[Lq // 3, 5] = float("nan")                                            # head 0 of one row
    got = run(qn, k)
    row = got[Lq // 3]
    assert torch.isnan(row[:D]).all(), "a NaN query must poison its row of that head"
    keep = torch.ones(Lq, dtype=torch.bool, device=DEV)
    keep[Lq // 3] = False
    assert torch.equal(got[keep], clean[keep]) and torch.equal(row[D:], clean[Lq // 3, D:])
    kn = k.clone()
    kn[Lk // 2, D + 7] = float("nan")                                        # head 1 of one key
    got = run(q, kn)
    assert torch.isnan(got[:, D:]).all(), "a NaN key must poison every row of its head"
    assert torch.equal(got[:, :D], clean[:, :D])


@pytest.mark.parametrize("Lk", [2048, 2104, 2112, 2184])
def test_flash_attention_long_key_kernel(Lk):
    """Lk >= 2048 selects the 12-wave-workgroup kernel (384 queries per workgroup, K / V^T tiles shared by 12 waves): even / odd tile
    counts, ragged last tile, a ragged last workgroup (Lq = 500), two stacked samples; against the fp64 softmax on sampled rows, the
    stacked launch bit-identical to the single ones, V = 1 -> exactly 1, nothing written past Lq."""
    Lq, H, D, B = 500, 2, 128, 2
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(Lk)
    q = torch.randn(B * Lq, C, generator=g, device=DEV).to(BF16)
    k = torch.randn(B * Lk, C, generator=g, device=DEV).to(BF16)
    v = torch.randn(B * Lk, C, generator=g, device=DEV).to(BF16)
    cols = (B - 1) * Lk + (Lk + 63) // 64 * 64
    vt = torch.zeros(C, cols, dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.t()
    out = torch.full((B * Lq + 8, C), 7.0, dtype=BF16, device=DEV)
    L().flash_attn(q, k, vt, out, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert (out[B * Lq:] == 7.0).all()
    for b in range(B):
        qs, ks, vs = (t[b * n:(b + 1) * n].double().view(n, H, D).transpose(0, 1) for t, n in ((q, Lq), (k, Lk), (v, Lk)))
        truth = (torch.softmax(qs @ ks.transpose(1, 2) / math.sqrt(D), -1) @ vs).transpose(0, 1).reshape(Lq, C)
        err = (out[b * Lq:(b + 1) * Lq].double() - truth).abs()
        assert (err <= 3 * bf16_ulp(truth.float()) + 2e-3 * float(truth.abs().max())).all(), f"sample {b}: max err {float(err.max()):.3e}"
        vt1 = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
        vt1[:, :Lk] = v[b * Lk:(b + 1) * Lk].t()
        o1 = torch.zeros(Lq, C, dtype=BF16, device=DEV)
        L().flash_attn(q[b * Lq:(b + 1) * Lq], k[b * Lk:(b + 1) * Lk], vt1, o1, Lq, Lk, H, D, D ** -0.5)
        assert torch.equal(out[b * Lq:(b + 1) * Lq], o1), f"sample {b}: stacked != single"
    ones = torch.ones(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
    ones[:, Lk:] = 1000.0
    L().flash_attn(q[:Lq], k[:Lk], ones, out, Lq, Lk, H, D, D ** -0.5)
    assert (out[:Lq].float() - 1).abs().max() <= 2 ** -7


@pytest.mark.parametrize("H", [4, 2])
def test_flash_attention_result_does_not_depend_on_the_block_cut(H):
    """flash_attn_fwd12_kernel under every kind of query-block cut (OPT_ATTN_CUT; plan_attn, csrc/attn_args.h) at 16 units per head: the
    automatic cut; 1 = two 12-unit blocks, the second with 4 units and 8 loader-only waves; 2 = one 12-unit block followed by one 8-unit
    block; 3 = two 8-unit blocks. H = 4 (8 heads in total): both block totals divide by 8 and the kernel takes its XCD-aware order; H = 2:
    the mixed cut's totals (4 + 4) do not, plain id order. All outputs bit-identical, one checked against the fp64 softmax, nothing
    written past Lq."""
    Lq, Lk, D, B = 500, 2104, 128, 2
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(77 + H)
    q = torch.randn(B * Lq, C, generator=g, device=DEV).to(BF16)
    k = torch.randn(B * Lk, C, generator=g, device=DEV).to(BF16)
    v = torch.randn(B * Lk, C, generator=g, device=DEV).to(BF16)
    vt = torch.zeros(C, (B - 1) * Lk + (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.t()
    outs = {}
    try:
        for cut, blocks in ((0, None), (1, (2, 0)), (2, (1, 1)), (3, (0, 2))):
            L().set_option(L().OPT_ATTN_CUT, cut)
            plan = L().attn_plan(Lq, Lk, D, B, H)
            assert plan["kernel"] == "flash_attn_fwd12_kernel" and plan["grid"] == plan["q_blocks"] * H * B
            if blocks is not None:
                assert (plan["n12"], plan["q_blocks"] - plan["n12"]) == blocks
            out = torch.full((B * Lq + 8, C), 7.0, dtype=BF16, device=DEV)
            L().flash_attn(q, k, vt, out, Lq, Lk, H, D, D ** -0.5, batch=B)
            assert (out[B * Lq:] == 7.0).all(), f"cut {cut} wrote past Lq"
            outs[cut] = out[:B * Lq]
    finally:
        L().reset_options()
    for cut in (1, 2, 3):
        assert torch.equal(outs[0].view(torch.int16), outs[cut].view(torch.int16)), f"cut {cut} changed the result"
    for b in range(B):
        qs, ks, vs = (t[b * n:(b + 1) * n].double().view(n, H, D).transpose(0, 1) for t, n in ((q, Lq), (k, Lk), (v, Lk)))
        truth = (torch.softmax(qs @ ks.transpose(1, 2) / math.sqrt(D), -1) @ vs).transpose(0, 1).reshape(Lq, C)
        err = (outs[1][b * Lq:(b + 1) * Lq].double() - truth).abs()
        assert (err <= 3 * bf16_ulp(truth.float()) + 2e-3 * float(truth.abs().max())).all(), f"sample {b}: max err {float(err.max()):.3e}"


@pytest.mark.parametrize("Lk,D", [(200, 128), (2104, 128), (200, 64)])
def test_flash_attention_direct_store_epilogue(Lk, D):
    """An output whose row stride is no multiple of 8 elements (ldo = C + 4: a view into a wider buffer, still 16-byte aligned) takes the
    kernels' direct O-row store instead of the transpose through LDS - flash_attn_fwd3_kernel (Lk 200), flash_attn_fwd12_kernel (Lk 2104)
    and flash_attn_fwd_kernel<64>, which has no other: bit-identical to the dense output, and neither the four columns between the rows
    nor the rows past Lq (ragged last wave and workgroup at Lq = 150) are touched."""
    Lq, H = 150, 2
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(Lk + D)
    q, k = (torch.randn(n, C, generator=g, device=DEV).to(BF16) for n in (Lq, Lk))
    vt = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
    vt[:, :Lk] = torch.randn(C, Lk, generator=g, device=DEV).to(BF16)
    dense = torch.full((Lq + 8, C), 7.0, dtype=BF16, device=DEV)
    L().flash_attn(q, k, vt, dense, Lq, Lk, H, D, D ** -0.5)
    wide = torch.full((Lq + 8, C + 4), 7.0, dtype=BF16, device=DEV)
    out = wide[:, :C]
    assert out.stride(0) % 8 == 4 and out.data_ptr() % 16 == 0
    L().flash_attn(q, k, vt, out, Lq, Lk, H, D, D ** -0.5)
    assert torch.isfinite(dense[:Lq].float()).all() and (dense[Lq:] == 7.0).all()
    assert torch.equal(out[:Lq].view(torch.int16), dense[:Lq].view(torch.int16))
    assert (wide[:, C:] == 7.0).all() and (wide[Lq:] == 7.0).all()


@pytest.mark.parametrize("Lq,Lk,B,scale,spike", [(2048, 2048, 1, 1.0, False), (2100, 2100, 1, 1.0, False), (700, 4000, 2, 1.0, False),
                                                 (3000, 2992, 2, 2.0, True), (11440, 11440, 2, 1.0, False)])
def test_flash_attention_pw4_kernel_is_bit_identical_to_fwd12(Lq, Lk, B, scale, spike):
    """The product's long-key self-attention kernel (12-wave workgroups, flash_attn_fwd12_kernel) and the DIAGNOSTIC 4-wave x 64-query
    kernel with asm-owned accumulator registers (tools/diag/attn_pw4.hip - out of the product library since round 4: bit-identical and
    10 % slower; built by __graft_entry__.build() into tools/diag/libuv_diag.so) perform the same per-query arithmetic in the same
    order: their outputs must agree BIT FOR BIT - full tiles, ragged last tile and ragged last workgroup, stacked samples, spiked keys
    that move the deferred softmax maximum late in the sequence, and the bench shape. Two independently scheduled implementations of
    one arithmetic: any hazard or staging slip in either shows up here (and did, four times)."""
    import ctypes
    diag_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "diag", "libuv_diag.so")
    if not os.path.exists(diag_path):
        pytest.skip("tools/diag/libuv_diag.so is not built (python tools/diag/build_diag.py)")
    diag = ctypes.CDLL(diag_path)
    P_, L_, I_ = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    diag.uv_diag_flash_attn_pw4.argtypes = [P_, L_, P_, L_, P_, L_, P_, L_, I_, I_, I_, I_, I_, ctypes.c_float, P_]
    H, D = 24 if Lq > 4096 else 4, 128
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(Lq + Lk)
    q = (torch.randn(B * Lq, C, generator=g, device=DEV) * scale).to(BF16)
    k = (torch.randn(B * Lk, C, generator=g, device=DEV) * scale).to(BF16)
    if spike:
        k[Lk // 2 + 37] *= 6.0
        k[Lk - 5] *= 9.0
    vt = torch.randn(C, (B - 1) * Lk + (Lk + 63) // 64 * 64, generator=g, device=DEV).to(BF16)
    outs = {}
    assert "fwd12" in L().attn_kernel_name(Lq, Lk, D, B, H=H)
    for kind in ("fwd12", "pw4"):
        o = torch.full((B * Lq + 8, C), 7.0, dtype=BF16, device=DEV)
        if kind == "fwd12":
            L().flash_attn(q, k, vt, o, Lq, Lk, H, D, D ** -0.5, batch=B)
        else:
            rc = diag.uv_diag_flash_attn_pw4(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), vt.data_ptr(), vt.stride(0), o.data_ptr(),
                                             o.stride(0), B, Lq, Lk, H, D, D ** -0.5, torch.cuda.current_stream().cuda_stream)
            assert rc == 0
        torch.cuda.synchronize()
        assert (o[B * Lq:] == 7.0).all(), f"{kind} wrote past Lq"
        outs[kind] = o
    assert torch.isfinite(outs["pw4"].float()).all()
    assert torch.equal(outs["fwd12"].view(torch.int16), outs["pw4"].view(torch.int16))


@pytest.mark.parametrize("spike", [4.0, 0.45, 0.2])
def test_flash_attention_rescale_branch_and_rowsum(spike):
    """A key that dominates late: spike 4 moves the softmax reference maximum (the rescale branch of the online softmax),
    0.45 and 0.2 grow a row's maximum by less than the deferral threshold (2^8 in the exponent domain), so P > 1 is
    accumulated against the old reference. Both must match the fp64 softmax; V = 1 must give exactly 1 for every query."""
    Lq, Lk, D = 256, 640, 128
    g = torch.Generator().manual_seed(9)
    q, k, v = torch.randn(Lq, D, generator=g).to(BF16), torch.randn(Lk, D, generator=g).to(BF16), torch.randn(Lk, D, generator=g).to(BF16)
    k[500] = (q[3].float() * spike).to(BF16)
    s = (q.double() @ k.double().t()) / math.sqrt(D)
    truth = torch.softmax(s, -1) @ v.double()
    out = torch.zeros(Lq, D, dtype=BF16, device=DEV)
    L().flash_attn(q.to(DEV), k.to(DEV), v.t().contiguous().to(DEV), out, Lq, Lk, 1, D, 1.0 / math.sqrt(D))
    assert ((out.double().cpu() - truth).abs() <= 3 * bf16_ulp(truth.float()) + 8e-3).all()
    if spike >= 4:
        assert (out[3].double().cpu() - v[500].double()).abs().max() < 2e-2   # query 3 attends (almost) only key 500
    ones = torch.ones(D, Lk, dtype=BF16, device=DEV)
    L().flash_attn(q.to(DEV), k.to(DEV), ones, out, Lq, Lk, 1, D, 1.0 / math.sqrt(D))
    assert (out.float() - 1).abs().max() <= 2 ** -7


def test_layernorm_modulate_and_rmsnorm_rope():
    from oracle import wan_dit
    g = torch.Generator().manual_seed(2)
    Lr, C = 70, 3072
    x = torch.randn(Lr, C, generator=g) * 2 + 0.3
    tab = torch.randn(2, 6 * C, generator=g) * 0.3
    tid = torch.randint(0, 2, (Lr,), generator=g, dtype=torch.int32)
    xd, tabd, tidd = x.to(DEV), tab.to(DEV), tid.to(DEV)
    out = torch.zeros(Lr, C, dtype=BF16, device=DEV)
    L().layernorm_mod(xd, out, Lr, C, 1e-6, mode=1, tab=tabd, shift_off=3 * C, scale_off=4 * C, tid=tidd)
    ref = (wan_dit.layer_norm(x, 1e-6).float() * (1 + tab[tid.long(), 4 * C:5 * C]) + tab[tid.long(), 3 * C:4 * C]).to(BF16)
    assert_bf16_kernel(out, ref, name="ln+modulate")
    xb = x.to(BF16)                                                  # block 0: bf16 stream, LN result rounded to bf16
    L().layernorm_mod(xb.float().to(DEV), out, Lr, C, 1e-6, mode=1, tab=tabd, shift_off=0, scale_off=C, tid=tidd, round_ln=True)
    ref = (wan_dit.layer_norm(xb, 1e-6).float() * (1 + tab[tid.long(), C:2 * C]) + tab[tid.long(), :C]).to(BF16)
    assert_bf16_kernel(out, ref, name="ln(round)+modulate")
    w, b = torch.randn(C, generator=g) * 0.1 + 1, torch.randn(C, generator=g) * 0.1
    L().layernorm_mod(xd, out, Lr, C, 1e-6, mode=2, w=w.to(DEV), b=b.to(DEV))
    assert_bf16_kernel(out, wan_dit.layer_norm(x, 1e-6, w, b).to(BF16), name="ln affine")
    o32 = torch.zeros(Lr, C, device=DEV)
    L().layernorm_mod(xd, o32, Lr, C, 1e-6, mode=0)
    assert_f32_close(o32, wan_dit.layer_norm(x, 1e-6), rtol=1e-5, atol=1e-5)
    for dim, heads, grid in [(3072, 24, (2, 5, 7)), (256, 4, (2, 5, 7)), (256, 2, (1, 7, 10))]:
        Lr = grid[0] * grid[1] * grid[2]
        xq = (torch.randn(1, Lr + 3, dim, generator=g) * 1.5).to(BF16)      # 3 padding rows: must pass through un-rotated
        wq = torch.randn(dim, generator=g) * 0.1 + 1
        freqs = wan_dit.rope_table(dim // heads)
        ref = wan_dit.rope_apply(wan_dit.rms_norm(xq, wq, 1e-6).view(1, Lr + 3, heads, dim // heads), torch.tensor([grid]), freqs)
        out = torch.zeros(Lr + 3, dim, dtype=BF16, device=DEV)
        L().rmsnorm_rope(xq[0].to(DEV), out, wq.to(DEV), Lr + 3, dim, dim // heads, 1e-6, torch.view_as_real(freqs).contiguous().to(DEV), grid)
        assert_bf16_kernel(out, ref.view(Lr + 3, dim).to(BF16), name=f"rmsnorm+rope {dim}")
        L().rmsnorm_rope(xq[0].to(DEV), out, wq.to(DEV), Lr + 3, dim, dim // heads, 1e-6)
        assert_bf16_kernel(out, wan_dit.rms_norm(xq, wq, 1e-6)[0].to(BF16), name=f"rmsnorm {dim}")


def test_full_size_glue_kernels_sampled_rows_vs_oracle():
    """VALUE checks at BASELINE's full size (cond + uncond stacked: 2 x 11 440 tokens x 3072): the row-wise kernels run on the
    whole tensors, and a sample of rows - first / last rows of each sample, tile and wave boundaries, random ones - is compared
    with the CPU oracle's functions on those rows: LayerNorm + AdaLN modulation, affine LayerNorm, QK RMSNorm + 3-axis RoPE
    through the fused q/k launch (positions restart per sample), and the gated fp32 residual epilogue of the persistent GEMM."""
    from oracle import wan_dit
    from univid_amd._lib import EPI_GATE_RESID_F32
    from univid_amd.wan.model import _freqs_device
    Ls, B, C, H = 11440, 2, 3072, 24
    grid = (13, 22, 40)
    M = B * Ls
    g = torch.Generator(device=DEV).manual_seed(17)
    rows = torch.unique(torch.cat([torch.tensor([0, 1, 3, 4, 255, 256, 879, 880, Ls - 1, Ls, Ls + 1, Ls + 879, Ls + 880, M - 2, M - 1]),
                                   torch.randint(0, M, (48,), generator=torch.Generator().manual_seed(170))]))
    x = torch.randn(M, C, device=DEV, generator=g) * 2 + 0.3
    tab = torch.randn(2, 6 * C, device=DEV, generator=g) * 0.3
    tid = (torch.arange(M, device=DEV) % Ls >= 880).to(torch.int32)          # i2v-like: first latent frame on its own row
    h = torch.empty(M, C, dtype=BF16, device=DEV)
    L().layernorm_mod(x, h, M, C, 1e-6, mode=1, tab=tab, shift_off=3 * C, scale_off=4 * C, tid=tid)
    xr, tr, tabc = x[rows].cpu(), tid[rows].long().cpu(), tab.cpu()
    ref = (wan_dit.layer_norm(xr, 1e-6).float() * (1 + tabc[tr, 4 * C:5 * C]) + tabc[tr, 3 * C:4 * C]).to(BF16)
    assert_bf16_kernel(h[rows], ref, name="full-size ln+modulate")
    w, b = torch.randn(C, device=DEV, generator=g) * 0.1 + 1, torch.randn(C, device=DEV, generator=g) * 0.1
    L().layernorm_mod(x, h, M, C, 1e-6, mode=2, w=w, b=b)
    assert_bf16_kernel(h[rows], wan_dit.layer_norm(xr, 1e-6, w.cpu(), b.cpu()).to(BF16), name="full-size ln affine")
    # QK RMSNorm + RoPE, q and k of both samples in one launch
    q = (torch.randn(M, C, device=DEV, generator=g) * 1.5).to(BF16)
    k = (torch.randn(M, C, device=DEV, generator=g) * 1.5).to(BF16)
    wq, wk = torch.randn(C, device=DEV, generator=g) * 0.1 + 1, torch.randn(C, device=DEV, generator=g) * 0.1 + 1
    q_in, k_in = q[rows].cpu(), k[rows].cpu()
    freqs = wan_dit.rope_table(C // H)
    L().rmsnorm_rope_qk(q, k, wq, wk, M, Ls, C, C // H, 1e-6, _freqs_device(freqs, torch.device(DEV)), grid)
    pos = (rows % Ls).tolist()
    for got, xin, wt, nm in ((q[rows], q_in, wq.cpu(), "q"), (k[rows], k_in, wk.cpu(), "k")):
        y = wan_dit.rms_norm(xin.unsqueeze(0), wt, 1e-6).view(len(pos), H, C // H)         # [rows, H, D] fp32
        # rope_apply on single-token "sequences" placed at their (f, h, w) position: rotate each sampled row with its own factors
        c = C // H // 2
        fa, fb, fc = freqs.split([c - 2 * (c // 3), c // 3, c // 3], dim=1)
        out_rows = []
        for i, pidx in enumerate(pos):
            f_, rem = divmod(pidx, grid[1] * grid[2])
            h_, w_ = divmod(rem, grid[2])
            fi = torch.cat([fa[f_], fb[h_], fc[w_]]).view(1, -1)
            xi = torch.view_as_complex(y[i].to(torch.float64).reshape(H, -1, 2))
            out_rows.append(torch.view_as_real(xi * fi).flatten(1).float())
        ref = torch.stack(out_rows).reshape(len(pos), C).to(BF16)
        # WanRMSNorm rounds the normalised value to bf16 BEFORE the weight and the rotation (model.py:79-96); kernel and oracle sum the
        # row's squares in different fp32 orders, which flips that rounding on about one element per million
        # (tests/manual/rope_ulp_stats.py: 23 of 22.4 M), and the rotation spreads the flip - one ulp of the larger element of the
        # rotated pair - over both outputs. Allowed: that much, on at most 2e-5 of the elements.
        ypair = y.reshape(len(pos), C // 2, 2).abs().amax(dim=2, keepdim=True).expand(-1, -1, 2).reshape(len(pos), C)
        assert_bf16_kernel(got, ref, name=f"full-size rmsnorm+rope {nm}", rare=(2e-5, 2.0 * bf16_ulp(ypair)))
    # gated fp32 residual epilogue (x + bf16(acc + bias) * gate[tid]) of the o-projection shape
    a = (torch.rand(M, C, device=DEV, generator=g) * 2 - 1).to(BF16)
    wo = ((torch.rand(C, C, device=DEV, generator=g) * 2 - 1) * 0.05).to(BF16)
    bias = (torch.rand(C, device=DEV, generator=g) - 0.5).to(BF16)
    x0 = x[rows].cpu().double()
    L().gemm_bf16(a, wo, bias, x, EPI_GATE_RESID_F32, gate=tab[:, 2 * C:3 * C], gate_tid=tid)
    acc = a[rows].cpu().double() @ wo.cpu().double().t() + bias.cpu().double()
    want = x0 + acc.to(BF16).double() * tabc[tr, 2 * C:3 * C].double()
    d = (x[rows].cpu().double() - want).abs()
    tol = (bf16_ulp(acc.float()).double() + 2e-5 * acc.abs().max()) * tabc[tr, 2 * C:3 * C].abs().double() + 1e-6
    assert (d <= tol).all() and (d <= 1e-6).float().mean() > 0.999, f"max err {float(d.max()):.3e}"


def test_rmsnorm_rope_qk_single_launch_equals_per_tensor_calls():
    """uv_rmsnorm_rope_qk (q and k of all stacked samples in one launch, RoPE positions restarting per sample) against the
    per-tensor, per-sample uv_rmsnorm_rope calls that are checked against the oracle above: bit-identical."""
    from univid_amd.wan.model import _freqs_device, rope_params
    C, D, grid, B = 3072, 128, (3, 6, 8), 2
    Ls = grid[0] * grid[1] * grid[2]
    d = D
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    fr = _freqs_device(freqs, torch.device(DEV))
    g = torch.Generator(device=DEV).manual_seed(3)
    for L_rows in (Ls, 4800):                                # small (1 row per wave) and large (4 rows per wave) launch shapes
        gr = grid if L_rows == Ls else (10, 20, 24)
        q = torch.randn(B * L_rows, C, device=DEV, generator=g).to(BF16)
        k = torch.randn(B * L_rows, C, device=DEV, generator=g).to(BF16)
        wq, wk = torch.randn(C, device=DEV, generator=g), torch.randn(C, device=DEV, generator=g)
        q1, k1 = q.clone(), k.clone()
        for b in range(B):
            rows = slice(b * L_rows, (b + 1) * L_rows)
            L().rmsnorm_rope(q1[rows], q1[rows], wq, L_rows, C, D, 1e-6, fr, gr)
            L().rmsnorm_rope(k1[rows], k1[rows], wk, L_rows, C, D, 1e-6, fr, gr)
        q2, k2 = q.clone(), k.clone()
        L().rmsnorm_rope_qk(q2, k2, wq, wk, B * L_rows, L_rows, C, D, 1e-6, fr, gr)
        assert torch.equal(q1, q2) and torch.equal(k1, k2) and not torch.equal(q2, q)


def test_unipc_and_cfg_kernels_are_bit_exact():
    """Given identical model outputs the HIP latent trajectory equals the CPU oracle's bit for bit (same host, so the
    same libm/LAPACK scalar coefficients), and the reference's golden trajectory (generated on another CPU, whose
    expm1/log/solve may differ in the last place) to 2e-6."""
    from oracle import unipc as ou
    from univid_amd.wan.fm_solvers_unipc import FlowUniPCMultistepScheduler
    g = load_golden("unipc")
    s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
    s.set_timesteps(10, device="cpu", shift=5.0)
    o = ou.FlowUniPC(1000, shift=1)
    o.set_timesteps(10, shift=5.0)
    lat, lo = g["x"].to(DEV), g["x"]
    for i, t in enumerate(s.timesteps):
        lat = s.step(g["model_outputs"][i].to(DEV), t, lat, return_dict=False)[0]
        lo = o.step(g["model_outputs"][i], t, lo)
        assert torch.equal(lat.cpu(), lo), f"UniPC step {i}: HIP update differs from the oracle"
        assert torch.allclose(lat.cpu(), g["trajectory"][i], rtol=2e-6, atol=2e-6), f"UniPC step {i} vs reference golden"
    # CFG + convert fused path == separate path
    s1 = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
    s1.set_timesteps(10, device="cpu", shift=5.0)
    c, u, x = g["model_outputs"][0].to(DEV), g["model_outputs"][1].to(DEV), g["x"].to(DEV)
    prev, npred = s1.step_cfg(c, u, 5.0, s1.timesteps[0], x, want_noise_pred=True)
    ref_np = g["model_outputs"][1] + 5.0 * (g["model_outputs"][0] - g["model_outputs"][1])
    assert torch.equal(npred.cpu(), ref_np)
    s2 = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
    s2.set_timesteps(10, device="cpu", shift=5.0)
    assert torch.equal(prev, s2.step(ref_np.to(DEV), s2.timesteps[0], x, return_dict=False)[0])


def test_dpmpp_kernel_is_bit_exact():
    """sample_solver='dpm++' (textimage2video.py:343-351): given identical model outputs the HIP DPM-Solver++ trajectory equals
    the CPU oracle's bit for bit at 10, 20, 2 and 1 steps (first-order warm-up, midpoint second-order steps, the final step onto
    sigma 0 where lambda is +inf), and the reference's golden trajectory to 2e-6 (another host's log/exp may differ in the
    last place)."""
    from oracle import dpmpp as od
    from univid_amd.wan.fm_solvers import FlowDPMSolverMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
    g = load_golden("dpmpp")
    for steps in (10, 20, 2, 1):
        s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        ts, n = retrieve_timesteps(s, device="cpu", sigmas=get_sampling_sigmas(steps, 5.0))
        assert n == steps
        if f"timesteps_{steps}_5.0" in g:
            assert torch.equal(ts, g[f"timesteps_{steps}_5.0"]) and torch.equal(s.sigmas, g[f"sigmas_{steps}_5.0"])
        o = od.FlowDPMpp(1000, shift=1)
        o.set_timesteps(sigmas=od.get_sampling_sigmas(steps, 5.0))
        lat, lo = g["x"].to(DEV), g["x"]
        for i, t in enumerate(ts):
            lat = s.step(g[f"model_outputs_{steps}"][i].to(DEV), t, lat, return_dict=False)[0]
            lo = o.step(g[f"model_outputs_{steps}"][i], t, lo)
            assert torch.equal(lat.cpu(), lo), f"DPM++ {steps} steps, step {i}: HIP update differs from the oracle"
            assert torch.allclose(lat.cpu(), g[f"trajectory_{steps}"][i], rtol=2e-6, atol=2e-6), f"DPM++ step {i} vs reference golden"
    # fused CFG + convert path == separate path
    s1 = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1)
    s1.set_timesteps(sigmas=get_sampling_sigmas(10, 5.0), device="cpu")
    mo = g["model_outputs_10"]
    c, u, x = mo[0].to(DEV), mo[1].to(DEV), g["x"].to(DEV)
    prev, npred = s1.step_cfg(c, u, 5.0, s1.timesteps[0], x, want_noise_pred=True)
    ref_np = mo[1] + 5.0 * (mo[0] - mo[1])
    assert torch.equal(npred.cpu(), ref_np)
    s2 = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1)
    s2.set_timesteps(sigmas=get_sampling_sigmas(10, 5.0), device="cpu")
    assert torch.equal(prev, s2.step(ref_np.to(DEV), s2.timesteps[0], x, return_dict=False)[0])
    with pytest.raises(NotImplementedError):
        FlowDPMSolverMultistepScheduler(solver_type="heun")


# ---------------------------------------------------------------------------------------------------------------
# DiT
# ---------------------------------------------------------------------------------------------------------------
def _tiny_model(seed=0, **over):
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG, **over)
    sd = wan_dit.make_state_dict(cfg, seed)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(sd)
    return cfg, sd, m.to(DEV).eval()


def _truth_forward(sd, cfg, *args, **kw):
    """The oracle with every bf16 rounding removed (fp32 everywhere): the "truth" both implementations approximate.
    On the GPU the fp32 SDPA of a long sequence goes through torch's math backend, which materialises heads x L x L scores (71 GB at
    L = 27 280): there the oracle's attention_core is run a few heads at a time (heads are independent: same function)."""
    from oracle import lora as ora_lora, wan_dit
    old, core = wan_dit.BF16, wan_dit.attention_core

    def core_by_heads(q, k, v, k_lens=None):
        if q.device.type != "cuda" or q.size(1) * k.size(1) < 2 ** 28:
            return core(q, k, v, k_lens)
        return torch.cat([core(q[:, :, h:h + 2], k[:, :, h:h + 2], v[:, :, h:h + 2], k_lens) for h in range(0, q.size(2), 2)], dim=2)

    wan_dit.BF16 = ora_lora.BF16 = torch.float32
    wan_dit.attention_core = core_by_heads
    try:
        return wan_dit.dit_forward(sd, cfg, *args, **kw)
    finally:
        wan_dit.BF16 = ora_lora.BF16 = old
        wan_dit.attention_core = core


def test_dit_tiny_forward_vs_golden():
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    Lt = 256
    with torch.no_grad():
        truth = _truth_forward(sd, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
        one = m([g["x"].to(DEV)], g["t_one"].to(DEV), [g["ctx"].to(DEV)], Lt)[0]
        two = m([g["x"].to(DEV)], g["t_two"].to(DEV), [g["ctx"].to(DEV)], Lt)[0]
        pad = m([g["x"].to(DEV)], torch.full((1, Lt + 32), 937.0, device=DEV), [g["ctx"].to(DEV)], Lt + 32)[0]
        t1d = m([g["x"].to(DEV)], torch.tensor([937.0], device=DEV), [g["ctx"].to(DEV)], Lt)[0]
    assert one.dtype == torch.float32 and tuple(one.shape) == (48, 4, 16, 16)
    assert_model_close(one, g["out_one"], truth, name="t scalar")
    assert_model_close(two, g["out_two"], name="two timesteps (i2v)")
    assert torch.equal(pad, one), "sequence padding changed the valid tokens"
    assert torch.equal(t1d, one), "t of shape [B] must equal the expanded [B, seq_len] form"


def test_attention_modules_reference_signatures():
    """WanSelfAttention.forward(x, seq_lens, grid_sizes, freqs) / WanCrossAttention.forward(x, context, None) as standalone
    modules (the signatures UniVid's hooks and the reference's SP patch call, model.py:126-180)."""
    from oracle import wan_dit
    from univid_amd import detinit
    from univid_amd.wan.model import WanCrossAttention, WanSelfAttention, rope_params
    dim, heads = 256, 2
    grids, lens = [(2, 5, 7), (2, 5, 6)], [70, 60]                    # two samples, each with its own grid and key count
    Lt = lens[0]
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, Lt + 6, dim, generator=g)                      # 6 / 16 padding tokens: masked as keys (k_lens = seq_lens)
    ctx = (torch.randn(2, 32, dim, generator=g) * 0.5).to(BF16)
    d = dim // heads
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    for cls, prefix in ((WanSelfAttention, "blocks.0.self_attn."), (WanCrossAttention, "blocks.0.cross_attn.")):
        with torch.device(DEV):
            mod = cls(dim, heads, (-1, -1), True, 1e-6)
        sd = {prefix + k: v for k, v in mod.state_dict(keep_vars=True).items()}
        detinit.init_state_dict_(sd, 4)
        sdc = {k: v.detach().cpu() for k, v in sd.items()}
        with torch.no_grad():
            if cls is WanSelfAttention:
                got = mod(x.to(DEV), torch.tensor(lens), torch.tensor(grids), freqs)
                ref = wan_dit.self_attention(sdc, prefix, x, torch.tensor(lens), torch.tensor(grids), freqs, heads, 1e-6)
                rows = lens                                            # outputs of padding queries are don't-care
            else:
                got = mod(x.to(DEV), ctx.to(DEV), None)
                ref = wan_dit.cross_attention(sdc, prefix, x, ctx, heads, 1e-6)
                rows = [x.size(1)] * 2
        assert got.dtype == BF16 and got.shape == ref.shape
        # composite op (3 GEMMs + norm + attention + GEMM): bf16 rounding flips of the attention output are mixed by
        # the o projection, so gate on the relative rms error and the max error instead of per-element ulps - per sample
        for b in range(2):
            r = ref[b, :rows[b]].float()
            d = got[b, :rows[b]].float().cpu() - r
            assert d.pow(2).mean().sqrt() <= 4e-3 * r.pow(2).mean().sqrt(), (cls.__name__, b)
            assert d.abs().max() <= 2e-2 * r.abs().max(), (cls.__name__, b)


def test_flash_attention_operator_seam():
    """`univid_amd.wan.attention.flash_attention` = the reference's operator (attention.py:24-130): [B, L, N, C] in any float
    dtype, per-sample k_lens, result in q's dtype. Against oracle.attention_core (bf16 operands, fp32 softmax) and the fp64
    softmax; fp32 callers get fp32 back (values on the bf16 grid), fp16 callers stay fp16."""
    from oracle import wan_dit
    from univid_amd.wan.attention import attention, flash_attention
    B, Lq, Lk, N, D = 3, 150, 136, 2, 128
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(B, n, N, D, generator=g) for n in (Lq, Lk, Lk))
    v[:, :, :, :] += 0.25

    def truth_of(q, k, v, kl):
        o = torch.zeros(B, Lq, N, D, dtype=torch.float64)
        for b in range(B):
            qf, kf, vf = (t[b].double().transpose(0, 1) for t in (q, k[:, :kl[b]], v[:, :kl[b]]))
            o[b] = (torch.softmax(qf @ kf.transpose(1, 2) / math.sqrt(D), -1) @ vf).transpose(0, 1)
        return o

    def check(got, ref, truth, name):
        e_hip, e_ora = (got.double().cpu() - truth).abs(), (ref.double() - truth).abs()
        tol = 3 * bf16_ulp(truth.float()) + 2e-3 * truth.abs().float().max()
        record_margin("flash_attention seam: " + name, max_err=e_hip.max(), rms_hip=e_hip.pow(2).mean().sqrt(), rms_oracle=e_ora.pow(2).mean().sqrt())
        assert (e_hip <= tol).all(), f"{name}: max err {float(e_hip.max()):.3e}"
        assert e_hip.pow(2).mean().sqrt() <= 1.5 * e_ora.pow(2).mean().sqrt() + 1e-5, name

    qb, kb, vb = q.to(BF16), k.to(BF16), v.to(BF16)
    # (1) fp32 tensors, ragged k_lens (the self-attention call, model.py:145-150): cast to bf16 inside, fp32 returned
    klens = torch.tensor([136, 77, 5])
    out = flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), k_lens=klens, window_size=(-1, -1))
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, Lq, N, D)
    assert torch.equal(out, out.to(BF16).float()), "an fp32 caller gets the bf16 result widened, not recomputed"
    ref = wan_dit.attention_core(q, k, v, k_lens=klens)
    check(out, ref, truth_of(qb, kb, vb, klens.tolist()), "fp32 in, ragged k_lens")
    # the same through attention(): the reference's dispatcher (attention.py:133-179)
    assert torch.equal(attention(q.to(DEV), k.to(DEV), v.to(DEV), k_lens=klens), out)
    # (2) bf16 tensors, no lens (the cross-attention call, model.py:175): one stacked launch; q_lens = Lq is accepted
    out2 = flash_attention(qb.to(DEV), kb.to(DEV), vb.to(DEV), q_lens=torch.tensor([Lq] * B))
    assert out2.dtype == BF16
    check(out2, wan_dit.attention_core(qb, kb, vb), truth_of(qb, kb, vb, [Lk] * B), "bf16 in, all keys")
    for b in range(B):   # stacked launch == per-sample launches, bit for bit
        one = flash_attention(qb[b:b + 1].to(DEV), kb[b:b + 1].to(DEV), vb[b:b + 1].to(DEV))
        assert torch.equal(one[0], out2[b])
    # (3) fp16 tensors stay fp16 (half dtypes are never re-cast, attention.py:59-60); softmax_scale is honoured
    qh, kh, vh = q.half(), k.half(), v.half()
    out3 = flash_attention(qh.to(DEV), kh.to(DEV), vh.to(DEV), softmax_scale=0.05, dtype=torch.float16)
    assert out3.dtype == torch.float16
    t3 = torch.zeros(B, Lq, N, D, dtype=torch.float64)
    for b in range(B):
        qf, kf, vf = (t[b].double().transpose(0, 1) for t in (qh, kh, vh))
        t3[b] = (torch.softmax(qf @ kf.transpose(1, 2) * 0.05, -1) @ vf).transpose(0, 1)
    assert (out3.double().cpu() - t3).abs().max() <= 4e-3 * t3.abs().max()
    # (4) head_dim 64, odd Lk (not a multiple of 8: per-sample launches), non-contiguous q
    q4 = torch.randn(2, 70, 4, 64, generator=g).to(BF16)
    k4, v4 = (torch.randn(2, 33, 4, 64, generator=g).to(BF16) for _ in range(2))
    qnc = q4.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    assert not qnc.is_contiguous()
    out4 = flash_attention(qnc, k4.to(DEV), v4.to(DEV))
    ref4 = wan_dit.attention_core(q4, k4, v4)
    assert (out4.float().cpu() - ref4.float()).abs().max() <= 3e-2 and (out4.cpu() == ref4).float().mean() > 0.9
    # (5) loud errors for what is not built
    for kw in (dict(causal=True), dict(window_size=(4, 4)), dict(dropout_p=0.1), dict(q_scale=2.0), dict(q_lens=torch.tensor([10, Lq, Lq]))):
        with pytest.raises((NotImplementedError, ValueError)):
            flash_attention(qb.to(DEV), kb.to(DEV), vb.to(DEV), **kw)
    with pytest.raises(L().UnividHipError):
        flash_attention(qb, kb, vb)                                   # host tensors: no CPU path


def test_flash_attention_stacked_samples_match_single_calls():
    """batch > 1: q/k/out rows and V^T COLUMNS are stacked per sample (what one UV_EPI_BF16_T GEMM over the stacked rows
    writes); every sample's result is bit-identical to its own batch-1 call, ragged last key tile included."""
    from univid_amd._lib import EPI_BF16_T
    H, D, Lq, Lk, B = 2, 128, 200, 136, 3
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(9)
    q = torch.randn(B * Lq, C, generator=g, device=DEV).to(BF16)
    k = torch.randn(B * Lk, C, generator=g, device=DEV).to(BF16)
    v = torch.randn(B * Lk, C, generator=g, device=DEV).to(BF16)
    eye = torch.eye(C, device=DEV).to(BF16)
    cols = (B - 1) * Lk + (Lk + 63) // 64 * 64
    vt = torch.zeros(C, cols, dtype=BF16, device=DEV)
    L().gemm_bf16(v, eye, None, vt, EPI_BF16_T)                      # V^T of the stacked rows in one launch
    assert torch.equal(vt[:, :B * Lk], v.t())
    out = torch.zeros(B * Lq, C, dtype=BF16, device=DEV)
    L().flash_attn(q, k, vt, out, Lq, Lk, H, D, D ** -0.5, batch=B)
    for b in range(B):
        vt1 = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=BF16, device=DEV)
        vt1[:, :Lk] = v[b * Lk:(b + 1) * Lk].t()
        o1 = torch.zeros(Lq, C, dtype=BF16, device=DEV)
        L().flash_attn(q[b * Lq:(b + 1) * Lq], k[b * Lk:(b + 1) * Lk], vt1, o1, Lq, Lk, H, D, D ** -0.5)
        assert torch.equal(out[b * Lq:(b + 1) * Lq], o1), f"sample {b}"


def test_dit_batched_forward_is_bit_identical_to_sequential():
    """Samples of equal shape run as one stacked pass (the CFG cond/uncond pair in WanTI2V.denoise): per-sample results
    must not change by a single bit; mixed shapes fall back to one-by-one."""
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    Lt = 256
    gen = torch.Generator().manual_seed(5)
    x2 = torch.randn(48, 4, 16, 16, generator=gen)
    ctx2 = torch.randn(7, cfg["text_dim"], generator=gen)
    xa, xb = g["x"].to(DEV), x2.to(DEV)
    ca, cb = g["ctx"].to(DEV), ctx2.to(DEV)
    ta, tb = g["t_two"].to(DEV), torch.full((1, Lt), 321.0, device=DEV)
    with torch.no_grad():
        a = m([xa], ta, [ca], Lt)[0]
        b = m([xb], tb, [cb], Lt)[0]
        both = m([xa, xb], torch.cat([ta, tb]), [ca, cb], Lt)
        small = torch.randn(48, 2, 8, 8, generator=gen).to(DEV)
        mixed = m([xa, small], torch.cat([ta, tb]), [ca, cb], Lt)
        s_alone = m([small], tb, [cb], Lt)[0]
    assert torch.equal(both[0], a) and torch.equal(both[1], b)
    assert torch.equal(mixed[0], a) and torch.equal(mixed[1], s_alone)


def test_cfg_twin_samples_share_block0_self_attention_bit_identically():
    """A sampling step stacks the SAME latent under two prompts (textimage2video.py:380-385). Until the first cross-attention the two
    samples' rows are identical, so block 0's self-attention half runs once and is copied (WanModel.dedup_twins): outputs must be
    bit-identical to the full computation - t2v (one timestep) and i2v (two timesteps per sample) - fewer entry-point calls must be
    made, and samples that only LOOK alike (equal values in two tensors, or different per-token timesteps) must not take the shortcut."""
    from univid_amd import _lib
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    Lt = 256
    x, ctx = g["x"].to(DEV), g["ctx"].to(DEV)
    ctx2 = (ctx * 0.5).contiguous()
    seen = []
    orig = m.blocks[0].self_attn._self_attn
    m.blocks[0].self_attn._self_attn = lambda h, L, grid, freqs, xr, gate, gt, batch=1, sp=None, **kw: (seen.append(batch), orig(h, L, grid, freqs, xr, gate, gt, batch, sp, **kw))[1]
    for t in (g["t_one"].to(DEV), g["t_two"].to(DEV)):
        tt = torch.cat([t, t])
        with torch.no_grad():
            m.dedup_twins = True
            a = m([x, x], tt, [ctx, ctx2], Lt)
            m.dedup_twins = False
            b = m([x, x], tt, [ctx, ctx2], Lt)
            m.dedup_twins = True
            c = m([x, x.clone()], tt, [ctx, ctx2], Lt)                       # equal values, two tensors: not detected, full computation
            t_other = torch.cat([t, torch.full_like(t, 123.0)])
            d = m([x, x], t_other, [ctx, ctx2], Lt)                          # same latent, different timesteps: must not share
            d_ref = m([x], t_other[1:], [ctx2], Lt)[0]
        assert seen == [1, 2, 2, 2, 1], seen                                   # block 0's self-attention: once for the twins only
        seen.clear()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], a[1])
        assert torch.equal(c[0], b[0]) and torch.equal(c[1], b[1])
        assert torch.equal(d[0], b[0]) and torch.equal(d[1], d_ref)


def test_context_cache_is_bit_identical_and_tracks_changes():
    """text_embedding and the blocks' cross-attention K / V^T of the context are computed once per context (they depend on
    neither latent nor timestep, model.py:170-172, 472-478): cached forwards must equal uncached ones bit for bit, an in-place
    edit of a context tensor or new weights must invalidate, and mixed-shape batches keep one entry per sample group."""
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    Lt = 256
    x, ctx = g["x"].to(DEV), g["ctx"].to(DEV).clone()
    ta, tb = g["t_one"].to(DEV), torch.full((1, Lt), 321.0, device=DEV)
    with torch.no_grad():
        m.cache_context = False
        ra, rb = m([x], ta, [ctx], Lt)[0], m([x], tb, [ctx], Lt)[0]
        m.cache_context = True
        a = m([x], ta, [ctx], Lt)[0]
        gen = m._ctx_gen
        b = m([x], tb, [ctx], Lt)[0]                      # second step: same context tensors -> cache hit
        assert m._ctx_gen == gen and len(m.blocks[0].cross_attn._kv_cache) == 1
        assert torch.equal(a, ra) and torch.equal(b, rb)
        ctx.mul_(0.5)                                     # in-place edit: _version changes -> recomputed
        c = m([x], ta, [ctx], Lt)[0]
        assert m._ctx_gen == gen + 1 and not torch.equal(c, ra)
        m.cache_context = False
        assert torch.equal(c, m([x], ta, [ctx], Lt)[0])
        m.cache_context = True
        # the CFG pair (stacked) and a mixed-shape batch (two groups) under one context generation
        small = torch.randn(48, 2, 8, 8, device=DEV)
        pair = m([x, x], torch.cat([ta, ta]), [ctx, ctx * 2], Lt)
        mixed = m([x, small], torch.cat([ta, ta]), [ctx, ctx * 2], Lt)
        assert torch.equal(pair[0], c) and torch.equal(mixed[0], c)
        # new weights: load_state_dict -> invalidate() -> nothing stale
        sd2 = {k: (v * 1.01 if "cross_attn.k.weight" in k else v) for k, v in sd.items()}
        m.load_state_dict(sd2)
        d = m([x], ta, [ctx], Lt)[0]
        assert not torch.equal(d, c)
        m.cache_context = False
        assert torch.equal(d, m([x], ta, [ctx], Lt)[0])


def test_dit_head_dim_128_and_odd_grid():
    from oracle import wan_dit
    cfg, sd, m = _tiny_model(3, num_heads=2)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(48, 3, 10, 12, generator=g)
    ctx = [torch.randn(32, cfg["text_dim"], generator=g)]            # full-length context (no padding rows)
    Lt = 3 * 5 * 6
    t = torch.full((1, Lt), 500.0)
    with torch.no_grad():
        ref = wan_dit.dit_forward(sd, cfg, [x], t, ctx, Lt)[0]
        truth = _truth_forward(sd, cfg, [x], t, ctx, Lt)[0]
        out = m([x.to(DEV)], t.to(DEV), [c.to(DEV) for c in ctx], Lt)[0]
    assert_model_close(out, ref, truth, name="head_dim 128")


def test_embedding_stages_and_head_ti2v5b_width_vs_oracle():
    """SURVEY rows a5 / a6 / a7 / a16 on their own at the production width (a TI2V-5B model with ZERO blocks: patch embedding ->
    head -> unpatchify, plus the time and text embeddings it computes on the way), two distinct timesteps (the i2v case), an odd
    grid and padding, each stage against the oracle's tensor for that stage."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TI2V_5B_CFG, num_layers=0)
    sd = wan_dit.make_state_dict(cfg, 5)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(48, 3, 10, 14, generator=g)                 # 3 x 5 x 7 = 105 tokens
    ctx = [torch.randn(77, 4096, generator=g) * 0.1]
    L = 105
    t = torch.cat([torch.zeros(35), torch.full((L + 7 - 35,), 937.0)]).unsqueeze(0)     # frame 0 at t = 0 (i2v mask), padded to L + 7
    with torch.no_grad():
        ref, _, st = wan_dit.dit_forward(sd, cfg, [x], t, ctx, L + 7, return_hidden=True)
        truth = _truth_forward(sd, cfg, [x], t, ctx, L + 7)
        out = m([x.to(DEV)], t.to(DEV), [c.to(DEV) for c in ctx], L + 7)[0]
        e_rows, e0_rows = m._time_rows(torch.tensor([0.0, 937.0], device=DEV))
        cemb = m.embed_context([c.to(DEV) for c in ctx])
    # a6: time embedding / projection rows (fp32 island, model.py:462-469)
    assert_f32_close(e_rows[0], st["e"][0, 0], name="time embedding t=0")
    assert_f32_close(e_rows[1], st["e"][0, 50], name="time embedding t=937")
    assert_f32_close(e0_rows[1].view(6, -1), st["e0"][0, 50], name="time projection t=937")
    # a7: text embedding of the zero-padded prompt embeddings (bf16 under autocast, model.py:472-478): 1 bf16 ulp
    d = (cemb[0].float().cpu() - st["ctx"][0].float()).abs()
    assert float((d / st["ctx"][0].float().abs().clamp_min(0.05)).max()) < 2 ** -7, "text embedding"
    assert (cemb[0][77:].float().cpu() - st["ctx"][0][77:].float()).abs().max() < 2e-2        # padded rows: bias path only
    # a5 + a16: patch embedding -> head (fp32 LayerNorm / modulation / Linear) -> unpatchify
    assert out.shape == ref[0].shape == (48, 3, 10, 14)
    # With no residual stream behind it, the head sees the patch embedding's bf16 rounding directly (one flipped bf16 ulp among its
    # 3072 inputs moves an output by ~1e-3 of its size), so the elementwise tolerance is not the informative gate here; the distance
    # to the unrounded result is: HIP must be as close to it as the reference arithmetic is.
    # Measured on MI355X: 38 % inside, max 1.7e-3 of the range, rms to the truth 0.87 x the oracle's own.
    assert_model_close(out, ref[0], truth[0], frac=0.31, max_rel=2.1e-3, truth_ratio=1.05, name="0-block TI2V-5B: patch embedding + head")


def test_dit_block_ti2v5b_width_vs_golden():
    """One TI2V-5B-width block (dim 3072, ffn 14336, 24 heads): fused path and the reference-signature forward."""
    from oracle import wan_dit
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock, rope_params
    g = load_golden("dit_block_3072")
    dim, ffn, heads, Lt = 3072, 14336, 24, 48
    with torch.device(DEV):
        blk = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, g["seed"])
    blk.eval()
    d = dim // heads
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    e0 = g["e_rows"][g["tid"]].unsqueeze(0)
    seq_lens = torch.tensor([Lt])
    with torch.no_grad():
        out = blk(g["x"].to(DEV), e0.to(DEV), seq_lens, g["grid"], freqs, g["ctx"].to(DEV), None)
        outb = blk(g["x"].to(BF16).to(DEV), e0.to(DEV), seq_lens, g["grid"], freqs, g["ctx"].to(DEV), None)
    assert out.dtype == torch.float32
    sdc = {k: v.detach().cpu() for k, v in sd.items()}
    old, wan_dit.BF16 = wan_dit.BF16, torch.float32                       # "truth": the same block with no bf16 rounding
    try:
        with torch.no_grad():
            truth = wan_dit.block_forward(sdc, "blocks.0.", g["x"], e0, seq_lens, g["grid"], wan_dit.rope_table(d), g["ctx"].float(), heads, 1e-6)
    finally:
        wan_dit.BF16 = old
    # at width 3072 the reference's own bf16 roundings put BOTH implementations ~1e-3 (rms) from the truth; the two
    # differ from each other by less than either differs from the truth
    assert_model_close(out[0], g["out_f32"][0], truth[0], frac=0.69, max_rel=2.5e-3, name="block f32 stream")   # measured 74.5 %, 1.7e-3, 1.003
    assert_model_close(outb[0], g["out_bf16"][0], frac=0.69, max_rel=2.5e-3, name="block bf16 stream (block 0)")   # measured 74.5 %, 2.1e-3
    # fused path: 2 modulation rows + token->row map instead of a per-token table
    from univid_amd.wan.model import _freqs_device
    x = g["x"][0].to(DEV).clone()
    with torch.no_grad():
        blk._run(x, Lt, g["e_rows"].reshape(2, -1).to(DEV), g["tid"].to(torch.int32).to(DEV), (2, 4, 6),
                 _freqs_device(freqs, torch.device(DEV)), g["ctx"][0].to(DEV), first_block=False)
    assert torch.equal(x, out[0]), "row-table modulation must equal the per-token modulation bit for bit"


def test_dit_block_ti2v5b_width_1014_tokens_vs_oracle():
    """BASELINE config 2 ("HIP DiT block vs reference eager, numerics gate") at a bounded size: one TI2V-5B-width block,
    L = 13 x 6 x 13 = 1014 tokens (16 KV tiles, ragged last tile, 8 query blocks), two distinct timesteps, against the CPU
    oracle run here (too large for a committed fixture)."""
    from oracle import wan_dit
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device, rope_params
    torch.set_num_threads(min(32, torch.get_num_threads()))
    dim, ffn, heads, grid = 3072, 14336, 24, (13, 6, 13)
    Lt = grid[0] * grid[1] * grid[2]
    with torch.device(DEV):
        blk = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, 11)
    blk.eval()
    sdc = {k: v.detach().cpu() for k, v in sd.items()}
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, Lt, dim, generator=g)
    e_rows = torch.randn(2, 6, dim, generator=g) * 0.3
    tid = (torch.arange(Lt) >= grid[1] * grid[2]).long()              # first latent frame at its own timestep (i2v)
    ctx = (torch.randn(1, 512, dim, generator=g) * 0.5).to(BF16)
    d = dim // heads
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    e0 = e_rows[tid].unsqueeze(0)
    with torch.no_grad():
        ref = wan_dit.block_forward(sdc, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        old, wan_dit.BF16 = wan_dit.BF16, torch.float32
        try:
            truth = wan_dit.block_forward(sdc, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx.float(), heads, 1e-6)
        finally:
            wan_dit.BF16 = old
        xs = x[0].to(DEV).clone()
        blk.prepare()
        blk._run(xs, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), grid, _freqs_device(freqs, torch.device(DEV)),
                 ctx[0].to(DEV), first_block=False)
    assert_model_close(xs, ref[0], truth[0], frac=0.81, max_rel=2.1e-3, name="TI2V-5B block, L=1014")   # measured 84.7 %, 1.7e-3, 1.0003


def test_dit_block_ti2v5b_width_full_length_vs_cpu_oracle():
    """The bench's own shape against the PINNED oracle, not against oracle text run by torch-ROCm eager: one TI2V-5B-width block at
    L = 13 x 22 x 40 = 11 440 tokens (the 49-frame 704 x 1280 latent: the long-key attention kernel with its 12- / 8-unit blocks, the
    persistent GEMM with its leftover-row launch, every glue kernel at its full-size instantiation), two distinct timesteps, against
    oracle/wan_dit.block_forward on the host cores (about 4 s per run on 32 threads) and its no-rounding truth run."""
    from oracle import wan_dit
    from univid_amd import detinit
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device, rope_params
    torch.set_num_threads(min(32, torch.get_num_threads()))
    dim, ffn, heads, grid = 3072, 14336, 24, (13, 22, 40)
    Lt = grid[0] * grid[1] * grid[2]
    with torch.device(DEV):
        blk = WanAttentionBlock(dim, ffn, heads, (-1, -1), True, True, 1e-6)
    sd = {"blocks.0." + k: v for k, v in blk.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, 12)
    blk.eval()
    sdc = {k: v.detach().cpu() for k, v in sd.items()}
    g = torch.Generator().manual_seed(22)
    x = torch.randn(1, Lt, dim, generator=g)
    e_rows = torch.randn(2, 6, dim, generator=g) * 0.3
    tid = (torch.arange(Lt) >= grid[1] * grid[2]).long()              # first latent frame at its own timestep (i2v)
    ctx = (torch.randn(1, 512, dim, generator=g) * 0.5).to(BF16)
    d = dim // heads
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    e0 = e_rows[tid].unsqueeze(0)
    with torch.no_grad():
        ref = wan_dit.block_forward(sdc, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        old, wan_dit.BF16 = wan_dit.BF16, torch.float32
        try:
            truth = wan_dit.block_forward(sdc, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx.float(), heads, 1e-6)
        finally:
            wan_dit.BF16 = old
        xs = x[0].to(DEV).clone()
        blk.prepare()
        blk._run(xs, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), grid, _freqs_device(freqs, torch.device(DEV)),
                 ctx[0].to(DEV), first_block=False)
    assert_model_close(xs, ref[0], truth[0], frac=0.83, max_rel=3.4e-3, name="TI2V-5B block, L=11440 (CPU oracle)")   # measured 86.2 %, 2.8e-3, 1.0008


def SAMPLER10_GATE(what):
    # 10 steps take 5x larger steps than 50. Measured on MI355X (profiles/r02_parity_margins.json): noise_pred 1.9e-3 (step 0) ->
    # 3.3e-3 (step 9), latents 1.4e-5 -> 5.2e-4. Gates = 1.5 x the largest measured value.
    return 4.0e-3 if what.startswith("noise_pred") else 6.3e-4      # x 1.2 since round 4


def test_sampler_trajectories_vs_golden():
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    keep = g["kept_steps"].tolist()
    for mode in ("t2v", "i2v"):
        rec = []
        with torch.no_grad():
            final = pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], g["steps"], g["shift"],
                                 g["guide_scale"], z=(g["z"].to(DEV) if mode == "i2v" else None), record=rec)
        assert len(rec) == g["steps"] and torch.equal(final, rec[-1][1])
        meas = {}
        for j, i in enumerate(keep):
            ref_np, ref_lat = g[f"{mode}_noise_pred"][j], g[f"{mode}_latents"][j]
            # CFG (x5) and the sampler steps amplify the bf16 noise of the DiT: gate on relative RMS error
            for got, ref, what in ((rec[i][0], ref_np, "noise_pred"), (rec[i][1], ref_lat, "latent")):
                meas[f"{what}_step{i}"] = _rel_rms(got, ref)
        record_margin(f"10-step {mode} trajectory (tiny DiT) rel rms vs reference", **meas)
        for k, v in meas.items():
            assert v < SAMPLER10_GATE(k), f"{mode} {k}: rel rms {v:.3e}"
        if mode == "i2v":
            assert torch.equal(final[:, 0].cpu(), g["z"][:, 0]), "i2v must keep the first latent frame pinned to z"


def test_graph_runner_serves_new_prompts_without_recapture_and_never_goes_stale():
    """One captured HIP graph per (latent shape, mode, prepared weights) serves every prompt: the step-constant context work lives in
    buffers the runner owns and WanTI2V.denoise refreshes them in place at the start of every call (_GraphedPair.refresh). Round-3
    advisor finding: tensors created under torch.inference_mode() have no version counter, so a prompt-embeds buffer refilled in place
    between two generations is invisible to any identity / version key - with the refresh there is nothing left to go stale. Checked:
    graph == eager for a first prompt, for the same buffer refilled in place under inference mode (the runner is REUSED), for different
    prompt tensors of another length, and for version-counted tensors edited in place; and the eager path's own context cache is not
    disturbed by the runner's buffers."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V, _GraphedPair
    g = load_golden("sampler_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    args = (2, g["shift"], g["guide_scale"])
    with torch.no_grad():
        # a runner built directly and used straight away (no refresh: its constructor fills its buffers with the code every later call
        # uses) equals the eager pair bit for bit - and building it leaves the model as it was found: no embedded context, no cached
        # K / V^T, the text weight (which the capture does not consult) untouched
        noise = g["noise"].to(DEV)
        ctx, ctxn = [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)]
        seq_len = noise.shape[1] * noise.shape[2] * noise.shape[3] // 4
        m.set_text_weight((0.5, 1.0), 4)
        tw = m._text_weight
        assert tw is not None
        direct = _GraphedPair(m, noise, ctx, ctxn, seq_len, None)
        assert m._ctx_cache is None and all(b.cross_attn._kv_cache == {} for b in m.blocks) and m._text_weight is tw
        m.set_text_weight(None)
        for tval in (937.0, 500.0):
            tvec = torch.full((1, seq_len), tval, device=DEV)
            want = m([noise, noise], t=torch.cat([tvec, tvec]), context=[ctx[0], ctxn[0]], seq_len=seq_len)
            got = direct(noise, tval)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], got[1])
        assert m._ctx_cache is None and all(b.cross_attn._kv_cache == {} for b in m.blocks)
        del direct
    with torch.inference_mode():
        noise = g["noise"].to(DEV)
        ctx, ctxn = [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()]
        a_graph = pipe.denoise(noise, ctx, ctxn, *args, graph=True).clone()
        r1 = pipe._runner
        assert r1 is not None
        a_eager = pipe.denoise(noise, ctx, ctxn, *args, graph=False)
        assert torch.equal(a_graph, a_eager)
        ctx[0].mul_(-0.5)                                  # same storage, same (absent) version: a new prompt in the old buffer
        b_graph = pipe.denoise(noise, ctx, ctxn, *args, graph=True).clone()
        assert pipe._runner is r1, "a new prompt must not cost a recapture"
        b_eager = pipe.denoise(noise, ctx, ctxn, *args, graph=False)
        assert torch.equal(b_graph, b_eager), "graph replay used the previous prompt's context"
        assert not torch.equal(b_graph, a_graph)
        other = [torch.randn(11, cfg["text_dim"], device=DEV)]             # other tensors, another prompt length
        c_graph = pipe.denoise(noise, other, ctxn, *args, graph=True).clone()
        assert pipe._runner is r1 and torch.equal(c_graph, pipe.denoise(noise, other, ctxn, *args, graph=False))
    with torch.no_grad():                                  # version-counted tensors
        ctx2, ctxn2 = [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()]
        d1 = pipe.denoise(g["noise"].to(DEV), ctx2, ctxn2, *args, graph=True).clone()
        assert pipe._runner is r1 and torch.equal(d1, a_graph)
        d2 = pipe.denoise(g["noise"].to(DEV), ctx2, ctxn2, *args, graph=True)       # unchanged tensors (round 5: refreshed all the same - no identity shortcut)
        assert torch.equal(d1, d2)
        ctx2[0].mul_(-0.5)                                 # in-place edit bumps the version: refreshed
        d3 = pipe.denoise(g["noise"].to(DEV), ctx2, ctxn2, *args, graph=True)
        assert pipe._runner is r1 and torch.equal(d3, b_graph)
        # i2v is another graph (other token -> timestep map); both stay captured (WanTI2V.max_graph_runners = 2): going back to t2v replays
        # the FIRST graph, with the prompt of THAT call, and alternating the two modes never captures again
        z = g["z"].to(DEV)
        e_graph = pipe.denoise(g["noise"].to(DEV), ctx2, ctxn2, *args, z=z, graph=True).clone()
        r2 = pipe._runner
        assert r2 is not r1
        assert torch.equal(e_graph, pipe.denoise(g["noise"].to(DEV), ctx2, ctxn2, *args, z=z, graph=False))
        ctx3 = [g["ctx"].to(DEV).clone()]
        f_graph = pipe.denoise(g["noise"].to(DEV), ctx3, ctxn2, *args, graph=True)
        assert pipe._runner is r1 and torch.equal(f_graph, a_graph), "back to t2v: the first graph, the current prompt"
        assert torch.equal(pipe.denoise(g["noise"].to(DEV), ctx2, ctxn2, *args, z=z, graph=True), e_graph) and pipe._runner is r2
        # a third shape evicts the least recently used (the t2v graph); the i2v graph survives
        shorter = g["noise"].to(DEV)[:, :1].contiguous()
        s_graph = pipe.denoise(shorter, ctx3, ctxn2, *args, graph=True).clone()
        assert len(pipe._runners) == 2 and r2 in pipe._runners.values() and r1 not in pipe._runners.values()
        assert torch.equal(s_graph, pipe.denoise(shorter, ctx3, ctxn2, *args, graph=False))
        assert torch.equal(pipe.denoise(g["noise"].to(DEV), ctx3, ctxn2, *args, graph=True), a_graph), "re-captured after eviction"
        # new prepared weights: every held graph is dropped at the next graph-mode call
        m._prep_gen += 1
        assert torch.equal(pipe.denoise(g["noise"].to(DEV), ctx3, ctxn2, *args, graph=True), a_graph) and len(pipe._runners) == 1
        pipe._runner = None
        assert pipe._runner is None and not pipe._runners


def test_sampler_dpmpp_trajectories_vs_golden():
    """The reference's other solver (sample_solver='dpm++', textimage2video.py:343-351, 535-543): 12 DPM-Solver++ steps of the
    tiny DiT, t2v and i2v, against the fixture generated from the reference's FlowDPMSolverMultistepScheduler; also through
    WanTI2V.t2v(sample_solver=...) and the unsupported-solver error."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny_dpmpp")
    cfg, sd, m = _tiny_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    keep = g["kept_steps"].tolist()
    for mode in ("t2v", "i2v"):
        rec = []
        with torch.no_grad():
            final = pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], g["steps"], g["shift"],
                                 g["guide_scale"], z=(g["z"].to(DEV) if mode == "i2v" else None), record=rec, sample_solver="dpm++")
        assert len(rec) == g["steps"] and torch.equal(final, rec[-1][1]) and torch.isfinite(final).all()
        meas = {}
        for j, i in enumerate(keep):
            meas[f"noise_pred_step{i}"] = _rel_rms(rec[i][0], g[f"{mode}_noise_pred"][j])
            meas[f"latent_step{i}"] = _rel_rms(rec[i][1], g[f"{mode}_latents"][j])
        record_margin(f"12-step DPM-Solver++ {mode} trajectory (tiny DiT) rel rms vs reference", **meas)
        for k, v in meas.items():
            assert v < SAMPLER10_GATE(k), f"{mode} {k}: rel rms {v:.3e}"
        if mode == "i2v":
            assert torch.equal(final[:, 0].cpu(), g["z"][:, 0])
    with torch.no_grad():
        lat = pipe.t2v("", size=(256, 256), frame_num=13, shift=g["shift"], sample_solver="dpm++", sampling_steps=g["steps"],
                       guide_scale=g["guide_scale"], prompt_embeds=[g["ctx"]], negative_prompt_embeds=[g["ctx_null"]],
                       noise=g["noise"].to(DEV), decode=False)
    assert torch.equal(lat, pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], g["steps"], g["shift"],
                                         g["guide_scale"], sample_solver="dpm++"))
    with pytest.raises(NotImplementedError):
        pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], 2, 5.0, 5.0, sample_solver="ddim")


def _rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def test_sampler_50_step_trajectories_vs_golden():
    """BASELINE config 2's step count: 50 UniPC flow steps (t2v and i2v) of the tiny DiT against the reference-generated
    fixture, 6 kept steps. CFG (x5) and the multistep solver amplify the DiT's bf16 rounding noise step by step; the growth is
    recorded (margins file) and gated at the measured level x 1.5."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny_50")
    cfg, sd, m = _tiny_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    keep = g["kept_steps"].tolist()
    assert g["steps"] == 50 and keep[-1] == 49
    for mode in ("t2v", "i2v"):
        rec = []
        with torch.no_grad():
            final = pipe.denoise(g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], g["steps"], g["shift"],
                                 g["guide_scale"], z=(g["z"].to(DEV) if mode == "i2v" else None), record=rec)
        assert len(rec) == 50 and torch.equal(final, rec[-1][1]) and torch.isfinite(final).all()
        meas = {}
        for j, i in enumerate(keep):
            meas[f"noise_pred_step{i}"] = _rel_rms(rec[i][0], g[f"{mode}_noise_pred"][j])
            meas[f"latent_step{i}"] = _rel_rms(rec[i][1], g[f"{mode}_latents"][j])
        record_margin(f"50-step {mode} trajectory (tiny DiT) rel rms vs reference", **meas)
        for k, v in meas.items():
            assert v < SAMPLER50_GATE(k), f"{mode} {k}: rel rms {v:.3e}"
        if mode == "i2v":
            assert torch.equal(final[:, 0].cpu(), g["z"][:, 0])


def SAMPLER50_GATE(what):
    # measured on MI355X (profiles/r02_parity_margins.json): noise_pred 1.9e-3 (step 0) growing to 3.0e-3 (step 49) - CFG's x5
    # on the DiT's bf16 noise -, latents 2.5e-6 growing to 2.1e-4 over the 50 steps. Gates = 1.5 x the largest measured value.
    return 3.7e-3 if what.startswith("noise_pred") else 2.6e-4      # x 1.2 since round 4


def test_dit_stack_ti2v5b_width_depth_vs_oracle():
    """DEPTH at TI2V-5B width: an 8-block, 3072-wide, 24-head stack at L = 4 x 10 x 13 = 520 tokens (two distinct timesteps,
    77-row prompt) through WanModel.forward, against the CPU oracle's dit_forward and its no-rounding truth run. The residual
    stream after blocks 1, 2, 4 and 8 and the final head output are compared; inside-fraction, max error and rms-vs-truth of
    both implementations are recorded per depth (reference stack: model.py:489-497, 30 blocks)."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    cfg = dict(wan_dit.TI2V_5B_CFG, num_layers=8)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(23)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    grid = (4, 10, 13)
    Lt = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(31)
    x = torch.randn(48, grid[0], 2 * grid[1], 2 * grid[2], generator=g)
    ctx = [torch.randn(77, cfg["text_dim"], generator=g) * 0.1]
    t = torch.full((1, Lt), 812.0)
    t[0, :grid[1] * grid[2]] = 0.0                                   # i2v: first latent frame at timestep 0
    hidden = []
    for blk in m.blocks:
        def run(xs, *a, _orig=blk._run, **kw):
            _orig(xs, *a, **kw)
            hidden.append(xs.clone())
        blk._run = run
    with torch.no_grad():
        out = m([x.to(DEV)], t.to(DEV), [c.to(DEV) for c in ctx], Lt)[0]
        ref, ref_h, _ = wan_dit.dit_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
        tru, tru_h, _ = _truth_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
    assert len(hidden) == 8
    for depth in (1, 2, 4, 8):
        assert_model_close(hidden[depth - 1], ref_h[depth - 1][0], tru_h[depth - 1][0], frac=DEPTH_GATE[depth][0],
                           max_rel=DEPTH_GATE[depth][1], truth_ratio=1.02, name=f"TI2V-5B width, residual stream after block {depth} (L=520)")
    assert_model_close(out, ref[0], tru[0], frac=DEPTH_GATE["out"][0], max_rel=DEPTH_GATE["out"][1], truth_ratio=1.02,
                       name="TI2V-5B width, 8-block forward output (L=520)")


# measured on MI355X (profiles/r03_parity_margins.json): inside 94.6 / 87.6 / 75.7 / 53.1 %, max error 3.8e-3 / 3.9e-3 / 3.8e-3 / 9.7e-4 of the
# range, rms-vs-truth ratio 0.9995-1.0000; gates = 1.5 x the measured outside fraction / maximum
FULL_LENGTH_GATE = {1: (0.93, 4.6e-3), 2: (0.85, 4.8e-3), 4: (0.70, 4.6e-3), "out": (0.44, 1.2e-3)}      # measured x 1.2 (round 4)


def test_dit_stack_full_length_vs_cpu_oracle():
    """DEPTH at the bench's own length against the PINNED oracle: a 4-block stack at TI2V-5B width and L = 13 x 22 x 40 = 11 440 tokens
    (two timesteps, 77-row prompt) through WanModel.forward - patch embedding, time embedding, text embedding, blocks, head,
    unpatchify - against oracle/wan_dit.dit_forward on the host cores and its no-rounding truth run (the 30-block full-length run is
    compared with the oracle text on torch-ROCm eager, test_real_shapes_vs_eager_oracle; this one ties the same shape to the CPU)."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    cfg = dict(wan_dit.TI2V_5B_CFG, num_layers=4)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(29)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    grid = (13, 22, 40)
    Lt = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(37)
    x = torch.randn(48, grid[0], 2 * grid[1], 2 * grid[2], generator=g)
    ctx = [torch.randn(77, cfg["text_dim"], generator=g) * 0.1]
    t = torch.full((1, Lt), 812.0)
    t[0, :grid[1] * grid[2]] = 0.0                                   # i2v: first latent frame at timestep 0
    hidden = []
    for blk in m.blocks:
        def run(xs, *a, _orig=blk._run, **kw):
            _orig(xs, *a, **kw)
            hidden.append(xs.clone())
        blk._run = run
    with torch.no_grad():
        out = m([x.to(DEV)], t.to(DEV), [c.to(DEV) for c in ctx], Lt)[0]
        ref, ref_h, _ = wan_dit.dit_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
        tru, tru_h, _ = _truth_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
    assert len(hidden) == 4
    for depth in (1, 2, 4):
        assert_model_close(hidden[depth - 1], ref_h[depth - 1][0], tru_h[depth - 1][0], frac=FULL_LENGTH_GATE[depth][0],
                           max_rel=FULL_LENGTH_GATE[depth][1], truth_ratio=1.02, name=f"TI2V-5B width, residual stream after block {depth} (L=11440, CPU oracle)")
    assert_model_close(out, ref[0], tru[0], frac=FULL_LENGTH_GATE["out"][0], max_rel=FULL_LENGTH_GATE["out"][1], truth_ratio=1.02,
                       name="TI2V-5B width, 4-block forward output (L=11440, CPU oracle)")


# measured on MI355X over rounds 3-5 by tests/manual/full_forward_vs_cpu_oracle.py (profiles/r05_full_forward_vs_cpu_oracle.log: inside 61.3 / 47.5 /
# 37.9 / 27.7 %, max error 3.42e-3 / 3.74e-3 / 3.66e-3 / 2.62e-3 of the range, rms-vs-truth ratio 1.0002-1.0007); gates = measured x 1.2
FULL_STACK_GATE = {8: (0.51, 4.2e-3), 16: (0.395, 4.5e-3), 30: (0.315, 4.4e-3), "out": (0.23, 3.15e-3)}


def test_dit_full_30_block_forward_vs_cpu_oracle():
    """THE headline configuration against the PINNED oracle, in the driver's suite (rounds 3-5 ran it by hand): the whole 30-block TI2V-5B
    DiT forward at the bench's length (L = 13 x 22 x 40 = 11 440 tokens, two timesteps, 77-row prompt) through WanModel.forward on the GPU
    against oracle/wan_dit.dit_forward on the host cores (32 threads, ~2 minutes); residual stream after blocks 8, 16, 30 and the output.
    The no-rounding truth run (another ~4 minutes of host time) is not repeated here: the rms-vs-truth ratio is gated on the same shape by
    test_dit_stack_full_length_vs_cpu_oracle (4 blocks) and was 1.0002-1.0007 over all 30 blocks in every hand-run round."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    n = 30
    cfg = dict(wan_dit.TI2V_5B_CFG, num_layers=n)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(0)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    grid = (13, 22, 40)
    Lt = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(41)
    x = torch.randn(48, grid[0], 2 * grid[1], 2 * grid[2], generator=g)
    ctx = [torch.randn(77, cfg["text_dim"], generator=g) * 0.1]
    t = torch.full((1, Lt), 812.0)
    t[0, :grid[1] * grid[2]] = 0.0
    depths = (8, 16, 30)
    hidden = {}
    for i, blk in enumerate(m.blocks):
        def run(xs, *a, _orig=blk._run, _d=i + 1, **kw):
            _orig(xs, *a, **kw)
            if _d in depths:
                hidden[_d] = xs.float().cpu()
        blk._run = run
    with torch.no_grad():
        out = m([x.to(DEV)], t.to(DEV), [c.to(DEV) for c in ctx], Lt)[0].cpu()
        del m
        torch.cuda.empty_cache()
        ref, ref_h, _ = wan_dit.dit_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
    for d in depths:
        assert_model_close(hidden[d], ref_h[d - 1][0], frac=FULL_STACK_GATE[d][0], max_rel=FULL_STACK_GATE[d][1],
                           name=f"TI2V-5B, residual stream after block {d} of 30 (L=11440, CPU oracle)")
    assert_model_close(out, ref[0], frac=FULL_STACK_GATE["out"][0], max_rel=FULL_STACK_GATE["out"][1], name="TI2V-5B, 30-block forward output (L=11440, CPU oracle)")


def _trained_regime_state_dict(sd, cfg, outliers=(5, 777, 1500, 3001)):
    """Pushes deterministic-init weights into the numeric regime of a TRAINED Wan checkpoint (the statistics the detinit / random-context
    parity runs do not exercise): a few residual-stream channels hundreds of times larger than the rest (outlier channels), attention
    logits with sigma ~ 8 (peaked softmax: the online-softmax rescale path is hot, single keys dominate rows), modulation gates of
    order 10 instead of order 1."""
    sd = {k: v.clone() for k, v in sd.items()}
    C = cfg["dim"]
    out = [c for c in outliers if c < C]
    sd["patch_embedding.weight"][out] *= 300.0                     # outlier channels enter with the patch embedding ...
    sd["patch_embedding.bias"][out] *= 300.0
    for i in range(cfg["num_layers"]):
        b = f"blocks.{i}."
        for att in ("self_attn", "cross_attn"):                     # QK-RMSNorm output scale sets the logit scale: sigma 1 -> 8
            sd[b + att + ".norm_q.weight"] *= 8.0 ** 0.5
            sd[b + att + ".norm_k.weight"] *= 8.0 ** 0.5
        sd[b + "ffn.2.weight"][out] *= 30.0                          # ... and every block keeps feeding them
        sd[b + "modulation"][:, 2] = sd[b + "modulation"][:, 2] * 10.0 + 3.0     # gates (chunks 2 and 5 of the 6-way modulation)
        sd[b + "modulation"][:, 5] = sd[b + "modulation"][:, 5] * 10.0 - 4.0
    g = 2 * C
    sd["time_projection.1.weight"][g:g + C] *= 10.0
    sd["time_projection.1.weight"][5 * C:] *= 10.0
    return sd


def test_dit_trained_weight_regime_stress_vs_oracle():
    """Parity under TRAINED-weight statistics (the reference runs real checkpoints, textimage2video.py:88-103; offline only their
    statistics can be imitated): a 3-block stack at TI2V-5B width, L = 520, two timesteps, with outlier residual channels (x300),
    attention logits of sigma ~ 8, modulation gates x10 and a prompt with a few rows 30x larger than the rest, against the CPU oracle
    and its no-rounding truth run. The HIP path must stay as close to the truth as the reference arithmetic does (ratio <= 1.02) in
    this regime too; inside-fraction and maximum error are recorded (profiles/r03_parity_margins.json)."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    cfg = dict(wan_dit.TI2V_5B_CFG, num_layers=3)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(29)
    sd = _trained_regime_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, cfg)
    m.load_state_dict(sd)
    grid = (4, 10, 13)
    Lt = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(37)
    x = torch.randn(48, grid[0], 2 * grid[1], 2 * grid[2], generator=g)
    c0 = torch.randn(77, cfg["text_dim"], generator=g) * 0.1
    c0[[3, 40, 76]] *= 30.0                                           # a few dominant prompt tokens
    ctx = [c0]
    t = torch.full((1, Lt), 812.0)
    t[0, :grid[1] * grid[2]] = 0.0
    hidden = []
    for blk in m.blocks:
        def run(xs, *a, _orig=blk._run, **kw):
            _orig(xs, *a, **kw)
            hidden.append(xs.clone())
        blk._run = run
    with torch.no_grad():
        out = m([x.to(DEV)], t.to(DEV), [c.to(DEV) for c in ctx], Lt)[0]
        ref, ref_h, _ = wan_dit.dit_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
        tru, tru_h, _ = _truth_forward(sd, cfg, [x], t, ctx, Lt, return_hidden=True)
    # the regime is what it claims to be: outlier channels dominate the stream, attention rows are peaked
    h1 = tru_h[0][0].float()
    chan = h1.abs().mean(0)
    assert chan.max() > 20 * chan.median(), "no outlier channels in the residual stream"
    for depth in (1, 3):
        assert_model_close(hidden[depth - 1], ref_h[depth - 1][0], tru_h[depth - 1][0], frac=STRESS_GATE[depth][0],
                           max_rel=STRESS_GATE[depth][1], truth_ratio=1.02, name=f"trained-weight regime, residual stream after block {depth}")
    assert_model_close(out, ref[0], tru[0], frac=STRESS_GATE["out"][0], max_rel=STRESS_GATE["out"][1], truth_ratio=1.02,
                       name="trained-weight regime, 3-block forward output")


# (min inside fraction, max |err| / range). Measured on MI355X (profiles/r03_parity_margins.json): in this regime the bf16 roundings of BOTH
# implementations are amplified (rms distance to the no-rounding truth 0.046 / 0.24 / 0.041 for the oracle, 0.9997 / 0.9952 / 0.9954 of
# that for the HIP path), so only 21 % / 3.6 % / 4.3 % of the elements agree to rtol 1e-3 / atol 1e-4 and the gate that carries the test
# is the truth ratio (<= 1.02); max error 4.4e-3 / 1.5e-2 / 2.1e-2 of the range, gates = x 1.2; the inside fractions get non-zero floors
# (round-3 verdict: a gate of 0.0 asserts nothing): 0.15 / 0.02 / 0.02 against the measured 0.209 / 0.036 / 0.043.
STRESS_GATE = {1: (0.15, 5.3e-3), 3: (0.02, 1.85e-2), "out": (0.02, 2.6e-2)}


def test_vae_heavy_tailed_input_stress_vs_oracle():
    """The VAE arithmetic on heavy-tailed activations (log-normal magnitudes plus a few x100 outliers in the latent, as trained latents
    and mid-network activations have, instead of unit gaussians): decode and encode of the small full-structure VAE against the fp32
    CPU oracle and an fp64 run of the same oracle. Both f32-grade modes must stay within a small multiple of the CPU's own fp32
    error against fp64 (rms ratio <= 3: measured 2.0 - the MFMA sums K = 27 C products in another order than the CPU's convolution -
    with a floor of 2e-6 of the output scale) and inside rtol 1e-3 / atol 1e-4 x the output scale."""
    from oracle import wan_vae
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = torch.Generator().manual_seed(53)
    z = torch.randn(48, 3, 6, 8, generator=g) * torch.exp(1.2 * torch.randn(48, 3, 6, 8, generator=g))
    z.view(-1)[torch.randint(0, z.numel(), (12,), generator=g)] *= 100.0
    vid = torch.tanh(torch.randn(3, 9, 48, 64, generator=g) * torch.exp(1.5 * torch.randn(3, 9, 48, 64, generator=g)))
    cfg = wan_vae.SMALL_CFG
    vae0 = Wan2_2_VAE(c_dim=cfg["dim"], dec_dim=cfg["dec_dim"], device=DEV, seed=3, precision="fp32")
    sd = {k: v.detach().cpu() for k, v in vae0.model.state_dict().items()}
    ora = wan_vae.WanVAE(sd, cfg)
    ora64 = wan_vae.WanVAE({k: v.double() for k, v in sd.items()}, cfg)
    with torch.no_grad():
        ref_d, ref_e = wan_vae.vae_decode(ora, [z])[0], wan_vae.vae_encode(ora, [vid])[0]
        tru_d = wan_vae.vae_decode(ora64, [z.double()], scale=wan_vae.scale_tensors(torch.float64))[0]
        tru_e = wan_vae.vae_encode(ora64, [vid.double()], scale=wan_vae.scale_tensors(torch.float64))[0]
    for prec in ("fp32", "bf16x6", "f16x3"):
        vae = vae0 if prec == "fp32" else Wan2_2_VAE(c_dim=cfg["dim"], dec_dim=cfg["dec_dim"], device=DEV, seed=3, precision=prec)
        with torch.no_grad():
            got_d, got_e = vae.decode([z.to(DEV)])[0].cpu(), vae.encode([vid.to(DEV)])[0].cpu()
        for name, got, ref, tru in (("decode", got_d, ref_d, tru_d), ("encode", got_e, ref_e, tru_e)):
            scale = float(tru.abs().max())
            e_hip = float((got.double() - tru).pow(2).mean().sqrt())
            e_ora = float((ref.double() - tru).pow(2).mean().sqrt())
            record_margin(f"VAE heavy-tailed {name} {prec}", rms_vs_fp64_hip=e_hip, rms_vs_fp64_oracle=e_ora, out_absmax=scale,
                          max_abs_err_vs_oracle=float((got - ref).abs().max()))
            assert torch.isfinite(got).all()
            assert e_hip <= 3.0 * e_ora + 2e-6 * scale, f"{name} {prec}: rms vs fp64 {e_hip:.3e}, the CPU fp32 oracle's own {e_ora:.3e}"
            assert ((got - ref).abs() <= 1e-4 * max(scale, 1.0) + 1e-3 * ref.abs()).all(), f"{name} {prec}"


# (min fraction inside rtol 1e-3 / atol 1e-4, max |err| / range). Measured on MI355X (profiles/r02_parity_margins.json): inside
# 94.8 / 87.6 / 75.4 / 60.5 % after 1 / 2 / 4 / 8 blocks and 41 % at the head output, max error 2.4-2.8e-3 of the range, relative
# rms vs the oracle 5.0e-4 x sqrt(depth) (a random walk of bf16 rounding flips), rms-vs-truth ratio 0.9999-1.0017 at every depth.
# Gates = 1.5 x the measured outside fraction / max error.
DEPTH_GATE = {1: (0.93, 2.9e-3), 2: (0.85, 3.0e-3), 4: (0.70, 3.0e-3), 8: (0.52, 4.2e-3), "out": (0.34, 1.8e-3)}      # measured x 1.2 (round 4)


# measured on MI355X (profiles/r02_parity_margins.json, r03_parity_margins.json) x 1.2 (inside fraction / 1.2; 1.2 x the larger max error
# of the two rounds): (latent shape, tokens, blocks, min inside fraction, max |err| / range). "default" = UniVid's own default workload,
# 121 frames 704 x 1280 (inference.py:48-50), first measured in round 4.
EAGER_SHAPES = {"config2": ((48, 13, 30, 52), 5070, 2, 0.19, 3.5e-3), "bench": ((48, 13, 44, 80), 11440, 2, 0.19, 3.7e-3),
                "bench30": ((48, 13, 44, 80), 11440, 30, 0.16, 5.6e-3), "default": ((48, 31, 44, 80), 27280, 2, 0.19, 3.5e-3)}      # default: measured 0.2333 / 2.91e-3 (round 4)


@pytest.mark.parametrize("which", ["config2", "bench", "bench30", "default"])
def test_real_shapes_vs_eager_oracle(which):
    """BASELINE config 2 at its REAL shape (49 frames 480x832 -> latent [48,13,30,52], L = 5 070) and the BENCH shape
    (49 frames 704x1280 -> [48,13,44,80], L = 11 440) at TI2V-5B width with two blocks, and the WHOLE 30-block TI2V-5B model at
    the bench shape ("bench30": the full configuration bench.py times), and UniVid's OWN DEFAULT workload ("default": 121 frames
    704 x 1280, inference.py:48-50 -> latent [48,31,44,80], L = 27 280, two blocks), VALUE-checked on every element. The CPU oracle
    would need minutes per block here, so the checker is the ORACLE TEXT executed by torch-ROCm eager on the same GPU
    (rocBLAS/hipBLASLt + SDPA kernels: the reference's own eager path is exactly this kind of second implementation), once as
    written (bf16 rounding points) and once with every rounding removed (truth). Plus the size-independent properties: padding
    invariance, stacked == sequential, determinism."""
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    shape, Lt, layers, frac, max_rel = EAGER_SHAPES[which]
    cfg = dict(wan_dit.TI2V_5B_CFG, num_layers=layers)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(41)
    sd = {k: v.detach() for k, v in m.state_dict().items()}          # on the GPU: the checker runs there too
    g = torch.Generator(device=DEV).manual_seed(42)
    x = torch.randn(*shape, device=DEV, generator=g)
    ctx = [torch.randn(77, cfg["text_dim"], device=DEV, generator=g) * 0.1]
    ctx_null = [torch.randn(12, cfg["text_dim"], device=DEV, generator=g) * 0.1]
    frame = (shape[2] // 2) * (shape[3] // 2)
    assert Lt == shape[1] * frame
    t = torch.full((1, Lt), 982.0, device=DEV)
    t[0, :frame] = 0.0
    with torch.no_grad():
        out = m([x], t, ctx, Lt)[0]
        again = m([x], t, ctx, Lt)[0]
        padded = m([x], torch.cat([t, t.new_full((1, 50), 982.0)], 1), ctx, Lt + 50)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx[0], ctx_null[0]], Lt)
        unc = m([x], t, ctx_null, Lt)[0]
        ref = wan_dit.dit_forward(sd, cfg, [x], t, ctx, Lt)[0]
        tru = _truth_forward(sd, cfg, [x], t, ctx, Lt)[0]
    assert out.shape == shape and torch.isfinite(out).all()
    assert torch.equal(out, again), "forward must be deterministic"
    assert torch.equal(out, padded), "sequence padding changed the valid tokens"
    assert torch.equal(pair[0], out) and torch.equal(pair[1], unc) and not torch.equal(out, unc)
    # measured: 2 blocks 23 % inside, max 2.9-3.0e-3 of the range, HIP rms-vs-truth 0.88x the eager run's own; 30 blocks 19.6 %
    # inside, max 3.8e-3, ratio 0.94 (torch-ROCm's SDPA / GEMM kernels sit further from the unrounded result than the HIP kernels)
    assert_model_close(out, ref, tru, frac=frac, max_rel=max_rel, truth_ratio=1.05,
                       name=f"{which} shape {list(shape)} L={Lt}, {layers} blocks, vs eager oracle on GPU")


def test_config2_full_run_50_steps_vs_eager_oracle():
    """BASELINE config 2 IN FULL: the 30-block TI2V-5B model, 49-frame 480p latent [48,13,30,52] (L = 5 070), 50 UniPC flow
    steps, shift 5, CFG 5, prompt embeds of 77 / 12 rows - WanTI2V.denoise on HIP against the oracle's loop
    (oracle.sampler.denoise = textimage2video.py:356-394) executed by torch-ROCm eager on the same GPU. Per-step noise
    predictions and latents at steps 0 / 9 / 24 / 49: relative rms, recorded and gated at measured x 1.5."""
    from oracle import sampler, wan_dit
    from univid_amd.wan.model import WanModel
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    cfg = dict(wan_dit.TI2V_5B_CFG)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(0)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    g = torch.Generator(device=DEV).manual_seed(42)
    noise = torch.randn(48, 13, 30, 52, device=DEV, generator=g)
    ctx = [torch.randn(77, cfg["text_dim"], device=DEV, generator=g) * 0.1]
    ctx_null = [torch.randn(12, cfg["text_dim"], device=DEV, generator=g) * 0.1]
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    rec, rec_ref = [], []
    with torch.no_grad():
        final = pipe.denoise(noise, ctx, ctx_null, 50, 5.0, 5.0, record=rec)
        ref_final = sampler.denoise(sd, cfg, noise, ctx, ctx_null, 50, 5.0, 5.0, record=rec_ref)
    assert len(rec) == len(rec_ref) == 50 and torch.isfinite(final).all()
    meas = {}
    for i in (0, 9, 24, 49):
        meas[f"noise_pred_step{i}"] = _rel_rms(rec[i][0], rec_ref[i][0])
        meas[f"latent_step{i}"] = _rel_rms(rec[i][1], rec_ref[i][1])
    record_margin("config 2 full run: 30-block TI2V-5B, [48,13,30,52], 50 steps, rel rms vs eager oracle on GPU", **meas)
    for k, v in meas.items():
        assert v < (CONFIG2_RUN_GATE[0] if k.startswith("noise_pred") else CONFIG2_RUN_GATE[1]), f"{k}: rel rms {v:.3e}"
    assert torch.equal(final, rec[-1][1])


# (noise_pred, latent). Measured on MI355X (profiles/r02_parity_margins.json): noise_pred 1.4-1.6e-2 at every step (CFG's x5 on the
# 3.5e-3 difference between the two 30-block forwards), latents 8e-5 (step 0) -> 3.0e-3 (step 49). Gates = 1.5 x the largest.
CONFIG2_RUN_GATE = (2.0e-2, 3.6e-3)      # measured 1.63e-2 / 2.97e-3 (rounds 2 and 3) x 1.2


def test_full_model_i2v_and_text_weight_hook_vs_eager_oracle():
    """The two other loop variants on the FULL 30-block TI2V-5B model at config 2's shape, 8 UniPC steps each, against the
    oracle's loop on torch-ROCm eager: (a) i2v - first latent frame pinned to z, per-token timesteps {0, t} (textimage2video.py
    :548-601); (b) UniVid's dynamic text-weight hook through Wan22ContextWrapper - the per-forward counter, the per-layer
    bf16 context mask and the un-fused reference-signature cross-attention path at width 3072 (model_pipeline.py:1699-1886)."""
    import logging
    from oracle import sampler, wan_dit
    from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
    from univid_amd.wan.model import WanModel
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    cfg = dict(wan_dit.TI2V_5B_CFG)
    with torch.device(DEV):
        m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m = m.eval().requires_grad_(False)
    m.init_weights(0)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    g = torch.Generator(device=DEV).manual_seed(43)
    noise = torch.randn(48, 13, 30, 52, device=DEV, generator=g)
    z = torch.randn(48, 1, 30, 52, device=DEV, generator=g)
    ctx = [torch.randn(77, cfg["text_dim"], device=DEV, generator=g) * 0.1]
    ctx_null = [torch.randn(12, cfg["text_dim"], device=DEV, generator=g) * 0.1]
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    steps = 8
    with torch.no_grad():
        got = pipe.denoise(noise, ctx, ctx_null, steps, 5.0, 5.0, z=z)
        ref = sampler.denoise(sd, cfg, noise, ctx, ctx_null, steps, 5.0, 5.0, z=z)
    assert torch.equal(got[:, 0], z[:, 0]), "i2v must keep the first latent frame pinned to z"
    i2v = _rel_rms(got, ref)
    with torch.no_grad():
        plain_hip = pipe.denoise(noise, ctx, ctx_null, steps, 5.0, 5.0)
    ccfg = CrossAttentionConfig(total_sampling_steps=steps, text_weight_transition_ratio=0.5, use_dynamic_text_weight=True)
    wr = Wan22ContextWrapper(pipe, None, logging.getLogger("t"), ccfg)
    wr.set_bagel_context(torch.zeros(1, 4, 8))
    with torch.no_grad():
        hooked = wr.generate(input_prompt="", size=(832, 480), frame_num=49, shift=5.0, sampling_steps=steps, guide_scale=5.0,
                             prompt_embeds=ctx, negative_prompt_embeds=ctx_null, noise=noise, decode=False)
        ref_h = sampler.denoise(sd, cfg, noise, ctx, ctx_null, steps, 5.0, 5.0, text_weight_cfg=dict(total_steps=steps, ratio=0.5))
        plain = sampler.denoise(sd, cfg, noise, ctx, ctx_null, steps, 5.0, 5.0)
    wr.restore_original_methods()
    hook, effect, plain_hip_vs_hooked = _rel_rms(hooked, ref_h), _rel_rms(plain, ref_h), _rel_rms(plain_hip, ref_h)
    record_margin("full 30-block model, [48,13,30,52], 8 steps: i2v and text-weight hook, rel rms of the final latent vs eager oracle",
                  i2v=i2v, hook=hook, hook_effect_in_the_oracle=effect, plain_hip_vs_hooked_oracle=plain_hip_vs_hooked,
                  plain=_rel_rms(plain_hip, plain))
    assert i2v < FULL_VARIANT_GATE and hook < FULL_VARIANT_GATE, (i2v, hook)
    # the hook's effect on the result (9.8e-3 in the oracle at these random weights) is of the size of the CFG-amplified bf16 noise
    # between the two implementations (7.6e-3): the discriminating check is that the hooked HIP run is closer to the hooked oracle
    # than the un-hooked HIP run is (measured 7.64e-3 vs 9.81e-3)
    assert hook < 0.9 * plain_hip_vs_hooked, "the hooked HIP run must follow the hooked oracle, not the plain one"


# measured on MI355X (profiles/r02_parity_margins.json): i2v 7.5e-3, hook 7.6e-3 after 8 steps (CFG x5 on 3.5e-3 per forward); x 1.5
FULL_VARIANT_GATE = 9.2e-3      # x 1.2 (round 4)


def test_text_weight_hook_path_matches_oracle():
    """UniVid's per-layer context hook (model_pipeline.py:1742-1810, 1844-1886) through the product's wrapper."""
    import logging
    from oracle import sampler
    from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    ccfg = CrossAttentionConfig(total_sampling_steps=10, text_weight_transition_ratio=0.4, use_dynamic_text_weight=True)
    wr = Wan22ContextWrapper(pipe, None, logging.getLogger("t"), ccfg)
    assert len(wr.original_forward_methods) == cfg["num_layers"]
    wr.set_bagel_context(torch.zeros(1, 4, 8))
    with torch.no_grad():
        ref = sampler.denoise(sd, cfg, g["noise"], [g["ctx"]], [g["ctx_null"]], 3, 5.0, 5.0,
                              text_weight_cfg=dict(total_steps=10, ratio=0.4))
        plain = sampler.denoise(sd, cfg, g["noise"], [g["ctx"]], [g["ctx_null"]], 3, 5.0, 5.0)
        got = wr.generate(input_prompt="", size=(256, 256), frame_num=13, shift=5.0, sampling_steps=3, guide_scale=5.0,
                          prompt_embeds=[g["ctx"]], negative_prompt_embeds=[g["ctx_null"]], noise=g["noise"].to(DEV), decode=False)
    assert "forward" not in m.__dict__ and not hasattr(wr, "sampling_step_counter")
    rel = lambda a, b: float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    assert rel(got.cpu(), ref) < 2e-2
    assert rel(got.cpu(), ref) < 0.5 * rel(plain, ref), "hooked HIP run must follow the hooked oracle, not the plain one"
    wr.restore_original_methods()
    assert all("forward" not in b.cross_attn.__dict__ for b in m.blocks)


def test_checkpoint_directory_written_independently_loads_and_runs(tmp_path):
    """SURVEY 8(f) rank 1, the wire formats: a checkpoint DIRECTORY whose files are built here with plain json / safetensors /
    torch.save calls (not with the product's writer) in the layouts the reference reads - diffusers `config.json` + three
    safetensors shards + index for the DiT (textimage2video.py:103), a `Wan2.2_VAE.pth` state dict (vae2_2.py:877-883), a T5
    `.pth` state dict (t5.py:496) - is loaded through WanModel.from_pretrained / WanTI2V(checkpoint_dir=...) and must reproduce
    the reference-generated goldens on the HIP path."""
    import json
    from safetensors.torch import save_file
    from oracle import t5 as ot5
    from oracle import wan_dit, wan_vae
    from univid_amd.wan.model import WanModel
    from univid_amd.wan.t5 import T5EncoderModel
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("dit_tiny")
    cfg = wan_dit.TINY_CFG
    sd = wan_dit.make_state_dict(cfg, g["seed"])
    d = tmp_path / "Wan2.2-TI2V-tiny"
    d.mkdir()
    # --- DiT: what diffusers' save_pretrained leaves behind (extra bookkeeping keys included)
    json.dump({"_class_name": "WanModel", "_diffusers_version": "0.35.1", "model_type": "ti2v", "patch_size": [1, 2, 2],
               "text_len": cfg["text_len"], "in_dim": 48, "dim": cfg["dim"], "ffn_dim": cfg["ffn_dim"], "freq_dim": 256,
               "text_dim": cfg["text_dim"], "out_dim": 48, "num_heads": cfg["num_heads"], "num_layers": cfg["num_layers"],
               "window_size": [-1, -1], "qk_norm": True, "cross_attn_norm": True, "eps": 1e-6}, open(d / "config.json", "w"))
    names = sorted(sd)
    cuts = [0, len(names) // 3, 2 * len(names) // 3, len(names)]
    weight_map = {}
    for i in range(3):
        fn = f"diffusion_pytorch_model-{i + 1:05d}-of-00003.safetensors"
        save_file({k: sd[k].contiguous() for k in names[cuts[i]:cuts[i + 1]]}, str(d / fn), metadata={"format": "pt"})
        weight_map.update({k: fn for k in names[cuts[i]:cuts[i + 1]]})
    json.dump({"metadata": {"total_size": sum(v.numel() * 4 for v in sd.values())}, "weight_map": weight_map},
              open(d / "diffusion_pytorch_model.safetensors.index.json", "w"))
    # --- VAE: a plain state dict (width-reduced topology of the golden fixture)
    gv = load_golden("vae_small")
    torch.save(wan_vae.make_state_dict(wan_vae.SMALL_CFG, gv["seed"]), str(d / "Wan2.2_VAE.pth"))
    # --- T5: a plain state dict + a tokenizer directory (tiny word-level vocabulary)
    gt = load_golden("t5_tiny")
    tcfg = ot5.TINY_CFG
    torch.save(ot5.make_state_dict(tcfg, int(gt["seed"])), str(d / "models_t5_tiny.pth"))

    m = WanModel.from_pretrained(str(d)).to(DEV)
    assert m.num_layers == cfg["num_layers"] and m.patch_size == (1, 2, 2)
    with torch.no_grad():
        one = m([g["x"].to(DEV)], g["t_one"].to(DEV), [g["ctx"].to(DEV)], 256)[0]
    assert_model_close(one, g["out_one"], name="DiT from an independently written sharded checkpoint")

    class TinyCfg(TI2VConfig):
        text_len = 48
        vae_kwargs = dict(c_dim=32, dec_dim=32)
        t5_checkpoint = "models_t5_tiny.pth"
        t5_tokenizer = "no-such-tokenizer-dir"           # absent: the text encoder stays injectable
    pipe = WanTI2V(TinyCfg, checkpoint_dir=str(d), device=DEV)
    assert pipe.vae is not None and pipe.text_encoder is None
    with torch.no_grad():
        two = pipe.model([g["x"].to(DEV)], g["t_two"].to(DEV), [g["ctx"].to(DEV)], 256)[0]
        dec = pipe.vae.decode([gv["dec_in_0"].to(DEV)])[0]
        enc = pipe.vae.encode([gv["enc_in_0"].to(DEV)])[0]
    assert_model_close(two, g["out_two"], name="DiT through WanTI2V(checkpoint_dir=...)")
    assert_f32_close(dec, gv["dec_out_0"], name="VAE decode from Wan2.2_VAE.pth")
    assert_f32_close(enc, gv["enc_out_0"], name="VAE encode from Wan2.2_VAE.pth")
    # T5 .pth through the reference-style wrapper (t5.py:473-513) with the tiny architecture
    ids = torch.zeros(1, 48, dtype=torch.long)
    ids[0, :33] = gt["ids_33"]
    mask = (torch.arange(48) < 33).long().unsqueeze(0)
    enc_model = T5EncoderModel(text_len=48, device=DEV, checkpoint_path=str(d / "models_t5_tiny.pth"), tokenizer=lambda texts, **kw: (ids, mask),
                               encoder_kwargs=dict(vocab=tcfg["vocab_size"], dim=tcfg["dim"], dim_attn=tcfg["dim_attn"], dim_ffn=tcfg["dim_ffn"],
                                                   num_heads=tcfg["num_heads"], num_layers=tcfg["num_layers"], num_buckets=tcfg["num_buckets"]))
    out = enc_model(["a prompt"], DEV)[0].float().cpu()
    ref = gt["out_33"].float()
    assert out.shape == ref.shape and _rel_rms(out, ref) < 3e-3 and (out == ref).float().mean() > 0.8
    # a directory whose shards miss a parameter must be refused, not half-loaded
    (d / "diffusion_pytorch_model-00003-of-00003.safetensors").unlink()
    save_file({k: sd[k].contiguous() for k in names[cuts[2]:cuts[3] - 1]}, str(d / "diffusion_pytorch_model-00003-of-00003.safetensors"))
    with pytest.raises(RuntimeError, match="does not match"):
        WanModel.from_pretrained(str(d))


def _write_adapter(path, factors, r, alpha, with_adapter_name=False, **cfg_over):
    """A PEFT adapter directory built by hand (adapter_config.json + adapter_model.safetensors with PEFT's key names), not by
    anything in univid_amd."""
    import json
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    cfg = dict(peft_type="LORA", r=r, lora_alpha=alpha, lora_dropout=0.0, bias="none", use_rslora=False, use_dora=False,
               fan_in_fan_out=False, target_modules=sorted(factors), task_type="FEATURE_EXTRACTION", inference_mode=True)
    cfg.update(cfg_over)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    mid = ".default" if with_adapter_name else ""
    t = {}
    for name, (a, b) in factors.items():
        t[f"base_model.model.{name}.lora_A{mid}.weight"] = a.contiguous()
        t[f"base_model.model.{name}.lora_B{mid}.weight"] = b.contiguous()
    save_file(t, os.path.join(path, "adapter_model.safetensors"))


def _lora_factors(cfg, names, r, seed, b_std=0.05):
    g = torch.Generator().manual_seed(seed)
    shapes = {"ffn.0": (cfg["ffn_dim"], cfg["dim"]), "ffn.2": (cfg["dim"], cfg["ffn_dim"])}
    out = {}
    for n in names:
        o, i = next((v for k, v in shapes.items() if n.endswith(k)), (cfg["dim"], cfg["dim"]))
        # lora_A ~ kaiming-uniform-like, lora_B as after training (PEFT starts it at zero): large enough that the adapter
        # moves the output far beyond the bf16 noise floor
        out[n] = (torch.randn(r, i, generator=g) / math.sqrt(i), torch.randn(o, r, generator=g) * b_std)
    return out


def _sd_with_adapter(sd, factors, scaling):
    sd = dict(sd)
    for n, (a, b) in factors.items():
        sd[n + ".lora_A.weight"], sd[n + ".lora_B.weight"], sd[n + ".lora_scaling"] = a, b, scaling
    return sd


def test_lora_adapter_directory_tiny_model_vs_unmerged_oracle(tmp_path):
    """inference.py --use_lora (reference inference.py:198-264 -> LoRAManager.load_lora_weights, model_pipeline.py:724-750): a PEFT
    adapter directory written by hand is loaded through `pipeline.lora_manager.load_lora_weights(dir, pipeline.dit_model)`, the HIP
    forward with the adapter folded in is compared with the oracle running the adapter UN-MERGED (PEFT's lora.Linear arithmetic
    restated in oracle/lora.py), and unloading restores the base model bit for bit."""
    from oracle import wan_dit
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    names = [f"blocks.{i}.{a}.{p}" for i in range(2) for a in ("cross_attn", "self_attn") for p in "qkvo"] + ["blocks.1.ffn.0", "blocks.0.ffn.2"]
    r, alpha = 8, 16
    factors = _lora_factors(cfg, names, r, 3, b_std=0.2)
    _write_adapter(str(tmp_path / "best"), factors, r, alpha, with_adapter_name=True)
    pipe = CrossAttentionFusionPipeline(CrossAttentionConfig(use_lora=True), wan_pipeline=WanTI2V(TI2VConfig, model=m, device=DEV))
    Lt = 256
    args = ([g["x"].to(DEV)], g["t_one"].to(DEV), [g["ctx"].to(DEV)], Lt)
    with torch.no_grad():
        base = pipe.dit_model(*args)[0]
        pipe.lora_manager.load_lora_weights(str(tmp_path / "best"), pipe.dit_model)
        got = pipe.dit_model(*args)[0]
        sd_l = _sd_with_adapter(sd, factors, alpha / r)
        ref = wan_dit.dit_forward(sd_l, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
        truth = _truth_forward(sd_l, cfg, [g["x"]], g["t_one"], [g["ctx"]], Lt)[0]
    effect = _rel_rms(ref, g["out_one"])
    assert effect > 0.05, f"the test adapter must move the output well above the bf16 noise floor (moved it by {effect:.3f})"
    # Merged and un-merged projections round differently (one bf16 rounding of W + dW against separate roundings of the two
    # branches), and this adapter is deliberately large: measured 63 % inside, max 1.2e-3 of the range - and the merged HIP result
    # is as close to the unrounded truth as PEFT's un-merged arithmetic is (rms ratio 0.985), which is the gate that matters.
    assert_model_close(got, ref, truth, frac=0.55, max_rel=1.5e-3, truth_ratio=1.05, name="tiny DiT + LoRA (merged on HIP vs un-merged oracle)")
    # the adapter's EFFECT is reproduced, not just the base model: (adapted - base) on HIP vs on the oracle
    d_hip, d_ref = (got - base).cpu(), ref - g["out_one"]
    rel = float((d_hip - d_ref).pow(2).mean().sqrt() / d_ref.pow(2).mean().sqrt())
    record_margin("tiny DiT + LoRA: error of the adapter's effect (rel rms)", effect_rel_rms=rel, effect_size=effect)
    assert rel < 1.2e-2, f"adapter effect off by {rel:.3e}"          # measured 7.6e-3 for an effect of 15 % of the output
    st = pipe.lora_manager.get_statistics()
    assert st["lora_modules"] == len(names) and st["module_breakdown"]["cross_attention"] == 8 and st["lora_config"]["rank"] == r
    with pytest.raises(RuntimeError):
        pipe.lora_manager.load_lora_weights(str(tmp_path / "best"), pipe.dit_model)       # already merged
    with torch.no_grad():
        pipe.lora_manager.unload()
        assert torch.equal(pipe.dit_model(*args)[0], base), "unload() must restore the base model bit for bit"


def test_lora_adapter_ti2v5b_width_block_vs_unmerged_oracle(tmp_path):
    """The same at the production width: one TI2V-5B block (L = 1014) with a rank-16 adapter on the cross- and self-attention
    projections and ffn.0 ('smart_wan_dit'-style targets, model_pipeline.py:501-506), merged on HIP vs un-merged in the oracle."""
    from oracle import wan_dit
    from univid_amd.lora import LoRAManager
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device, rope_params
    cfg = wan_dit.TI2V_5B_CFG
    dim, heads = cfg["dim"], cfg["num_heads"]
    sd = wan_dit.make_state_dict(dict(cfg, num_layers=1), 11)
    sd = {k: v for k, v in sd.items() if k.startswith("blocks.0.")}
    names = [f"blocks.0.{a}.{p}" for a in ("cross_attn", "self_attn") for p in "qkvo"] + ["blocks.0.ffn.0"]
    r, alpha = 16, 32
    factors = _lora_factors(cfg, names, r, 4)
    _write_adapter(str(tmp_path / "ad"), factors, r, alpha)
    gen = torch.Generator().manual_seed(23)
    Lt, grid = 1014, (3, 13, 26)
    x = torch.randn(1, Lt, dim, generator=gen)
    e_rows = torch.randn(2, 6, dim, generator=gen) * 0.3
    tid = (torch.arange(Lt) >= 338).long()
    ctx = (torch.randn(1, 512, dim, generator=gen) * 0.5).to(BF16)
    e0 = e_rows[tid].unsqueeze(0)
    freqs = wan_dit.rope_table(dim // heads)
    sd_l = _sd_with_adapter(sd, factors, alpha / r)
    from oracle import lora as ora_lora
    with torch.no_grad():
        ref = wan_dit.block_forward(sd_l, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        ref_base = wan_dit.block_forward(sd, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        wan_dit.BF16 = ora_lora.BF16 = torch.float32          # the unrounded truth of the adapted block
        try:
            truth = wan_dit.block_forward(sd_l, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        finally:
            wan_dit.BF16 = ora_lora.BF16 = BF16
    holder = torch.nn.Module()
    holder.blocks = torch.nn.ModuleList([WanAttentionBlock(dim, cfg["ffn_dim"], heads, cross_attn_norm=True, eps=1e-6)])
    holder.load_state_dict(sd)
    holder = holder.to(DEV).eval()
    LoRAManager().load_lora_weights(str(tmp_path / "ad"), holder)
    blk = holder.blocks[0]
    xs = x[0].to(DEV).contiguous()
    with torch.no_grad():
        blk.prepare()
        blk._run(xs, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), grid, _freqs_device(freqs, torch.device(DEV)),
                 ctx[0].to(DEV), first_block=False)
    effect = _rel_rms(ref[0] - x[0], ref_base[0] - x[0])
    assert effect > 0.05, f"adapter effect on the block's update only {effect:.3f}"
    # measured: 60 % inside, max 2.7e-3 of the range (the un-adapted block: 84.7 %, 1.7e-3)
    assert_model_close(xs, ref[0], truth[0], frac=0.51, max_rel=3.2e-3, truth_ratio=1.05, name="TI2V-5B block + LoRA r16 (merged on HIP vs un-merged oracle)")


def test_model_errors_are_loud():
    from univid_amd._lib import UnividHipError
    cfg, sd, m = _tiny_model(0)
    x = torch.randn(48, 2, 4, 4, device=DEV)
    with pytest.raises(AssertionError):
        m([x], torch.tensor([5.0], device=DEV), [torch.randn(3, 64, device=DEV)], 2)           # seq_len too small (model.py:453)
    with pytest.raises(ValueError):
        m([x], torch.tensor([5.0], device=DEV), [torch.randn(40, 64, device=DEV)], 8)          # context longer than text_len


# ---------------------------------------------------------------------------------------------------------------
# VAE
# ---------------------------------------------------------------------------------------------------------------
def _small_vae(seed):
    from oracle import wan_vae
    from univid_amd.wan.vae2_2 import WanVAE_
    cfg = wan_vae.SMALL_CFG
    m = WanVAE_(dim=cfg["dim"], dec_dim=cfg["dec_dim"], z_dim=cfg["z_dim"], dim_mult=cfg["dim_mult"],
                temperal_downsample=cfg["temperal_downsample"])
    m.load_state_dict(wan_vae.make_state_dict(cfg, seed))
    return m.to(DEV).eval(), [s.to(DEV) for s in wan_vae.scale_tensors()]


def test_vae_encode_decode_vs_golden():
    g = load_golden("vae_small")
    m, scale = _small_vae(g["seed"])
    for i in range(3):
        with torch.no_grad():
            z = m.encode(g[f"enc_in_{i}"].unsqueeze(0).to(DEV), scale)[0]
            v = m.decode(g[f"dec_in_{i}"].unsqueeze(0).to(DEV), scale)[0]
        assert_f32_close(z, g[f"enc_out_{i}"], name=f"encode {i}")
        assert_f32_close(v, g[f"dec_out_{i}"], name=f"decode {i}")
        assert v.abs().max() <= 1.0


def test_vae_list_api_and_state_is_reset_between_calls():
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = load_golden("vae_small")
    vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"])
    # non-list input: logged, answered with None (the reference's `except TypeError`, vae2_2.py:1024-1051)
    assert vae.decode(g["dec_in_0"]) is None and vae.encode(g["enc_in_0"]) is None
    with torch.no_grad():
        a = vae.decode([g["dec_in_0"].to(DEV), g["dec_in_1"].to(DEV)])
        b = vae.decode([g["dec_in_1"].to(DEV)])
        e = vae.encode([g["enc_in_0"].to(DEV)])
    assert torch.equal(a[1], b[0]), "feature caches must be cleared between clips (clear_cache, vae2_2.py:813,838)"
    assert_f32_close(a[0], g["dec_out_0"])
    assert_f32_close(e[0], g["enc_out_0"])


def test_vae_workspace_arena_repeat_calls_allocate_nothing_on_the_device():
    """WanVAE_._arena: a decode / encode draws everything but its result from a memory pool the VAE owns. After one call at a clip shape,
    repeat calls at that shape cause NO device allocation (torch's num_device_alloc = hipMalloc calls) - also after the rest of the
    process churned the shared pool and called empty_cache() in between - and give the same bits; a model without the arena
    (use_arena = False) gives the same bits too. Also: the result tensor is the caller's (it survives dropping the VAE)."""
    import gc
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=3)
    g = torch.Generator(device=DEV).manual_seed(1)
    z = torch.randn(48, 5, 6, 10, device=DEV, generator=g)
    with torch.no_grad():
        v0 = vae.decode([z])[0]
        e0 = vae.encode([v0.clamp(-1, 1)])[0]
        torch.cuda.synchronize()
        junk = [torch.empty(3 << 20, device=DEV) for _ in range(8)]           # churn in the shared pool
        del junk
        gc.collect()
        torch.cuda.empty_cache()
        vc = v0.clamp(-1, 1)
        n1 = torch.cuda.memory_stats(DEV)["num_device_alloc"]
        v1 = vae.decode([z])[0]
        e1 = vae.encode([vc])[0]
        torch.cuda.synchronize()
        n2 = torch.cuda.memory_stats(DEV)["num_device_alloc"]
    assert torch.equal(v0, v1) and torch.equal(e0, e1)
    # (the two RESULTS are the caller's tensors and come from the shared pool, which empty_cache() just emptied: at most one segment each)
    assert n2 - n1 <= 2, f"repeat VAE calls allocated on the device: {n2 - n1} hipMalloc(s) for two result tensors"
    plain = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=3)
    plain.model.use_arena = False
    with torch.no_grad():
        v2 = plain.decode([z])[0]
    assert torch.equal(v0, v2)
    del vae, plain
    gc.collect()
    torch.cuda.empty_cache()
    assert torch.isfinite(v1).all() and torch.equal(v1, v2)


def test_vae_out_of_memory_retry_releases_the_arena_and_gives_the_same_bits():
    """WanVAE_._with_pass_length with the arena ON (round-5 advisor finding: only stubs exercised it): a decode that runs out of memory at
    the configured pass length - simulated: the pass body raises torch.cuda.OutOfMemoryError from INSIDE the arena scope, after the
    engine has filled the pool, exactly where a real allocation failure surfaces - is retried at half the length; the engine and the pool
    of the failed pass are dropped once the handler has exited (the traceback no longer pins their blocks), so the memory the pool
    reserved really returns to the device before the retry allocates, and the result has the bits of an undisturbed decode."""
    import gc
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=3)
    g = torch.Generator(device=DEV).manual_seed(2)
    z = torch.randn(48, 5, 6, 10, device=DEV, generator=g)
    m = vae.model
    with torch.no_grad():
        ref = vae.decode([z])[0]
        torch.cuda.synchronize()
        pool0 = m._pool
        assert pool0 is not None and m._engine is not None
        orig, seen = m._decode, []

        def failing(G, zz, scale):
            seen.append(G)
            if len(seen) == 1:
                with m._arena():
                    ballast = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)     # lives in the arena, referenced by this frame only
                    raise torch.cuda.OutOfMemoryError("simulated: HIP out of memory")
            assert m._engine is None and m._pool is None, "the failed pass's engine and pool must be gone before the retry"
            return orig(G, zz, scale)
        m._decode = failing
        try:
            del pool0
            gc.collect()
            r0 = torch.cuda.memory_reserved(DEV)
            out = vae.decode([z])[0]
        finally:
            del m._decode
        torch.cuda.synchronize()
    assert seen == [4, 2], seen
    assert torch.equal(out, ref)
    assert m._pool is not None and torch.cuda.memory_reserved(DEV) <= r0 + (8 << 20), "the arena of the failed pass was not released"


def test_vae_pass_length_does_not_change_the_result():
    """Decoder passes of several latent frames / encoder passes of several 4-frame chunks (WanVAE_.frames_per_pass) against the
    reference's one-at-a-time streaming (vae2_2.py:797-806, 824-835): every layer is time-causal with a 2-frame cache, so the values
    must be IDENTICAL bit for bit - including pass lengths that do not divide the clip, every precision mode, and a second clip through the
    same object (caches cleared, shared scratch reused)."""
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = torch.Generator().manual_seed(12)
    z = torch.randn(48, 6, 2, 3, generator=g)                    # 6 latent frames -> 21 output frames
    vid = torch.tanh(torch.randn(3, 21, 32, 48, generator=g))    # 1 + 5 chunks of 4 frames
    z2 = torch.randn(48, 3, 3, 2, generator=g)
    for prec in ("fp32", "bf16x6", "f16x3", "bf16x3"):
        ref = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=3, precision=prec, frames_per_pass=1)
        with torch.no_grad():
            d1, e1, d1b = ref.decode([z.to(DEV)])[0], ref.encode([vid.to(DEV)])[0], ref.decode([z2.to(DEV)])[0]
        assert d1.shape == (3, 21, 32, 48) and e1.shape == (48, 6, 2, 3)
        for G in (2, 3, 4, 16):
            vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=3, precision=prec, frames_per_pass=G)
            with torch.no_grad():
                d, e, db = vae.decode([z.to(DEV)])[0], vae.encode([vid.to(DEV)])[0], vae.decode([z2.to(DEV)])[0]
            assert torch.equal(d, d1), f"{prec}: decode with {G} latent frames per pass differs from streaming"
            assert torch.equal(e, e1), f"{prec}: encode with {G} chunks per pass differs from streaming"
            assert torch.equal(db, d1b), f"{prec}: second clip (other shape) through the same object, G={G}"


def test_vae_bf16x3_precision_mode():
    """Opt-in split-bf16 (3-pass MFMA) convolutions: same function within the north star's rtol 1e-3 / atol 1e-4 on every
    element against the fp32 reference output (measured ~5e-5 max), results differ from the exact-fp32 mode."""
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = load_golden("vae_small")
    fast = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision="bf16x3")
    exact = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision="fp32")
    with pytest.raises(ValueError):
        Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, precision="fp16").decode([g["dec_in_1"].to(DEV)])
    for i in range(3):
        with torch.no_grad():
            v = fast.decode([g[f"dec_in_{i}"].to(DEV)])[0]
            z = fast.encode([g[f"enc_in_{i}"].to(DEV)])[0]
        assert_f32_close(v, g[f"dec_out_{i}"], name=f"bf16x3 decode {i}")
        assert_f32_close(z, g[f"enc_out_{i}"], name=f"bf16x3 encode {i}")
    with torch.no_grad():
        assert not torch.equal(fast.decode([g["dec_in_0"].to(DEV)])[0], exact.decode([g["dec_in_0"].to(DEV)])[0])


def test_vae_bf16x6_precision_mode_vs_golden():
    """precision='bf16x6' (f32-grade arithmetic on the bf16 matrix pipe): the small-VAE goldens at the same tolerance as fp32."""
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = load_golden("vae_small")
    vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision="bf16x6")
    exact = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision="fp32")
    for i in range(3):
        with torch.no_grad():
            v, z = vae.decode([g[f"dec_in_{i}"].to(DEV)])[0], vae.encode([g[f"enc_in_{i}"].to(DEV)])[0]
            v0, z0 = exact.decode([g[f"dec_in_{i}"].to(DEV)])[0], exact.encode([g[f"enc_in_{i}"].to(DEV)])[0]
        assert_f32_close(v, g[f"dec_out_{i}"], name=f"bf16x6 decode {i}")
        assert_f32_close(z, g[f"enc_out_{i}"], name=f"bf16x6 encode {i}")
        # and as close to the reference output as the exact-f32 mode is (both differ from it by accumulation order only)
        e6, e0 = (v.cpu() - g[f"dec_out_{i}"]).abs().max().item(), (v0.cpu() - g[f"dec_out_{i}"]).abs().max().item()
        assert e6 < 2.0 * e0 + 1e-6, (i, e6, e0)


def test_vae_f16x3_precision_mode_vs_golden():
    """precision='f16x3' (f32-grade in three fp16 MFMA passes for the convolutions behind an RMS_norm, bf16x6 for the others): the
    small-VAE goldens at the same tolerance as fp32, as close to the reference output as the exact-f32 mode is, and the range guard: a
    norm whose sqrt(C) max|gamma| bound exceeds fp16's range keeps its convolution on bf16x6 (finite output, same tolerance)."""
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = load_golden("vae_small")
    vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision="f16x3")
    exact = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision="fp32")
    for i in range(3):
        with torch.no_grad():
            v, z = vae.decode([g[f"dec_in_{i}"].to(DEV)])[0], vae.encode([g[f"enc_in_{i}"].to(DEV)])[0]
            v0, z0 = exact.decode([g[f"dec_in_{i}"].to(DEV)])[0], exact.encode([g[f"enc_in_{i}"].to(DEV)])[0]
        assert_f32_close(v, g[f"dec_out_{i}"], name=f"f16x3 decode {i}")
        assert_f32_close(z, g[f"enc_out_{i}"], name=f"f16x3 encode {i}")
        e3, e0 = (v.cpu() - g[f"dec_out_{i}"]).abs().max().item(), (v0.cpu() - g[f"dec_out_{i}"]).abs().max().item()
        assert e3 < 2.0 * e0 + 1e-6, (i, e3, e0)
    eng = vae.model._eng()
    used = sorted(set(eng._fmt.values()))
    assert used == [2], f"every RMS_norm of the small VAE is inside fp16's range: {used}"
    # a huge gamma (x 1e5): sqrt(C) max|gamma| is out of fp16's range -> THAT norm keeps f32 rows and its convolution runs as bf16x6 (exact
    # splitting, no range limit); checked against the exact-f32 mode on the same modified weights (the activations behind it reach ~1e5)
    pair = {}
    for prec in ("f16x3", "fp32"):
        big = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision=prec)
        with torch.no_grad():
            big.model.decoder.middle[0].residual[0].gamma.mul_(1e5)
            big.model.decoder.middle[0].residual[2].weight.mul_(1e-5)
        big.model.invalidate()
        with torch.no_grad():
            pair[prec] = big.decode([g["dec_in_1"].to(DEV)])[0]
        if prec == "f16x3":
            fmts = list(big.model._eng()._fmt.values())
            assert fmts.count(0) == 1 and set(fmts) == {0, 2}, fmts
    assert torch.isfinite(pair["f16x3"]).all()
    assert_f32_close(pair["f16x3"], pair["fp32"], name="f16x3 with one norm outside fp16's range vs exact f32")


def test_vae_split_f16_per_tensor_scale():
    """uv_vae_split_f16 (fp16 pieces of a RAW feature map for uv_conv3d_f16x3: Resample's convolutions read un-normed residual-stream rows):
    for ordinary magnitudes the scale is 1 and the bytes equal the unscaled split; with an element of 3e6 - beyond fp16's range - the
    device picks the power of two that brings the maximum into [2^14, 2^15), reports its inverse, and the convolution fed with both is
    finite and as close to F.conv3d as the exact kernel (relative to the output's scale)."""
    import torch.nn.functional as F
    from univid_amd import _lib
    g = torch.Generator().manual_seed(31)
    x = torch.randn(1, 64, 2, 9, 11, generator=g)
    w, b = torch.randn(128, 64, 1, 3, 3, generator=g) * 0.05, torch.randn(128, generator=g)
    wp = w.permute(0, 2, 3, 4, 1).reshape(128, -1).contiguous().to(DEV)
    wsp, wscale = _split_f16_weights(wp)
    for big in (False, True):
        xx = x.clone()
        if big:
            xx[0, 5, 1, 4, 6] = 3.0e6
            xx[0, 9, 0, 0, 0] = -7.0e4
        x_cl = xx[0].permute(1, 2, 3, 0).contiguous().to(DEV)
        xs, sc = torch.empty_like(x_cl), torch.full((2,), 7.0, device=DEV)
        _lib.call("uv_vae_split_f16", _lib.ptr(x_cl), 64, _lib.ptr(xs), 64, x_cl.numel() // 64, 64, _lib.ptr(sc), _lib.stream_ptr())
        inv = float(sc[0])
        # rows with a larger leading dimension (the strided form of the kernel) must give the same pieces and the same scale
        wide_in, wide_out, sc2 = torch.full((x_cl.numel() // 64, 96), 5.0, device=DEV), torch.zeros(x_cl.numel() // 64, 96, device=DEV), torch.zeros(2, device=DEV)
        wide_in[:, :64] = x_cl.view(-1, 64)
        _lib.call("uv_vae_split_f16", _lib.ptr(wide_in), 96, _lib.ptr(wide_out), 96, x_cl.numel() // 64, 64, _lib.ptr(sc2), _lib.stream_ptr())
        assert torch.equal(wide_out[:, :64].contiguous().view(torch.int32), xs.view(-1, 64).view(torch.int32)) and torch.equal(sc2, sc)
        assert float(wide_out[:, 64:].abs().max()) == 0.0
        if not big:
            assert inv == 1.0 and torch.equal(xs.view(torch.int32), _split_f16_acts(x_cl).view(torch.int32))
        else:
            assert inv == 2.0 ** 7 and float(sc[1]) == 3.0e6, (inv, float(sc[1]))       # 3e6 / 128 = 23 437 in [2^14, 2^15)
            assert torch.isfinite(xs.view(torch.float16).float()).all()
        out = torch.empty(2, 9, 11, 128, device=DEV)
        _lib.call("uv_conv3d_f16x3", _lib.ptr(xs), 64, 2, 9, 11, _lib.ptr(wsp), _lib.ptr(b.to(DEV)), _lib.ptr(out), 128, 2, 9, 11, 64, 128,
                  1, 3, 3, 1, 1, 1, 0, 1, 1, 0, 0, None, 0, wscale, _lib.ptr(sc), _lib.stream_ptr())
        ref = F.conv3d(F.pad(xx.double(), (1, 1, 1, 1)), w.double(), b.double())[0].permute(1, 2, 3, 0)
        err = (out.cpu().double() - ref).abs().max().item()
        assert torch.isfinite(out).all() and err <= 2e-6 * float(ref.abs().max()) + 1e-5, (big, err, float(ref.abs().max()))


def test_vae_phase_upsample_equals_the_3x3_form():
    """The fast modes run Resample's "nearest-exact 2x + 3x3 convolution" as four 2x2 output-phase convolutions with pre-summed weights
    (2.25 x fewer multiply-adds, _ConvOp.phases): the decode must agree with the 3x3 form of the same mode to f32 rounding noise, incl.
    the first chunk ("Rep") and the time-upsampling stages; precision='fp32' never uses it."""
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    g = load_golden("vae_small")
    for prec in ("bf16x6", "f16x3"):
        vae = Wan2_2_VAE(c_dim=32, dec_dim=32, device=DEV, seed=g["seed"], precision=prec)
        with torch.no_grad():
            a = vae.decode([g["dec_in_0"].to(DEV)])[0]
            assert vae.model._eng().phase_upsample
            vae.model._eng().phase_upsample = False
            b = vae.decode([g["dec_in_0"].to(DEV)])[0]
        assert not torch.equal(a, b) and (a - b).abs().max() <= 2e-5 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def test_vae_full_width_vs_oracle():
    """The production VAE widths (encoder 160..640, decoder 1024..256 channels, z = 48) on a small clip, fp32 mode and
    bf16x3 mode, against the CPU oracle run here."""
    from oracle import wan_vae
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    torch.set_num_threads(min(32, torch.get_num_threads()))
    cfg = wan_vae.FULL_CFG
    sd = wan_vae.make_state_dict(cfg, 2)
    ora = wan_vae.WanVAE(sd, cfg)
    g = torch.Generator().manual_seed(8)
    z = torch.randn(48, 2, 2, 3, generator=g)
    vid = torch.tanh(torch.randn(3, 5, 32, 48, generator=g))
    with torch.no_grad():
        ref_dec = wan_vae.vae_decode(ora, [z])[0]
        ref_enc = wan_vae.vae_encode(ora, [vid])[0]
    for prec in ("fp32", "bf16x6", "f16x3", "bf16x3"):
        vae = Wan2_2_VAE(device=DEV, precision=prec)
        vae.model.load_state_dict(sd)
        with torch.no_grad():
            assert_f32_close(vae.decode([z.to(DEV)])[0], ref_dec, name=f"full-width decode {prec}")
            assert_f32_close(vae.encode([vid.to(DEV)])[0], ref_enc, name=f"full-width encode {prec}")


@pytest.mark.parametrize("prec", ["fp32", "bf16x6", "f16x3"])
def test_vae_config4_full_resolution_frame_vs_cpu_oracle(prec):
    """BASELINE config 4 at its REAL spatial size, every element value-checked against the pinned CPU oracle: the full-width decoder
    on one latent frame [48, 1, 45, 80] -> one 720 x 1280 RGB frame (every decoder layer at its full 90x160 .. 720x1280 geometry: 57 600 /
    230 400 / 921 600 pixels per frame) and the full-width encoder on one 720 x 1280 frame -> [48, 1, 45, 80]; rtol 1e-3 / atol 1e-4 on
    EVERY element, exact-f32 MFMA mode and the f32-grade bf16x6 mode (vae2_2.py:783-839)."""
    from oracle import wan_vae
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    torch.set_num_threads(min(32, torch.get_num_threads()))
    cfg = wan_vae.FULL_CFG
    sd = wan_vae.make_state_dict(cfg, 2)
    ora = wan_vae.WanVAE(sd, cfg)
    g = torch.Generator().manual_seed(41)
    z = torch.randn(48, 1, 45, 80, generator=g)
    vid = torch.tanh(torch.randn(3, 1, 720, 1280, generator=g))
    with torch.no_grad():
        ref_dec = wan_vae.vae_decode(ora, [z])[0]
        ref_enc = wan_vae.vae_encode(ora, [vid])[0]
    assert ref_dec.shape == (3, 1, 720, 1280) and ref_enc.shape == (48, 1, 45, 80)
    vae = Wan2_2_VAE(device=DEV, precision=prec)
    vae.model.load_state_dict(sd)
    with torch.no_grad():
        assert_f32_close(vae.decode([z.to(DEV)])[0], ref_dec, name=f"720x1280 frame decode {prec}")
        assert_f32_close(vae.encode([vid.to(DEV)])[0], ref_enc, name=f"720x1280 frame encode {prec}")


def test_vae_config4_full_clip_encode_decode_properties():
    """BASELINE config 4 in full: the 49 x 720 x 1280 clip through the full-width encoder and the resulting [48, 13, 45, 80] latent
    through the decoder. The CPU oracle needs ~10 minutes per direction at this size, so the whole-clip checks are the
    size-independent properties: shapes, finiteness, bounded outputs, determinism, the FIRST frame of the whole-clip decode equal
    (bit for bit) to decoding the first latent frame alone - which test_vae_config4_full_resolution_frame_vs_cpu_oracle value-checks
    against the oracle - and time-causality: the first 13 frames do not depend on later latent frames. Pass-length independence is
    bit-exact at every size (test_vae_pass_length_does_not_change_the_result) and is re-checked here on the first 3 latent frames."""
    from oracle import wan_vae
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    sd = wan_vae.make_state_dict(wan_vae.FULL_CFG, 2)
    vae = Wan2_2_VAE(device=DEV, precision="fp32")
    vae.model.load_state_dict(sd)
    g = torch.Generator(device=DEV).manual_seed(43)
    vid = torch.tanh(torch.randn(3, 49, 720, 1280, generator=g, device=DEV))
    with torch.no_grad():
        z = vae.encode([vid])[0]
        assert z.shape == (48, 13, 45, 80) and torch.isfinite(z).all()
        z1 = vae.encode([vid[:, :1]])[0]
        assert torch.equal(z1, z[:, :1]), "causal encoder: the first latent frame must not depend on later frames"
        out = vae.decode([z])[0]
        assert out.shape == (3, 49, 720, 1280) and torch.isfinite(out).all()
        assert out.abs().max() <= 1.0, "decode clamps to [-1, 1] (vae2_2.py:1047)"
        first = vae.decode([z[:, :1]])[0]
        assert torch.equal(first, out[:, :1]), "first frame of the whole-clip decode != decoding the first latent frame alone"
        head = vae.decode([z[:, :4]])[0]
        assert torch.equal(head, out[:, :13]), "causal decoder: frames 0..12 must not depend on latent frames 4.."
        del out
        vae1 = Wan2_2_VAE(device=DEV, precision="fp32", frames_per_pass=1)
        vae1.model.load_state_dict(sd)
        assert torch.equal(vae1.decode([z[:, :3]])[0], head[:, :9]), "pass length 1 vs 4 at full resolution"


def _split6(wp):
    """uv_split_weights_bf16x6 of a [Cout, K] f32 weight matrix (+ a check that the three planes sum back to it exactly)."""
    from univid_amd import _lib
    out = torch.empty(wp.numel() * 3, dtype=BF16, device=wp.device)
    _lib.call("uv_split_weights_bf16x6", _lib.ptr(wp), _lib.ptr(out), wp.numel(), _lib.stream_ptr())
    pl = out.view(wp.shape[0], -1, 3, 32).float()
    assert torch.equal((pl[:, :, 0] + pl[:, :, 1]) + pl[:, :, 2], wp.view(wp.shape[0], -1, 32)), "w != p0 + p1 + p2"
    return out


def _split_f16_weights(wp):
    """uv_split_weights_f16x3 of a [Cout, K] f32 weight matrix with the engine's scale rule (max |w| * scale in [2^13, 2^14)) + a check
    that hi + lo reproduces w * scale to 2^-22 relative (of the row's largest weights: tiny weights have subnormal lo pieces)."""
    from univid_amd import _lib
    mx = float(wp.abs().max())
    scale = 2.0 ** (13 - math.floor(math.log2(mx)))
    out = torch.empty(wp.numel() * 2, dtype=torch.float16, device=wp.device)
    _lib.call("uv_split_weights_f16x3", _lib.ptr(wp), _lib.ptr(out), wp.numel(), scale, _lib.stream_ptr())
    pl = out.view(wp.shape[0], -1, 2, 32).double()
    back = (pl[:, :, 0] + pl[:, :, 1]) / scale
    assert ((back - wp.view(wp.shape[0], -1, 32).double()).abs() <= 2.0 ** -22 * wp.abs().double().view(wp.shape[0], -1, 32) + 2.0 ** -25 / scale).all(), "w != (hi + lo) / scale"
    return out, scale


def _split_f16_acts(x_cl):
    """[.., C] f32 (C % 32 == 0) -> the same bytes holding [C/32][32 hi | 32 lo] IEEE fp16 per pixel: what uv_vae_rms_silu(split_out=2) writes."""
    hi = x_cl.half()
    lo = (x_cl - hi.float()).half()
    C = x_cl.shape[-1]
    both = torch.stack((hi.view(*x_cl.shape[:-1], C // 32, 32), lo.view(*x_cl.shape[:-1], C // 32, 32)), dim=-2)   # [.., C/32, 2, 32]
    return both.reshape(*x_cl.shape[:-1], 2 * C).contiguous().view(torch.float32)                                 # [.., C] f32-sized


def _phase_weights(w, a, b):
    """[Cout, Cin, 1, 3, 3] -> the [Cout, Cin, 1, 2, 2] weights of output phase (a, b) of "nearest-exact 2x + 3x3 convolution": per output-row
    parity the three taps of a row collapse onto two source rows ({0} | {1, 2} and {0, 1} | {2}; columns alike), summed in fp64."""
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    wp = torch.zeros(w.shape[0], w.shape[1], 1, 2, 2, dtype=torch.float64)
    for i, dys in enumerate(rows[a]):
        for j, dxs in enumerate(rows[b]):
            for dy in dys:
                for dx in dxs:
                    wp[:, :, 0, i, j] += w[:, :, 0, dy, dx].double()
    return wp.float()


@pytest.mark.parametrize("entry", ["uv_conv3d_f32", "uv_conv3d_bf16x6", "uv_conv3d_f16x3"])
def test_conv3d_kernel_geometries(entry):
    """Every convolution geometry the VAE uses, against F.conv3d / F.conv2d: the exact-f32 MFMA kernel, the same kernel with
    the products on the bf16 matrix pipe by exact three-way operand splitting (same memory formats, same tolerance), and the f32-grade
    three-pass fp16 form on pre-split operands (uv_conv3d_f16x3; same tolerance)."""
    import torch.nn.functional as F
    from univid_amd import _lib
    g = torch.Generator().manual_seed(4)

    def run(x_cl, w, b, Tout, Hout, Wout, **kw):
        T, H, W, C = x_cl.shape
        co, ci, kt, kh, kw_ = w.shape
        wp = w.permute(0, 2, 3, 4, 1).reshape(co, -1).contiguous().to(DEV)
        extra = ()
        if entry == "uv_conv3d_bf16x6":
            wp = _split6(wp)
        elif entry == "uv_conv3d_f16x3":        # both operands as two fp16 pieces (activations pre-split, as uv_vae_rms_silu writes them)
            wp, scale = _split_f16_weights(wp)
            x_cl = _split_f16_acts(x_cl)
            extra = (scale, None)
        inter = kw.get("interleave", 0)
        out = torch.empty(Tout * (2 if inter else 1), Hout, Wout, co // (2 if inter else 1), device=DEV)
        _lib.call(entry, _lib.ptr(x_cl), C, T, H, W, _lib.ptr(wp), _lib.ptr(b.to(DEV)), _lib.ptr(out), out.shape[-1],
                  Tout, Hout, Wout, C, co, kt, kh, kw_, kw.get("st", 1), kw.get("sh", 1), kw.get("sw", 1), kw.get("t_off", 0),
                  kw.get("ph", 0), kw.get("pw", 0), kw.get("up", 0), inter, None, 0, *extra, _lib.stream_ptr())
        return out.cpu()

    x = torch.randn(1, 64, 5, 6, 7, generator=g)
    cl = lambda t: t[0].permute(1, 2, 3, 0).contiguous().to(DEV)
    w, b = torch.randn(96, 64, 3, 3, 3, generator=g) * 0.05, torch.randn(96, generator=g)
    ref = F.conv3d(F.pad(x, (1, 1, 1, 1, 2, 0)), w, b)                                     # causal 3x3x3
    got = run(cl(F.pad(x, (0, 0, 0, 0, 2, 0))), w, b, 5, 6, 7, ph=1, pw=1)
    assert_f32_close(got.permute(3, 0, 1, 2), ref[0], rtol=1e-4, atol=1e-4, name="3x3x3")
    w2, b2 = torch.randn(64, 64, 1, 3, 3, generator=g) * 0.05, torch.randn(64, generator=g)
    ref = F.conv3d(F.pad(x, (0, 1, 0, 1)), w2, b2, stride=(1, 2, 2))                       # ZeroPad2d(0,1,0,1) + stride 2
    got = run(cl(x), w2, b2, 5, 3, 3, sh=2, sw=2)
    assert_f32_close(got.permute(3, 0, 1, 2), ref[0], rtol=1e-4, atol=1e-4, name="down")
    up = F.interpolate(x[0].permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)[None]
    ref = F.conv3d(F.pad(up, (1, 1, 1, 1)), w2, b2)                                        # nearest-exact 2x + 3x3
    got = run(cl(x), w2, b2, 5, 12, 14, ph=1, pw=1, up=1)
    assert_f32_close(got.permute(3, 0, 1, 2), ref[0], rtol=1e-4, atol=1e-4, name="up")
    # the same layer as four 2x2 OUTPUT-PHASE launches (up = 2 + 2a + b) with the collapsed taps' weights summed beforehand
    T_, H_, W_ = 5, 6, 7
    x_cl = cl(x)

    def phases(embed, reps):
        """embed: each 2x2 phase kernel inside a 3x3 one, zeros elsewhere (tap i at padding 1 - a = tap i + a at padding 1); reps: the layer's
        output channels that many times over"""
        co = 64 * reps
        outp = torch.full((T_, 2 * H_, 2 * W_, co), 7.0, device=DEV)
        for a in (0, 1):
            for b_ in (0, 1):
                wq = _phase_weights(w2, a, b_)
                if embed:
                    w33 = torch.zeros(64, 64, 1, 3, 3)
                    w33[:, :, :, a:a + 2, b_:b_ + 2] = wq
                    wq = w33
                k, pad = (3, (1, 1)) if embed else (2, (1 - a, 1 - b_))
                wq = wq.repeat(reps, 1, 1, 1, 1).permute(0, 2, 3, 4, 1).reshape(co, -1).contiguous().to(DEV)
                src, extra = x_cl, ()
                if entry == "uv_conv3d_bf16x6":
                    wq = _split6(wq)
                elif entry == "uv_conv3d_f16x3":
                    (wq, scale), src = _split_f16_weights(wq), _split_f16_acts(x_cl)
                    extra = (scale, None)
                _lib.call(entry, _lib.ptr(src), 64, T_, H_, W_, _lib.ptr(wq), _lib.ptr(b2.repeat(reps).to(DEV)), _lib.ptr(outp), co, T_, H_, W_, 64, co,
                          1, k, k, 1, 1, 1, 0, pad[0], pad[1], 2 + 2 * a + b_, 0, None, 0, *extra, _lib.stream_ptr())
        return outp.cpu().permute(3, 0, 1, 2)

    assert_f32_close(phases(False, 1), ref[0], rtol=1e-4, atol=1e-4, name="up as four output phases")
    # 3x3 taps, padding 1 and Hin == Hout are the LDS-halo kernels' geometry, but those store to plain positions: with the halo kernels forced on
    # an output-phase launch must still take the gather kernel. 64 output channels as above, and 128 (whole output tiles of the halo kernels).
    _lib.set_option(_lib.OPT_CONV_HALO, 1)
    try:
        for reps in (1, 2):
            assert_f32_close(phases(True, reps), ref[0].repeat(reps, 1, 1, 1), rtol=1e-4, atol=1e-4, name=f"up as four 3x3 output phases, halo forced, Cout {64 * reps}")
    finally:
        _lib.set_option(_lib.OPT_CONV_HALO, -1)
    w3, b3 = torch.randn(128, 64, 3, 1, 1, generator=g) * 0.05, torch.randn(128, generator=g)
    y = F.conv3d(F.pad(x, (0, 0, 0, 0, 2, 0)), w3, b3)                                     # time_conv + interleave
    ref = torch.stack((y[:, :64], y[:, 64:]), 3).reshape(1, 64, 10, 6, 7)
    got = run(cl(F.pad(x, (0, 0, 0, 0, 2, 0))), w3, b3, 5, 6, 7, interleave=1)
    assert_f32_close(got.permute(3, 0, 1, 2), ref[0], rtol=1e-4, atol=1e-4, name="time_conv interleave")
    w4, b4 = torch.randn(64, 64, 3, 1, 1, generator=g) * 0.05, torch.randn(64, generator=g)
    ref = F.conv3d(x, w4, b4, stride=(2, 1, 1))                                            # downsample3d time_conv
    got = run(cl(x), w4, b4, 2, 6, 7, st=2)
    assert_f32_close(got.permute(3, 0, 1, 2), ref[0], rtol=1e-4, atol=1e-4, name="time stride 2")
    # column-tile choices of the exact-f32 kernel: 256 x 16 tiles for Cout <= 16 (the decoder's 256 -> 12 head convolution),
    # 160-wide tiles for the encoder's 160 / 320-channel stages, 128-wide otherwise (ragged last column tile at Cout = 96 above)
    xl = torch.randn(1, 64, 3, 19, 23, generator=g)                                        # 1311 pixels: ragged row tiles too
    for co in (12, 160, 320, 256):
        wc, bc = torch.randn(co, 64, 3, 3, 3, generator=g) * 0.05, torch.randn(co, generator=g)
        ref = F.conv3d(F.pad(xl, (1, 1, 1, 1, 2, 0)), wc, bc)
        got = run(cl(F.pad(xl, (0, 0, 0, 0, 2, 0))), wc, bc, 3, 19, 23, ph=1, pw=1)
        assert_f32_close(got.permute(3, 0, 1, 2), ref[0], rtol=1e-4, atol=1e-4, name=f"3x3x3, Cout {co}")


@pytest.mark.parametrize("entry", ["uv_conv3d_f32", "uv_conv3d_bf16x6", "uv_conv3d_f16x3"])
def test_conv3d_halo_kernel_geometries(entry):
    """The LDS-halo kernels of the 3x3(x3) stride-1 convolutions (conv3d_halo.hip, and conv3d_halo16.hip for the f16x3 entry;
    vae2_2.py:17-42 as ResidualBlock uses it) against
    F.conv3d AND against the gather kernel it replaces (UV_CONV_HALO=0), forced on for launches too small to pick it by themselves:
    frames that are not whole 8 x 32 patches, one and several patches per frame, causal zero frames in front, two channel blocks
    and two output-channel tiles, a residual input, and the 1x3x3 form. Both arithmetics are the gather kernel's, term for term;
    only the k ORDER of the sum differs (taps inside a channel block instead of channel blocks inside a tap), so the two kernels
    agree to f32 summation-order noise (1e-5 of the output scale), not bit for bit."""
    import torch.nn.functional as F
    from univid_amd import _lib
    g = torch.Generator().manual_seed(14)

    def run(x_cl, w, b, Tout, Hout, Wout, halo, resid=None, t_off=0, up=0):
        _lib.set_option(_lib.OPT_CONV_HALO, 1 if halo else 0)
        T, H, W, C = x_cl.shape
        co, ci, kt, kh, kw_ = w.shape
        wp = w.permute(0, 2, 3, 4, 1).reshape(co, -1).contiguous().to(DEV)
        extra = ()
        if entry == "uv_conv3d_bf16x6":
            wp = _split6(wp)
        elif entry == "uv_conv3d_f16x3":       # conv3d_halo16.hip: pre-split operands, halo image filled by LDS-DMA
            wp, scale = _split_f16_weights(wp)
            x_cl = _split_f16_acts(x_cl)
            extra = (scale, None)
        out = torch.full((Tout, Hout, Wout, co), 7.0, device=DEV)
        _lib.call(entry, _lib.ptr(x_cl), C, T, H, W, _lib.ptr(wp), _lib.ptr(b.to(DEV)), _lib.ptr(out), co, Tout, Hout, Wout, C, co,
                  kt, kh, kw_, 1, 1, 1, t_off, 1, 1, up, 0, _lib.ptr(resid), 0 if resid is None else co, *extra, _lib.stream_ptr())
        return out.cpu()

    cl = lambda t: t[0].permute(1, 2, 3, 0).contiguous().to(DEV)
    # Resample's nearest-exact 2x + Conv2d 3x3 (vae2_2.py:86-96, 153-155): the halo image is filled through the upsampling map
    for (T, H, W, ci, co) in ((2, 9, 13, 64, 128), (3, 20, 35, 32, 256)):
        x = torch.randn(1, ci, T, H, W, generator=g)
        w, b = torch.randn(co, ci, 1, 3, 3, generator=g) * 0.05, torch.randn(co, generator=g)
        up = F.interpolate(x[0].permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)[None]
        ref = F.conv3d(F.pad(up, (1, 1, 1, 1)), w, b)[0].permute(1, 2, 3, 0)
        got = run(cl(x), w, b, T, 2 * H, 2 * W, True, up=1)
        old = run(cl(x), w, b, T, 2 * H, 2 * W, False, up=1)
        assert_f32_close(got.permute(3, 0, 1, 2), ref.permute(3, 0, 1, 2), rtol=1e-4, atol=1e-4, name=f"halo up {entry} {T}x{H}x{W} {ci}->{co}")
        assert (got - old).abs().max() <= 1e-5 * max(1.0, float(old.abs().max()))
    # (Cout 160 / 320: the exact-f32 kernel's 160-wide output tile - the encoder's stages; the bf16x6 entry keeps the gather kernel there)
    # (Cout 12: the decoder's head convolution - the f16x3 entry has a narrow-output halo kernel for it, the others keep the gather kernel)
    for (T, H, W, ci, co, kt) in ((3, 19, 23, 64, 128, 3), (2, 8, 32, 32, 256, 3), (2, 40, 70, 64, 128, 3), (4, 16, 64, 96, 128, 1),
                                  (2, 19, 23, 64, 160, 3), (2, 16, 33, 32, 320, 3), (3, 19, 40, 64, 12, 3), (2, 8, 32, 32, 16, 1),
                                  (2, 17, 40, 128, 128, 3), (3, 16, 64, 64, 256, 1),
                                  # frames that cut into fewer 16 x 16 than 8 x 32 patches (the 45 x 80 stage: 15 against 18): the f16x3 entry's square-patch form
                                  (2, 45, 80, 64, 128, 3), (1, 13, 48, 64, 256, 1), (2, 16, 16, 64, 128, 3)):
        x = torch.randn(1, ci, T, H, W, generator=g)
        w, b = torch.randn(co, ci, kt, 3, 3, generator=g) * 0.05, torch.randn(co, generator=g)
        res = torch.randn(T, H, W, co, generator=g).to(DEV)
        tpad = 2 if kt == 3 else 0
        ref = F.conv3d(F.pad(x, (1, 1, 1, 1, tpad, 0)), w, b)[0].permute(1, 2, 3, 0) + res.cpu()
        xin = cl(F.pad(x, (0, 0, 0, 0, tpad, 0)))
        got = run(xin, w, b, T, H, W, True, resid=res)
        old = run(xin, w, b, T, H, W, False, resid=res)
        assert_f32_close(got.permute(3, 0, 1, 2), ref.permute(3, 0, 1, 2), rtol=1e-4, atol=1e-4, name=f"halo {entry} {T}x{H}x{W} {ci}->{co} kt={kt}")
        assert (got - old).abs().max() <= 1e-5 * max(1.0, float(old.abs().max()))


def test_conv3d_bf16x6_is_f32_grade():
    """uv_conv3d_bf16x6 (three bf16 planes per f32 operand, the six product terms with i + j <= 2, f32 accumulate) against an fp64
    convolution of the same f32 operands, next to the exact-f32 MFMA kernel: at the decoder's channel counts (K = 27 C up to 27 648)
    its error must not exceed the f32 kernel's (measured: 0.87-0.89 x) - it is the f32 arithmetic on another pipe, not a narrower
    one (the 2-way split bf16x3 drops the lo.lo term and is ~20 x further from fp64).
    uv_conv3d_f16x3 (two IEEE fp16 pieces per operand = 22 significant bits, three fp16 MFMA passes) is measured beside them: its
    operands ARE narrower than f32 (2^-22 against 2^-24 relative), but at these K the error of every one of these kernels against fp64 is
    the f32 ACCUMULATION's (~1e-6), which the 22-bit operands raise by a few per cent: gate <= 1.25 x the exact-f32 kernel's error."""
    import torch.nn.functional as F
    from univid_amd import _lib
    g = torch.Generator().manual_seed(0)
    meas = {}
    for C, co in ((256, 256), (1024, 1024)):
        T, H, W = 2, 12, 16
        x = F.silu(torch.randn(1, C, T + 2, H, W, generator=g))
        w = torch.randn(co, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5
        b = torch.randn(co, generator=g) * 0.1
        ref = F.conv3d(F.pad(x.double(), (1, 1, 1, 1, 0, 0)), w.double(), b.double())[0].permute(1, 2, 3, 0)
        x_cl = x[0].permute(1, 2, 3, 0).contiguous().to(DEV)
        wp = w.permute(0, 2, 3, 4, 1).reshape(co, -1).contiguous().to(DEV)
        err = {}
        for name in ("uv_conv3d_f32", "uv_conv3d_bf16x6", "uv_conv3d_f16x3"):
            out = torch.empty(T, H, W, co, device=DEV)
            src, wt, extra = x_cl, wp, ()
            if name.endswith("x6"):
                wt = _split6(wp)
            elif name.endswith("f16x3"):
                wt, scale = _split_f16_weights(wp)
                src, extra = _split_f16_acts(x_cl), (scale, None)
            _lib.call(name, _lib.ptr(src), C, T + 2, H, W, _lib.ptr(wt), _lib.ptr(b.to(DEV)), _lib.ptr(out), co, T, H, W, C, co, 3, 3, 3,
                      1, 1, 1, 0, 1, 1, 0, 0, None, 0, *extra, _lib.stream_ptr())
            d = out.cpu().double() - ref
            err[name] = float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        meas[f"C{C}_f32_mfma_rel_rms_vs_fp64"] = err["uv_conv3d_f32"]
        meas[f"C{C}_bf16x6_rel_rms_vs_fp64"] = err["uv_conv3d_bf16x6"]
        meas[f"C{C}_f16x3_rel_rms_vs_fp64"] = err["uv_conv3d_f16x3"]
        assert err["uv_conv3d_bf16x6"] <= 1.05 * err["uv_conv3d_f32"], (C, err)
        assert err["uv_conv3d_bf16x6"] < 5e-6
        assert err["uv_conv3d_f16x3"] <= 1.25 * err["uv_conv3d_f32"], (C, err)
    record_margin("conv3d 3x3x3: error against fp64 (exact-f32 MFMA vs bf16x6 vs f16x3)", **meas)


# ---------------------------------------------------------------------------------------------------------------
# BASELINE-size properties (size-independent checks at the full shapes the bench runs)
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_attention_and_gemm_properties():
    """L = 11 440 tokens, 24 heads x 128: attention of V = 1 is exactly 1 (softmax rows sum to 1, ragged last tile masked);
    sampled rows of the full-size GEMMs equal fp64 dot products."""
    from univid_amd._lib import EPI_BF16
    Lt, H, D = 11440, 24, 128
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(Lt, C, device=DEV, generator=g).to(BF16)
    k = torch.randn(Lt, C, device=DEV, generator=g).to(BF16)
    vt = torch.ones(C, (Lt + 63) // 64 * 64, dtype=BF16, device=DEV)
    vt[:, Lt:] = 7.0                                                   # padding columns must never be attended
    out = torch.zeros(Lt, C, dtype=BF16, device=DEV)
    L().flash_attn(q, k, vt, out, Lt, Lt, H, D, 1.0 / math.sqrt(D))
    assert (out.float() - 1).abs().max() <= 2 ** -7
    # one head, a few queries, against an fp64 softmax
    v = torch.randn(Lt, C, device=DEV, generator=g).to(BF16)
    vt[:, :Lt] = v.t()
    L().flash_attn(q, k, vt, out, Lt, Lt, H, D, 1.0 / math.sqrt(D))
    rows = torch.tensor([0, 1, 4097, 11439], device=DEV)
    for h in (0, 23):
        sl = slice(h * D, (h + 1) * D)
        s = (q[rows, sl].double() @ k[:, sl].double().t()) / math.sqrt(D)
        truth = torch.softmax(s, -1) @ v[:, sl].double()
        assert (out[rows, sl].double() - truth).abs().max() < 3e-3
    w = (torch.randn(14336, C, device=DEV, generator=g) * 0.02).to(BF16)
    y = torch.empty(Lt, 14336, dtype=BF16, device=DEV)
    L().gemm_bf16(q, w, None, y, EPI_BF16)
    truth = (q[rows].double() @ w.double().t())
    d = (y[rows].double() - truth).abs()
    assert (d <= bf16_ulp(truth.float()).double() + 1e-6).all()


# ---------------------------------------------------------------------------------------------------------------
# BASELINE.json's full size (49-frame 704x1280 latent, L = 11 440 tokens, TI2V-5B widths): size-independent properties
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_attention_properties():
    """Self-attention at the bench shape (L = 11 440, 24 heads x 128, cond+uncond stacked): sampled query rows against an fp64
    softmax computed here, V = 1 gives exactly 1, and attention is linear in V."""
    Lq = Lk = 11440
    H, D, B = 24, 128, 2
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(21)
    q = torch.randn(B * Lq, C, device=DEV, generator=g).to(BF16)
    k = torch.randn(B * Lk, C, device=DEV, generator=g).to(BF16)
    v = torch.randn(B * Lk, C, device=DEV, generator=g).to(BF16)
    cols = (B - 1) * Lk + (Lk + 63) // 64 * 64
    vt = torch.zeros(C, cols, dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.t()
    out = torch.empty(B * Lq, C, dtype=BF16, device=DEV)
    L().flash_attn(q, k, vt, out, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert torch.isfinite(out.float()).all()
    rows = torch.tensor([0, 1, 31, 32, 255, 256, 5000, 11439], device=DEV)
    for b in range(B):
        for hd in (0, 11, 23):
            sl = slice(hd * D, (hd + 1) * D)
            qs = q[b * Lq + rows][:, sl].double()
            ks, vs = k[b * Lk:(b + 1) * Lk, sl].double(), v[b * Lk:(b + 1) * Lk, sl].double()
            truth = torch.softmax(qs @ ks.t() / math.sqrt(D), -1) @ vs
            got = out[b * Lq + rows][:, sl].double()
            tol = 3 * bf16_ulp(truth.float().cpu()).to(DEV) + 2e-3 * truth.abs().max()
            assert ((got - truth).abs() <= tol).all(), f"sample {b} head {hd}: max err {float((got - truth).abs().max()):.3e}"
    ones = torch.ones_like(vt)
    o1 = torch.empty_like(out)
    L().flash_attn(q, k, ones, o1, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert (o1.float() - 1).abs().max() <= 2 ** -7
    vt2 = (vt.float() * 0.5).to(BF16)                       # exact scaling: attention is linear in V
    o2 = torch.empty_like(out)
    L().flash_attn(q, k, vt2, o2, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert ((o2.float() * 2 - out.float()).abs() <= 2 * bf16_ulp(out.float().cpu()).to(DEV)).all()


def test_default_workload_attention_and_gemm_properties():
    """UniVid's default workload (inference.py:48-50: 121 frames 704 x 1280 -> L = 27 280 tokens, the CFG pair stacked = 54 560 rows,
    24 heads x 128): self-attention of V = 1 is exactly 1 over every row of both samples (softmax rows sum to 1; 27 280 = 426 key tiles
    + a ragged 16-key tile), sampled query rows against an fp64 softmax, linearity in V, and sampled rows of the three GEMM shapes
    (3072 -> 3072 bf16, 3072 -> 14336 GELU, 14336 -> 3072 gated fp32 residual) at 54 560 rows - whole rounds of the persistent kernel
    plus the leftover-row strip - against fp64 dot products."""
    from univid_amd._lib import EPI_BF16, EPI_GATE_RESID_F32
    Lq = Lk = 27280
    H, D, B = 24, 128, 2
    C = H * D
    g = torch.Generator(device=DEV).manual_seed(27)
    q = torch.randn(B * Lq, C, device=DEV, generator=g).to(BF16)
    k = torch.randn(B * Lk, C, device=DEV, generator=g).to(BF16)
    v = torch.randn(B * Lk, C, device=DEV, generator=g).to(BF16)
    cols = (B - 1) * Lk + (Lk + 63) // 64 * 64
    vt = torch.zeros(C, cols, dtype=BF16, device=DEV)
    vt[:, :B * Lk] = v.t()
    out = torch.empty(B * Lq, C, dtype=BF16, device=DEV)
    L().flash_attn(q, k, vt, out, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert torch.isfinite(out.float()).all()
    rows = torch.tensor([0, 31, 32, 383, 384, 4097, 13000, 27247, 27279], device=DEV)
    for b in range(B):
        for hd in (0, 13, 23):
            sl = slice(hd * D, (hd + 1) * D)
            qs = q[b * Lq + rows][:, sl].double()
            ks, vs = k[b * Lk:(b + 1) * Lk, sl].double(), v[b * Lk:(b + 1) * Lk, sl].double()
            truth = torch.softmax(qs @ ks.t() / math.sqrt(D), -1) @ vs
            got = out[b * Lq + rows][:, sl].double()
            tol = 3 * bf16_ulp(truth.float().cpu()).to(DEV) + 2e-3 * truth.abs().max()
            assert ((got - truth).abs() <= tol).all(), f"sample {b} head {hd}: max err {float((got - truth).abs().max()):.3e}"
    ones = torch.ones_like(vt)
    ones[:, B * Lk:] = 7.0                                   # the ragged tile's padding columns must never be attended
    o1 = torch.empty_like(out)
    L().flash_attn(q, k, ones, o1, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert (o1.float() - 1).abs().max() <= 2 ** -7
    vt2 = (vt.float() * 0.5).to(BF16)
    L().flash_attn(q, k, vt2, o1, Lq, Lk, H, D, D ** -0.5, batch=B)
    assert ((o1.float() * 2 - out.float()).abs() <= 2 * bf16_ulp(out.float().cpu()).to(DEV)).all()
    del ones, o1, vt2, vt, v, k
    # GEMMs at 54 560 rows: sampled rows (first / last rows of the persistent part, rows of the leftover strip) against fp64
    M = B * Lq
    rows = torch.tensor([0, 255, 256, 30000, 54271, 54272, 54400, 54559], device=DEV)
    w = (torch.randn(14336, C, device=DEV, generator=g) * 0.02).to(BF16)
    y = torch.empty(M, 14336, dtype=BF16, device=DEV)
    L().gemm_bf16(q, w, None, y, EPI_BF16)
    truth = q[rows].double() @ w.double().t()
    assert ((y[rows].double() - truth).abs() <= bf16_ulp(truth.float()).double() + 1e-6).all(), "ffn.0-shape GEMM rows"
    w2 = (torch.randn(C, 14336, device=DEV, generator=g) * 0.02).to(BF16)
    x = torch.randn(M, C, device=DEV, generator=g)
    x0 = x[rows].clone()
    gate = torch.randn(2, C, device=DEV, generator=g)
    tid = (torch.arange(M, device=DEV) >= Lq).to(torch.int32)           # sample 0 -> gate row 0, sample 1 -> row 1
    L().gemm_bf16(y, w2, None, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid)
    acc = y[rows].double() @ w2.double().t()
    gr = gate[tid[rows].long()].double()
    want = x0.double() + acc.to(BF16).double() * gr                     # the epilogue rounds the product to bf16 first (model.py:255)
    d = (x[rows].double() - want).abs()
    tol = (bf16_ulp(acc.float()).double() + 2e-5 * acc.abs().max()) * gr.abs() + 1e-6
    assert (d <= tol).all() and (d <= 1e-6).float().mean() > 0.999, f"ffn.2-shape gated residual rows: max err {float(d.max()):.3e}"
    wq = (torch.randn(C, C, device=DEV, generator=g) * 0.02).to(BF16)
    yq = torch.empty(M, C, dtype=BF16, device=DEV)
    L().gemm_bf16(q, wq, None, yq, EPI_BF16)
    truth = q[rows].double() @ wq.double().t()
    assert ((yq[rows].double() - truth).abs() <= bf16_ulp(truth.float()).double() + 1e-6).all(), "q-shape GEMM rows"


def test_default_workload_vae_decode_properties():
    """UniVid's default clip through the VAE decoder: latent [48, 31, 44, 80] -> 121 x 704 x 1280 RGB (inference.py:48-50,
    vae2_2.py:812-839), exact-f32 mode, with the size-independent properties of test_vae_config4_full_clip_encode_decode_properties:
    shape, finiteness, clamp, first frame == decoding the first latent frame alone, frames 0..12 == decoding latents 0..3 alone
    (causal decoder), pass length 1 == 4 on the first three latent frames; and the f32-grade bf16x6 mode within rtol 1e-3 / atol 1e-4
    of the exact mode on every element of the 121 frames. The memory high-water mark of the decode is recorded."""
    from oracle import wan_vae
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    sd = wan_vae.make_state_dict(wan_vae.FULL_CFG, 2)
    vae = Wan2_2_VAE(device=DEV, precision="fp32")
    vae.model.load_state_dict(sd)
    g = torch.Generator(device=DEV).manual_seed(47)
    z = torch.randn(48, 31, 44, 80, generator=g, device=DEV)
    with torch.no_grad():
        import gc
        gc.collect()                                  # earlier tests' models (reference cycles through their hooks) are garbage by now
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = vae.decode([z])[0]
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30      # high-water mark of the decode itself (weights excluded)
        assert out.shape == (3, 121, 704, 1280) and torch.isfinite(out).all()
        assert out.abs().max() <= 1.0
        first = vae.decode([z[:, :1]])[0]
        assert torch.equal(first, out[:, :1]), "first frame of the whole-clip decode != decoding the first latent frame alone"
        head = vae.decode([z[:, :4]])[0]
        assert torch.equal(head, out[:, :13]), "causal decoder: frames 0..12 must not depend on latent frames 4.."
        vae1 = Wan2_2_VAE(device=DEV, precision="fp32", frames_per_pass=1)
        vae1.model.load_state_dict(sd)
        assert torch.equal(vae1.decode([z[:, :3]])[0], head[:, :9]), "pass length 1 vs 4"
        del vae1, first, head
        vae6 = Wan2_2_VAE(device=DEV, precision="bf16x6")
        vae6.model.load_state_dict(sd)
        out6 = vae6.decode([z])[0]
        d = (out6 - out).abs()
        bad = int((d > 1e-4 + 1e-3 * out.abs()).sum())
        record_margin("default workload VAE decode 121x704x1280", peak_GiB=peak, bf16x6_vs_f32_max_abs=float(d.max()), outside=bad)
        assert bad == 0, f"bf16x6 vs exact f32: {bad} of {out.numel()} elements outside rtol 1e-3 / atol 1e-4"


def test_full_size_dit_stack_equals_sequential():
    """Two TI2V-5B-width blocks at the bench sequence length: the stacked CFG pair is bit-identical to two single forwards,
    everything finite, and the result depends on the context (cond != uncond)."""
    from univid_amd.wan.model import WanModel
    from univid_amd.wan.textimage2video import TI2VConfig
    cfg = dict(TI2VConfig.dit, num_layers=2)
    with torch.device(DEV):
        m = WanModel.from_config(cfg)
    m = m.eval().requires_grad_(False)
    m.init_weights(5)
    m.prepare()
    g = torch.Generator(device=DEV).manual_seed(4)
    lat = torch.randn(48, 13, 44, 80, device=DEV, generator=g)
    ca = torch.randn(77, cfg["text_dim"], device=DEV, generator=g) * 0.1
    cb = torch.randn(12, cfg["text_dim"], device=DEV, generator=g) * 0.1
    Ltok = 13 * 22 * 40
    tv = torch.full((1, Ltok), 431.0, device=DEV)
    with torch.no_grad():
        both = m([lat, lat], t=torch.cat([tv, tv]), context=[ca, cb], seq_len=Ltok)
        a = m([lat], t=tv, context=[ca], seq_len=Ltok)[0]
        b = m([lat], t=tv, context=[cb], seq_len=Ltok)[0]
    assert both[0].shape == (48, 13, 44, 80) and torch.isfinite(both[0]).all() and torch.isfinite(both[1]).all()
    assert torch.equal(both[0], a) and torch.equal(both[1], b)
    assert not torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# Ulysses sequence parallelism: two processes share THE one GPU of the test box and talk over gloo
# (RCCL needs one device per rank), so the exchanges go through the host-memory emulation while every kernel is the HIP one.
# The sharded forward must reproduce the plain forward bit for bit: GEMM rows, RMSNorm/RoPE rows and (query, head) attention
# problems are the same arithmetic wherever they run.
# ---------------------------------------------------------------------------------------------------------------
def _init_group(rank, world, port, nccl):
    """gloo: the ranks share the test box's one GPU (exchanges go through the host-memory emulation of univid_amd.parallel);
    nccl: one GPU per rank, RCCL over xGMI - the transport the product uses (runs where the box has >= `world` GPUs)."""
    import torch.distributed as dist
    torch.set_num_threads(8)          # spawned workers: several processes share the host (and 256 threads each is pathological)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if nccl:
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _spawn(worker, world, nccl, timeout=300):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q, nccl)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=timeout) for _ in procs)
    for p in procs:
        p.join(60)
    return res


def _need_gpus(n):
    if torch.cuda.device_count() < n:
        pytest.skip(f"needs {n} GPUs (RCCL, one device per rank); this box has {torch.cuda.device_count()}")


def _sp_gpu_worker(rank, world, port, q, nccl=False):
    dist = _init_group(rank, world, port, nccl)
    try:
        g = load_golden("dit_tiny")
        cfg, sd, m = _tiny_model(g["seed"], num_heads=4)
        gen = torch.Generator().manual_seed(5)
        x2 = torch.randn(48, 4, 16, 16, generator=gen)
        ctx2 = torch.randn(7, cfg["text_dim"], generator=gen)
        Lt = 256
        xa, xb = g["x"].to(DEV), x2.to(DEV)
        ca, cb = g["ctx"].to(DEV), ctx2.to(DEV)
        ta, tb = g["t_two"].to(DEV), torch.full((1, Lt), 321.0, device=DEV)
        odd = torch.randn(48, 3, 10, 12, generator=gen).to(DEV)          # 90 tokens: not a multiple of 8 -> must refuse
        with torch.no_grad():
            plain = m([xa, xb], torch.cat([ta, tb]), [ca, cb], Lt)
            m.enable_sequence_parallel()
            assert m.sp.size == world
            sharded = m([xa, xb], torch.cat([ta, tb]), [ca, cb], Lt)       # stacked pair, two timesteps in sample a
            single = m([xb], tb, [cb], Lt)[0]
            refused = False
            try:
                m([odd], torch.full((1, 90), 500.0, device=DEV), [cb], 90)
            except NotImplementedError:
                refused = True
        ok = torch.equal(sharded[0], plain[0]) and torch.equal(sharded[1], plain[1]) and torch.equal(single, plain[1])
        if rank == 0:
            # not only sharded == plain (HIP vs HIP): the SHARDED forward against the PINNED golden output (oracle == reference bit for
            # bit when the fixture was generated; two timesteps in one sample, i.e. the i2v form) and against the no-rounding truth
            # run, with the tiny-DiT gates. The oracle re-run on THIS host must reproduce the golden up to the last-place differences
            # of oneDNN's bf16 kernels between CPU generations (bit-identical in the build container: tests/test_oracle_golden.py).
            try:
                from oracle import wan_dit
                with torch.no_grad():
                    here = wan_dit.dit_forward(sd, cfg, [g["x"]], g["t_two"], [g["ctx"]], Lt)[0]
                    truth = _truth_forward(sd, cfg, [g["x"]], g["t_two"], [g["ctx"]], Lt)[0]
                ref = g["out_two"]
                drift = _rel_rms(here, ref)
                assert drift <= 1e-3, f"the CPU oracle on this host is {drift:.2e} rel rms from the pinned golden"
                assert_model_close(sharded[0], ref, truth, name=f"sequence-parallel forward, {world} ranks, vs pinned golden")
            except BaseException as ex:      # report instead of leaving the parent to wait for the queue timeout
                q.put((rank, False, f"rank 0 check failed: {ex!r}"[:500], float("nan")))
                raise
        q.put((rank, bool(ok), refused, float((sharded[0] - plain[0]).abs().max())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sequence_parallel_forward_is_bit_identical(world):
    res = _spawn(_sp_gpu_worker, world, nccl=False)
    assert all(ok and refused for _, ok, refused, _ in res), res


@pytest.mark.parametrize("world", [2, 4])
def test_sequence_parallel_forward_over_rccl(world):
    """The same check with one GPU per rank and RCCL all-to-alls / all-gathers over xGMI (parallel.py's `backend == "nccl"`
    branches; reference distributed/ulysses.py:9-47, util.py:6-51): bit-identical to the unsharded forward on every rank."""
    _need_gpus(world)
    res = _spawn(_sp_gpu_worker, world, nccl=True)
    assert all(ok and refused for _, ok, refused, _ in res), res


def _rccl_one_rank_worker(rank, world, port, q, nccl=True):
    dist = _init_group(rank, world, port, nccl)
    try:
        from univid_amd import parallel
        x = torch.arange(12, dtype=torch.float32, device=DEV).view(3, 4)
        dist.barrier()
        got = parallel.gather_latents([x, x + 1], 2)
        t = torch.tensor([1.5], device=DEV, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        sp = parallel.SeqParallel()
        out = torch.empty(8, 4, dtype=BF16, device=DEV)
        sp.heads_to_tokens(torch.ones(8, 4, dtype=BF16, device=DEV), 8, out)
        q.put((rank, dist.get_backend(), bool(torch.equal(got[0], x) and torch.equal(got[1], x + 1) and float(t) == 1.5 and bool((out == 1).all()))))
    finally:
        dist.destroy_process_group()


def test_rccl_process_group_on_this_box():
    """RCCL itself on whatever the box has: a ONE-rank process group on backend "nccl" (init with device_id, barrier,
    all_gather through parallel.gather_latents, all_reduce MAX of the float64 timing scalar bench.py reduces, the size-1
    sequence-parallel exchange). The multi-rank variants above need one GPU per rank; this one runs everywhere and catches an
    RCCL / IPC environment that cannot even initialise."""
    res = _spawn(_rccl_one_rank_worker, 1, nccl=True)
    assert res == [(0, "nccl", True)], res


def _cfgp_gpu_worker(rank, world, port, q, nccl=False):
    dist = _init_group(rank, world, port, nccl)
    try:
        from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
        g = load_golden("sampler_tiny")
        cfg, sd, m = _tiny_model(g["seed"])
        pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
        args = (g["noise"].to(DEV), [g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], 4, g["shift"], g["guide_scale"])
        with torch.no_grad():
            plain = pipe.denoise(*args)
            plain_i2v = pipe.denoise(*args, z=g["z"].to(DEV))
            # UniVid's dynamic text weight (native schedule): the single-process loop gives the CFG pair the counter's two consecutive
            # values; under CFG parallelism each rank runs ONE of the two forwards and must take that forward's value
            import logging
            from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
            wr = Wan22ContextWrapper(pipe, None, logging.getLogger("t"), CrossAttentionConfig(use_dynamic_text_weight=True, total_sampling_steps=8,
                                                                                             text_weight_transition_ratio=0.75, text_weight_schedule="linear"))
            wr.set_bagel_context(torch.zeros(1, 2, 2))
            with wr.scheduled():
                weighted = pipe.denoise(*args)
            pipe.enable_cfg_parallel()
            rec = []
            split = pipe.denoise(*args, record=rec)
            split_i2v = pipe.denoise(*args, z=g["z"].to(DEV))
            with wr.scheduled():
                split_weighted = pipe.denoise(*args)
        ok = torch.equal(split, plain) and torch.equal(split_i2v, plain_i2v) and len(rec) == 4
        ok = ok and torch.equal(split_weighted, weighted) and not torch.equal(weighted, plain)
        q.put((rank, bool(ok), pipe.cfgp.branch, float((split - plain).abs().max())))
    finally:
        dist.destroy_process_group()


def test_cfg_parallel_denoise_is_bit_identical():
    """SURVEY 8(e) intra-sample sharding: cond on rank 0, uncond on rank 1, one all-gather of the prediction per step; both ranks
    must end every step with the latent of the single-process loop, bit for bit (t2v and i2v). Two processes on the one GPU, gloo."""
    res = _spawn(_cfgp_gpu_worker, 2, nccl=False)
    assert all(ok for _, ok, _, _ in res), res
    assert [b for _, _, b, _ in res] == ["cond", "uncond"]


def test_cfg_parallel_denoise_over_rccl():
    """CFG pair on two GPUs, the prediction exchanged by an RCCL all-gather per step: bit-identical to the single-GPU loop."""
    _need_gpus(2)
    res = _spawn(_cfgp_gpu_worker, 2, nccl=True)
    assert all(ok for _, ok, _, _ in res), res
    assert [b for _, _, b, _ in res] == ["cond", "uncond"]


def _replica_gpu_worker(rank, world, port, q, nccl=False):
    """The metric's multi-GPU mode (bench.py --gpus N): independent samples sharded over the ranks, weights replicated,
    ONE all-gather of the final latents; every rank must end with every sample's latent, bit-identical to denoising all samples
    on one GPU."""
    dist = _init_group(rank, world, port, nccl)
    try:
        from univid_amd import parallel
        from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
        g = load_golden("sampler_tiny")
        cfg, sd, m = _tiny_model(g["seed"])
        pipe = WanTI2V(TI2VConfig, model=m, device=torch.device("cuda", torch.cuda.current_device()))
        n = world + 1                                                  # uneven shards: the first rank owns two samples
        gens = [torch.Generator().manual_seed(parallel.sample_seed(100, i)) for i in range(n)]
        noises = [torch.randn(48, 4, 16, 16, generator=gg).to(DEV) for gg in gens]
        ctxs = [[(g["ctx"] * (1 + 0.1 * i)).to(DEV)] for i in range(n)]
        nulls = [[g["ctx_null"].to(DEV)] for _ in range(n)]
        with torch.no_grad():
            alone = [pipe.denoise(noises[i], ctxs[i], nulls[i], 3, g["shift"], g["guide_scale"]) for i in range(n)]
            got = parallel.denoise_batch(pipe, noises, ctxs, nulls, 3, g["shift"], g["guide_scale"])
            # the pipeline path (round 5): every sample one generation under this rank's Wan22ContextWrapper (forward counter per sample)
            import logging
            from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
            wr = Wan22ContextWrapper(pipe, None, logging.getLogger("t"), CrossAttentionConfig(use_dynamic_text_weight=True, total_sampling_steps=6,
                                                                                             text_weight_transition_ratio=0.7))
            wr.set_bagel_context(torch.zeros(1, 2, 2))
            alone_w = []
            for i in range(n):
                with wr.scheduled():
                    alone_w.append(pipe.denoise(noises[i], ctxs[i], nulls[i], 3, g["shift"], g["guide_scale"]).clone())
            got_w = parallel.denoise_batch(pipe, noises, ctxs, nulls, 3, g["shift"], g["guide_scale"], wrapper=wr)
        ok = len(got) == n and all(torch.equal(a, b) for a, b in zip(got, alone))
        ok = ok and len(got_w) == n and all(torch.equal(a, b) for a, b in zip(got_w, alone_w)) and not torch.equal(alone_w[0], alone[0])
        q.put((rank, bool(ok), str(got[0].device)))
    finally:
        dist.destroy_process_group()


def test_sample_replicas_and_latent_all_gather_shared_gpu():
    res = _spawn(_replica_gpu_worker, 2, nccl=False)
    assert all(ok for _, ok, _ in res), res


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sample_replicas_and_latent_all_gather_over_rccl(world):
    """One GPU per rank, the all-gather of the final latents on RCCL over xGMI (the single collective of the path)."""
    _need_gpus(world)
    res = _spawn(_replica_gpu_worker, world, nccl=True)
    assert all(ok for _, ok, _ in res), res
    assert sorted(d for _, _, d in res) == sorted(f"cuda:{r}" for r in range(world))


def test_model_on_second_gpu_without_set_device():
    """The reference's manual model placement (`wan_gpu=1`, model_pipeline.py): a model living on cuda:1 must run there while the
    process's current device stays cuda:0 - every launch follows the device of its tensors (univid_amd._lib.call)."""
    _need_gpus(2)
    g = load_golden("dit_tiny")
    cfg, sd, m0 = _tiny_model(g["seed"])
    from univid_amd.wan.model import WanModel
    m1 = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m1.load_state_dict(sd)
    m1 = m1.to("cuda:1").eval()
    assert torch.cuda.current_device() == 0
    with torch.no_grad():
        a = m0([g["x"].to("cuda:0")], g["t_two"].to("cuda:0"), [g["ctx"].to("cuda:0")], 256)[0]
        b = m1([g["x"].to("cuda:1")], g["t_two"].to("cuda:1"), [g["ctx"].to("cuda:1")], 256)[0]
    assert b.device == torch.device("cuda:1") and torch.cuda.current_device() == 0
    assert torch.equal(a.cpu(), b.cpu())
    with pytest.raises(L().UnividHipError):
        L().gemm_bf16(torch.zeros(64, 64, dtype=BF16, device="cuda:0"), torch.zeros(64, 64, dtype=BF16, device="cuda:1"), None,
                      torch.zeros(64, 64, dtype=BF16, device="cuda:0"), 0)


def _sp_full_worker(rank, world, port, q, nccl=False):
    dist = _init_group(rank, world, port, nccl)
    try:
        from univid_amd.wan.model import WanModel
        from univid_amd.wan.textimage2video import TI2VConfig
        cfg = dict(TI2VConfig.dit, num_layers=1)
        with torch.device(DEV):
            m = WanModel.from_config(cfg)
        m = m.eval().requires_grad_(False)
        m.init_weights(5)
        m.prepare()
        g = torch.Generator(device=DEV).manual_seed(4)
        lat = torch.randn(48, 13, 44, 80, device=DEV, generator=g)
        ca = torch.randn(77, cfg["text_dim"], device=DEV, generator=g) * 0.1
        cb = torch.randn(12, cfg["text_dim"], device=DEV, generator=g) * 0.1
        Ltok = 13 * 22 * 40
        tv = torch.full((1, Ltok), 431.0, device=DEV)
        with torch.no_grad():
            plain = m([lat, lat], t=torch.cat([tv, tv]), context=[ca, cb], seq_len=Ltok)
            m.enable_sequence_parallel()
            sharded = m([lat, lat], t=torch.cat([tv, tv]), context=[ca, cb], seq_len=Ltok)
        q.put((rank, bool(torch.equal(sharded[0], plain[0]) and torch.equal(sharded[1], plain[1]))))
    finally:
        dist.destroy_process_group()


def test_full_size_sequence_parallel_bit_identical():
    """The bench shape (11 440 tokens, 24 heads x 128, cond+uncond stacked), one TI2V-5B-width block, 2 ranks: token shards of
    5 720, 12 heads per rank in the exchanged attention; bit-identical to the unsharded forward."""
    res = _spawn(_sp_full_worker, 2, nccl=False, timeout=600)
    assert all(ok for _, ok in res), res


def test_full_size_sequence_parallel_over_rccl():
    """The bench shape on 2 GPUs: 8.8 MB all-to-alls per tensor over RCCL / xGMI; bit-identical to the unsharded forward."""
    _need_gpus(2)
    res = _spawn(_sp_full_worker, 2, nccl=True, timeout=600)
    assert all(ok for _, ok in res), res


def test_full_size_t2v_and_i2v_end_to_end():
    """The whole product path at the bench size with the production model sizes (30-block TI2V-5B DiT, full-width VAE, random-init
    weights): WanTI2V.t2v for 2 sampler steps + VAE decode of the 49-frame 704x1280 clip, and an i2v start from its first frame
    (VAE encode of one image + masked denoising). Shapes, value range, determinism (same seed -> same bits)."""
    from univid_amd.wan.model import WanModel
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    with torch.device(DEV):
        m = WanModel.from_config(TI2VConfig.dit)
    m = m.eval().requires_grad_(False)
    m.init_weights(0)
    m.prepare()
    vae = Wan2_2_VAE(device=DEV, seed=0)
    pipe = WanTI2V(model=m, vae=vae, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    pe = [torch.randn(40, 4096, device=DEV, generator=g) * 0.1]
    ne = [torch.randn(9, 4096, device=DEV, generator=g) * 0.1]
    with torch.no_grad():
        v1 = pipe.t2v("", size=(1280, 704), frame_num=49, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne)
        lat2 = pipe.t2v("", size=(1280, 704), frame_num=49, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne,
                        decode=False)
        lat3 = pipe.t2v("", size=(1280, 704), frame_num=49, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne,
                        decode=False)
        img = v1[:, 0].clamp(-1, 1).contiguous()
        li = pipe.i2v("", img, max_area=704 * 1280, frame_num=49, sampling_steps=2, seed=3, prompt_embeds=pe,
                      negative_prompt_embeds=ne, decode=False)
    assert v1.shape == (3, 49, 704, 1280) and torch.isfinite(v1).all() and v1.abs().max() <= 1.0
    assert lat2.shape == (48, 13, 44, 80) and torch.equal(lat2, lat3)
    assert li.shape == (48, 13, 44, 80) and torch.isfinite(li).all()
    # the same clip through UniVid's own entry point (inference.py:311,377 -> model_pipeline.py:2577-2655) at full size: with the weight
    # schedule flat (max = min = 1) it IS the plain path - video and i2v latent bit for bit -; with inference.py's schedule it runs on the
    # same graph replay (no re-assigned forwards anywhere), differs, and stays finite
    import types
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    bagel = types.SimpleNamespace(extract_semantic_tokens=lambda text, image: torch.zeros(1, 128, 3584, device=DEV, dtype=BF16))
    kw = dict(steps=2, guidance_scale=5.0, frames=49, size=(1280, 704), shift=5.0, prompt_embeds=pe, negative_prompt_embeds=ne)
    flat = CrossAttentionFusionPipeline(CrossAttentionConfig(use_lora=False, text_weight_max=1.0, text_weight_min=1.0, total_sampling_steps=2),
                                        wan_pipeline=pipe, bagel_extractor=bagel)
    sched = CrossAttentionFusionPipeline(CrossAttentionConfig(use_lora=False, total_sampling_steps=10), wan_pipeline=pipe, bagel_extractor=bagel)
    with torch.no_grad():
        pv, path = flat.generate_video_with_bagel_context("", seed=7, **kw)
        assert path is None and torch.equal(pv, v1)
        del pv
        pli, _ = flat.generate_video_with_bagel_context("", image=img, seed=3, decode=False, **kw)
        assert torch.equal(pli, li)
        runner = pipe._runner
        wl, _ = sched.generate_video_with_bagel_context("", seed=7, decode=False, **kw)
    assert pipe._runner is not None and all("forward" not in b.cross_attn.__dict__ for b in m.blocks) and "forward" not in m.__dict__
    assert torch.isfinite(wl).all() and not torch.equal(wl, lat2)
    assert any(s != (1.0, 1.0) for s in pipe._runner.state), "2 of 10 scheduled steps ran: the runner's K / V^T must still hold weighted context"


# ---------------------------------------------------------------------------------------------------------------
# BASELINE config 5: the SigLIP2 frame ranker (eval_understanding.py:171-240). The towers run on the DiT's GEMM / attention /
# LayerNorm kernels with bf16 operands and an fp32 residual stream; the golden is transformers' fp32 forward, so the gate is the
# one that matters for a ranker: cosine similarity of every embedding with the reference embedding, the similarity values, and
# the ranking itself.
# ---------------------------------------------------------------------------------------------------------------
class _StubProcessor:
    """Stands in for HF's AutoProcessor: 'images' are already NaFlex-patchified tensors, 'text' is looked up in a table."""

    def __init__(self, ids):
        self.ids = ids

    def __call__(self, images=None, text=None, return_tensors="pt"):
        if text is not None:
            return {"input_ids": self.ids[text[0]]}
        pv = torch.stack([im[0] for im in images])
        mask = torch.stack([im[1] for im in images])
        shp = torch.stack([im[2] for im in images])
        return {"pixel_values": pv, "pixel_attention_mask": mask, "spatial_shapes": shp}


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1)


def test_siglip2_towers_vs_transformers_golden():
    from oracle import siglip2 as osl
    from univid_amd.understanding import Siglip2Model, Siglip2Scorer, mmr_select
    g = load_golden("siglip2_tiny")
    m = Siglip2Model(osl.TINY_CFG)
    m.load_state_dict(osl.make_state_dict(osl.TINY_CFG, int(g["seed"])), strict=False)
    m = m.to(DEV).eval()
    for dt, cmin, rmax in ((torch.float16, 0.99999, 4e-3), (torch.bfloat16, 0.9995, 2e-2)):     # fp16 = the reference's dtype
        m.set_operand_dtype(dt)
        fi = m.get_image_features(g["pixel_values"], g["pixel_attention_mask"], g["spatial_shapes"])   # mixed grids, padded images
        ft = m.get_text_features(g["input_ids"])
        ftm = m.get_text_features(g["input_ids"], g["attention_mask"])
        for got, ref, name in ((fi, g["image_features"], "image"), (ft, g["text_features"], "text"), (ftm, g["text_features_masked"], "text+mask")):
            c = _cos(got, ref)
            rel = ((got.cpu().double() - ref.double()).norm(dim=-1) / ref.double().norm(dim=-1)).max()
            assert c.min() > cmin and rel < rmax, f"{dt} {name}: min cosine {float(c.min()):.6f}, max relative error {float(rel):.3e}"
    # the scorer facade: rank_frames / emb_imgs / emb_text / mmr_select on the same data
    frames = [(g["pixel_values"][i], g["pixel_attention_mask"][i], g["spatial_shapes"][i]) for i in range(g["pixel_values"].shape[0])]
    sc = Siglip2Scorer(device=DEV, model=m, processor=_StubProcessor({"q": g["input_ids"][:1]}))
    idx, vals = sc.rank_frames(frames, "q", topk=4, bs=4)
    ref_sims = torch.nn.functional.normalize(g["image_features"], dim=-1) @ torch.nn.functional.normalize(g["text_features"][:1], dim=-1).T
    assert torch.allclose(torch.tensor(vals), ref_sims.squeeze(-1)[idx].float(), atol=5e-3)
    assert sorted(vals, reverse=True) == vals and len(idx) == 4
    gaps = ref_sims.squeeze(-1).sort(descending=True).values
    if float((gaps[:4] - gaps[1:5]).min()) > 1e-2:          # ranking is only well-defined where the reference scores are separated
        assert idx == g["rank_idx"].tolist()
    v = sc.emb_imgs(frames, bs=64)
    assert torch.allclose(v.norm(dim=-1).cpu(), torch.ones(len(frames)), atol=1e-5)
    assert sc.rank_frames([], "q", 3) == ([], [])
    # the text tower on its side stream beside the vision tower (the default) == one tower after the other, bit for bit, call after call
    assert sc.overlap_towers
    both = [sc.rank_frames(frames, "q", topk=4, bs=4) for _ in range(3)]
    sc.overlap_towers = False
    serial = sc.rank_frames(frames, "q", topk=4, bs=4)
    sc.overlap_towers = True
    assert all(b == serial for b in both) and serial == (idx, vals)
    sel = mmr_select(v, sc.emb_text("q"), 3)
    assert len(sel) == 3 and len(set(sel)) == 3
    with pytest.raises(NotImplementedError):
        Siglip2Scorer(device=DEV, model=m, processor=_StubProcessor({}), dtype=torch.float32)


def test_siglip2_base_width_vs_oracle():
    """SigLIP2-base geometry (768-d, 12 heads x 64, 12 layers, patch 16, 256 patches) on BASELINE config 5's 64 keyframes: HIP towers vs
    the fp32 CPU oracle on a sample of the frames with the same deterministic weights (text tower with a small vocabulary: the 256 000-row embedding table is a lookup)."""
    from oracle import siglip2 as osl
    from univid_amd.understanding import Siglip2Model
    cfg = dict(vision=dict(osl.BASE_CFG["vision"]), text=dict(osl.BASE_CFG["text"], vocab_size=1000))
    sd = osl.make_state_dict(cfg, 1)
    m = Siglip2Model(cfg)
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    B, N = 64, 256                         # BASELINE config 5: 64 keyframes per video; the oracle runs on a sample of them
    sample = [0, 7, 22, 31, 40, 63]        # (the vision tower treats frames independently: row i depends on frame i only)
    pv = torch.randn(B, N, 768, generator=g)
    mask = torch.ones(B, N, dtype=torch.int64)
    shapes = torch.tensor([[16, 16]] * B)
    ids = torch.randint(0, 1000, (1, 64), generator=g)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        ref_i = osl.image_features(sd, cfg, pv[sample], mask[sample], shapes[sample])
        ref_t = osl.text_features(sd, cfg, ids)
    sims_ref = torch.nn.functional.normalize(ref_i, dim=-1) @ torch.nn.functional.normalize(ref_t, dim=-1).T
    for dt, cmin, smax in ((torch.float16, 0.99999, 1e-3), (torch.bfloat16, 0.9995, 5e-3)):
        m.set_operand_dtype(dt)
        got_all, got_t = m.get_image_features(pv, mask, shapes), m.get_text_features(ids)
        assert got_all.shape[0] == B and torch.isfinite(got_all).all()
        got8 = m.get_image_features(pv[:8], mask[:8], shapes[:8])
        assert _cos(got8, got_all[:8]).min() > 0.999999, "a frame's embedding must not depend on the batch it is encoded in"
        got_i = got_all[sample]
        assert _cos(got_i, ref_i).min() > cmin and _cos(got_t, ref_t).min() > cmin, (dt, float(_cos(got_i, ref_i).min()))
        sims_got = torch.nn.functional.normalize(got_i.cpu(), dim=-1) @ torch.nn.functional.normalize(got_t.cpu(), dim=-1).T
        assert (sims_ref - sims_got).abs().max() < smax, (dt, float((sims_ref - sims_got).abs().max()))


def test_fp16_operand_kernels():
    """The fp16 instantiations of the GEMM (every epilogue, big ping-pong path and small ring path) and of the attention kernel
    against fp64 references: same structure as the bf16 kernels, IEEE fp16 operands / outputs (the ranker's reference dtype)."""
    from univid_amd._lib import EPI_BF16, EPI_BF16_T, EPI_F32_FROM_BF16, EPI_GELU_BF16, EPI_RESID_F32
    F16 = torch.float16

    def ulp16(x):
        return torch.ldexp(torch.ones_like(x), torch.floor(torch.log2(x.abs().clamp_min(6.2e-5))) - 10)

    for (M, N, K) in [(300, 512, 256), (4100, 1024, 768)]:
        g = torch.Generator(device=DEV).manual_seed(M)
        a = (torch.randn(M, K, generator=g, device=DEV) * 0.5).to(F16)
        w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(F16)
        bias = (torch.randn(N, generator=g, device=DEV) * 0.1).to(F16)
        acc = a.double() @ w.double().t() + bias.double()
        y16 = acc.to(F16)
        out = torch.zeros(M, N, dtype=F16, device=DEV)
        L().gemm_bf16(a, w, bias, out, EPI_BF16)
        d = (out.double() - acc).abs()
        assert (d <= 0.51 * ulp16(acc.float()).double() + 2e-5 * acc.abs().max()).all(), f"f16 gemm {M}x{N}x{K}: {float(d.max()):.3e}"
        assert (out == y16).float().mean() > 0.999
        L().gemm_bf16(a, w, bias, out, EPI_GELU_BF16)
        ref = torch.nn.functional.gelu(y16.float(), approximate="tanh")
        assert ((out.float() - ref).abs() <= 1.0 * ulp16(ref) + 1.2 * ulp16(y16.float()) + 2e-5 * ref.abs().max()).all()
        o32 = torch.zeros(M, N, dtype=torch.float32, device=DEV)
        L().gemm_bf16(a, w, bias, o32, EPI_F32_FROM_BF16)
        assert (o32 == y16.float()).float().mean() > 0.999
        x0 = torch.randn(M, N, generator=g, device=DEV)
        x = x0.clone()
        L().gemm_bf16(a, w, bias, x, EPI_RESID_F32)
        assert ((x - (x0 + y16.float())).abs() <= ulp16(y16.float()) + 1e-6).all()
        outT = torch.zeros(N, (M + 63) // 64 * 64, dtype=F16, device=DEV)
        L().gemm_bf16(a, w, bias, outT, EPI_BF16_T)
        assert (outT[:, :M] == y16.t()).float().mean() > 0.999 and (outT[:, M:] == 0).all()
        with pytest.raises(Exception):
            L().gemm_bf16(a, w, bias, out, EPI_BF16, tile_cfg=5)           # explicit tile configs are bf16-only
    for (Lq, Lk, H, D) in [(300, 300, 2, 64), (1, 256, 12, 64), (260, 200, 2, 128)]:
        g = torch.Generator(device=DEV).manual_seed(Lq + Lk)
        C = H * D
        q, k, v = (torch.randn(n, C, generator=g, device=DEV).to(F16) for n in (Lq, Lk, Lk))
        qf, kf, vf = (t.double().view(-1, H, D).transpose(0, 1) for t in (q, k, v))
        truth = (torch.softmax(qf @ kf.transpose(1, 2) / math.sqrt(D), -1) @ vf).transpose(0, 1).reshape(Lq, C)
        vt = torch.zeros(C, (Lk + 63) // 64 * 64, dtype=F16, device=DEV)
        vt[:, :Lk] = v.t()
        out = torch.zeros(Lq, C, dtype=F16, device=DEV)
        L().flash_attn(q, k, vt, out, Lq, Lk, H, D, 1.0 / math.sqrt(D))
        err = (out.double() - truth).abs()
        assert (err <= 3 * ulp16(truth.float()).double() + 5e-4 * truth.abs().max()).all(), f"f16 attention: {float(err.max()):.3e}"


def test_context_projector_vs_reference_golden():
    """univid_amd.model_pipeline.ContextProjector (HIP) against the outputs of the reference's own class (model_pipeline.py:1506-
    1574, bf16 module): token counts equal to / below / above the target length (linear resampling of the token axis)."""
    import types
    from oracle import projector
    from univid_amd.model_pipeline import ContextProjector
    g = load_golden("context_projector")
    cfg = types.SimpleNamespace(bagel_hidden_dim=128, wan_text_dim=256, wan_text_length=32, use_semantic_alignment=False)
    m = ContextProjector(cfg)
    m.load_state_dict(projector.make_state_dict(128, 256, int(g["seed"])))
    m = m.to(DEV).eval()
    for L in (32, 20, 77):
        outs = m(g[f"tokens_{L}"])
        assert len(outs) == 2 and all(o.shape == (32, 256) and o.dtype == BF16 for o in outs)
        got, ref = torch.stack(outs).float().cpu(), g[f"out_{L}"].float()
        d = (got - ref).abs()
        rel_rms = float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        # six bf16-rounded stages (Linear, LayerNorm, GELU, Linear, LayerNorm, resampling): a one-ulp flip early on moves a
        # LayerNorm row by a few ulps, so the gate is rms error + a bound in ulps of the OUTPUT RANGE + the bit-identical share
        assert rel_rms < 1.5e-3 and float(d.max()) <= 4 * float(bf16_ulp(ref.abs().max())), f"L={L}: rel rms {rel_rms:.2e}, max {float(d.max()):.2e}"
        if L == 32:
            assert (d == 0).float().mean() > 0.9, f"only {float((d == 0).float().mean()):.4f} bit-identical"
        else:
            # the resampling kernel alone: bit-exact against F.interpolate on the same bf16 rows
            cfg.wan_text_length = L
            pre = torch.stack(m(g[f"tokens_{L}"])).cpu()
            cfg.wan_text_length = 32
            want = torch.nn.functional.interpolate(pre.transpose(1, 2), size=32, mode="linear", align_corners=False).transpose(1, 2)
            assert torch.equal(torch.stack(outs).cpu(), want), f"L={L} interpolation"
    m.train()
    with pytest.raises(NotImplementedError):
        m(g["tokens_32"])


def test_umt5_encoder_vs_reference_golden():
    """univid_amd.wan.t5.T5Encoder (HIP) against the reference T5Encoder's bf16 outputs (t5.py:267-312): prompts of 48, 33 and 5
    tokens (the latter two padded + masked in the reference). The kernels keep the reference's rounding points, so most elements
    are bit-identical; GEMM accumulation order accounts for the rest."""
    from oracle import t5 as ot5
    from univid_amd.wan.t5 import T5Encoder, T5EncoderModel
    g = load_golden("t5_tiny")
    cfg = ot5.TINY_CFG
    m = T5Encoder(vocab=cfg["vocab_size"], dim=cfg["dim"], dim_attn=cfg["dim_attn"], dim_ffn=cfg["dim_ffn"], num_heads=cfg["num_heads"],
                  num_layers=cfg["num_layers"], num_buckets=cfg["num_buckets"])
    m.load_state_dict(ot5.make_state_dict(cfg, int(g["seed"])))
    m = m.to(device=DEV, dtype=BF16).eval()
    assert torch.equal(m.blocks[0].pos_embedding.bucket(g["rel"].to(DEV)).cpu(), g["buckets"])
    for n in (48, 33, 5):
        got, ref = m.encode(g[f"ids_{n}"]).float().cpu(), g[f"out_{n}"].float()
        d = (got - ref).abs()
        rel_rms = float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        assert rel_rms < 3e-3 and float(d.max()) <= 6 * float(bf16_ulp(ref.abs().max())), f"n={n}: rel rms {rel_rms:.2e} max {float(d.max()):.2e}"
        assert (d == 0).float().mean() > 0.8, f"n={n}: only {float((d == 0).float().mean()):.3f} bit-identical"
    # reference-signature forward and the T5EncoderModel wrapper (tokenizer injected)
    ids = torch.zeros(2, 48, dtype=torch.long)
    ids[0, :33], ids[1, :5] = g["ids_33"], g["ids_5"]
    mask = torch.stack([(torch.arange(48) < 33).long(), (torch.arange(48) < 5).long()])
    full = m(ids.to(DEV), mask.to(DEV))
    assert full.shape == (2, 48, cfg["dim"]) and (full[0, 33:] == 0).all() and torch.equal(full[1, :5], m.encode(g["ids_5"]))
    enc = T5EncoderModel(text_len=48, device=DEV, model=m, tokenizer=lambda texts, **kw: (ids, mask))
    ctx = enc(["a", "b"], DEV)
    assert [c.shape[0] for c in ctx] == [33, 5] and torch.equal(ctx[0], full[0, :33])


def test_pipeline_composes_native_text_encoder_projector_dit():
    """CrossAttentionFusionPipeline.generate_video_with_bagel_context (model_pipeline.py:2577-2655) with every stage native: prompt ->
    tokenizer (injected) -> umT5 encoder on HIP -> contexts; BAGEL tokens (stub extractor) -> ContextProjector on HIP; tiny DiT + UniPC
    loop with the per-layer text-weight hook. The result must equal the same loop driven with the encoder's embeddings passed in
    directly, be deterministic, and differ from the run without the dynamic text weight."""
    import types
    from oracle import projector, t5 as ot5
    from univid_amd.model_pipeline import ContextProjector, CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.t5 import T5Encoder, T5EncoderModel
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g5 = load_golden("t5_tiny")
    tcfg = ot5.TINY_CFG
    enc_m = T5Encoder(vocab=tcfg["vocab_size"], dim=tcfg["dim"], dim_attn=tcfg["dim_attn"], dim_ffn=tcfg["dim_ffn"], num_heads=tcfg["num_heads"],
                      num_layers=tcfg["num_layers"], num_buckets=tcfg["num_buckets"])
    enc_m.load_state_dict(ot5.make_state_dict(tcfg, int(g5["seed"])))
    prompts = {"a cat": g5["ids_33"], "": g5["ids_5"]}

    def tokenizer(texts, **kw):
        ids = torch.zeros(len(texts), 48, dtype=torch.long)
        mask = torch.zeros(len(texts), 48, dtype=torch.long)
        for i, t in enumerate(texts):
            n = prompts[t].numel()
            ids[i, :n], mask[i, :n] = prompts[t], 1
        return ids, mask

    enc = T5EncoderModel(text_len=48, device=DEV, model=enc_m, tokenizer=tokenizer)
    cfg, sd, m = _tiny_model(load_golden("dit_tiny")["seed"], text_dim=tcfg["dim"], text_len=48)
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV, text_encoder=enc)
    pipe.sample_neg_prompt = ""
    pcfg = types.SimpleNamespace(bagel_hidden_dim=128, wan_text_dim=tcfg["dim"], wan_text_length=32, use_semantic_alignment=False)
    proj = ContextProjector(pcfg)
    proj.load_state_dict(projector.make_state_dict(128, tcfg["dim"], 3))
    proj = proj.to(DEV).eval()
    bagel = types.SimpleNamespace(extract_semantic_tokens=lambda text, image: torch.randn(1, 20, 128, generator=torch.Generator().manual_seed(1)))
    ccfg = CrossAttentionConfig(total_sampling_steps=3, text_weight_transition_ratio=0.7, use_dynamic_text_weight=True, bagel_sequence_length=16)
    fusion = CrossAttentionFusionPipeline(ccfg, wan_pipeline=pipe, bagel_extractor=bagel, context_projector=proj)
    kw = dict(steps=3, guidance_scale=5.0, frames=13, size=(256, 256), shift=5.0, seed=11, decode=False)
    with torch.no_grad():
        lat, path = fusion.generate_video_with_bagel_context("a cat", **kw)
        lat2, _ = fusion.generate_video_with_bagel_context("a cat", **kw)
        emb, emb_n = enc(["a cat"], DEV), enc([""], DEV)
        lat3, _ = fusion.generate_video_with_bagel_context("ignored", prompt_embeds=emb, negative_prompt_embeds=emb_n, **kw)
    assert path is None and lat.shape == (48, 4, 16, 16) and torch.isfinite(lat).all()
    assert torch.equal(lat, lat2) and torch.equal(lat, lat3)
    assert emb[0].shape == (33, tcfg["dim"]) and emb_n[0].shape == (5, tcfg["dim"])
    assert fusion.get_fusion_info()["hooked_layers"] == cfg["num_layers"] and not fusion.wan_wrapper.use_bagel_context
    fusion.cleanup_resources()
    plain = CrossAttentionFusionPipeline(CrossAttentionConfig(total_sampling_steps=3, use_dynamic_text_weight=False), wan_pipeline=pipe,
                                         bagel_extractor=bagel, context_projector=proj)
    with torch.no_grad():
        lat4, _ = plain.generate_video_with_bagel_context("a cat", **kw)
    assert torch.isfinite(lat4).all() and not torch.equal(lat, lat4)
    plain.cleanup_resources()


def test_bench_multi_rank_branch_runs_with_two_ranks_sharing_the_gpu():
    """bench.py's N > 1 branch - the bare `--gpus N` launcher (a child torch.distributed.run started before the parent touches the GPU), one rank per
    process, the barrier-bracketed timed region, the all-gather of the final latents, the max-over-ranks time, the per-rank HIP-event split and
    the ranks' host policy (blocking sync; `--host-sync blocking` adds AMD_DIRECT_DISPATCH=0) - has never met a multi-GPU box in six rounds. Here it runs for real on this
    box's single GPU: two ranks on cuda:0 over gloo (UV_BENCH_SHARE_GPU=1, a test hook the line itself labels), 2 DiT blocks, 2 timed steps.
    Checks the contract of the ONE JSON line rank 0 prints; the numbers are not a measurement."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, UV_BENCH_SHARE_GPU="1")
    env.pop("AMD_DIRECT_DISPATCH", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--layers", "2", "--no-cpu-baseline",
                        "--host-sync", "blocking"], env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-400:], r.stderr[-800:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["finite"] is True
    assert d["metric"] == "denoise_steps_per_sec" and d["value"] > 0 and abs(d["value"] - 2 * 2 / (d["ms_per_step"] * 2 / 1e3)) < 1e-2 * d["value"]
    assert d["rccl_ranks"] == 0 and "UV_BENCH_SHARE_GPU" in d["transport"]
    assert d["host_env"]["AMD_DIRECT_DISPATCH"] == "0" and d["host_sync"] == "blocking"      # (auto leaves the dispatch mode alone)
    pr = d["per_rank"]
    assert [x["rank"] for x in pr["ranks"]] == [0, 1]
    assert all(x["ms_per_step"] > 0 and x["allgather_us"] is not None and x["allgather_us"] >= 0 for x in pr["ranks"])
    assert pr["ms_per_step_max"] <= d["ms_per_step"] * 1.05 and pr["allgather_us_max"] is not None
    assert "pipeline_path" not in d and d["cpu_baseline"] is None
