"""GPU (-m gpu): the text side - umT5-XXL encoder and ContextProjector kernels - at production width.

tests/test_gpu_parity.py checks these stages at toy width only (dim 256, 4 heads, prompts <= 48 tokens, a 128 -> 512 -> 256 projector).
The production path runs code that width never reaches: T5 attention key groups >= 1 and relative positions past the bucket clamp,
the C = 4096 RMSNorm and the C = 4096 / 8192 LayerNorm instantiations (64 KB of LDS staging at 8192), grid-stride loops that iterate,
the resampling at 512 rows, and the GEMM paths at K = 10 240 and at the projector's M x 8192 x 3584. Every kernel here is compared
with a plain high-precision reference of the same operation (fp64 where the operation has no intermediate rounding, the reference's
rounding points spelled out otherwise); the two modules against the CPU oracle and a no-rounding fp64 truth run, with the gates of
test_gpu_parity.py's header (measured on MI355X x 1.2; the measured values go to the margins file through `record_margin`).
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import bf16_ulp, record_margin
from test_gpu_parity import assert_bf16_kernel, assert_model_close

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()
    # the CPU oracles below are GEMM-heavy: no more intra-op threads than the job was given (OMP_NUM_THREADS), restored afterwards
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(n, int(os.environ.get("OMP_NUM_THREADS", n)))))
    yield
    torch.set_num_threads(n)


@pytest.fixture(autouse=True)
def _default_options():
    from univid_amd import _lib
    _lib.reset_options()
    yield
    _lib.reset_options()


def L():
    from univid_amd import _lib
    return _lib


def _round_up(a, b):
    return (a + b - 1) // b * b


def _record_bf16(name, got, ref):
    """Measured agreement of a bf16 kernel with its oracle: bit-identical share, share beyond 1 ulp, largest error in ulps."""
    got, ref = got.float().cpu(), ref.float().cpu()
    d = (got - ref).abs()
    ulp = bf16_ulp(torch.maximum(ref.abs(), got.abs()))
    record_margin(name, exact_frac=(d == 0).float().mean(), over_1ulp_frac=(d > ulp).float().mean(), max_err_ulp=(d / ulp).max(),
                  numel=d.numel())


# ---------------------------------------------------------------------------------------------------------------
# umT5 attention
# ---------------------------------------------------------------------------------------------------------------
H5 = 64          # umT5-XXL heads (head_dim 64)


def _t5_bias_weight():
    """[32 buckets, 64 heads] bf16 relative-position embedding as oracle.t5.make_state_dict builds it (x 4: visible biases)."""
    from univid_amd import detinit
    w = torch.empty(32, H5)
    detinit.fill_("blocks.0.pos_embedding.embedding.weight", w, 5)
    return (w * 4.0).to(BF16)


def _t5_attention_oracle(q, k, v, bw, n):
    """The reference's rounding points (oracle/t5.py encode): bf16(q.k), bf16(+ bias), softmax normalised before its bf16 rounding,
    bf16(P.V) - each operation evaluated in fp64 and rounded once, on the CPU. Also the fp64 truth (no intermediate rounding).
    q, k, v: [n, 64 * H] bf16 CPU -> ([n, 64 * H] bf16, [n, 64 * H] fp64)."""
    from oracle import t5 as ot5
    rel = torch.arange(n).unsqueeze(0) - torch.arange(n).unsqueeze(1)          # key - query
    e = bw[ot5.relative_position_bucket(rel)].permute(2, 0, 1)                  # [H, n, n] bf16
    out, truth = torch.empty(n, H5 * 64, dtype=BF16), torch.empty(n, H5 * 64, dtype=torch.float64)
    for h0 in range(0, H5, 16):
        cs = slice(h0 * 64, (h0 + 16) * 64)
        qh, kh, vh = (t[:, cs].double().view(n, 16, 64).transpose(0, 1) for t in (q, k, v))
        s64 = qh @ kh.transpose(1, 2)
        eh = e[h0:h0 + 16]
        s = (s64.to(BF16).float() + eh.float()).to(BF16)
        p = torch.softmax(s.double(), -1).to(BF16)
        out[:, cs] = (p.double() @ vh).to(BF16).transpose(0, 1).reshape(n, -1)
        truth[:, cs] = (torch.softmax(s64 + eh.double(), -1) @ vh).transpose(0, 1).reshape(n, -1)
    return out, truth


def _t5_attention_call(q, k, v, out, n, table, span):
    _lib = L()
    _lib.call("uv_t5_attention_bf16", _lib.ptr(q), q.stride(0), _lib.ptr(k), k.stride(0), _lib.ptr(v), v.stride(0), _lib.ptr(out),
              out.stride(0), n, H5, _lib.ptr(table), span, _lib.stream_ptr())


@pytest.mark.parametrize("n,span", [(n, _round_up(n, 512)) for n in (1, 5, 63, 64, 65, 127, 128, 129, 333, 511, 512, 700, 1024)] + [(77, 1024)])
def test_t5_attention_production_shapes(n, span):
    """uv_t5_attention_bf16 at umT5-XXL's 64 heads for prompts up to the kernel's 1024 keys: every key group of the 16 unrolled ones,
    relative positions past the bucket clamp (|r| >= 128), span = round_up(n, 512) as T5Encoder.encode passes it, and a span larger
    than that. q / k / v / out are column slices of wider buffers (ld != C, the layout of a fused QKV projection); the output buffer's
    other columns must come back untouched. Per-head score standard deviations from 0.3 to 3.1 cover flat and peaked softmax.

    Gate: >= 99.9 % bit-identical, every element within 1 bf16 ulp of the oracle except a `rare` share. The kernel sums q.k in fp32
    (the reference on its GPU too), the oracle in fp64: now and then that flips the bf16 rounding of a score, which moves its
    probability by exp(1 ulp of the score) - 2^-4 relative at |scores| >= 8 in the peaked heads - and the second rounding
    point (bf16 P) carries it into the output. Measured on MI355X: at most 1.16e-4 of the elements beyond 1 ulp (n = 1024; 0 for
    n < 64), their error at most 3.1e-2 (n = 128) on values of unit rms; bit-identical >= 99.93 %. Gate: measured x 1.2 (1.4e-4 of
    the elements may exceed the 1-ulp bound, by at most 0.0375). The rms error against the fp64 truth equals the oracle's own
    (ratio 0.9998-1.00005; gate 1.02)."""
    from univid_amd.wan.t5 import T5RelativeEmbedding
    C = H5 * 64
    g = torch.Generator().manual_seed(1000 + n)
    hs = torch.linspace(0.2, 0.62, H5).repeat_interleave(64)                     # q.k std 8 s^2 per head
    qkv = torch.zeros(n, 3 * C + 16, dtype=BF16)
    qkv[:, :C] = (torch.randn(n, C, generator=g) * hs).to(BF16)
    qkv[:, C:2 * C] = (torch.randn(n, C, generator=g) * hs).to(BF16)
    qkv[:, 2 * C + 8:3 * C + 8] = torch.randn(n, C, generator=g).to(BF16)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C + 8:3 * C + 8]
    bw = _t5_bias_weight()
    emb = T5RelativeEmbedding(32, H5).to(DEV)
    emb.embedding.weight.data = bw.to(DEV)
    table = emb.table(span)
    assert table.shape == (H5, 2 * span - 1) and table.dtype == torch.float32
    qkv_d = qkv.to(DEV)
    buf = torch.full((n, C + 64), 7.0, dtype=BF16, device=DEV)
    out = buf[:, 32:32 + C]
    _t5_attention_call(qkv_d[:, :C], qkv_d[:, C:2 * C], qkv_d[:, 2 * C + 8:3 * C + 8], out, n, table, span)
    torch.cuda.synchronize()
    b = buf.cpu()
    assert (b[:, :32] == 7.0).all() and (b[:, 32 + C:] == 7.0).all(), "columns outside the output slice were written"
    ref, truth = _t5_attention_oracle(q, k, v, bw, n)
    got = out.cpu()
    _record_bf16(f"t5 attention n={n} span={span}", got, ref)
    e_hip = (got.double() - truth).pow(2).mean().sqrt().item()
    e_ora = (ref.double() - truth).pow(2).mean().sqrt().item()
    record_margin(f"t5 attention n={n} span={span} vs fp64 truth", rms_vs_truth_hip=e_hip, rms_vs_truth_oracle=e_ora,
                  truth_ratio=e_hip / max(e_ora, 1e-30))
    assert_bf16_kernel(got, ref, max_ulp=1.0, min_exact=0.999, name=f"t5 attention n={n}", rare=(1.4e-4, 0.0375))
    assert e_hip <= 1.02 * e_ora + 1e-7, f"n={n}: rms vs truth {e_hip:.3e}, oracle's own {e_ora:.3e}"


def test_t5_attention_rejects_bad_shapes():
    """n above the kernel's 1024 keys, or a bias table shorter than the prompt, must fail in the entry point (before any launch)."""
    from univid_amd._lib import UnividHipError
    n, C = 1025, H5 * 64
    q = torch.zeros(n, C, dtype=BF16, device=DEV)
    out = torch.full((n, C), 3.0, dtype=BF16, device=DEV)
    table = torch.zeros(H5, 2 * 1024 - 1, device=DEV)
    with pytest.raises(UnividHipError):
        _t5_attention_call(q, q, q, out, 1025, table, 1024)
    with pytest.raises(UnividHipError):
        _t5_attention_call(q, q, q, out, 600, table, 512)            # span < n
    with pytest.raises(UnividHipError):
        _t5_attention_call(q, q, q, out, 0, table, 512)
    torch.cuda.synchronize()
    assert (out == 3.0).all()


def test_t5_relative_buckets_full_range():
    """T5RelativeEmbedding.bucket on the device for every relative position a 1024-token prompt has (the golden covers +-200 only)."""
    from oracle import t5 as ot5
    from univid_amd.wan.t5 import T5RelativeEmbedding
    rel = torch.arange(-1023, 1024)
    got = T5RelativeEmbedding(32, H5).to(DEV).bucket(rel.to(DEV)).cpu()
    assert torch.equal(got, ot5.relative_position_bucket(rel))
    assert got.min() == 0 and got.max() == 31


# ---------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------
def _heavy_rows(Lr, C, g):
    """Rows of different scales (2^-6 ... 2^6) with heavy-tailed values (a Student-t-like mix: a few entries 20-50x the row's rms)."""
    x = torch.randn(Lr, C, generator=g) * torch.exp2(torch.randint(-6, 7, (Lr, 1), generator=g).float())
    spikes = torch.rand(Lr, C, generator=g) < 2e-3
    return torch.where(spikes, x * (20 + 30 * torch.rand(Lr, C, generator=g)), x)


@pytest.mark.parametrize("Lr", [1, 77, 512, 4100])
def test_umt5_rmsnorm_c4096(Lr):
    """uv_rmsnorm_rope without RoPE at umT5's C = 4096 (D = 64) - the <8,1,true> instantiation, and <8,4,true> at L >= 4096 (4100:
    a partial last block) - against oracle.t5._norm, the reference's T5LayerNorm on bf16 (fp32 statistics, bf16 normalised value,
    bf16 weight product). The weight is fp32 holding the bf16 parameter, as T5Encoder passes it.

    The normalised value is rounded to bf16 before the weight product: a rounding flip there (fp32 sum-of-squares order) moves the
    output by 1 ulp of the intermediate times |w| (up to ~2.5 here), i.e. up to 2 output ulps. Measured on MI355X: 1.8e-6 of the
    elements beyond 1 ulp (L = 4100; 1e-6 at 512, 0 at 1 and 77), never beyond 2 ulps; gate rare = (2.2e-6, 1 ulp)."""
    from oracle import t5 as ot5
    C = 4096
    g = torch.Generator().manual_seed(Lr)
    x = _heavy_rows(Lr, C, g).to(BF16)
    w = (1 + 0.5 * torch.randn(C, generator=g)).to(BF16)
    y = torch.full((Lr, C), 5.0, dtype=BF16, device=DEV)
    L().rmsnorm_rope(x.to(DEV), y, w.float().to(DEV), Lr, C, 64, 1e-6)
    ref = ot5._norm(x, w)
    _record_bf16(f"umT5 rmsnorm C=4096 L={Lr}", y, ref)
    assert_bf16_kernel(y, ref, name=f"umT5 rmsnorm L={Lr}", rare=(2.2e-6, bf16_ulp(ref.float())))


def _ln_rows(Lr, C, g):
    """bf16-valued fp32 rows (the projector's GEMM output held as fp32): row 0 offset by +1000 with a few +-60 outliers (a one-pass
    E[x^2] - E[x]^2 variance loses it in fp32), the rest of different scales."""
    x = torch.randn(Lr, C, generator=g) * torch.exp2(torch.randint(-4, 5, (Lr, 1), generator=g).float())
    x[0] = 1000.0 + torch.randn(C, generator=g)
    idx = torch.randint(0, C, (8,), generator=g)
    x[0, idx] += 60.0 * torch.sign(torch.randn(8, generator=g))
    return x.to(BF16).float()


@pytest.mark.parametrize("C", [4096, 8192])
@pytest.mark.parametrize("Lr", [1, 5, 77, 512, 2300])
def test_layernorm_mod_projector_widths(C, Lr):
    """uv_layernorm_mod at the projector's C = 8192 (<32,1>: 32 float4 per lane, 64 KB of dynamic LDS staging w|b) and 4096 (<16,1>):
    mode 2 with affine w / b whose two halves are drawn differently (staging only part of the LDS would show), bf16 output as the
    projector calls it, and mode 0 with bf16 and f32 outputs. Oracle: F.layer_norm in fp64 (-> bf16 for bf16 outputs).

    Row 0 sits at mean 1000: its fp32 mean (ours and torch's alike) is off by ~1e-4 of the unit-scale result, which flips a bf16
    rounding on a few % of that row; its bit-identical share is gated separately (>= 95 %), every element of every row within 1 ulp
    (+ the 2e-5 x range floor: where y * w cancels against b the result is many ulps OF ITSELF off; measured up to 11). f32 output of
    mode 0, measured on MI355X: max error 1.5e-5 on the offset row, 1.2e-6 elsewhere; gates x 1.2."""
    g = torch.Generator().manual_seed(C + Lr)
    x = _ln_rows(Lr, C, g)
    h = C // 2
    w = torch.cat([1 + 0.3 * torch.randn(h, generator=g), -0.5 + 0.1 * torch.randn(h, generator=g)]).to(BF16).float()
    b = torch.cat([0.2 * torch.randn(h, generator=g), 3.0 + 0.5 * torch.randn(h, generator=g)]).to(BF16).float()
    xd = x.to(DEV)
    ref_aff = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
    ref_plain = F.layer_norm(x.double(), (C,), None, None, 1e-5)
    for mode, ref, dt in ((2, ref_aff, BF16), (0, ref_plain, BF16), (0, ref_plain, torch.float32)):
        out = torch.full((Lr, C), 9.0, dtype=dt, device=DEV)
        if mode == 2:
            L().layernorm_mod(xd, out, Lr, C, 1e-5, mode=2, w=w.to(DEV), b=b.to(DEV))
        else:
            L().layernorm_mod(xd, out, Lr, C, 1e-5, mode=0)
        got = out.cpu()
        name = f"layernorm_mod C={C} L={Lr} mode {mode} {str(dt)[6:]}"
        if dt == BF16:
            rb = ref.to(BF16)
            _record_bf16(name, got, rb)
            assert_bf16_kernel(got[:1], rb[:1], min_exact=0.95, name=name + " (offset row)")
            if Lr > 1:
                assert_bf16_kernel(got[1:], rb[1:], name=name)
        else:
            err = (got.double() - ref).abs()
            record_margin(name, max_abs_err_row0=err[0].max(), max_abs_err_rest=err[1:].max() if Lr > 1 else 0.0)
            assert err[0].max() <= 1.8e-5, f"{name}: offset row max err {float(err[0].max()):.3e}"
            if Lr > 1:
                assert err[1:].max() <= 1.5e-6, f"{name}: max err {float(err[1:].max()):.3e}"


# ---------------------------------------------------------------------------------------------------------------
# elementwise glue, in place
# ---------------------------------------------------------------------------------------------------------------
def _gate_cpu_gpu(name, got, cpu_ref, gpu_ref, well=None):
    """>= 99.9 % bit-identical and <= 1 ulp against the oracle on the CPU and against the same torch expression on the GPU (the
    reference's device); where CPU and GPU torch themselves disagree, that share is recorded. `well`: the elements where the CPU
    oracle is well-conditioned - only there is the bit-identical share against it gated (the 1-ulp bound holds everywhere)."""
    got, gpu_ref = got.cpu(), gpu_ref.cpu()
    record_margin(name + ": cpu torch vs gpu torch", differ_frac=(cpu_ref.float() != gpu_ref.float()).float().mean())
    _record_bf16(name + " vs cpu torch", got, cpu_ref)
    _record_bf16(name + " vs gpu torch", got, gpu_ref)
    if well is None:
        assert_bf16_kernel(got, cpu_ref, name=name + " vs cpu torch")
    else:
        assert_bf16_kernel(got, cpu_ref, min_exact=0.0, name=name + " vs cpu torch")
        exact = (got[well] == cpu_ref[well]).float().mean().item()
        record_margin(name + " vs cpu torch, well-conditioned", exact_frac=exact)
        assert exact >= 0.999, f"{name}: only {exact:.5f} bit-identical with the CPU oracle where it is well-conditioned"
    assert_bf16_kernel(got, gpu_ref, name=name + " vs gpu torch")


@pytest.mark.parametrize("n", [512 * 10240, 1_048_583])
def test_t5_gated_gelu_and_add_production_sizes(n):
    """uv_t5_gated_gelu_bf16 (in place over fc1, as T5Encoder calls it) and uv_add_bf16 (in place over x) on umT5's 512 x 10240 FFN
    activation and an odd length > 1 M: grids capped at 4096 blocks, so every thread's grid-stride loop iterates. Oracle: the
    reference's op-by-op bf16 GELU (oracle.t5._gelu) times fc1 on CPU bf16 tensors, and x + y. Measured on MI355X: bit-identical
    to both the CPU and the GPU evaluation (which agree with each other), so the add is gated bit-exact."""
    from oracle import t5 as ot5
    g = torch.Generator().manual_seed(n)
    gate = (torch.randn(n, generator=g) * 2.0).to(BF16)
    fc1 = torch.randn(n, generator=g).to(BF16)
    gd, fd = gate.to(DEV), fc1.to(DEV)
    gpu_ref = fd * ot5._gelu(gd)
    _lib = L()
    _lib.call("uv_t5_gated_gelu_bf16", _lib.ptr(gd), _lib.ptr(fd), _lib.ptr(fd), n, _lib.stream_ptr())
    _gate_cpu_gpu(f"t5 gated gelu n={n}", fd, fc1 * ot5._gelu(gate), gpu_ref)
    x = torch.randn(n, generator=g).to(BF16)
    y = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 4, (n,), generator=g).float())).to(BF16)
    xd, yd = x.to(DEV), y.to(DEV)
    gpu_sum = xd + yd
    _lib.call("uv_add_bf16", _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(xd), n, _lib.stream_ptr())
    assert torch.equal(xd.cpu(), x + y) and torch.equal(xd, gpu_sum)


@pytest.mark.parametrize("n", [2300 * 8192, 1_048_583, 3])
def test_gelu_erf_production_sizes(n):
    """uv_gelu_erf_bf16 in place (the projector's y1) on 2300 x 8192 (grid-stride loop iterates) and odd lengths (the scalar tail
    branch, alone at n = 3). Oracle: F.gelu (erf) on bf16 tensors, CPU and GPU.

    CPU and GPU torch DISAGREE here: measured on the MI355X box, CPU torch's bf16 GELU differs from GPU torch's on 2.8 % of these
    elements, all in the tail x < -3 where 1 + erf(x / sqrt 2) cancels (results below 5e-3 of the range; errors up to 85 ulps of such a
    result, inside the 2e-5 x range floor). The kernel is bit-identical to GPU torch - the reference's device - on every element;
    against the CPU it is gated bit-identical where x > -3 and within the 1-ulp bound everywhere."""
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 3.0).to(BF16)
    xd = x.to(DEV)
    gpu_ref = F.gelu(xd)
    _lib = L()
    _lib.call("uv_gelu_erf_bf16", _lib.ptr(xd), _lib.ptr(xd), n, _lib.stream_ptr())
    _gate_cpu_gpu(f"gelu erf n={n}", xd, F.gelu(x), gpu_ref, well=x.float() > -3)


# ---------------------------------------------------------------------------------------------------------------
# resampling
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lin,Lout", [(Lin, 512) for Lin in (1, 2, 77, 128, 129, 333, 511, 513, 700, 2300)] + [(700, 300)])
def test_interp_linear_rows_c4096(Lin, Lout):
    """uv_interp_linear_rows_bf16 at the projector's C = 4096 resampling L BAGEL tokens to wan_text_length 512 rows (and one downsample
    to 300), against oracle.projector.interpolate_rows(..., "device") - fp32 index, weights and blend, one bf16 rounding: what
    the reference's op computes on its GPU - and against torch's own F.interpolate on the GPU bf16 tensor.

    Measured on MI355X: bit-identical to both at every Lin -> 512 (the scale Lin / 512 is exact in fp32, so source index and weights
    carry few bits, both products w0 * a and w1 * b are exact and every evaluation order of the blend gives the same value). At
    700 -> 300 the weights carry full 24-bit mantissas and the kernel's two separately rounded products (-ffp-contract=off) differ
    from torch's evaluation of the blend (CPU and GPU alike) on 1.2e-4 of the elements by one bf16 rounding; gate: 1 ulp everywhere,
    bit-identical >= 1 - 1.2 x 1.2e-4."""
    from oracle import projector
    C = 4096
    x = torch.randn(Lin, C, generator=torch.Generator().manual_seed(Lin)).to(BF16)
    xd = x.to(DEV)
    out = torch.empty(Lout, C, dtype=BF16, device=DEV)
    _lib = L()
    _lib.call("uv_interp_linear_rows_bf16", _lib.ptr(xd), xd.stride(0), _lib.ptr(out), out.stride(0), Lin, Lout, C, _lib.stream_ptr())
    ref = projector.interpolate_rows(x.unsqueeze(0), Lout, "device")[0]
    gpu = F.interpolate(xd.t().unsqueeze(0), size=Lout, mode="linear", align_corners=False)[0].t().cpu()
    got = out.cpu()
    _record_bf16(f"interp {Lin}->{Lout} vs device oracle", got, ref)
    _record_bf16(f"interp {Lin}->{Lout} vs gpu F.interpolate", got, gpu)
    record_margin(f"interp {Lin}->{Lout}: device oracle vs gpu F.interpolate", differ_frac=(ref.float() != gpu.float()).float().mean())
    min_exact = 1.0 if Lout == 512 else 0.99985
    assert_bf16_kernel(got, ref, min_exact=min_exact, name=f"interp {Lin}->{Lout}")
    assert_bf16_kernel(got, gpu, min_exact=min_exact, name=f"interp {Lin}->{Lout} vs gpu F.interpolate")


# ---------------------------------------------------------------------------------------------------------------
# GEMM at the text-side shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 4096, 4096), (77, 10240, 4096), (512, 10240, 4096), (512, 4096, 10240),
                                   (77, 8192, 3584), (1100, 8192, 3584), (2300, 8192, 3584), (512, 4096, 8192)])
def test_gemm_text_side_shapes(M, N, K):
    """uv_gemm_bf16_nt, tile_cfg 0 (automatic), bias, EPI_BF16 and EPI_F32_FROM_BF16 at the umT5 projections (K = 4096 / 10 240) and
    the projector's (M x 8192 x 3584: the 128x128 path, and at M = 2300 the persistent ping-pong kernel plus its leftover-row strip)
    against the fp64 product rounded once to bf16. Measured on MI355X: 99.958-100 % bit-identical, at most 2.7e-5 of the elements
    beyond 1 ulp and all of them inside the 2e-5 x range floor (results small through cancellation)."""
    from univid_amd._lib import EPI_BF16, EPI_F32_FROM_BF16
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(BF16).to(DEV)
    w = (torch.randn(N, K, generator=g) * (2.0 / math.sqrt(K))).to(BF16).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16).to(DEV)
    ref = (a.double() @ w.double().t() + bias.double()).to(BF16).cpu()
    out = torch.full((M, N), 5.0, dtype=BF16, device=DEV)
    L().gemm_bf16(a, w, bias, out, EPI_BF16)
    _record_bf16(f"gemm {M}x{N}x{K} EPI_BF16", out, ref)
    assert_bf16_kernel(out, ref, name=f"gemm {M}x{N}x{K} EPI_BF16")
    o32 = torch.full((M, N), 5.0, dtype=torch.float32, device=DEV)
    L().gemm_bf16(a, w, bias, o32, EPI_F32_FROM_BF16)
    o32 = o32.cpu()
    assert torch.equal(o32.to(BF16).float(), o32), "EPI_F32_FROM_BF16 must hold bf16-rounded values"
    assert torch.equal(o32, out.cpu().float())


# ---------------------------------------------------------------------------------------------------------------
# modules at production width
# ---------------------------------------------------------------------------------------------------------------
def _umt5_2layer_cfg():
    from oracle import t5 as ot5
    return dict(ot5.UMT5_XXL_CFG, num_layers=2, vocab_size=4096)


def _t5_truth(sd, cfg, ids, dev):
    """oracle.t5.encode without any bf16 rounding: the same forward in fp64 on `dev`."""
    from oracle import t5 as ot5
    w = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    H = cfg["num_heads"]
    x = w["token_embedding.weight"][ids.to(dev)]
    n = x.shape[0]
    rel = torch.arange(n).unsqueeze(0) - torch.arange(n).unsqueeze(1)
    buckets = ot5.relative_position_bucket(rel, cfg["num_buckets"]).to(dev)

    def norm(t, wt):
        return t * torch.rsqrt(t.pow(2).mean(dim=-1, keepdim=True) + 1e-6) * wt

    def gelu(t):
        return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t.pow(3))))

    for i in range(cfg["num_layers"]):
        p = f"blocks.{i}."
        e = w[p + "pos_embedding.embedding.weight"][buckets].permute(2, 0, 1)
        y = norm(x, w[p + "norm1.weight"])
        c = cfg["dim_attn"] // H
        q, k, v = (F.linear(y, w[p + f"attn.{nm}.weight"]).view(n, H, c) for nm in "qkv")
        a = torch.softmax(torch.einsum("inc,jnc->nij", q, k) + e, -1)
        x = x + F.linear(torch.einsum("nij,jnc->inc", a, v).reshape(n, H * c), w[p + "attn.o.weight"])
        y = norm(x, w[p + "norm2.weight"])
        x = x + F.linear(F.linear(y, w[p + "ffn.fc1.weight"]) * gelu(F.linear(y, w[p + "ffn.gate.0.weight"])), w[p + "ffn.fc2.weight"])
    return norm(x, w["norm.weight"])


@pytest.fixture(scope="module")
def umt5_2layer():
    from oracle import t5 as ot5
    from univid_amd.wan.t5 import T5Encoder
    cfg = _umt5_2layer_cfg()
    sd = ot5.make_state_dict(cfg, 21)
    with torch.device(DEV):
        m = T5Encoder(vocab=cfg["vocab_size"], dim=cfg["dim"], dim_attn=cfg["dim_attn"], dim_ffn=cfg["dim_ffn"], num_heads=cfg["num_heads"],
                      num_layers=cfg["num_layers"], num_buckets=cfg["num_buckets"])
    m.load_state_dict(sd)
    m = m.to(dtype=BF16).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(22)
    ids = {n: torch.randint(1, cfg["vocab_size"], (n,), generator=g) for n in (1, 77, 512)}
    yield cfg, sd, m, ids
    del m
    torch.cuda.empty_cache()


# measured on MI355X, gates by the rule of test_gpu_parity.py's header (see the test's docstring)
T5_GATES = {1: dict(frac=0.569, max_rel=0.0103), 77: dict(frac=0.146, max_rel=0.0218), 512: dict(frac=0.129, max_rel=0.0233)}


@pytest.mark.parametrize("n", [1, 77, 512])
def test_umt5_encoder_xxl_width(umt5_2layer, n):
    """T5Encoder.encode at umT5-XXL width (dim 4096, ffn 10 240, 64 heads, 32 buckets; 2 layers, vocabulary cut to 4096 rows) against
    oracle.t5.encode on the CPU (the reference's bf16 op-by-op forward) and an fp64 truth run of the same forward without rounding.

    Measured on MI355X (inside rtol 1e-3 / atol 1e-4 | max error / range | rms vs truth, HIP / oracle):
        n = 1     0.641 | 0.0086 | 1.0044
        n = 77    0.176 | 0.0181 | 0.991
        n = 512   0.155 | 0.0193 | 0.9986
    The low inside fractions are the reference's own arithmetic, not the kernels': at this width its bf16 rounding points put the
    ORACLE 6.6e-3 (n = 1) to 7.8e-2 (n = 512) rms from the unrounded result, rtol 1e-3 is a quarter of a bf16 ulp, and every
    GEMM accumulation-order flip propagates through two layers; the HIP result is exactly as far from the truth as the oracle (ratio
    <= 1.0044). Gates: fraction = the tighter of 1 - 1.2 x outside and inside / 1.2, max error x 1.2, truth ratio 1.02."""
    from oracle import t5 as ot5
    cfg, sd, m, ids = umt5_2layer
    got = m.encode(ids[n])
    assert got.shape == (n, cfg["dim"]) and got.dtype == BF16
    ref = ot5.encode(sd, cfg, ids[n])
    truth = _t5_truth(sd, cfg, ids[n], DEV)
    assert_model_close(got, ref, truth, name=f"umT5-XXL width 2 layers n={n}", **T5_GATES[n])


def test_umt5_encoder_model_batch_equals_single_prompts(umt5_2layer):
    """T5EncoderModel.__call__ on a batch of a 77- and a 512-token prompt (tokenizer injected, padded to text_len 512) returns the
    single-prompt encodings bit for bit."""
    from univid_amd.wan.t5 import T5EncoderModel
    cfg, sd, m, ids = umt5_2layer
    T = 512
    tok = torch.zeros(2, T, dtype=torch.long)
    tok[0, :77], tok[1, :512] = ids[77], ids[512]
    mask = torch.stack([(torch.arange(T) < 77).long(), torch.ones(T, dtype=torch.long)])
    enc = T5EncoderModel(text_len=T, device=DEV, model=m, tokenizer=lambda texts, **kw: (tok, mask))
    ctx = enc(["a", "b"], DEV)
    assert [c.shape for c in ctx] == [(77, cfg["dim"]), (512, cfg["dim"])]
    assert torch.equal(ctx[0], m.encode(ids[77])) and torch.equal(ctx[1], m.encode(ids[512]))


def _projector_truth(sd, tokens, T, dev):
    """oracle.projector.forward without any bf16 rounding: fp64 on `dev`."""
    p = "bagel_to_t5_projector."
    w = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    x = tokens.to(dev, torch.float64)
    x = F.layer_norm(F.linear(x, w[p + "0.weight"], w[p + "0.bias"]), (w[p + "1.weight"].numel(),), w[p + "1.weight"], w[p + "1.bias"], 1e-5)
    x = F.linear(F.gelu(x), w[p + "4.weight"], w[p + "4.bias"])
    x = F.layer_norm(x, (x.shape[-1],), w[p + "5.weight"], w[p + "5.bias"], 1e-5)
    if x.shape[1] != T:
        x = F.interpolate(x.transpose(1, 2), size=T, mode="linear", align_corners=False).transpose(1, 2)
    return x


PROJ_GATES = {77: dict(frac=0.982, max_rel=0.00834), 512: dict(frac=0.9817, max_rel=0.00719), 700: dict(frac=0.9825, max_rel=0.00795),
              2300: dict(frac=0.9815, max_rel=0.00775)}


@pytest.fixture(scope="module")
def projector_xl():
    import types
    from oracle import projector
    from univid_amd.model_pipeline import ContextProjector
    cfg = types.SimpleNamespace(bagel_hidden_dim=3584, wan_text_dim=4096, wan_text_length=512, use_semantic_alignment=False)
    sd = projector.make_state_dict(3584, 4096, 31)
    m = ContextProjector(cfg)
    m.load_state_dict(sd)
    yield sd, m.to(DEV).eval()


@pytest.mark.parametrize("Lt", [77, 512, 700, 2300])
def test_context_projector_production_width(projector_xl, Lt):
    """ContextProjector at 3584 -> 8192 -> 4096 with wan_text_length 512: L BAGEL tokens below, at (no resampling) and above 512,
    against oracle.projector.forward(..., interp="device") on the CPU and an fp64 truth run.

    Measured on MI355X (inside rtol 1e-3 / atol 1e-4 | max error / range | rms vs truth, HIP / oracle):
        L = 77     0.9850 | 0.0069 | 0.99997
        L = 512    0.9848 | 0.0060 | 0.99991
        L = 700    0.9855 | 0.0066 | 0.99996
        L = 2300   0.9846 | 0.0065 | 0.99992
    (the largest errors are one bf16 ulp at the output's largest values). Gates as for the encoder."""
    from oracle import projector
    sd, m = projector_xl
    tokens = torch.randn(1, Lt, 3584, generator=torch.Generator().manual_seed(Lt))
    got = m(tokens)
    assert len(got) == 1 and got[0].shape == (512, 4096) and got[0].dtype == BF16
    ref = projector.forward(sd, tokens, 512, interp="device")[0]
    truth = _projector_truth(sd, tokens, 512, DEV)[0]
    assert_model_close(got[0], ref, truth, name=f"ContextProjector 3584->8192->4096 L={Lt}", **PROJ_GATES[Lt])
