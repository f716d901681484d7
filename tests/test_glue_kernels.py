"""GPU (-m gpu): the small VAE / DiT / attention-seam glue kernels, each called directly through the C ABI at edge shapes.

The whole-model tests reach these kernels only at the model widths and behind statistical gates (VAE: rtol 1e-3 / atol 1e-4; DiT:
fractions inside 1e-3 / 1e-4), which cannot see a one-ulp error or a launch path the model widths never take. Here every entry point
is compared with a plain CPU reference of the same operation - the oracle's own functions (oracle.wan_vae / oracle.wan_dit), in fp64
where the operation has no intermediate rounding, in the oracle's fp32 expression where the kernel reproduces the reference's roundings
op by op - at the smallest shapes that reach each path: odd sizes, tails of the rows-per-wave launches, grid-stride loops that
iterate, every template instantiation of the launchers.

Gates (eps = 2^-24):
  * bit-exact where the kernel is a permutation, a cast or one or two correctly rounded fp32 operations in the reference's order;
  * derived fp32 bounds against the fp64 reference where only the summation order differs (stated in each test);
  * sinusoid: within one fp32 ulp, >= 99.9 % bit-identical (device and host fp64 pow / cos may differ in the last place);
  * rmsnorm_rope: test_gpu_parity.assert_bf16_kernel with rare = (max(2e-5, 2 / numel), 2 bf16 ulp of the pair's larger element).

Every output buffer is larger than what the kernel should write (a wider leading dimension, extra rows or frames) and pre-filled with
a sentinel that must be intact afterwards: an out-of-range store shows up as a failed assertion. The measured margins go to the
margins file through `record_margin` (profiles/glue_kernel_margins.json).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import bf16_ulp, record_margin
from test_gpu_parity import _split_f16_acts, assert_bf16_kernel

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
F64 = torch.float64
DEV = "cuda"
EPS = 2.0 ** -24
SENT = -7.25            # exact in fp32, bf16 and fp16
FLT_MIN = 2.0 ** -126   # smallest normal fp32


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


def _call(name, *args):
    """One entry point through _lib.call: tensors become device pointers, the current stream is appended."""
    _lib = L()
    _lib.call(name, *[_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _lib.stream_ptr())


def _round_up(a, b):
    return (a + b - 1) // b * b


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sent(*shape, dtype=F32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


_INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16, torch.int16: torch.int16}


def _assert_bits(got, ref, name=""):
    """Bit for bit (so -0.0 != +0.0), except that a NaN is compared as NaN, not by payload."""
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    if got.dtype.is_floating_point:
        gn, rn = torch.isnan(got), torch.isnan(ref)
        assert torch.equal(gn, rn), f"{name}: NaN positions differ ({int(gn.sum())} got, {int(rn.sum())} expected)"
        gi = torch.where(gn, torch.zeros_like(got), got).view(_INT[got.dtype])
        ri = torch.where(rn, torch.zeros_like(ref), ref).view(_INT[ref.dtype])
    else:
        gi, ri = got, ref
    bad = gi != ri
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got {got[i].item()!r}, expected {ref[i].item()!r}")


def _assert_untouched(buf, written, name=""):
    """`buf` (the whole oversized buffer, on the CPU) still holds the sentinel wherever the bool mask `written` is False."""
    out = buf[~written]
    assert (out == SENT).all(), f"{name}: {int((out != SENT).sum())} elements outside the output region were written"


def _mask(buf, *index):
    m = torch.zeros(buf.shape, dtype=torch.bool)
    m[index] = True
    return m


_RUNNING = {}


def _margin(name, **values):
    """Running maximum over the cases of a parametrised test, written through record_margin under glue/<name>."""
    cur = _RUNNING.setdefault(name, {"cases": 0})
    cur["cases"] += 1
    for k, v in values.items():
        v = float(v)
        cur[k] = min(cur.get(k, v), v) if k.startswith("min_") else max(cur.get(k, v), v)
    record_margin("glue/" + name, **cur)


def _f32_ulp(x):
    x = x.abs().double().clamp_min(FLT_MIN)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


def _reject(match, name, *args):
    with pytest.raises(L().UnividHipError, match=match):
        _call(name, *args)


# ---------------------------------------------------------------------------------------------------------------
# vae_glue.hip
# ---------------------------------------------------------------------------------------------------------------
# c of the SiLU gate below = 2 x the largest excess over the norm-only term measured on MI355X against the fp64 reference. Measured: 0 -
# no element of the 54 (C, P) cases exceeds 1.1 |t| 8 eps at all (the largest error is 9.6 eps |silu(t)|, at negative t where
# |t| / |silu(t)| is large, and at most 0.20 of the bound that c = 16 would have given; the norm-only run reaches 3.9 eps of its 8).
# So c = 0: the norm bound carried through SiLU is the whole gate.
C_SILU = 0.0


def _rms_silu_inputs(C, P):
    g = _gen(1000 * C + P)
    x = torch.randn(P, C, generator=g) * torch.logspace(-3, math.log10(50.0), P).view(P, 1)      # row scales 1e-3 ... 50
    if P >= 3:
        x[P // 2] = 0.0                                                                             # one all-zero row
    gamma = torch.randn(C, generator=g) * 0.3 + 1.0
    return x, gamma


def _rms_silu_run(x, gamma, do_silu, split_out):
    P, C = x.shape
    ld_in, ld_out = C + 8, C + 12
    xin = torch.zeros(P, ld_in)
    xin[:, :C] = x
    xin[:, C:] = float("nan")                         # a read past the row would poison the sum of squares
    buf = _sent(P + 2, ld_out)
    _call("uv_vae_rms_silu", xin.to(DEV), ld_in, gamma.to(DEV), buf, ld_out, P, C, do_silu, split_out)
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("do_silu", [0, 1])
@pytest.mark.parametrize("P", [1, 3, 15, 16, 17, 33])
@pytest.mark.parametrize("C", [4, 160, 256, 260, 320, 640, 1024, 1028, 2048])
def test_vae_rms_silu(C, P, do_silu):
    """uv_vae_rms_silu against oracle.wan_vae.rms_norm (+ F.silu) in fp64. C covers MAXV = 1, 1, 1, 2, 2, 3, 4, 8 with clamped lanes
    (1028) and 8 full (2048: no VAE width runs the MAXV = 8 instantiation); P the tails of 4, 2 and 1 rows per wave. Padded leading
    dimensions (the input's padding holds NaN), rows of scale 1e-3 ... 50, one all-zero row (-> zeros).

    do_silu = 0: relative error <= 8 eps (measured on the CPU: the kernel's lane-then-butterfly summation emulated in numpy fp32
    against fp64 for C = 4 ... 2048 gave at most 4.1 eps, torch's own fp32 evaluation 4.7 eps).
    do_silu = 1: |err| <= 1.1 |t| 8 eps + c eps |silu(t)|, t the pre-activation: the norm bound carried through SiLU (|silu'| <= 1.1)
    plus expf and the division. c = 2 x the largest excess over the norm-only term measured on MI355X = 0 (see C_SILU).
    Measured on MI355X: 3.9 eps without SiLU; with SiLU no excess over the norm-only term."""
    from oracle import wan_vae
    x, gamma = _rms_silu_inputs(C, P)
    buf = _rms_silu_run(x, gamma, do_silu, 0)
    _assert_untouched(buf, _mask(buf, slice(0, P), slice(0, C)), "rms_silu")
    got = buf[:P, :C].double()
    assert torch.isfinite(got).all()
    t = wan_vae.rms_norm(x.double().t().unsqueeze(0), gamma.double().view(1, C, 1))[0].t()          # [P, C] fp64
    if P >= 3:
        assert (got[P // 2] == 0).all(), "the all-zero row must give zeros"
    if not do_silu:
        err = (got - t).abs()
        _margin("vae_rms_silu", max_rel_err_eps=(err / t.abs().clamp_min(1e-300)).max() / EPS)
        assert (err <= 8 * EPS * t.abs()).all(), f"max relative error {float((err / t.abs().clamp_min(1e-300)).max() / EPS):.2f} eps"
        return
    ref = F.silu(t)
    err = (got - ref).abs()
    norm_term = 1.1 * t.abs() * 8 * EPS
    nz = ref != 0
    excess = ((err - norm_term)[nz] / (EPS * ref.abs()[nz])).clamp_min(0).max() if nz.any() else torch.tensor(0.0)
    _margin("vae_rms_silu_silu", max_excess_over_norm_term_eps=excess, max_err_over_silu_eps=(err[nz] / ref.abs()[nz]).max() / EPS if nz.any() else 0.0,
            max_err_over_bound=(err / (norm_term + C_SILU * EPS * ref.abs()).clamp_min(1e-300)).max())
    assert (err <= norm_term + C_SILU * EPS * ref.abs()).all(), f"excess over the norm-only term {float(excess):.2f} eps |silu(t)| (c = {C_SILU})"


def _split_bf16_acts(x_cl):
    """bf16 counterpart of test_gpu_parity._split_f16_acts: [.., C] f32 (C % 32 == 0) -> the same bytes holding [C/32][32 hi | 32 lo]
    bf16 per pixel (hi = bf16(y), lo = bf16(y - hi)): what uv_vae_rms_silu(split_out=1) writes."""
    hi = x_cl.to(BF16)
    lo = (x_cl - hi.float()).to(BF16)
    C = x_cl.shape[-1]
    both = torch.stack((hi.view(*x_cl.shape[:-1], C // 32, 32), lo.view(*x_cl.shape[:-1], C // 32, 32)), dim=-2)
    return both.reshape(*x_cl.shape[:-1], 2 * C).contiguous().view(torch.float32)


@pytest.mark.parametrize("split_out", [1, 2])
@pytest.mark.parametrize("C", [160, 256, 320, 640, 1024, 2048])
def test_vae_rms_silu_split_layout(C, split_out):
    """split_out = 1 (bf16 pieces) and 2 (fp16 pieces): the pieces and the [C/32][32 hi | 32 lo] layout, bit for bit against a CPU split
    of the SAME kernel's split_out = 0 output - a layout error is thereby separated from arithmetic."""
    P = 5
    x, gamma = _rms_silu_inputs(C, P)
    plain = _rms_silu_run(x, gamma, 1, 0)
    buf = _rms_silu_run(x, gamma, 1, split_out)
    want = plain.clone()
    want[:P, :C] = (_split_bf16_acts if split_out == 1 else _split_f16_acts)(plain[:P, :C].contiguous())
    assert torch.equal(buf.view(torch.int32), want.view(torch.int32)), f"split_out={split_out} C={C}"


def test_vae_rms_silu_rejects_unsupported_widths():
    x, g, o = torch.zeros(2, 2064, device=DEV), torch.ones(2064, device=DEV), _sent(2, 2064)
    _reject(r"uv_vae_rms_silu: C=2052 unsupported", "uv_vae_rms_silu", x, 2064, g, o, 2064, 2, 2052, 0, 0)
    _reject(r"uv_vae_rms_silu: split output needs C % 32 == 0 \(C=48\)", "uv_vae_rms_silu", x, 2064, g, o, 2064, 2, 48, 0, 1)
    _reject(r"uv_vae_rms_silu: split output needs C % 32 == 0 \(C=48\)", "uv_vae_rms_silu", x, 2064, g, o, 2064, 2, 48, 0, 2)
    torch.cuda.synchronize()
    assert (o == SENT).all()


SOFTMAX_C = 1024           # the decoder's middle width: scale = 1 / 32, exact in fp32


def _softmax_check(x, scale, wide):
    """x [R, n] logits; runs the in-place kernel inside a wider buffer and checks it against fp64. Bound: relative error
    <= (2 max|x scale| + n / 64 + 12) eps per row - the fp32 rounding of x * scale and of its difference with the maximum enter the
    exponent as absolute errors (<= eps max|x scale| each, for the element and for the maximum), the n / 64 serial additions per lane,
    the butterfly, expf, the reciprocal and the final product are the rest. A result below the smallest normal fp32 (a logit 87 below
    the maximum) has no relative accuracy in the format: + 2^-126 absolute."""
    R, n = x.shape
    ld = _round_up(n, 4) + 4
    buf = _sent(R + 1, ld)
    buf[:R, :n] = x.to(DEV)
    _call("uv_softmax_rows_f32", buf, ld, R, n, scale)
    torch.cuda.synchronize()
    b = buf.cpu()
    _assert_untouched(b, _mask(b, slice(0, R), slice(0, n)), "softmax")
    got = b[:R, :n].double()
    xs = x.double() * scale
    ref = torch.softmax(xs, -1)
    k = 2 * xs.abs().amax(-1, keepdim=True) + n / 64 + 12
    err = (got - ref).abs()
    tol = k * EPS * ref + FLT_MIN
    _margin("softmax_rows" + ("_wide" if wide else ""), max_err_over_bound=(err / tol).max(), max_rel_err_eps=(err / ref.clamp_min(FLT_MIN)).max() / EPS)
    assert torch.isfinite(got).all() and (err <= tol).all(), f"max err / bound {float((err / tol).max()):.3f}"
    assert ((got.sum(-1) - 1).abs() <= (n / 64 + 14) * EPS + n * FLT_MIN).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
@pytest.mark.parametrize("R", [1, 3, 4, 5, 130])
def test_softmax_rows(R, n):
    """uv_softmax_rows_f32 (in place, one wave per row) against torch.softmax in fp64: ld = n rounded up to 4, + 4 - the columns from
    n on must stay untouched; scale 1 / sqrt(C); the last row's logits spread over +-60 after scaling."""
    g = _gen(100 * R + n)
    scale = 1.0 / math.sqrt(SOFTMAX_C)
    x = torch.randn(R, n, generator=g) * (3.0 / scale)
    x[R - 1] = (torch.linspace(-60, 60, n) if n > 1 else torch.tensor([60.0]))[torch.randperm(n, generator=g)] / scale
    _softmax_check(x, scale, wide=False)


def test_softmax_rows_needs_the_max_subtraction():
    """Logits spread over +-100 after scaling: exp() of the raw value overflows fp32 (> 88.7), so only the subtraction of the row maximum
    keeps the row finite (at +-60 an implementation without it is still within the bound: exp(60) = 1e26 is an ordinary fp32)."""
    g = _gen(7)
    scale = 1.0 / math.sqrt(SOFTMAX_C)
    x = torch.randn(3, 100, generator=g) * (3.0 / scale)
    x[1] = torch.linspace(-100, 100, 100)[torch.randperm(100, generator=g)] / scale
    x[2] = torch.linspace(40, 100, 100)[torch.randperm(100, generator=g)] / scale
    _softmax_check(x, scale, wide=True)


def _cl(x_cf):
    """[1, C, T, H, W] -> channels-last [T, H, W, C]"""
    return x_cf[0].permute(1, 2, 3, 0).contiguous()


def _cf(x_cl):
    """channels-last [T, H, W, C] -> [1, C, T, H, W]"""
    return x_cl.permute(3, 0, 1, 2).unsqueeze(0).contiguous()


DUPUP_CASES = [(1, 3, 5, 8, 8, 2, 1, 0), (2, 3, 5, 8, 8, 2, 0, 0), (2, 3, 5, 8, 4, 2, 0, 0), (2, 3, 5, 8, 4, 1, 0, 0),
               (1, 2, 3, 12, 6, 1, 0, 0),             # Cout % 4 != 0: the scalar kernel
               (2, 3, 5, 8, 8, 2, 0, 1),              # `out` offset by one float: misaligned for 16-byte accesses, the scalar kernel again
               (1, 260, 260, 64, 64, 1, 0, 0),        # 4 326 400 float4 > 16384 * 256: the vector kernel's grid-stride loop iterates
               (1, 300, 300, 12, 6, 1, 0, 0)]         # 2 160 000 floats > 8192 * 256: the scalar kernel's


@pytest.mark.parametrize("T,H,W,Cin,Cout,ft,drop,off", DUPUP_CASES)
def test_vae_dupup_add(T, H, W, Cin, Cout, ft, drop, off):
    """uv_vae_dupup_add: out += WanVAE.dup_up3d(x) (drop = ft - 1 leading frames on the first chunk), one fp32 addition per element:
    bit-exact. `out` starts as random values; one extra frame behind it (and the float in front of an offset pointer) keeps the sentinel."""
    from oracle.wan_vae import WanVAE
    g = _gen(T * 1000 + Cin * 10 + Cout + ft + off)
    x = torch.randn(T, H, W, Cin, generator=g)
    To = T * ft - drop
    out0 = torch.randn(To, 2 * H, 2 * W, Cout, generator=g)
    n = out0.numel()
    frame = 4 * H * W * Cout
    buf = _sent(off + n + frame)
    buf[off:off + n] = out0.flatten().to(DEV)
    _call("uv_vae_dupup_add", x.to(DEV), buf[off:], T, H, W, Cin, Cout, ft, drop)
    torch.cuda.synchronize()
    want = torch.full((off + n + frame,), SENT)
    want[off:off + n] = (out0 + _cl(WanVAE.dup_up3d(_cf(x), Cout, ft, 2, first_chunk=drop > 0))).flatten()
    _assert_bits(buf, want, "dupup_add")


AVGDOWN_CFG = [(4, 6, 4, 4, 1, 1), (4, 6, 4, 8, 1, 2), (4, 6, 4, 4, 2, 2)]          # group 1, 2, 8


@pytest.mark.parametrize("T,H,W,Cin,Cout,ft,fs", [(T, *c) for T in (1, 3, 4) for c in AVGDOWN_CFG] + [(1, 1040, 1040, 4, 8, 1, 2)])
def test_vae_avgdown_add(T, H, W, Cin, Cout, ft, fs):
    """uv_vae_avgdown_add: out += WanVAE.avg_down3d(x) in fp64. T = 1, 3, 4 with ft = 2: 1, 1 and 0 frames of front padding; groups of
    1, 2 and 8; 2 163 200 outputs (> 8192 * 256: the grid-stride loop iterates).
    Bound: |err| <= (group + 1) eps mean_g|x| + eps |out| - group - 1 serial additions and the division on a sum of at most
    group mean_g|x| (one eps each, first order), and the rounding of the final addition onto out."""
    from oracle.wan_vae import WanVAE
    g = _gen(T * 100 + Cout * 10 + ft + fs)
    x = torch.randn(T, H, W, Cin, generator=g)
    group = Cin * ft * fs * fs // Cout
    To, Ho, Wo = (T + ft - 1) // ft, H // fs, W // fs
    out0 = torch.randn(To, Ho, Wo, Cout, generator=g)
    n = out0.numel()
    buf = _sent(n + Ho * Wo * Cout)
    buf[:n] = out0.flatten().to(DEV)
    _call("uv_vae_avgdown_add", x.to(DEV), buf, T, H, W, Cin, Cout, ft, fs)
    torch.cuda.synchronize()
    b = buf.cpu()
    assert (b[n:] == SENT).all(), "the frame behind the output was written"
    mean = _cl(WanVAE.avg_down3d(_cf(x).double(), Cout, ft, fs))
    assert mean.shape == out0.shape
    mean_abs = _cl(WanVAE.avg_down3d(_cf(x).double().abs(), Cout, ft, fs))
    ref = out0.double() + mean
    err = (b[:n].view_as(out0).double() - ref).abs()
    tol = (group + 1) * EPS * mean_abs + EPS * ref.abs()
    _margin("vae_avgdown_add", max_err_over_bound=(err / tol.clamp_min(1e-300)).max())
    assert (err <= tol).all(), f"max err / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}"


LATENT_GRIDS = {1: (1, 1, 1), 77: (1, 7, 11), 22000: (10, 40, 55)}     # 22 000 x 48 > 4096 * 256: the grid-stride loop iterates


@pytest.mark.parametrize("ld", [48, 96])
@pytest.mark.parametrize("P", [1, 77, 22000])
def test_vae_latent_in(P, ld):
    """uv_vae_latent_in: z [Z, f, h, w] -> channels-last rows of z / inv_std + mean, the expression of WanVAE.decode with scale_tensors()
    in fp32: one correctly rounded division and one addition, bit-exact."""
    from oracle import wan_vae
    Z = 48
    f, h, w = LATENT_GRIDS[P]
    scale = wan_vae.scale_tensors()
    z = torch.randn(1, Z, f, h, w, generator=_gen(P + ld)) * 1.5
    buf = _sent(P + 1, ld)
    _call("uv_vae_latent_in", z.to(DEV), scale[0].to(DEV), scale[1].to(DEV), buf, ld, Z, P)
    torch.cuda.synchronize()
    ref = z / scale[1].view(1, Z, 1, 1, 1) + scale[0].view(1, Z, 1, 1, 1)                    # wan_vae.WanVAE.decode's first line
    want = torch.full((P + 1, ld), SENT)
    want[:P, :Z] = _cl(ref).reshape(P, Z)
    _assert_bits(buf, want, "latent_in")


@pytest.mark.parametrize("ld", [48, 96])
@pytest.mark.parametrize("P", [1, 77, 22000])
def test_vae_latent_out(P, ld):
    """uv_vae_latent_out: rows [P, ld] whose first Z channels are mu (ld = 96: the encoder's 2 Z channels) -> [Z, f, h, w] of
    (mu - mean) * inv_std, the expression of WanVAE.encode: bit-exact."""
    from oracle import wan_vae
    Z = 48
    f, h, w = LATENT_GRIDS[P]
    scale = wan_vae.scale_tensors()
    rows = torch.randn(P, ld, generator=_gen(2 * P + ld)) * 1.5
    buf = _sent(Z * P + 64)
    _call("uv_vae_latent_out", rows.to(DEV), ld, scale[0].to(DEV), scale[1].to(DEV), buf, Z, P)
    torch.cuda.synchronize()
    mu = _cf(rows[:, :Z].reshape(f, h, w, Z))
    ref = (mu - scale[0].view(1, Z, 1, 1, 1)) * scale[1].view(1, Z, 1, 1, 1)                  # wan_vae.WanVAE.encode's last line
    want = torch.full((Z * P + 64,), SENT)
    want[:Z * P] = ref.flatten()
    _assert_bits(buf, want, "latent_out")


VIDEO_FHW = (5, 6, 10)


def _vae_patchify(x):
    """the patchify expression of oracle.wan_vae.WanVAE.encode: [b, c, f, h, w] -> [b, 4 c, f, h / 2, w / 2]"""
    b, c, f, h, w = x.shape
    return x.view(b, c, f, h // 2, 2, w // 2, 2).permute(0, 1, 6, 4, 2, 3, 5).reshape(b, c * 4, f, h // 2, w // 2)


def _vae_unpatchify(out):
    """the unpatchify expression of oracle.wan_vae.WanVAE.decode: [b, c, f, h, w] -> [b, c / 4, f, 2 h, 2 w]"""
    b, c, f, h, w = out.shape
    return out.view(b, c // 4, 2, 2, f, h, w).permute(0, 1, 4, 5, 3, 6, 2).reshape(b, c // 4, f, h * 2, w * 2)


def test_vae_patch_expressions_are_the_oracles():
    """The two expressions above, copied from WanVAE.encode / decode, are inverses of each other and what the oracle runs (a drift of
    either copy from oracle/wan_vae.py would show as a failure of the golden VAE tests' kernels against THIS file's reference)."""
    x = torch.randn(1, 3, 2, 4, 6, generator=_gen(0))
    assert torch.equal(_vae_unpatchify(_vae_patchify(x)), x)


@pytest.mark.parametrize("ld", [12, 16])
@pytest.mark.parametrize("f0,T", [(0, 1), (1, 4), (4, 1)])
def test_vae_video_in(f0, T, ld):
    """uv_vae_video_in: frames [f0, f0 + T) of a [3, F, H, W] video -> patchified channels-last rows, bit-exact against the patchify
    expression of WanVAE.encode; columns 12 ... ld and the frame behind the output keep the sentinel."""
    Fr, H, W = VIDEO_FHW
    vid = torch.randn(3, Fr, H, W, generator=_gen(f0 * 10 + T))
    buf = _sent(T + 1, H // 2, W // 2, ld)
    _call("uv_vae_video_in", vid.to(DEV), buf, ld, Fr, H, W, f0, T)
    torch.cuda.synchronize()
    want = torch.full((T + 1, H // 2, W // 2, ld), SENT)
    want[:T, :, :, :12] = _cl(_vae_patchify(vid.unsqueeze(0))[:, :, f0:f0 + T])
    _assert_bits(buf, want, "video_in")


@pytest.mark.parametrize("ld", [12, 16])
@pytest.mark.parametrize("f0,T", [(0, 1), (1, 4), (4, 1)])
def test_vae_video_out(f0, T, ld):
    """uv_vae_video_out: head rows [T, Hp, Wp, ld] -> frames [f0, f0 + T) of the video, clamped: bit-exact against the unpatchify
    expression of WanVAE.decode and torch.clamp(x, -1, 1) on values beyond +-1, exactly +-1, -0.0, +-inf and NaN - torch.clamp keeps a
    NaN (the reference's clamp_(-1, 1), vae2_2.py:1045), so a decode that went NaN must not come out as a valid dark video. Frames of
    the destination outside [f0, f0 + T) keep the sentinel."""
    Fr, H, W = VIDEO_FHW
    Hp, Wp = H // 2, W // 2
    g = _gen(f0 * 10 + T + 100)
    y = torch.randn(T, Hp, Wp, ld, generator=g) * 1.5
    special = torch.tensor([1.0, -1.0, -0.0, 0.0, float("inf"), float("-inf"), float("nan"), 1.0000001, -1.0000001, 0.99999994, 3.5, -2.25])
    vals = y[..., :12].reshape(-1)
    vals[torch.randperm(vals.numel(), generator=g)[:3 * len(special)]] = special.repeat(3)
    y[..., :12] = vals.view(T, Hp, Wp, 12)
    assert torch.isnan(y[..., :12]).sum() == 3 and torch.isinf(y[..., :12]).sum() == 6
    n = 3 * Fr * H * W
    buf = _sent(n + H * W)                                     # [3, F, H, W] and one frame behind it
    _call("uv_vae_video_out", y.to(DEV), ld, buf, Fr, Hp, Wp, f0, T)
    torch.cuda.synchronize()
    want = torch.full((3, Fr, H, W), SENT)
    want[:, f0:f0 + T] = torch.clamp(_vae_unpatchify(_cf(y[..., :12])), -1, 1)[0]
    _assert_bits(buf, torch.cat([want.flatten(), torch.full((H * W,), SENT)]), "video_out")


# ---------------------------------------------------------------------------------------------------------------
# dit_glue.hip
# ---------------------------------------------------------------------------------------------------------------
PATCH_CASES = [(48, (1, 2, 2), 192, (2, 5, 6)),        # H = 5 with ph = 2: the last row is dropped
               (3, (2, 2, 2), 64, (2, 5, 6)),          # 24 real columns, the rest of Kpad must be zero
               (48, (1, 2, 2), 192, (1, 150, 150))]    # 5625 x 192 = 1 080 000 elements > 4096 * 256: the grid-stride loop iterates


@pytest.mark.parametrize("Cin,patch,Kpad,fhw", PATCH_CASES)
def test_patchify_bf16(Cin, patch, Kpad, fhw):
    """uv_patchify_bf16 against the patch embedding's own operator: F.conv3d(stride = kernel = patch) with the identity as its weight
    yields, per token, the column order of Conv3d.weight.flatten(1) (exact: every product is x * 1 or x * 0), then the bf16 cast of
    oracle.wan_dit.dit_forward. Bit-exact; columns K ... Kpad are zero, columns Kpad ... ldo and the row behind the last keep the sentinel."""
    Fr, H, W = fhw
    K = Cin * math.prod(patch)
    x = torch.randn(Cin, Fr, H, W, generator=_gen(Cin + Kpad + H))
    cols = F.conv3d(x.unsqueeze(0).double(), torch.eye(K, dtype=F64).view(K, Cin, *patch), stride=patch)     # [1, K, Fp, Hp, Wp]
    Ltok = cols[0, 0].numel()
    assert Ltok == (Fr // patch[0]) * (H // patch[1]) * (W // patch[2])
    ldo = Kpad + 8
    buf = _sent(Ltok + 1, ldo, dtype=BF16)
    _call("uv_patchify_bf16", x.to(DEV), buf, ldo, Cin, Fr, H, W, *patch, Kpad)
    torch.cuda.synchronize()
    want = torch.full((Ltok + 1, ldo), SENT, dtype=BF16)
    want[:Ltok, :Kpad] = 0
    want[:Ltok, :K] = cols[0].flatten(1).t().float().to(BF16)
    _assert_bits(buf, want, "patchify")


@pytest.mark.parametrize("Cout,patch,grid", [(48, (1, 2, 2), (2, 2, 3)), (4, (1, 2, 2), (2, 2, 3)), (48, (2, 2, 2), (1, 2, 3)), (4, (2, 2, 2), (3, 1, 2)),
                                             (48, (1, 2, 2), (1, 75, 75))])         # 1 080 000 elements > 4096 * 256
def test_unpatchify_f32(Cout, patch, grid):
    """uv_unpatchify_f32 against oracle.wan_dit.unpatchify, bit-exact; ldi larger than the row, sentinel behind the output."""
    from oracle import wan_dit
    Ltok, row = math.prod(grid), math.prod(patch) * Cout
    ldi = row + 4
    xin = torch.randn(Ltok, ldi, generator=_gen(Cout + Ltok))
    n = Ltok * row
    buf = _sent(n + 64)
    _call("uv_unpatchify_f32", xin.to(DEV), ldi, buf, Cout, *grid, *patch)
    torch.cuda.synchronize()
    ref = wan_dit.unpatchify(xin[:, :row].contiguous().unsqueeze(0), torch.tensor([grid]), patch, Cout)[0]
    want = torch.full((n + 64,), SENT)
    want[:n] = ref.flatten()
    _assert_bits(buf, want, "unpatchify")


@pytest.mark.parametrize("n", [1, 2, 300])
@pytest.mark.parametrize("dim", [2, 256])
def test_sinusoid_f32(dim, n):
    """uv_sinusoid_f32 against oracle.wan_dit.sinusoidal_embedding_1d (fp64, rounded to fp32 once): every element within one fp32 ulp
    and >= 99.9 % bit-identical - device and host fp64 pow / cos may differ in the last place, which moves the fp32 rounding only next
    to a tie. t among 0, 0.5, 999, 1000 and random fractions."""
    from oracle import wan_dit
    g = _gen(dim + n)
    t = torch.cat([torch.tensor([0.0, 0.5, 999.0, 1000.0]), torch.rand(max(n, 4), generator=g) * 1000])
    t = torch.cat([t[:2], t[4:]])[:n] if n < 4 else t[:n]
    buf = _sent(n + 1, dim)
    _call("uv_sinusoid_f32", t.to(DEV), buf, n, dim)
    torch.cuda.synchronize()
    b = buf.cpu()
    assert (b[n:] == SENT).all()
    ref = wan_dit.sinusoidal_embedding_1d(dim, t).float()
    got = b[:n]
    d = (got.double() - ref.double()).abs()
    exact = (got == ref).float().mean().item()
    _margin("sinusoid", max_err_ulp=(d / _f32_ulp(ref)).max(), min_exact_frac=exact)
    assert (d <= _f32_ulp(ref)).all(), f"max error {float((d / _f32_ulp(ref)).max()):.2f} ulp"
    assert exact >= 0.999, f"only {exact:.5f} bit-identical"


@pytest.mark.parametrize("K", [4, 252, 256, 260, 1000])
@pytest.mark.parametrize("N", [1, 6, 130])
@pytest.mark.parametrize("R", [1, 2, 3, 5, 7])
def test_linear_rows_f32(R, N, K):
    """uv_linear_rows_f32 against F.linear in fp64 (act_in = 1: on F.silu(x)): R covers every combination of the 4-, 2- and 1-row launches,
    N the partial last block of 4 columns, K the partial last pass of 256; bias present and None; ldx > K, ldo > N.
    Bound: |err| <= (K / 64 + 12) eps (|act(x)| |W|^T) + eps |b| - K / 256 serial steps of four products per lane, the butterfly,
    the SiLU's expf and division, and the bias addition."""
    g = _gen(R * 10000 + N * 100 + K)
    ldx, ldo = K + 4, N + 3
    x = torch.randn(R, ldx, generator=g) * 2
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
    for act_in in (0, 1):
        for bias in (b, None):
            buf = _sent(R + 1, ldo)
            _call("uv_linear_rows_f32", xd, ldx, Wd, None if bias is None else bd, buf, ldo, R, N, K, act_in)
            torch.cuda.synchronize()
            o = buf.cpu()
            _assert_untouched(o, _mask(o, slice(0, R), slice(0, N)), "linear_rows")
            a = x[:, :K].double()
            a = F.silu(a) if act_in else a
            ref = F.linear(a, W.double(), None if bias is None else bias.double())
            tol = (K / 64 + 12) * EPS * (a.abs() @ W.double().abs().t()) + (0 if bias is None else EPS * bias.double().abs())
            err = (o[:R, :N].double() - ref).abs()
            _margin("linear_rows", max_err_over_bound=(err / tol).max())
            assert (err <= tol).all(), f"act_in={act_in} bias={bias is not None}: max err / bound {float((err / tol).max()):.3f}"


@pytest.mark.parametrize("R,n", [(1, 1), (2, 7), (3, 1536), (3, 184320)])      # 552 960 elements > 2048 * 256: the grid-stride loop iterates
def test_add_rows_f32(R, n):
    """uv_add_rows_f32: out[r] = mod + e0[r], one fp32 addition: bit-exact (the block's `modulation.unsqueeze(0) + e`)."""
    g = _gen(R + n)
    mod, e0 = torch.randn(n, generator=g), torch.randn(R, n, generator=g)
    buf = _sent(R * n + 64)
    _call("uv_add_rows_f32", mod.to(DEV), e0.to(DEV), buf, R, n)
    torch.cuda.synchronize()
    want = torch.full((R * n + 64,), SENT)
    want[:R * n] = (mod.unsqueeze(0) + e0).flatten()
    _assert_bits(buf, want, "add_rows")


@pytest.mark.parametrize("Lr,C,ldx,ldy", [(1, 4, 8, 8), (5, 12, 16, 20), (3, 260, 264, 272), (1100, 3840, 3844, 3848)])   # 1 056 000 float4 > 4096 * 256
def test_add_bf16_resid(Lr, C, ldx, ldy):
    """uv_add_bf16_resid: x += float(y), one fp32 addition: bit-exact; the padding columns of x keep the sentinel."""
    g = _gen(Lr + C)
    x0 = torch.randn(Lr, C, generator=g)
    y = torch.full((Lr, ldy), float("nan"), dtype=BF16)
    y[:, :C] = torch.randn(Lr, C, generator=g).to(BF16)
    buf = _sent(Lr + 1, ldx)
    buf[:Lr, :C] = x0.to(DEV)
    _call("uv_add_bf16_resid", buf, ldx, y.to(DEV), ldy, Lr, C)
    torch.cuda.synchronize()
    want = torch.full((Lr + 1, ldx), SENT)
    want[:Lr, :C] = x0 + y[:, :C].float()
    _assert_bits(buf, want, "add_bf16_resid")


# ---- casts ----------------------------------------------------------------------------------------------------
CAST_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 4100 + 3]          # the last: > 4096 blocks of 256 float4, and a 3-element tail
SPECIAL_F32 = [0.0, -0.0, 1e-45, -1e-40, 2.0 ** -127, -(2.0 ** -133),                        # +-0, fp32 subnormals
               1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),     # exact bf16 ties, even and odd neighbour below
               1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),  # exact fp16 ties of both parities
               2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 65519.996, 65520.0, -65520.0,             # fp16 subnormal ties, the fp16 overflow threshold
               3.4028234663852886e38, -3.4028234663852886e38,                                # the largest finite fp32: inf in both 16-bit types
               float("inf"), float("-inf"), float("nan")]


def _cast_input(n):
    """randn with the special values at the front and, rotated by n, at the end (the scalar tail path sees different ones per n)."""
    x = torch.randn(n, generator=_gen(n)) * 3
    s = torch.tensor(SPECIAL_F32, dtype=F32)
    k = min(n, len(s))
    x[:k] = s[:k]
    tail = s.roll(n % len(s))[:k]
    if n > len(s):
        x[n - k:] = tail
    else:
        x[:] = tail
    return x


@pytest.mark.parametrize("n", CAST_N)
def test_cast_f32_bf16(n):
    """uv_cast_f32_bf16 against torch's fp32 -> bf16 (round to nearest even), bit-exact including subnormals, ties, overflow to inf, NaN."""
    x = _cast_input(n)
    buf = _sent(n + 8, dtype=BF16)
    _call("uv_cast_f32_bf16", x.to(DEV), buf, n)
    torch.cuda.synchronize()
    want = torch.full((n + 8,), SENT, dtype=BF16)
    want[:n] = x.to(BF16)
    _assert_bits(buf, want, "cast_f32_bf16")


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("n", CAST_N)
def test_cast_f32_to16(n, f16):
    """uv_cast_f32_to16 (bf16 / IEEE fp16) against torch's casts, bit-exact."""
    dt = F16 if f16 else BF16
    x = _cast_input(n)
    buf = _sent(n + 8, dtype=dt)
    _call("uv_cast_f32_to16", x.to(DEV), buf, n, f16)
    torch.cuda.synchronize()
    want = torch.full((n + 8,), SENT, dtype=dt)
    want[:n] = x.to(dt)
    _assert_bits(buf, want, f"cast_f32_to16 f16={f16}")


@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("n", CAST_N)
def test_cast_16_to_f32(n, f16):
    """uv_cast_16_to_f32 against torch's (exact) widening: random 16-bit patterns (every class: subnormals, inf, NaN) + the rounded specials."""
    dt = F16 if f16 else BF16
    x = torch.randint(-32768, 32768, (n,), generator=_gen(n + f16), dtype=torch.int32).to(torch.int16).view(dt)
    s = _cast_input(min(n, len(SPECIAL_F32))).to(dt)
    x[:len(s)] = s
    buf = _sent(n + 8)
    _call("uv_cast_16_to_f32", x.to(DEV), buf, n, f16)
    torch.cuda.synchronize()
    want = torch.full((n + 8,), SENT)
    want[:n] = x.float()
    _assert_bits(buf, want, f"cast_16_to_f32 f16={f16}")


@pytest.mark.parametrize("R,C", [(1, 4), (3, 8), (3, 12), (2, 1020), (2, 1024), (3, 1028), (1030, 4112)])    # 1 058 840 float4 > 4096 * 256
def test_cast_f32_bf16_rows(R, C):
    """uv_cast_f32_bf16_rows: C at and around the 4-element vector width (the entry rejects C % 4 != 0), both leading dimensions padded
    (the input's padding holds NaN, the output's keeps the sentinel); bit-exact."""
    ldi, ldo = C + 4, C + 8
    x = torch.full((R, ldi), float("nan"))
    x[:, :C] = _cast_input(R * C).view(R, C)
    buf = _sent(R + 1, ldo, dtype=BF16)
    _call("uv_cast_f32_bf16_rows", x.to(DEV), ldi, buf, ldo, R, C)
    torch.cuda.synchronize()
    want = torch.full((R + 1, ldo), SENT, dtype=BF16)
    want[:R, :C] = x[:, :C].to(BF16)
    _assert_bits(buf, want, "cast_f32_bf16_rows")


def test_cast_f32_bf16_rows_rejects_odd_widths():
    x, o = torch.zeros(2, 16, device=DEV), _sent(2, 16, dtype=BF16)
    for C, ldi, ldo in ((6, 16, 16), (8, 14, 16), (8, 16, 4)):
        _reject("uv_cast_f32_bf16_rows: bad arguments", "uv_cast_f32_bf16_rows", x, ldi, o, ldo, 2, C)
    torch.cuda.synchronize()
    assert (o == SENT).all()


@pytest.mark.parametrize("Lr,C,Lpad", [(1, 8, 64), (63, 65, 64), (64, 64, 64), (65, 130, 128), (200, 72, 256)])
def test_transpose_16(Lr, C, Lpad):
    """uv_transpose_16: out[c][l] = in[l][c], columns L ... Lpad - 1 ZERO, everything beyond Lpad and beyond row C - 1 the sentinel;
    16-bit patterns of every class, bit-exact. ldi > C, ldo > Lpad."""
    ldi, ldo = C + 8, Lpad + 8
    x = torch.randint(-32768, 32768, (Lr, ldi), generator=_gen(Lr + C), dtype=torch.int32).to(torch.int16)
    buf = _sent(C + 1, ldo, dtype=BF16)
    _call("uv_transpose_16", x.to(DEV), ldi, buf, ldo, Lr, C, Lpad)
    torch.cuda.synchronize()
    want = torch.full((C + 1, ldo), SENT, dtype=BF16).view(torch.int16)
    want[:C, :Lpad] = 0
    want[:C, :Lr] = x[:, :C].t()
    _assert_bits(buf.view(torch.int16), want, "transpose_16")


@pytest.mark.parametrize("C", [1, 63, 64, 65, 768, 1152])
@pytest.mark.parametrize("R", [1, 5])
def test_l2_normalize_rows_f32(R, C):
    """uv_l2_normalize_rows_f32 against F.normalize in fp64: relative error <= 8 eps (the figure of test_vae_rms_silu: the same
    lane-then-butterfly sum of squares, one division); a zero row gives zeros through the eps clamp; padded strides."""
    ldx, ldo = C + 3, C + 5
    x = torch.full((R, ldx), float("nan"))
    x[:, :C] = torch.randn(R, C, generator=_gen(R + C)) * torch.logspace(-3, 1.7, R).view(R, 1)
    if R > 1:
        x[2, :C] = 0.0
    buf = _sent(R + 1, ldo)
    _call("uv_l2_normalize_rows_f32", x.to(DEV), ldx, buf, ldo, R, C, 1e-12)
    torch.cuda.synchronize()
    o = buf.cpu()
    _assert_untouched(o, _mask(o, slice(0, R), slice(0, C)), "l2_normalize")
    ref = F.normalize(x[:, :C].double(), dim=-1, eps=1e-12)
    got = o[:R, :C].double()
    if R > 1:
        assert (got[2] == 0).all()
    err = (got - ref).abs()
    _margin("l2_normalize_rows", max_rel_err_eps=(err / ref.abs().clamp_min(1e-300)).max() / EPS)
    assert (err <= 8 * EPS * ref.abs()).all(), f"max relative error {float((err / ref.abs().clamp_min(1e-300)).max() / EPS):.2f} eps"


# ---- QK RMSNorm + RoPE: the instantiations and run-time paths of rmsnorm_rope_launch --------------------------
def _rope_oracle(x, w, D, grid, freqs):
    """x [B, Ls, C] bf16 -> (oracle.wan_dit.rms_norm [+ rope_apply] rounded to bf16, |larger element of each pair| of the norm output)."""
    from oracle import wan_dit
    B, Ls, C = x.shape
    y = wan_dit.rms_norm(x, w, 1e-6)                                                      # fp32 [B, Ls, C]
    ref = y if freqs is None else wan_dit.rope_apply(y.view(B, Ls, C // D, D), torch.tensor([list(grid)] * B), freqs).reshape(B, Ls, C)
    ypair = y.view(B, Ls, C // 2, 2).abs().amax(dim=3, keepdim=True).expand(-1, -1, -1, 2).reshape(B, Ls, C)
    return ref.to(BF16), ypair


def _rope_gate(got, ref, ypair, name):
    """assert_bf16_kernel with the issue's rare term: kernel and oracle add the squares in different orders, which flips the intermediate
    bf16 rounding on about 1.3e-5 of the elements (tests/manual/rope_ulp_stats.py); at most max(2, 2e-5 numel) elements may exceed one
    ulp, none by more than 2 bf16 ulp of the rotated pair's larger element."""
    got, ref = got.float().cpu(), ref.float().cpu()
    d = (got - ref).abs()
    ulp = bf16_ulp(torch.maximum(ref.abs(), got.abs()))
    _margin("rmsnorm_rope", max_over_1ulp_count=(d > ulp + 2e-5 * ref.abs().max()).sum(), max_err_ulp=(d / ulp).max(), min_exact_frac=(d == 0).float().mean())
    assert_bf16_kernel(got, ref, name=name, rare=(max(2e-5, 2.0 / got.numel()), 2.0 * bf16_ulp(ypair.reshape(got.shape))))


# (C, head_dim, L, grid): grid[0] * grid[1] * grid[2] < L, so the last rows are sequence padding and pass through un-rotated
ROPE_CASES = [(768, 96, 33, (2, 3, 5)),              # head_dim 96 does not divide 512: same_cols false, <2,1>
              (1536, 96, 33, (2, 3, 5)),             # same_cols false, <8,1>
              (2048, 128, 33, (2, 3, 5)),            # exact by arithmetic, no exact instantiation: the non-exact <8,1>
              (2560, 64, 33, (2, 3, 5)),             # 5 chunks: <8,1>
              (2560, 64, 4102, (5, 20, 41)),         # 5 chunks at L >= 4096: <6,4>, and 4102 % 4 = 2 rows in the last wave
              (5120, 128, 33, (2, 3, 5)),            # <16,1>
              (1024, 128, 4102, (5, 20, 41)),        # <2,4,true>
              (768, 64, 4102, (5, 20, 41)),          # <2,4> with a remainder chunk
              (768, 96, 4102, (5, 20, 41))]          # same_cols false with four rows per wave


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("C,D,Lr,grid", ROPE_CASES)
def test_rmsnorm_rope_instantiations(C, D, Lr, grid, rope):
    """uv_rmsnorm_rope against oracle.wan_dit.rms_norm + rope_apply + rope_table on every row, with and without RoPE, padded leading
    dimensions on both sides. Seeds: 1000 C + D + L, the only ones tried."""
    from oracle import wan_dit
    g = _gen(1000 * C + D + Lr)
    x = (torch.randn(1, Lr, C, generator=g) * 1.5).to(BF16)
    w = torch.randn(C, generator=g) * 0.1 + 1
    freqs = wan_dit.rope_table(D) if rope else None
    ldx, ldo = C + 8, C + 16
    xin = torch.full((Lr, ldx), float("nan"), dtype=BF16)
    xin[:, :C] = x[0]
    buf = _sent(Lr + 1, ldo, dtype=BF16)
    _call("uv_rmsnorm_rope", xin.to(DEV), ldx, buf, ldo, w.to(DEV), Lr, C, D, 1e-6,
          torch.view_as_real(freqs).contiguous().to(DEV) if rope else None, *(grid if rope else (0, 0, 0)), 0)
    torch.cuda.synchronize()
    o = buf.cpu()
    _assert_untouched(o, _mask(o, slice(0, Lr), slice(0, C)), "rmsnorm_rope")
    ref, ypair = _rope_oracle(x, w, D, grid, freqs)
    _rope_gate(o[:Lr, :C], ref[0], ypair[0], f"rmsnorm_rope C={C} D={D} L={Lr} rope={rope}")
    if rope:                                         # the padding rows equal the un-rotated norm, exactly as the no-RoPE oracle
        s = math.prod(grid)
        assert torch.equal(ref[0, s:], _rope_oracle(x[:, s:], w, D, grid, None)[0][0])


@pytest.mark.parametrize("rope", [True, False])
def test_rmsnorm_rope_qk_odd_sample_length(rope):
    """uv_rmsnorm_rope_qk at L = 2 x 2051: four rows per wave and an odd sample length, so a wave's rows straddle the sample boundary;
    the RoPE positions must restart per sample (compared with the oracle per sample, rope_apply's batch loop). head_dim 96: the
    per-chunk factor fetch (same_cols false) under four rows per wave. q and k have their own weights. Seed 96, the only one tried."""
    from oracle import wan_dit
    C, D, Ls, B, grid = 768, 96, 2051, 2, (1, 41, 50)
    g = _gen(96)
    freqs = wan_dit.rope_table(D) if rope else None
    ldx, ldo = C + 8, C + 16
    xs, ws, bufs, xins = [], [], [], []
    for _ in range(2):
        x = (torch.randn(B, Ls, C, generator=g) * 1.5).to(BF16)
        xin = torch.full((B * Ls, ldx), float("nan"), dtype=BF16)
        xin[:, :C] = x.view(B * Ls, C)
        xs.append(x), ws.append(torch.randn(C, generator=g) * 0.1 + 1), xins.append(xin.to(DEV)), bufs.append(_sent(B * Ls + 1, ldo, dtype=BF16))
    wd = [w.to(DEV) for w in ws]
    _call("uv_rmsnorm_rope_qk", xins[0], bufs[0], wd[0], xins[1], bufs[1], wd[1], ldx, ldo, B * Ls, Ls, C, D, 1e-6,
          torch.view_as_real(freqs).contiguous().to(DEV) if rope else None, *(grid if rope else (0, 0, 0)), 0)
    torch.cuda.synchronize()
    for x, w, buf, nm in zip(xs, ws, bufs, "qk"):
        o = buf.cpu()
        _assert_untouched(o, _mask(o, slice(0, B * Ls), slice(0, C)), "rmsnorm_rope_qk " + nm)
        ref, ypair = _rope_oracle(x, w, D, grid, freqs)
        _rope_gate(o[:B * Ls, :C], ref.view(B * Ls, C), ypair.view(B * Ls, C), f"rmsnorm_rope_qk {nm} rope={rope}")


@pytest.mark.parametrize("C,D", [(768, 96), (1024, 128)])
def test_rmsnorm_rope_row0_offset(C, D):
    """A row0 > 0 call (a sequence-parallel shard) against the oracle on the shifted token range: rows 7 ... 32 of a 33-token
    sequence on a (2, 3, 5) grid, the last three of them padding. Seed 7 + C, the only one tried."""
    from oracle import wan_dit
    Lfull, grid, row0 = 33, (2, 3, 5), 7
    g = _gen(7 + C)
    x = (torch.randn(1, Lfull, C, generator=g) * 1.5).to(BF16)
    w = torch.randn(C, generator=g) * 0.1 + 1
    freqs = wan_dit.rope_table(D)
    Lr = Lfull - row0
    buf = _sent(Lr + 1, C + 8, dtype=BF16)
    _call("uv_rmsnorm_rope", x[0, row0:].contiguous().to(DEV), C, buf, C + 8, w.to(DEV), Lr, C, D, 1e-6,
          torch.view_as_real(freqs).contiguous().to(DEV), *grid, row0)
    torch.cuda.synchronize()
    o = buf.cpu()
    _assert_untouched(o, _mask(o, slice(0, Lr), slice(0, C)), "rmsnorm_rope row0")
    ref, ypair = _rope_oracle(x, w, D, grid, freqs)
    _rope_gate(o[:Lr, :C], ref[0, row0:], ypair[0, row0:], f"rmsnorm_rope row0 C={C}")
