"""GPU (-m gpu): the single-pass fp16 convolution uv_conv3d_f16 (the VAE's opt-in precision="f16") through the C ABI, in every kernel it
can run: the plain-row instantiations of the four "+4" gather tiles and of the four HALO_F16_* kernels.

The case table is test_conv_kernels.py's, every prec == 4 case with Cin doubled: a uv_conv3d_f16 call plans as an f16x3 call of HALF its
channels (its 64-channel rows are the 128-byte rows of 32 split channels), so the expected kernel is the one conv_plan(4, .., Cin / 2, ..)
names - asserted before every launch - and geometries, wide leading dimensions, sentinels, act_scale cases and UV_OPT_CONV_HALO pinning
are the ones there.

Arithmetic contract: out = (sum_k fp16(x_k s_a) fp16(w_k s_w)) / (s_a s_w) + bias (+ resid), products exact, f32 accumulate. The tests
hand over operands that ARE fp16 numbers (the activations as stored, the weights times their power-of-two scale), so the reference is the
fp64 convolution of exactly what the kernel reads.

Gates:
  (a) bit-exact on designed fp16 operands - small integers, and +-(1 + {-1, 0, 1} 2^-9) with one live 32-channel block per output channel,
      a different one from channel to channel, so that each half of a 64-channel row is live for some output channel;
  (b) random operands: |got - ref64| <= (K + 2) 2^-24 S, err / bound recorded;
  (c) sentinels around every output; (d) halo against gather on the same call to 1e-5 max(1, max|out|);
  (e) Cin % 64, ld_in % 8, a w_scale that is no power of two, and split_out = 3 with C % 64 != 0 raise and write nothing.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import record_margin
from test_conv_kernels import (ACT_SCALE, CASES as CASES_X3, DEV, SENT, _assert_bits, _assert_sentinels, _geom, _phase_weights, _rand_int,
                               _unfold, _widen, _wmat)

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
PLAIN_KERNELS = {"G256x16+4", "G128x128+4", "G256x128+4", "G256x256+4", "HALO_F16_N16", "HALO_F16_160", "HALO_F16_SQUARE", "HALO_F16_128"}

# every f16x3 case of test_conv_kernels.py with twice the input channels
CASES = [c._replace(Cin=2 * c.Cin) for c in CASES_X3 if c.prec == 4]
IDS = [f"{i:02d}-{c.kernel}-{c.geom}-{c.T}x{c.H}x{c.W}-{c.Cin}to{c.Cout}" + ("-r" if c.resid else "") + ("-wide" if c.wide else "") +
       ("-as" if c.ascale else "") for i, c in enumerate(CASES)]


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


def _w_scale(w):
    """uv_split_weights_f16x3's rule: the power of two that puts max |w| into [2^13, 2^14)"""
    return 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))


def _cast_weights(wp, scale):
    """uv_cast_weights_f16 of a [Cout, K] f32 matrix (+ a check against the cast in torch)"""
    _lib = L()
    out = torch.empty(wp.numel(), dtype=F16, device=wp.device)
    _lib.call("uv_cast_weights_f16", _lib.ptr(wp), _lib.ptr(out), wp.numel(), scale, _lib.stream_ptr())
    assert torch.equal(out.view(wp.shape), (wp * scale).to(F16)), "uv_cast_weights_f16"
    return out


def _launch(c, g, x16, wp, scale, bias, resid, halo=None):
    """One uv_conv3d_f16 call. x16 [Tin, Hin, Win, Cin] fp16: the activations as stored (with ascale: the activations * 2^-7, and the
    device scalar is 2^7); wp [Cout, K] f32, cast here under `scale`. Returns (got [M, Cout], the whole output buffer, the mask of what the
    launch had to write)."""
    _lib = L()
    _lib.set_option(_lib.OPT_CONV_HALO, c.halo if halo is None else halo)
    if halo is None:
        plan = _lib.conv_plan(4, g.Tout, g.Hout, g.Wout, g.Hin, g.Win, c.Cin // 2, c.Cout, g.kt, g.kh, g.kw, g.st, g.sh, g.sw, g.ph, g.pw, g.up, g.inter)
        assert plan["kernel"] == c.kernel, f"planned {plan}, the case expects {c.kernel}"
    ld_in, ldr = (c.Cin + 64, c.Cout + 12) if c.wide else (c.Cin, c.Cout)          # ld_in in CHANNELS (fp16 elements)
    co = c.Cout // 2 if g.inter else c.Cout
    ldo = co + 8 if c.wide else co
    wb = _cast_weights(wp, scale)
    asc = torch.full((4,), ACT_SCALE, device=DEV) if c.ascale else None
    xin = _widen(x16.contiguous().view(F32), ld_in // 2)        # rows of Cin / 2 f32-sized slots; the slack is 28 672 per fp16 half
    rin = None if resid is None else _widen(resid, ldr)
    if g.inter:
        shape, frames = (2 * g.Tout + 1, g.Hout, g.Wout, ldo), 2 * g.Tout
    elif g.up >= 2:
        shape, frames = (g.Tout + 1, 2 * g.Hout, 2 * g.Wout, ldo), g.Tout
    else:
        shape, frames = (g.Tout + 1, g.Hout, g.Wout, ldo), g.Tout
    out = torch.full(shape, SENT, device=DEV)
    _lib.call("uv_conv3d_f16", _lib.ptr(xin), ld_in, g.Tin, g.Hin, g.Win, _lib.ptr(wb), _lib.ptr(bias), _lib.ptr(out), ldo, g.Tout, g.Hout, g.Wout,
              c.Cin, c.Cout, g.kt, g.kh, g.kw, g.st, g.sh, g.sw, 0, g.ph, g.pw, g.up, g.inter, _lib.ptr(rin), 0 if rin is None else ldr, scale,
              _lib.ptr(asc), _lib.stream_ptr())
    torch.cuda.synchronize()
    written = torch.zeros(shape, dtype=torch.bool, device=DEV)
    if g.inter:
        written[:frames, :, :, :co] = True
        got = out[:frames, :, :, :co].reshape(g.Tout, 2, g.Hout, g.Wout, co).permute(0, 2, 3, 1, 4).reshape(g.M, c.Cout)
    elif g.up >= 2:
        a, b = (g.up - 2) >> 1, (g.up - 2) & 1
        written[:frames, a::2, b::2, :co] = True
        got = out[:frames, a::2, b::2, :co].reshape(g.M, c.Cout)
    else:
        written[:frames, :, :, :co] = True
        got = out[:frames, :, :, :co].reshape(g.M, c.Cout)
    return got, out, written


def _reference(c, g, x16, w, scale, bias, resid):
    """(ref, S) in fp64 from the fp16 operands the kernel reads: x16 as stored and fp16(w * scale); S = conv(|x|, |w|) + |bias| + |resid|."""
    s = ACT_SCALE if c.ascale else 1.0
    w16 = (w * scale).to(F16).double() / scale
    A = _unfold(g, x16.double()) * s
    ref = A @ w16.T + bias.double()
    S = A.abs() @ w16.abs().T + bias.double().abs()
    if resid is not None:
        ref, S = ref + resid.double(), S + resid.double().abs()
    return ref, S


# ---------------------------------------------------------------------------------------------------------------
# (a) bit-exact on designed operands
# ---------------------------------------------------------------------------------------------------------------
def _magnitudes(K):
    """(max |x|, max |w|), small integers with K max|x| max|w| + 6 < 2^13, the largest such pair"""
    for a, w in ((3, 3), (3, 2), (2, 2), (3, 1), (2, 1), (1, 1)):
        if K * a * w + 6 < 2 ** 13:
            return a, w
    raise AssertionError(f"K = {K}: no exact operand family")


def _designed(c, g, family, gen):
    """(x [Tin, Hin, Win, Cin], w [Cout, K], bias, resid | None) f32 on the CPU; the causal zero frames in front stay zero."""
    xs, ws = (g.Tin, g.Hin, g.Win, c.Cin), (c.Cout, g.K)
    if family == "int":
        amax, wmax = _magnitudes(g.K)
        x, w = _rand_int(gen, xs, -amax, amax), _rand_int(gen, ws, -wmax, wmax)
    else:       # "block": +-(1 + {-1, 0, 1} 2^-9), one live (tap, 32-channel block) per output channel: output channel n reads block n mod K / 32
        x = (2 * _rand_int(gen, xs, 0, 1) - 1) * (1 + _rand_int(gen, xs, -1, 1) * 2.0 ** -9)
        w = (2 * _rand_int(gen, ws, 0, 1) - 1) * (1 + _rand_int(gen, ws, -1, 1) * 2.0 ** -9)
        w = w * (torch.arange(c.Cout)[:, None] % (g.K // 32) == torch.arange(g.K)[None, :] // 32)
    x[:g.Tin - c.T] = 0
    bias = _rand_int(gen, (c.Cout,), -3, 3)
    resid = _rand_int(gen, (g.M, c.Cout), -3, 3) if c.resid else None
    return x, w, bias, resid


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv_f16_is_bit_exact_on_designed_operands(c):
    """Gates (a) and (c). Two families of operands that are fp16 numbers as they stand (also times the weights' power-of-two scale and the
    2^-7 of the act_scale cases), with every product and every partial sum exact in fp32:
      int    small integers with K max|x| max|w| + 6 < 2^13: integer products, every partial sum in any order below 2^13;
      block  both operands +-(1 + {-1, 0, 1} 2^-9), per output channel ONE live 32-channel block of K, block n mod (K / 32) for channel n -
             so both halves of a 64-channel row are live for some output channel, and a swapped or dropped half, tap or block shows;
             products are multiples of 2^-18, sums of 32 of them + bias + residual stay below 2^6: 24 bits.
    The kernel must then EQUAL the fp64 convolution of those fp16 values bit for bit. The conditions - operands exactly fp16, the sum
    bound, the fp32 round trip of the reference - are asserted on the reference before it is trusted."""
    g = _geom(c)
    assert g.K // 32 >= 2
    for fi, family in enumerate(("int", "block")):
        gen = torch.Generator().manual_seed(3000 * CASES.index(c) + fi)
        x, w, bias, resid = (None if t is None else t.to(DEV) for t in _designed(c, g, family, gen))
        xs = x / ACT_SCALE if c.ascale else x
        scale = _w_scale(w)
        x16 = xs.to(F16)
        assert torch.equal(x16.float(), xs) and torch.equal((w * scale).to(F16).float(), w * scale), "the designed operands are not fp16 numbers"
        ref, S = _reference(c, g, x16, w, scale, bias, resid)
        lim = 2.0 ** 13 if family == "int" else 2.0 ** 6
        assert float(S.max()) < lim, f"sum |x||w| = {float(S.max())} is not below {lim}"
        assert torch.equal(ref.float().double(), ref), "the fp64 reference is not an fp32 number"
        if family == "block":       # each half of the 64-channel rows is the live block of some output channel
            assert {int(n) % (g.K // 32) % 2 for n in range(c.Cout)} == {0, 1}
        got, out, written = _launch(c, g, x16, w, scale, bias, resid)
        name = f"{c.kernel} (plain) family {family}"
        _assert_sentinels(out, written, name)
        _assert_bits(got, ref, name)


# ---------------------------------------------------------------------------------------------------------------
# (b) random operands, (d) halo against gather
# ---------------------------------------------------------------------------------------------------------------
_MARGINS = {}


def _random(c, g, gen):
    x = F.silu(torch.randn(g.Tin, g.Hin, g.Win, c.Cin, generator=gen))            # what uv_vae_rms_silu writes
    x[:g.Tin - c.T] = 0
    if g.up >= 2:
        w = _wmat(_phase_weights(torch.randn(c.Cout, c.Cin, 1, 3, 3, generator=gen) * 0.05, (g.up - 2) >> 1, (g.up - 2) & 1))
    else:
        w = _wmat(torch.randn(c.Cout, c.Cin, g.kt, g.kh, g.kw, generator=gen) * 0.05)
    bias = torch.randn(c.Cout, generator=gen)
    resid = torch.randn(g.M, c.Cout, generator=gen) if c.resid else None
    return x, w, bias, resid


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv_f16_error_bound_on_random_operands(c):
    """Gates (b), (c), (d). SiLU(randn) activations rounded to fp16 (stored * 2^-7 with act_scale 2^7 where the case says so), randn * 0.05
    weights, randn bias and residual. Against the fp64 convolution of the fp16 operands the kernel reads, elementwise

        |got - ref64| <= (K + 2) 2^-24 S,      S = conv(|x16|, |w16|) + |bias| + |resid|:

    the products of two fp16 numbers are exact in fp32, so all that is left is K products summed in fp32 in any order and the bias and
    residual added, each step within half an ulp of a partial sum that S bounds; the descale is a power of two. A bound, not a
    measurement: loose at large K, which is why gate (a) exists. The largest err / bound per kernel is recorded."""
    g = _geom(c)
    gen = torch.Generator().manual_seed(88000 + CASES.index(c))
    x, w, bias, resid = (None if t is None else t.to(DEV) for t in _random(c, g, gen))
    x16 = (x / ACT_SCALE if c.ascale else x).to(F16)
    scale = _w_scale(w)
    ref, S = _reference(c, g, x16, w, scale, bias, resid)
    bound = (g.K + 2) * 2.0 ** -24 * S
    got, out, written = _launch(c, g, x16, w, scale, bias, resid)
    _assert_sentinels(out, written, c.kernel)
    ratio = (got.double() - ref).abs() / bound
    worst = float(ratio.max())
    cur = _MARGINS.setdefault(c.kernel, 0.0)
    _MARGINS[c.kernel] = max(cur, worst)
    record_margin("conv_f16/test_conv_f16_error_bound_on_random_operands", **dict(sorted(_MARGINS.items())))
    print(f"{c.kernel} (plain): K = {g.K}, max err / bound = {worst:.4f}, max |err| = {float((got.double() - ref).abs().max()):.3e}")
    assert bool((ratio <= 1.0).all()), f"{c.kernel}: err / bound reaches {worst} (K = {g.K})"
    if c.halo == 1:
        old, out0, written0 = _launch(c, g, x16, w, scale, bias, resid, halo=0)
        _assert_sentinels(out0, written0, c.kernel + " (gather)")
        assert float((got - old).abs().max()) <= 1e-5 * max(1.0, float(old.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# the table, the rejections
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_hits_all_eight_plain_instantiations():
    """The expected kernels of the table are exactly the eight that have a plain-row instantiation; both gather and halo kernels have a
    wide-row case, an act_scale case and a residual case; the big tiles each have a 1 x 326 x 400 case."""
    assert {c.kernel for c in CASES} == PLAIN_KERNELS
    assert all(c.Cin % 64 == 0 for c in CASES)
    for fam in ("G", "HALO"):
        mine = [c for c in CASES if c.kernel.startswith(fam)]
        assert any(c.wide for c in mine) and any(c.ascale for c in mine) and any(c.resid for c in mine)
    assert {c.kernel for c in CASES if (c.T, c.H, c.W) == (1, 326, 400)} == {"G256x128+4", "G256x256+4"}


def test_conv_f16_rejections():
    """Gate (e): Cin % 64 != 0, ld_in % 8 != 0 and a w_scale that is no power of two raise before any launch and leave a sentinel-filled
    output untouched; so does what conv_common refuses on the halved units (a row narrower than Cin); uv_vae_rms_silu(split_out = 3) raises
    for C % 64 != 0 and writes nothing."""
    _lib = L()
    x = torch.zeros(2, 6, 7, 96, device=DEV)
    w = torch.zeros(64 * 192 * 9, dtype=F16, device=DEV)
    bias = torch.zeros(64, device=DEV)
    out = torch.full((3, 6, 7, 64), SENT, device=DEV)
    ok = dict(ld_in=128, Cin=128, w_scale=4096.0)
    for over, match in [(dict(Cin=96, ld_in=96), "multiple of 64"), (dict(Cin=32, ld_in=32), "multiple of 64"), (dict(Cin=64, ld_in=68), "multiple of 8"),
                        (dict(w_scale=3.0), "power of two"), (dict(w_scale=0.0), "power of two"), (dict(ld_in=64), "leading")]:
        a = dict(ok)
        a.update(over)
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call("uv_conv3d_f16", _lib.ptr(x), a["ld_in"], 2, 6, 7, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), 64, 2, 6, 7, a["Cin"], 64,
                      1, 3, 3, 1, 1, 1, 0, 1, 1, 0, 0, None, 0, a["w_scale"], None, _lib.stream_ptr())
    rows, gamma = torch.randn(5, 96, device=DEV), torch.ones(96, device=DEV)
    dst = torch.full((5, 96), SENT, device=DEV)
    with pytest.raises(_lib.UnividHipError, match="64"):
        _lib.call("uv_vae_rms_silu", _lib.ptr(rows), 96, _lib.ptr(gamma), _lib.ptr(dst), 96, 5, 96, 1, 3, _lib.stream_ptr())
    with pytest.raises(_lib.UnividHipError, match="64"):
        _lib.vae_rms_silu(rows, gamma, dst, split=3)
    with pytest.raises(_lib.UnividHipError, match="split_out"):
        _lib.call("uv_vae_rms_silu", _lib.ptr(rows), 96, _lib.ptr(gamma), _lib.ptr(dst), 96, 5, 96, 1, 4, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((dst == SENT).all()), "a rejected call wrote to its output"
