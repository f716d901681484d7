"""GPU (-m gpu): every VAE convolution kernel the launch planner (plan_conv, csrc/conv_args.h) can select, called directly through the C ABI
and compared with an fp64 convolution of the same f32 operands.

The whole file is driven by ONE table (CASES). Every case names the kernel it expects, asserts `conv_plan(...)["kernel"]` before it
launches (UV_OPT_CONV_HALO 1 / 0 pins halo against gather; the big-tile thresholds are literal numbers, not CU counts), and the names in
the table are exactly the 23 of the library's name table (test_case_table_names_every_kernel).

Reference: the input is padded / upsampled with F.pad / F.interpolate(mode="nearest-exact") exactly as the geometry tests of
test_gpu_parity.py build it, unfolded (Tensor.unfold) into the [M, K] matrix of the implicit GEMM and multiplied in fp64;
test_unfold_reference_equals_conv3d ties that unfold to F.conv3d on the CPU at every small geometry of the table.

Gates:
  (a) bit-exact on designed operands (test_conv_kernel_is_bit_exact_on_designed_operands): every retained partial product and every
      partial sum is exact in fp32, so the result equals the fp64 reference bit for bit in every arithmetic and every kernel;
  (b) a derived elementwise bound on random operands (test_conv_kernel_error_bound_on_random_operands);
  (c) sentinels: every output buffer has a wider leading dimension where the case says so and one frame of slack behind it, pre-filled
      with SENT, and everything the kernel must not write - the slack, the columns behind Cout, the other three phases of an output-phase
      launch - is SENT afterwards; the slack columns of a wider input / residual row hold a huge finite value;
  (d) where a halo kernel and the gather kernel serve the same call they agree to 1e-5 x max(1, max|out|) (k order only);
  (e) what conv_common refuses raises UnividHipError and leaves the output untouched (test_conv_rejections).
The measured err / bound of (b) goes to the margins file through `record_margin` (profiles/conv_kernel_margins.json).
"""
import math
import os
import re
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from conftest import record_margin
from test_gpu_parity import _phase_weights, _split6, _split_f16_acts, _split_f16_weights

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
F64 = torch.float64
DEV = "cuda"
SENT = -7.25            # exact in fp32, bf16 and fp16
ENTRY = {0: "uv_conv3d_f32", 1: "uv_conv3d_bf16x3", 2: "uv_conv3d_bf16x3", 3: "uv_conv3d_bf16x6", 4: "uv_conv3d_f16x3"}
PIECE = {1: BF16, 2: BF16, 4: F16}       # the two-piece arithmetics' piece format
ACT_SCALE = 2.0 ** 7                     # the act_scale cases: activations stored as x * 2^-7, the device scalar is 2^7


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
# kernel: the name uv_conv3d_plan must report; halo: UV_OPT_CONV_HALO for the launch; geom (T, H, W = the input's frames and size,
# causal zero frames not counted):
#   c333   causal 3x3x3, two zero frames in front          c133  1x3x3, padding 1             c111  1x1x1
#   down   1x3x3 stride 2 behind ZeroPad2d(0, 1, 0, 1)     up    nearest-exact 2x + 1x3x3 (up = 1)
#   ph<u>  one 1x2x2 output-phase launch, up = u = 2 + 2a + b, padding (1 - a, 1 - b), stored at (2y + a, 2x + b)
#   tci    time_conv 3x1x1, two zero frames in front, channel halves interleaved into frames          ts2   3x1x1, time stride 2
# resid: a residual input; wide: ld_in = Cin + 32, ldo = Cout + 8, ldr = Cout + 12; ascale: uv_conv3d_f16x3's act_scale
Case = namedtuple("Case", "kernel prec halo geom T H W Cin Cout resid wide ascale")


def _c(kernel, prec, halo, geom, T, H, W, Cin, Cout, resid=False, wide=True, ascale=False):
    return Case(kernel, prec, halo, geom, T, H, W, Cin, Cout, resid, wide, ascale)


CASES = []
for _p in (1, 2, 4):
    # the big-tile gather kernels: >= 256 workgroups of 256 rows. 32 600 pixels = 127 whole row tiles and one of 88 rows; Cout 160 = one
    # 128-wide tile and 32 columns, 320 = one 256-wide tile and 64, 640 = two and a half
    CASES += [
        _c(f"G256x128+{_p}", _p, 0, "down", 1, 326, 400, 32, 160),
        _c(f"G256x256+{_p}", _p, 0, "down", 1, 326, 400, 32, 320, wide=_p != 1),
        _c(f"G256x256+{_p}", _p, 0, "tci", 1, 163, 200, 32, 512),
        _c(f"G256x256+{_p}", _p, 0, "ph3", 1, 163, 200, 32, 320),
        _c(f"G256x256+{_p}", _p, 0, "ph4", 1, 163, 200, 32, 320, wide=_p != 2),
        _c(f"G256x256+{_p}", _p, 0, "c111", 1, 110, 200, 32, 640, resid=True),
        _c(f"G256x128+{_p}", _p, 0, "c111", 1, 127, 256, 32, 320, resid=True, wide=False),
    ]
CASES += [
    _c("G256x256+4", 4, 0, "down", 1, 326, 400, 32, 320, ascale=True),
    _c("G256x128+4", 4, 0, "ph5", 1, 163, 200, 32, 160, ascale=True),
]
for _p in (1, 2):
    # uv_conv3d_bf16x3, in_split 0 / 1, at every geometry of test_conv3d_kernel_geometries (all on the 128 x 128 tile)
    _w = _p == 2
    CASES += [
        _c(f"G128x128+{_p}", _p, -1, "c333", 5, 6, 7, 64, 96, wide=_w),
        _c(f"G128x128+{_p}", _p, -1, "down", 5, 6, 7, 64, 64, wide=not _w),
        _c(f"G128x128+{_p}", _p, -1, "up", 5, 6, 7, 64, 64, wide=_w),
        _c(f"G128x128+{_p}", _p, -1, "ph2", 5, 6, 7, 64, 64, wide=not _w),
        _c(f"G128x128+{_p}", _p, -1, "ph3", 5, 6, 7, 64, 64, wide=_w),
        _c(f"G128x128+{_p}", _p, -1, "ph4", 5, 6, 7, 64, 64, wide=not _w),
        _c(f"G128x128+{_p}", _p, -1, "ph5", 5, 6, 7, 64, 64, wide=_w),
        _c(f"G128x128+{_p}", _p, -1, "tci", 5, 6, 7, 64, 128, wide=not _w),
        _c(f"G128x128+{_p}", _p, -1, "ts2", 5, 6, 7, 64, 64, wide=_w),
        _c(f"G128x128+{_p}", _p, -1, "c333", 3, 19, 23, 64, 12, wide=not _w),
        _c(f"G128x128+{_p}", _p, -1, "c333", 3, 19, 23, 64, 96, resid=True, wide=_w),
        _c(f"G128x128+{_p}", _p, -1, "c333", 3, 19, 23, 64, 160, wide=not _w),
        _c(f"G128x128+{_p}", _p, -1, "c333", 3, 19, 23, 64, 320, wide=_w),
    ]
CASES += [
    # the small gather kernels: frames that are no whole tiles, several workgroups, Cin 64 / 96
    _c("G256x16+0", 0, 0, "c333", 3, 19, 23, 64, 12),
    _c("G256x16+3", 3, 0, "c133", 3, 19, 23, 96, 16, resid=True),
    _c("G256x16+4", 4, 0, "c333", 3, 19, 23, 64, 12, ascale=True),
    _c("G160+0", 0, 0, "c133", 2, 19, 23, 96, 160, resid=True),
    _c("G160+0", 0, 0, "tci", 2, 19, 23, 64, 320),
    _c("G160+3", 3, 0, "c333", 2, 19, 23, 64, 320),
    _c("G160+3", 3, 0, "ph4", 2, 19, 23, 64, 160),
    _c("G128x128+0", 0, 0, "c333", 2, 19, 23, 96, 96, resid=True),
    _c("G128x128+0", 0, 0, "ph3", 2, 19, 23, 64, 128),
    _c("G128x128+3", 3, 0, "up", 2, 9, 13, 64, 128),
    _c("G128x128+3", 3, 0, "tci", 2, 19, 23, 64, 256),
    _c("G128x128+4", 4, 0, "down", 3, 19, 23, 64, 256),
    _c("G128x128+4", 4, 0, "tci", 2, 19, 23, 96, 128),
    _c("G128x128+4", 4, 0, "ph2", 2, 19, 23, 64, 96, wide=False),
    # the seven LDS-halo kernels (forced on: these launches are too small to take them by themselves)
    _c("HALO_BF16X6", 3, 1, "c333", 2, 19, 23, 64, 128, resid=True),
    _c("HALO_BF16X6", 3, 1, "up", 2, 9, 13, 32, 256),
    _c("HALO_F32_160", 0, 1, "c333", 2, 19, 23, 64, 160, resid=True),
    _c("HALO_F32_160", 0, 1, "c133", 2, 16, 33, 96, 320, wide=False),
    _c("HALO_F32_128", 0, 1, "c133", 2, 17, 40, 96, 128, resid=True),
    _c("HALO_F32_128", 0, 1, "up", 2, 9, 13, 64, 256),
    _c("HALO_F16_N16", 4, 1, "c333", 3, 19, 40, 64, 12, resid=True),
    _c("HALO_F16_N16", 4, 1, "c133", 2, 9, 33, 96, 16, ascale=True),
    _c("HALO_F16_160", 4, 1, "c333", 2, 16, 33, 32, 320, resid=True),
    _c("HALO_F16_160", 4, 1, "up", 2, 9, 13, 96, 160, ascale=True),
    _c("HALO_F16_SQUARE", 4, 1, "c133", 1, 13, 48, 64, 256, resid=True),
    _c("HALO_F16_SQUARE", 4, 1, "c333", 2, 45, 80, 64, 128, wide=False),
    _c("HALO_F16_128", 4, 1, "c333", 3, 19, 23, 64, 128, resid=True),
    _c("HALO_F16_128", 4, 1, "up", 2, 9, 13, 128, 128, ascale=True),
]
IDS = [f"{i:02d}-{c.kernel}-{c.geom}-{c.T}x{c.H}x{c.W}-{c.Cin}to{c.Cout}" + ("-r" if c.resid else "") + ("-wide" if c.wide else "") +
       ("-as" if c.ascale else "") for i, c in enumerate(CASES)]

Geom = namedtuple("Geom", "Tin Hin Win Tout Hout Wout kt kh kw st sh sw ph pw up inter M K")


def _geom(c):
    T, H, W = c.T, c.H, c.W
    g = dict(Tin=T, Hin=H, Win=W, Tout=T, Hout=H, Wout=W, kt=1, kh=1, kw=1, st=1, sh=1, sw=1, ph=0, pw=0, up=0, inter=0)
    if c.geom == "c333":
        g.update(Tin=T + 2, kt=3, kh=3, kw=3, ph=1, pw=1)
    elif c.geom == "c133":
        g.update(kh=3, kw=3, ph=1, pw=1)
    elif c.geom == "down":
        g.update(kh=3, kw=3, sh=2, sw=2, Hout=(H - 2) // 2 + 1, Wout=(W - 2) // 2 + 1)
    elif c.geom == "up":
        g.update(kh=3, kw=3, ph=1, pw=1, up=1, Hout=2 * H, Wout=2 * W)
    elif c.geom.startswith("ph"):
        u = int(c.geom[2:])
        g.update(kh=2, kw=2, up=u, ph=1 - ((u - 2) >> 1), pw=1 - ((u - 2) & 1))
    elif c.geom == "tci":
        g.update(Tin=T + 2, kt=3, inter=1)
    elif c.geom == "ts2":
        g.update(kt=3, st=2, Tout=(T - 3) // 2 + 1)
    else:
        assert c.geom == "c111", c.geom
    g["M"] = g["Tout"] * g["Hout"] * g["Wout"]
    g["K"] = g["kt"] * g["kh"] * g["kw"] * c.Cin
    return Geom(**g)


def _plan(c, g):
    return L().conv_plan(c.prec, g.Tout, g.Hout, g.Wout, g.Hin, g.Win, c.Cin, c.Cout, g.kt, g.kh, g.kw, g.st, g.sh, g.sw, g.ph, g.pw, g.up, g.inter)


# ---------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------------------------------------------
def _unfold(g, x):
    """x [Tin, Hin, Win, C] -> the [M, K] matrix of the implicit GEMM, k = (tap, channel) as the weights [Cout, kt, kh, kw, Cin] are laid
    out: upsample (up = 1), zero padding (left: the call's ph / pw; right: what the last output pixel's taps reach), sliding windows."""
    v = x.permute(3, 0, 1, 2)                                     # [C, T, H, W]
    if g.up == 1:
        v = F.interpolate(v.permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)
    He, We = v.shape[2:]
    v = F.pad(v, (g.pw, (g.Wout - 1) * g.sw + g.kw - We - g.pw, g.ph, (g.Hout - 1) * g.sh + g.kh - He - g.ph))
    assert (g.Tout - 1) * g.st + g.kt <= g.Tin
    u = v.unfold(1, g.kt, g.st).unfold(2, g.kh, g.sh).unfold(3, g.kw, g.sw)      # [C, To, Ho, Wo, kt, kh, kw]
    assert tuple(u.shape[1:4]) == (g.Tout, g.Hout, g.Wout), (tuple(u.shape), g)
    return u.permute(1, 2, 3, 4, 5, 6, 0).reshape(g.M, g.K)


def _wmat(w):
    """[Cout, Cin, kt, kh, kw] -> [Cout, K] with k = (tap, channel): the layout of every uv_conv3d_* weight argument"""
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# operands in the kernels' memory formats
# ---------------------------------------------------------------------------------------------------------------
def _pieces(x, dt):
    """hi = dt(x), lo = dt(x - hi), round to nearest: the two-piece split of bf16x3 (dt = bf16) and f16x3 (dt = fp16), as f32 values"""
    hi = x.to(dt).float()
    return hi, (x - hi).to(dt).float()


def _planes3(x):
    """the three bf16 planes of bf16x6"""
    p0 = x.to(BF16).float()
    p1 = (x - p0).to(BF16).float()
    return p0, p1, ((x - p0) - p1).to(BF16).float()


def _split_bf16_weights(wp):
    """uv_split_weights_bf16x3 of a [Cout, K] f32 weight matrix: [Cout][K / 32][32 hi | 32 lo] bf16 (+ a check against the split in torch)"""
    _lib = L()
    out = torch.empty(wp.numel() * 2, dtype=BF16, device=wp.device)
    _lib.call("uv_split_weights_bf16x3", _lib.ptr(wp), _lib.ptr(out), wp.numel(), _lib.stream_ptr())
    hi, lo = _pieces(wp, BF16)
    pl = out.view(wp.shape[0], -1, 2, 32).float()
    assert torch.equal(pl[:, :, 0], hi.view(wp.shape[0], -1, 32)) and torch.equal(pl[:, :, 1], lo.view(wp.shape[0], -1, 32)), "bf16x3 weight split"
    return out


def _split_bf16_acts(x_cl):
    """[.., C] f32 (C % 32 == 0) -> the same bytes holding [C/32][32 hi | 32 lo] bf16 per pixel: what uv_vae_rms_silu(split_out=1) writes."""
    hi = x_cl.to(BF16)
    lo = (x_cl - hi.float()).to(BF16)
    C = x_cl.shape[-1]
    both = torch.stack((hi.view(*x_cl.shape[:-1], C // 32, 32), lo.view(*x_cl.shape[:-1], C // 32, 32)), dim=-2)
    return both.reshape(*x_cl.shape[:-1], 2 * C).contiguous().view(F32)


def _slack(*shape):
    """A buffer of huge finite values whichever way its bytes are read: 0x77007700 is 2.6e33 as f32, 2^111 per bf16 half, 28 672 per fp16
    half. A kernel that reads the slack of a wide row cannot stay inside any gate."""
    return torch.full(shape, 0x77007700, dtype=torch.int32, device=DEV).view(F32)


def _widen(t, ld):
    """[.., C] f32-sized rows -> the first C slots of [.., ld] rows, the rest slack"""
    if ld == t.shape[-1]:
        return t.contiguous()
    buf = _slack(*t.shape[:-1], ld)
    buf[..., :t.shape[-1]] = t
    return buf


def _launch(c, g, x, wp, bias, resid, halo=None):
    """One call of the case's entry point on f32 operands x [Tin, Hin, Win, Cin], wp [Cout, K], bias [Cout], resid [M, Cout] | None (all on
    the device; with ascale, x is what the caller stores: the activations * 2^-7). Returns (got [M, Cout], the whole output buffer,
    the mask of what the launch had to write)."""
    _lib = L()
    _lib.set_option(_lib.OPT_CONV_HALO, c.halo if halo is None else halo)
    if halo is None:
        plan = _plan(c, g)
        assert plan["kernel"] == c.kernel, f"planned {plan}, the case expects {c.kernel}"
    ld_in, ldr = (c.Cin + 32, c.Cout + 12) if c.wide else (c.Cin, c.Cout)
    co = c.Cout // 2 if g.inter else c.Cout                       # channels of an output pixel
    ldo = co + 8 if c.wide else co
    extra = ()
    if c.prec == 3:
        wb = _split6(wp)
    elif c.prec == 4:
        wb, scale = _split_f16_weights(wp)
        hi, lo = _pieces(wp * scale, F16)
        pl = wb.view(c.Cout, -1, 2, 32).float()
        assert torch.equal(pl[:, :, 0], hi.view(c.Cout, -1, 32)) and torch.equal(pl[:, :, 1], lo.view(c.Cout, -1, 32)), "f16x3 weight split"
        asc = torch.full((4,), ACT_SCALE, device=DEV) if c.ascale else None
        extra = (scale, _lib.ptr(asc))
    elif c.prec in (1, 2):
        wb = _split_bf16_weights(wp)
        extra = (int(c.prec == 2),)
    else:
        wb = wp
    xin = _widen({2: _split_bf16_acts, 4: _split_f16_acts}.get(c.prec, lambda t: t)(x), ld_in)
    rin = None if resid is None else _widen(resid, ldr)
    # the output: [frames + one of slack, rows, columns, ldo], all SENT
    if g.inter:
        shape, frames = (2 * g.Tout + 1, g.Hout, g.Wout, ldo), 2 * g.Tout
    elif g.up >= 2:
        shape, frames = (g.Tout + 1, 2 * g.Hout, 2 * g.Wout, ldo), g.Tout
    else:
        shape, frames = (g.Tout + 1, g.Hout, g.Wout, ldo), g.Tout
    out = torch.full(shape, SENT, device=DEV)
    _lib.call(ENTRY[c.prec], _lib.ptr(xin), ld_in, g.Tin, g.Hin, g.Win, _lib.ptr(wb), _lib.ptr(bias), _lib.ptr(out), ldo, g.Tout, g.Hout, g.Wout,
              c.Cin, c.Cout, g.kt, g.kh, g.kw, g.st, g.sh, g.sw, 0, g.ph, g.pw, g.up, g.inter, _lib.ptr(rin), 0 if rin is None else ldr, *extra,
              _lib.stream_ptr())
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


def _assert_sentinels(out, written, name):
    rest = out[~written]
    assert rest.numel() > 0
    bad = int((rest != SENT).sum())
    assert bad == 0, f"{name}: {bad} elements outside the output region were written"
    inside = out[written]
    assert not bool((inside == SENT).all()), f"{name}: nothing was written"


def _assert_bits(got, ref64, name):
    """got (f32) equals the fp64 reference bit for bit (the reference is exactly representable: the caller checked)"""
    ref = ref64.float()
    bad = (got.view(torch.int32) != ref.view(torch.int32)) & ~((got == 0) & (ref == 0))       # +0 / -0: a sum that cancels may be either
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 reference; first at (pixel, channel) {i}: "
                             f"got {got[i].item()!r}, expected {ref[i].item()!r}")


# ---------------------------------------------------------------------------------------------------------------
# (a) bit-exact on designed operands
# ---------------------------------------------------------------------------------------------------------------
def _magnitudes(K):
    """(max |a| of the two-piece operand, max |integer operand|) with K (|a| + 2^-11) |w| + |bias| + |resid| < 2^13, the largest such pair"""
    for a, w in ((3, 3), (3, 2), (2, 2), (3, 1), (2, 1), (1, 1)):
        if K * (a + 2.0 ** -11) * w + 6 < 2 ** 13:
            return a, w
    raise AssertionError(f"K = {K}: no exact operand family")


def _rand_int(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _designed(c, g, family, gen):
    """(x [Tin, Hin, Win, Cin], w [Cout, K], bias, resid | None) f32 on the CPU; the causal zero frames in front stay zero."""
    amax, wmax = _magnitudes(g.K)
    xs, ws = (g.Tin, g.Hin, g.Win, c.Cin), (c.Cout, g.K)
    if family == "i":          # activations a + b 2^-11, everything else small integers
        x = _rand_int(gen, xs, -amax, amax) + _rand_int(gen, xs, -1, 1) * 2.0 ** -11
        w = _rand_int(gen, ws, -wmax, wmax)
    elif family == "ii":       # the mirror image: the weights carry the second piece
        x = _rand_int(gen, xs, -wmax, wmax)
        w = _rand_int(gen, ws, -amax, amax) + _rand_int(gen, ws, -1, 1) * 2.0 ** -11
    else:                      # iii / iii16: both operands +-1 + {-1, 0, 1} 2^-9 (2^-11: two pieces in fp16 too); effective K = 32: per output
        e = 2.0 ** -9 if family == "iii" else 2.0 ** -11      # channel ONE live (tap, 32-channel block), a different one from channel to channel
        lo = -1 if family == "iii" else 0                     # iii16: +-(1 + {0, 1} 2^-11) - 1 - 2^-11 is ONE fp16, and its square needs 2^-22
        x = (2 * _rand_int(gen, xs, 0, 1) - 1) * (1 + _rand_int(gen, xs, lo, 1) * e)
        w = (2 * _rand_int(gen, ws, 0, 1) - 1) * (1 + _rand_int(gen, ws, lo, 1) * e)
        live = torch.arange(c.Cout)[:, None] % (g.K // 32) == torch.arange(g.K)[None, :] // 32
        w = w * live
    x[:g.Tin - c.T] = 0
    bias = _rand_int(gen, (c.Cout,), -3, 3)
    resid = _rand_int(gen, (g.M, c.Cout), -3, 3) if c.resid else None
    return x, w, bias, resid


def _exact_reference(c, g, family, x, w, bias, resid):
    """The fp64 value of what the arithmetic retains, from operands on the device, and the three conditions under which the kernel must
    reproduce it bit for bit - asserted here, on the reference alone:
      1. the arithmetic's split reproduces both operands exactly;
      2. sum |x| |w| + |bias| + |resid| < 2^13 in families i and ii, where every product is a multiple of 2^-11 (one operand is an integer):
         every partial sum, in any order, under the accumulators' power-of-two scale or not, is a multiple of 2^-11 below 2^13 = 24 bits;
         < 2^6 in family iii, where the retained products are multiples of 2^-18 (iii16: of 2^-11);
      3. the fp64 result round-trips through fp32."""
    x64, w64 = x.double(), w.double()
    s = ACT_SCALE if c.ascale else 1.0              # x is stored as activations / s: powers of two, exact
    if c.prec in PIECE:
        sw = 1.0
        if c.prec == 4:
            sw = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))          # _split_f16_weights' scale rule
        xh, xl = _pieces(x, PIECE[c.prec])
        wh, wl = _pieces(w * sw, PIECE[c.prec])
        assert torch.equal(xh + xl, x) and torch.equal(wh + wl, w * sw), "the two-piece split does not reproduce the designed operands"
        Ah, Al = _unfold(g, xh.double()), _unfold(g, xl.double())
        ref = (Ah @ wh.double().T + Ah @ wl.double().T + Al @ wh.double().T) * (s / sw)         # the three retained terms
        if family in ("i", "ii"):
            assert float((Al @ wl.double().T).abs().max()) == 0.0, "families i / ii have no lo.lo term"
    else:
        if c.prec == 3:
            p = _planes3(x)
            q = _planes3(w)
            assert torch.equal((p[0] + p[1]) + p[2], x) and torch.equal((q[0] + q[1]) + q[2], w), "three bf16 planes do not reproduce the designed operands"
            assert float(p[2].abs().max()) == 0.0 and float(q[2].abs().max()) == 0.0       # so no term with i + j > 2 exists
        ref = _unfold(g, x64) @ w64.T * s
    S = _unfold(g, x64.abs()) @ w64.abs().T * s + bias.double().abs()
    ref = ref + bias.double()
    if resid is not None:
        ref = ref + resid.double()
        S = S + resid.double().abs()
    lim = 2.0 ** 13 if family in ("i", "ii") else 2.0 ** 6
    assert float(S.max()) < lim, f"sum |x||w| = {float(S.max())} is not below {lim}"
    assert torch.equal(ref.float().double(), ref), "the fp64 reference is not an fp32 number"
    return ref


def _families(c):
    return ("i", "ii", "iii") + (("iii16",) if c.prec == 4 else ())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv_kernel_is_bit_exact_on_designed_operands(c):
    """Gate (a) + (c). Operands whose every retained partial product and partial sum is exact in fp32:
      i     activations a + b 2^-11 (a integer, |a| <= 3, b in {-1, 0, 1}), weights / bias / residual small integers;
      ii    the mirror image, the weights carry the second piece;
      iii   both operands +-1 + {-1, 0, 1} 2^-9, one live (tap, 32-channel block) per output channel - a different one from channel to
            channel -, so the effective K is 32; iii16 (f16x3 only): +-(1 + {0, 1} 2^-11), which fp16 needs two pieces for (1 + 2^-9 is
            one fp16 number, and so is 1 - 2^-11).
    |a| and the integer range are chosen per case so that K max|x| max|w| + 6 < 2^13 (_magnitudes). In i and ii every product is a multiple
    of 2^-11 and every partial sum is below 2^13: 24 bits, exact in an fp32 accumulator in ANY order, under the power-of-two weight / activation
    scales of f16x3 too. In iii the retained products are multiples of 2^-18 (2^-9 for the three-pass modes, whose lo.lo term is dropped)
    and the sums stay below 2^6. bf16 (8 bits) and fp16 (11 bits) pieces hold a and b 2^-11 / 2^-9 apart exactly, three bf16 planes hold them
    with the third plane zero. So the kernel's result must EQUAL the fp64 value of what its arithmetic retains - the full product for
    f32 and bf16x6, hi.hi + hi.lo + lo.hi from the pieces for bf16x3 and f16x3 (identical to the full product in i and ii, where lo.lo = 0)
    - bit for bit: any wrong tap, channel block, lane, parity, interleave half or tile-edge row, any dropped or doubled pass shows.
    _exact_reference asserts the three conditions (split exact, sum bound, fp32 round trip) on the reference before it is trusted."""
    g = _geom(c)
    for fi, family in enumerate(_families(c)):
        gen = torch.Generator().manual_seed(1000 * CASES.index(c) + fi)
        x, w, bias, resid = (None if t is None else t.to(DEV) for t in _designed(c, g, family, gen))
        xs = x / ACT_SCALE if c.ascale else x
        ref = _exact_reference(c, g, family, xs, w, bias, resid)
        got, out, written = _launch(c, g, xs, w, bias, resid)
        name = f"{c.kernel} family {family}"
        _assert_sentinels(out, written, name)
        _assert_bits(got, ref, name)


# ---------------------------------------------------------------------------------------------------------------
# (b) derived bound on random operands
# ---------------------------------------------------------------------------------------------------------------
# u: the relative error of a product x w as the arithmetic represents it (eps16 = 2^-9 for a bf16 piece, 2^-11 for an fp16 piece: half an
# ulp of 8 / 11 significand bits).
#   two pieces, three passes: x = xh + xl + ex with |xl| <= eps16 (1 + eps16) |x| and |ex| <= eps16^2 |x|, w alike;
#     x w - (xh wh + xh wl + xl wh) = xl wl + ex w + (xh + xl) ew, so |.| <= 3 eps16^2 (1 + 4 eps16) |x w|:
#     bf16x3 (prec 1, 2): 3 2^-18 (1 + 2^-7); f16x3 (prec 4): 3 2^-22 (1 + 2^-9)
#   bf16x6 (prec 3): the planes hold x exactly, |x1| <= 2^-9 (1 + 2^-9) |x|, |x2| <= 2^-18 |x|; dropped: x1 w2 + x2 w1 + x2 w2
#     <= (2 2^-27 (1 + 2^-9) + 2^-36) |x w| < 2^-25 |x w|
#   f32: 0
U_REP = {0: 0.0, 1: 3 * 2.0 ** -18 * (1 + 2.0 ** -7), 2: 3 * 2.0 ** -18 * (1 + 2.0 ** -7), 3: 2.0 ** -25, 4: 3 * 2.0 ** -22 * (1 + 2.0 ** -9)}
_MARGINS = {}


def _random(c, g, gen):
    x = torch.randn(g.Tin, g.Hin, g.Win, c.Cin, generator=gen)
    if c.prec in (2, 4):
        x = F.silu(x)            # the pre-split forms take what uv_vae_rms_silu writes
    x[:g.Tin - c.T] = 0
    if g.up >= 2:                # an output-phase launch: the 3x3 weights of the upsampling convolution collapsed onto the phase's 2x2 taps
        w3 = torch.randn(c.Cout, c.Cin, 1, 3, 3, generator=gen) * 0.05
        w = _wmat(_phase_weights(w3, (g.up - 2) >> 1, (g.up - 2) & 1))
    else:
        w = _wmat(torch.randn(c.Cout, c.Cin, g.kt, g.kh, g.kw, generator=gen) * 0.05)
    bias = torch.randn(c.Cout, generator=gen)
    resid = torch.randn(g.M, c.Cout, generator=gen) if c.resid else None
    return x, w, bias, resid


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv_kernel_error_bound_on_random_operands(c):
    """Gates (b), (c), (d). randn activations (through SiLU for the pre-split forms, as the engine produces them; stored * 2^-7 with
    act_scale 2^7 where the case says so), randn * 0.05 weights, randn bias and residual. Elementwise against the fp64 convolution of
    the same f32 operands:

        |got - ref64| <= ((K + 2) 2^-24 + u) S + floor,      S = conv(|x|, |w|) + |bias| + |resid|

    (K + 2) 2^-24 S: K products summed in fp32 in any order, the bias and the residual added, each step within half an ulp of a partial
    sum that S bounds. u: the arithmetic's representation of a product, derived above U_REP. floor: fp16 lo pieces below 2^-14 are subnormal,
    spaced 2^-24: |x - xh - xl| <= 2^-25 absolutely (also where xh itself is subnormal), for the stored activations x / s and for the scaled
    weights w * scale; through the product and the descale, floor = 2^-25 (1 + 2^-9) (s sum_k |w_k| + sum_k |x_k| / scale) + K 2^-48 s / scale
    (the last term: both lo pieces subnormal), s = act_scale or 1, scale = the weights' power of two. Zero for the other arithmetics: bf16 has
    fp32's exponent range. This is a bound, not a measurement; at large K it is loose (it grows with K, the error with sqrt(K)), which is
    why gate (a) exists. The largest err / bound per kernel is recorded."""
    g = _geom(c)
    gen = torch.Generator().manual_seed(77000 + CASES.index(c))
    x, w, bias, resid = (None if t is None else t.to(DEV) for t in _random(c, g, gen))
    s = ACT_SCALE if c.ascale else 1.0
    xs = x / s                                                            # exact; what the caller stores
    A = _unfold(g, x.double())
    ref = A @ w.double().T + bias.double()
    S = A.abs() @ w.double().abs().T + bias.double().abs()
    if resid is not None:
        ref, S = ref + resid.double(), S + resid.double().abs()
    bound = ((g.K + 2) * 2.0 ** -24 + U_REP[c.prec]) * S
    if c.prec == 4:
        scale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
        bound = bound + 2.0 ** -25 * (1 + 2.0 ** -9) * (s * w.double().abs().sum(1)[None, :] + A.abs().sum(1)[:, None] / scale) + g.K * 2.0 ** -48 * s / scale
    got, out, written = _launch(c, g, xs, w, bias, resid)
    _assert_sentinels(out, written, c.kernel)
    ratio = (got.double() - ref).abs() / bound
    worst = float(ratio.max())
    cur = _MARGINS.setdefault(c.kernel, {"cases": 0, "max_err_over_bound": 0.0})
    cur["cases"] += 1
    cur["max_err_over_bound"] = max(cur["max_err_over_bound"], worst)
    record_margin("conv/test_conv_kernel_error_bound_on_random_operands", **{k: v["max_err_over_bound"] for k, v in sorted(_MARGINS.items())})
    print(f"{c.kernel}: K = {g.K}, max err / bound = {worst:.4f}, max |err| = {float((got.double() - ref).abs().max()):.3e}")
    assert bool((ratio <= 1.0).all()), f"{c.kernel}: err / bound reaches {worst} (K = {g.K})"
    if c.halo == 1:
        # (d) the gather kernel on the same call: the same terms in another k order
        old, out0, written0 = _launch(c, g, xs, w, bias, resid, halo=0)
        _assert_sentinels(out0, written0, c.kernel + " (gather)")
        assert float((got - old).abs().max()) <= 1e-5 * max(1.0, float(old.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# the table itself, the reference, the rejections
# ---------------------------------------------------------------------------------------------------------------
def test_case_table_names_every_kernel():
    """The kernels the cases expect are exactly the 23 of the library's name table (kConvKernelName next to enum ConvKernel); every kernel is
    under gates (a) i / ii / iii, (b) and (c), at least one case of each family - gather, halo, halo16 - and of each output form - plain,
    interleave, phase - has the wider leading dimensions, and both uv_conv3d_bf16x3 forms cover the geometries of test_conv3d_kernel_geometries."""
    src = open(os.path.join(os.path.dirname(L().LIB_PATH), "csrc", "conv_args.h")).read()
    names = re.findall(r'"([^"]+)"', re.search(r"kConvKernelName\[[^\]]*\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1))
    assert len(names) == 23 and len(set(names)) == 23
    assert {c.kernel for c in CASES} == set(names)
    fam = lambda c: "halo16" if c.kernel.startswith("HALO_F16") else "halo" if c.kernel.startswith("HALO") else "gather"
    form = lambda c: "interleave" if c.geom == "tci" else "phase" if c.geom.startswith("ph") else "plain"
    wide = {(fam(c), form(c)) for c in CASES if c.wide}
    assert wide == {("gather", "plain"), ("gather", "interleave"), ("gather", "phase"), ("halo", "plain"), ("halo16", "plain")}
    for p in (1, 2):
        have = {(c.geom, c.Cout) for c in CASES if c.prec == p and c.kernel.startswith("G128x128")}
        assert have >= {("c333", 96), ("down", 64), ("up", 64), ("ph2", 64), ("ph3", 64), ("ph4", 64), ("ph5", 64), ("tci", 128), ("ts2", 64),
                        ("c333", 12), ("c333", 160), ("c333", 320)}
    assert any(c.ascale and c.kernel.startswith("G") for c in CASES) and any(c.ascale and c.kernel.startswith("HALO") for c in CASES)


def test_unfold_reference_equals_conv3d():
    """The reference of this file (pad / upsample, Tensor.unfold, fp64 matmul) against F.conv3d in fp64 on the CPU, at every geometry
    of the table with at most 4 000 output pixels: the two are the same sum in another order, so they agree to 1e-12 of sum |x||w|."""
    seen = set()
    for c in CASES:
        g = _geom(c)
        key = (c.geom, c.T, c.H, c.W, c.Cin, c.Cout)
        if g.M > 4000 or key in seen:
            continue
        seen.add(key)
        gen = torch.Generator().manual_seed(len(seen))
        x = torch.randn(g.Tin, g.Hin, g.Win, c.Cin, generator=gen, dtype=F64)
        w = torch.randn(c.Cout, c.Cin, g.kt, g.kh, g.kw, generator=gen, dtype=F64)
        mine = _unfold(g, x) @ _wmat(w).T
        v = x.permute(3, 0, 1, 2)[None]
        if g.up == 1:
            v = F.interpolate(v[0].permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest-exact").permute(1, 0, 2, 3)[None]
        He, We = v.shape[3:]
        v = F.pad(v, (g.pw, (g.Wout - 1) * g.sw + g.kw - We - g.pw, g.ph, (g.Hout - 1) * g.sh + g.kh - He - g.ph))
        ref = F.conv3d(v, w, stride=(g.st, g.sh, g.sw))[0, :, :g.Tout].permute(1, 2, 3, 0).reshape(g.M, c.Cout)
        S = _unfold(g, x.abs()) @ _wmat(w).abs().T
        assert bool(((mine - ref).abs() <= 1e-12 * S + 1e-300).all()), key
    assert len(seen) >= 30


def test_conv_rejections():
    """Gate (e): what conv_common (and uv_conv3d_f16x3 for its scale) refuses raises UnividHipError before any launch and leaves a
    sentinel-filled output untouched - through every entry point."""
    _lib = L()
    x = torch.zeros(2, 6, 7, 96, device=DEV)
    w = torch.zeros(64 * 96 * 9 * 3, device=DEV)              # room for every weight format at Cout <= 64, K <= 9 * 96
    bias, res = torch.zeros(64, device=DEV), torch.zeros(2 * 6 * 7, 64, device=DEV)
    out = torch.full((5, 12, 14, 64), SENT, device=DEV)
    ok = dict(ld_in=64, Cin=64, Cout=64, kt=1, kh=3, kw=3, st=1, sh=1, sw=1, ph=1, pw=1, up=0, inter=0, resid=None, ldo=64)
    bad = [(dict(Cin=48, ld_in=48), "multiple of 32"), (dict(Cout=10), "multiple of 4"), (dict(inter=1, kh=1, kw=1, ph=0, pw=0, resid=res), "interleave"),
           (dict(inter=1, kh=1, kw=1, ph=0, pw=0, Cout=12), "interleave"), (dict(up=3, kh=2, kw=2, sh=2, sw=2), "output-phase"),
           (dict(up=2, kh=2, kw=2, resid=res), "output-phase"), (dict(up=6), "up=6"), (dict(ld_in=32), "leading"), (dict(ld_in=66), "leading"),
           (dict(ldo=62), "leading"), (dict(kt=0), "geometry")]
    for prec in (0, 1, 2, 3, 4):
        extra = {1: (0,), 2: (1,), 4: (4096.0, None)}.get(prec, ())
        for over, match in bad + ([(dict(w_scale=3.0), "power of two"), (dict(w_scale=0.0), "power of two")] if prec == 4 else []):
            a = dict(ok)
            a.update(over)
            if "w_scale" in a:
                extra = (a["w_scale"], None)
            with pytest.raises(_lib.UnividHipError, match=match):
                _lib.call(ENTRY[prec], _lib.ptr(x), a["ld_in"], 2, 6, 7, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), a["ldo"], 2, 6, 7, a["Cin"], a["Cout"],
                          a["kt"], a["kh"], a["kw"], a["st"], a["sh"], a["sw"], 0, a["ph"], a["pw"], a["up"], a["inter"], _lib.ptr(a["resid"]),
                          0 if a["resid"] is None else 64, *extra, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "a rejected call wrote to its output"
