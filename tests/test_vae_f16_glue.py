"""GPU (-m gpu): the producers of the single-pass fp16 convolution's operands (the VAE's opt-in precision="f16"), through the C ABI:
uv_vae_rms_silu(split_out = 3), uv_vae_cast_f16 and uv_cast_weights_f16. Each writes PLAIN fp16 that must equal, bit for bit, the hi
pieces of the corresponding f16x3 producer (split_out = 2, uv_vae_split_f16, uv_split_weights_f16x3) - those are tested against torch
elsewhere (test_glue_kernels.py, test_gpu_parity.py) - and nothing outside the C / 2 f32-sized slots of a row.
"""
import math

import pytest
import torch

from test_conv_kernels import DEV, SENT, _c, _geom, _unfold, _wmat

pytestmark = pytest.mark.gpu

F16, F32, I16 = torch.float16, torch.float32, torch.int16


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


def L():
    from univid_amd import _lib
    return _lib


def _hi_pieces(split_rows, C):
    """[P, >= C] f32-sized rows holding [C/32][32 hi | 32 lo] fp16 -> the hi pieces [P, C] as int16 bit patterns"""
    P = split_rows.shape[0]
    return split_rows[:, :C].contiguous().view(I16).view(P, C // 32, 2, 32)[:, :, 0].reshape(P, C)


def _plain(rows, C):
    """[P, >= C / 2] f32-sized rows holding C plain fp16 -> [P, C] int16 bit patterns"""
    return rows[:, :C // 2].contiguous().view(I16)


@pytest.mark.parametrize("C", [64, 256, 320, 1024])
@pytest.mark.parametrize("P", [1, 3, 17, 33])
def test_rms_silu_plain_fp16_equals_the_hi_pieces(C, P):
    """split_out = 3 against split_out = 2 on the same rows (wide input rows, wide output rows, with and without SiLU): the C fp16 values
    in the first C / 2 slots are the hi pieces bit for bit; the slots behind C / 2 and the slack rows keep the sentinel. Row counts around
    the kernel's rows per wave (4 / 2 / 1) and per block; C = 320 has a partly filled last chunk per lane."""
    _lib = L()
    gen = torch.Generator().manual_seed(100 * C + P)
    ld_in, ld_out = C + 12, C + 8
    x = torch.full((P, ld_in), 1.0e30)
    x[:, :C] = torch.randn(P, C, generator=gen) * torch.rand(P, 1, generator=gen) * 4
    gamma = torch.randn(C, generator=gen)
    x, gamma = x.to(DEV), gamma.to(DEV)
    for silu in (1, 0):
        two = torch.full((P + 2, ld_out), SENT, device=DEV)
        three = torch.full((P + 2, ld_out), SENT, device=DEV)
        _lib.call("uv_vae_rms_silu", _lib.ptr(x), ld_in, _lib.ptr(gamma), _lib.ptr(two), ld_out, P, C, silu, 2, _lib.stream_ptr())
        _lib.call("uv_vae_rms_silu", _lib.ptr(x), ld_in, _lib.ptr(gamma), _lib.ptr(three), ld_out, P, C, silu, 3, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(_plain(three[:P], C), _hi_pieces(two[:P], C))
        assert bool((three[:P, C // 2:] == SENT).all()) and bool((three[P:] == SENT).all())
        assert bool(torch.isfinite(three[:P, :C // 2].contiguous().view(F16).float()).all())
    # the checked wrapper: out may be exactly C / 2 slots wide
    narrow = torch.full((P, C // 2), SENT, device=DEV)
    _lib.vae_rms_silu(x[:, :C], gamma, narrow, silu=False, split=3)
    assert torch.equal(narrow.view(I16), _plain(three[:P], C))


def test_cast_weights_f16_equals_the_hi_pieces():
    """uv_cast_weights_f16 against uv_split_weights_f16x3 under the same power-of-two scale, and against the cast in torch; a scale that is
    no power of two, or a length that is no multiple of 64, raises."""
    _lib = L()
    gen = torch.Generator().manual_seed(5)
    w = (torch.randn(96, 9 * 64, generator=gen) * 0.05).to(DEV)
    w[0, 0], w[1, 1] = 1.0e-10, 0.0                                   # a weight whose scaled value is a subnormal fp16, and a zero
    scale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    split = torch.empty(2 * w.numel(), dtype=F16, device=DEV)
    plain = torch.full((w.numel() + 64,), SENT, dtype=F16, device=DEV)
    _lib.call("uv_split_weights_f16x3", _lib.ptr(w), _lib.ptr(split), w.numel(), scale, _lib.stream_ptr())
    _lib.call("uv_cast_weights_f16", _lib.ptr(w), _lib.ptr(plain), w.numel(), scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    hi = split.view(-1, 2, 32)[:, 0].reshape(-1)
    assert torch.equal(plain[:w.numel()].view(I16), hi.view(I16)) and torch.equal(plain[:w.numel()], (w * scale).to(F16).view(-1))
    assert bool((plain[w.numel():] == SENT).all())
    assert torch.equal(_lib.cast_weights_f16(w, torch.empty(w.numel(), dtype=F16, device=DEV), scale), plain[:w.numel()])
    for n, s, match in ((w.numel(), 3.0, "power of two"), (w.numel() - 32, scale, "multiple of 64")):
        with pytest.raises(_lib.UnividHipError, match=match):
            _lib.call("uv_cast_weights_f16", _lib.ptr(w), _lib.ptr(plain), n, s, _lib.stream_ptr())


@pytest.mark.parametrize("big", [False, True], ids=["ordinary", "3e6"])
def test_vae_cast_f16_scale_and_codes(big):
    """uv_vae_cast_f16 against uv_vae_split_f16 on the same raw feature map (contiguous and wide rows). Ordinary magnitudes: scale 1 and
    bytes equal to the hi pieces. With an element of 3e6: the same 1 / s = 2^7 that uv_vae_split_f16 reports, codes equal to fp16(x s) and
    to its hi pieces, and a uv_conv3d_f16 fed with codes and scale is finite and inside the random-operand bound of test_conv_f16.py,
    |got - ref64| <= (K + 2) 2^-24 S, against the fp64 convolution of the codes."""
    _lib = L()
    gen = torch.Generator().manual_seed(31)
    T, H, W, C, Cout = 2, 9, 11, 128, 96
    x = torch.randn(T, H, W, C, generator=gen)
    if big:
        x[1, 4, 6, 5] = 3.0e6
        x[0, 0, 0, 9] = -7.0e4
    x = x.to(DEV)
    P = T * H * W
    codes, sc = torch.full((P + 1, C // 2), SENT, device=DEV), torch.full((2,), 7.0, device=DEV)
    split, sc2 = torch.empty(P, C, device=DEV), torch.full((2,), 7.0, device=DEV)
    _lib.call("uv_vae_cast_f16", _lib.ptr(x), C, _lib.ptr(codes), C // 2, P, C, _lib.ptr(sc), _lib.stream_ptr())
    _lib.call("uv_vae_split_f16", _lib.ptr(x), C, _lib.ptr(split), C, P, C, _lib.ptr(sc2), _lib.stream_ptr())
    torch.cuda.synchronize()
    inv = float(sc[0])
    assert torch.equal(sc, sc2), (sc, sc2)
    assert inv == (2.0 ** 7 if big else 1.0), inv
    assert torch.equal(_plain(codes[:P], C), _hi_pieces(split, C))
    assert torch.equal(codes[:P].contiguous().view(F16), (x.view(P, C) / inv).to(F16))
    assert bool((codes[P:] == SENT).all())
    # wide rows in and out: the same codes and scale, nothing behind C / 2
    wide_in, wide_out, sc3 = torch.full((P, C + 32), 5.0e8, device=DEV), torch.full((P + 1, C // 2 + 8), SENT, device=DEV), torch.zeros(2, device=DEV)
    wide_in[:, :C] = x.view(P, C)
    _lib.call("uv_vae_cast_f16", _lib.ptr(wide_in), C + 32, _lib.ptr(wide_out), C // 2 + 8, P, C, _lib.ptr(sc3), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(wide_out[:P, :C // 2], codes[:P]) and torch.equal(sc3, sc)
    assert bool((wide_out[:P, C // 2:] == SENT).all()) and bool((wide_out[P:] == SENT).all())
    # the checked wrapper
    out_w, sc_w = torch.empty(T, H, W, C // 2, device=DEV), torch.empty(2, device=DEV)
    _lib.vae_cast_f16(x, out_w, sc_w)
    assert torch.equal(out_w.view(P, C // 2), codes[:P]) and torch.equal(sc_w, sc)
    for bad_c, ldo in ((96, 64), (128, 32)):
        with pytest.raises(_lib.UnividHipError):
            _lib.call("uv_vae_cast_f16", _lib.ptr(x), C, _lib.ptr(codes), ldo, P, bad_c, _lib.ptr(sc3), _lib.stream_ptr())
    # a 1x3x3 convolution fed with codes and scale
    c = _c("-", 4, 0, "c133", T, H, W, C, Cout)
    g = _geom(c)
    w = (_wmat(torch.randn(Cout, C, 1, 3, 3, generator=gen) * 0.05)).to(DEV)
    bias = torch.randn(Cout, generator=gen).to(DEV)
    scale = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    w16 = torch.empty(w.numel(), dtype=F16, device=DEV)
    _lib.call("uv_cast_weights_f16", _lib.ptr(w), _lib.ptr(w16), w.numel(), scale, _lib.stream_ptr())
    out = torch.empty(T, H, W, Cout, device=DEV)
    _lib.call("uv_conv3d_f16", _lib.ptr(codes), C, T, H, W, _lib.ptr(w16), _lib.ptr(bias), _lib.ptr(out), Cout, T, H, W, C, Cout,
              1, 3, 3, 1, 1, 1, 0, 1, 1, 0, 0, None, 0, scale, _lib.ptr(sc), _lib.stream_ptr())
    torch.cuda.synchronize()
    A = _unfold(g, codes[:P].contiguous().view(F16).view(T, H, W, C).double()) * inv
    wd = w16.view(Cout, -1).double() / scale
    ref = A @ wd.T + bias.double()
    S = A.abs() @ wd.abs().T + bias.double().abs()
    assert bool(torch.isfinite(out).all())
    err = (out.view(P, Cout).double() - ref).abs()
    assert bool((err <= (g.K + 2) * 2.0 ** -24 * S).all()), float((err / S).max())
    # and against the convolution of the f32 operands: two operands rounded to 11 bits, 2^-11 relative each (2^-9 leaves room for the
    # elements that x * s makes subnormal)
    full = _unfold(g, x.double()) @ w.double().T + bias.double()
    assert float((out.view(P, Cout).double() - full).abs().max()) <= 2.0 ** -9 * float(S.max())
