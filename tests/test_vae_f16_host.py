"""CPU: the host side of the VAE's opt-in narrow arithmetic precision="f16" - error texts, the configuration field, the ctypes
signatures of the four new C ABI entries against include/univid_hip.h, and the wrappers' argument checks (which run before the library is
touched, so CPU tensors exercise them)."""
import dataclasses
import os
import re

import pytest
import torch

from univid_amd import _lib
from univid_amd.model_pipeline import CrossAttentionConfig
from univid_amd.wan import vae2_2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small():
    return vae2_2.WanVAE_(dim=32, dec_dim=32, z_dim=48)


def test_engine_error_text_names_f16_and_other_strings_still_raise():
    m = _small()
    for bad in ("fp16", "f16x2", "half", ""):
        with pytest.raises(ValueError, match="'f16'") as e:
            vae2_2._Engine(m, bad)
        assert "'f16x3'" in str(e.value) and "'fp32'" in str(e.value)
    eng = vae2_2._Engine(m, "f16")              # construction needs no GPU
    assert eng.precision == "f16"


def test_prepare_refuses_a_cpu_model_in_the_mode_too():
    with pytest.raises(_lib.UnividHipError, match="no CPU path"):
        _small().prepare("f16")


def test_split_fmt_is_plain_only_for_whole_64_channel_rows():
    m = _small()
    norm = vae2_2.RMS_norm(64, images=False)
    f16, x3 = vae2_2._Engine(m, "f16"), vae2_2._Engine(m, "f16x3")
    assert [f16.split_fmt(norm, c, 64) for c in (32, 64, 96, 128, 160, 320, 1024)] == [2, 3, 2, 3, 2, 3, 3]
    assert [x3.split_fmt(norm, c, 64) for c in (32, 64, 96, 128)] == [2, 2, 2, 2]
    assert f16.split_fmt(norm, 48, 64) == 0 and f16.split_fmt(norm, 64, 6) == 0
    big = vae2_2.RMS_norm(64, images=False)
    with torch.no_grad():
        big.gamma.mul_(1e5)
    assert f16.split_fmt(big, 64, 64) == 0 and f16._fmt[big] == 0 and f16._fmt[norm] == 2


def test_conv_op_carries_the_fp16_weight_operand():
    op = vae2_2._ConvOp(torch.nn.Conv2d(64, 64, 3, padding=1), is2d=True)
    assert op.w_f16 is None and op.w_split_f16 is None
    for ph in op.phases():
        assert ph.w_f16 is None and ph.w_split_f16 is None and (ph.kh, ph.kw) == (2, 2)
    assert op.cache(4, 4).shape == (2, 4, 4, 64) and op.cache(4, 4, slots=32).shape == (2, 4, 4, 32)
    assert op.cache(4, 4) is op.cache(4, 4, slots=64) and op.cache(4, 4, slots=32) is not op.cache(4, 4)


def test_config_field_defaults_to_none():
    f = {x.name: x for x in dataclasses.fields(CrossAttentionConfig)}["vae_precision"]
    assert f.default is None and CrossAttentionConfig().vae_precision is None
    assert CrossAttentionConfig(vae_precision="f16").vae_precision == "f16"


def test_signatures_of_the_new_entries_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "univid_hip.h")).read()
    P, L, I, F = _lib._P, _lib._L, _lib._I, _lib._F

    def cls(t):
        t = t.strip()
        return P if "*" in t else {"long": L, "int": I, "float": F}[t.rsplit(" ", 1)[0].replace("const ", "").strip()]
    for name in ("uv_conv3d_f16", "uv_cast_weights_f16", "uv_vae_cast_f16", "uv_vae_rms_silu"):
        args = re.search(rf"\bint {name}\((.*?)\);", hdr, flags=re.S).group(1)
        assert [cls(a) for a in args.split(",")] == _lib.SIGNATURES[name], name
    # uv_conv3d_f16 takes the argument list of uv_conv3d_f16x3
    assert _lib.SIGNATURES["uv_conv3d_f16"] == _lib.SIGNATURES["uv_conv3d_f16x3"]
    assert _lib.SIGNATURES["uv_vae_cast_f16"] == _lib.SIGNATURES["uv_vae_split_f16"]
    assert _lib.SIGNATURES["uv_cast_weights_f16"] == _lib.SIGNATURES["uv_split_weights_f16x3"]
    assert _lib._CONV["f16"] == ("uv_conv3d_f16", torch.float16, 1)


def test_wrappers_check_the_plain_formats_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a rejected call reached the library"))
    E = _lib.UnividHipError
    z = torch.zeros
    w16 = z(4, 64, dtype=torch.float16)
    conv = lambda prec, src, split, Cin=64: _lib.conv3d(prec, src, lambda kind: (w16, 1.0), z(4), z(3, 2, 2, 4), 3, 2, 2, 3, 2, 2, Cin, 4, 1, 1, 1,
                                                         in_split=split)
    with pytest.raises(E, match="conv3d.src: tensor must live on the GPU"):       # well-formed: plain rows are Cin / 2 f32-sized slots
        conv("f16", z(3, 2, 2, 32), 3)
    with pytest.raises(E, match="conv3d.src: the kernel addresses"):
        conv("f16", z(3, 2, 2, 16), 3)
    with pytest.raises(E, match="belong to precision 'f16'"):
        conv("f16x3", z(3, 2, 2, 32), 3)
    with pytest.raises(E, match="Cin % 64"):
        _lib.conv3d("f16", z(3, 2, 2, 16), lambda kind: (z(4, 32, dtype=torch.float16), 1.0), z(4), z(3, 2, 2, 4), 3, 2, 2, 3, 2, 2, 32, 4, 1, 1, 1, in_split=3)
    with pytest.raises(E, match="conv3d.weights: expected"):
        _lib.conv3d("f16", z(3, 2, 2, 32), lambda kind: (z(4, 64), 1.0), z(4), z(3, 2, 2, 4), 3, 2, 2, 3, 2, 2, 64, 4, 1, 1, 1, in_split=3)
    # in f16 mode the other formats keep their entries
    seen = []
    monkeypatch.setattr(_lib, "_check", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: seen.append(name))
    monkeypatch.setattr(_lib, "ptr", lambda t: 0)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    for split in (0, 2, 3):
        conv("f16", z(3, 2, 2, 64), split)
    assert seen == ["uv_conv3d_bf16x6", "uv_conv3d_f16x3", "uv_conv3d_f16"]
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a rejected call reached the library"))
    with pytest.raises(E, match="vae_rms_silu.out: tensor must live on the GPU|vae_rms_silu.x: tensor must live"):
        _lib.vae_rms_silu(z(5, 64), z(64), z(5, 32), split=3)
    with pytest.raises(E, match="vae_rms_silu.out: the kernel addresses"):
        _lib.vae_rms_silu(z(5, 64), z(64), z(5, 16), split=3)
    with pytest.raises(E, match="C % 64"):
        _lib.vae_rms_silu(z(5, 96), z(96), z(5, 96), split=3)
    with pytest.raises(E, match="vae_cast_f16.x: tensor must live on the GPU"):
        _lib.vae_cast_f16(z(5, 64), z(5, 32), z(2))
    with pytest.raises(E, match="vae_cast_f16.out: the kernel addresses"):
        _lib.vae_cast_f16(z(5, 64), z(5, 16), z(2))
    with pytest.raises(E, match="multiple of 64"):
        _lib.vae_cast_f16(z(5, 96), z(5, 48), z(2))
    with pytest.raises(E, match="cast_weights_f16.out: expected"):
        _lib.cast_weights_f16(z(4, 64), z(4, 64), 2.0)
    with pytest.raises(E, match="cast_weights_f16.w: tensor must live on the GPU"):
        _lib.cast_weights_f16(z(4, 64), w16, 2.0)
