"""GPU (-m gpu): the VAE's opt-in narrow arithmetic precision="f16": every convolution that f16x3 runs in three fp16 MFMA passes and whose
input channel count is a multiple of 64 runs ONE pass on plain fp16 operands; everything else is f16x3's.

References, both on the CPU from oracle/wan_vae.py (nothing there changes):
  truth      the oracle in fp64;
  emulation  the same oracle in fp64 with the covered convolutions' operands rounded to fp16 the way the engine hands them over
             (_F16Oracle below): activations fp16(x), weights fp16(w s_w) / s_w under the power-of-two rule of uv_split_weights_f16x3,
             the upsampling 3x3 convolutions in their four-phase form with the PHASE weights rounded.
Widths: a 64-wide VAE (every three-pass convolution covered) and the production widths, both at z [48, 2, 2, 3] / video [3, 5, 32, 48].

Gates: 1 finite; 2 rms(hip - truth) / rms(emulation - truth) <= 1.02 (the project's truth-ratio gate); 3 rel_rms(hip, emulation) <=
measured x 1.2 (GATE3, profiles/vae_f16_parity_margins.json); 4 rms(f16 - truth) >= 50 x rms(f16x3 - truth): a mode that silently ran
three passes fails it.
Measured on MI355X: truth ratios 0.95-0.99; f16 lands 303 x (decode) / 334 x (encode) further from the truth than f16x3 at full width,
615 x / 671 x at 64 channels. Gate 3's distance (5.2e-4 .. 7.5e-4 relative) is of the size of the mode's own error, not below it: the
engine rounds f32 values, the emulation fp64 ones, a rounding that falls the other way is a perturbation as large as any other rounding of
the format, and the later layers carry it on. It pins the engine to the emulation's neighbourhood; gate 2 is the statistical one.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import record_margin
from test_gpu_parity import _phase_weights, _tiny_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F64 = torch.float16, torch.float64
# rel_rms(hip, emulation) measured on MI355X (profiles/vae_f16_parity_margins.json) x 1.2
GATE3 = {("w64", "dec"): 9.05e-4, ("w64", "enc"): 6.63e-4, ("full", "dec"): 8.08e-4, ("full", "enc"): 6.23e-4}


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def _rel_rms(a, b):
    return _rms(a.double().cpu() - b.double().cpu()) / _rms(b)


# ---------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------
def _r16(x):
    """fp16(x) as the engine stores an activation: the per-tensor scale of uv_vae_cast_f16 is 1 below 2^15 (asserted)"""
    assert float(x.abs().max()) < 2.0 ** 15
    return x.to(F16).to(x.dtype)


def _w16(w):
    """fp16(w s) / s, s the power of two that puts max |w| into [2^13, 2^14) (one scale per convolution)"""
    s = 2.0 ** (13 - math.floor(math.log2(float(w.abs().max()))))
    return (w * s).to(F16).to(w.dtype) / s


def _make_emulation():
    from oracle import wan_vae

    class _F16Oracle(wan_vae.WanVAE):
        """oracle/wan_vae.WanVAE with the operands of the convolutions precision="f16" covers rounded to fp16. Covered, as in
        univid_amd/wan/vae2_2.py: the convolutions behind an RMS_norm (ResidualBlock residual.2 / residual.6, the heads) whose norm passes
        the sqrt(C) max|gamma| < 6e4 range check, Resample's 3x3 convolutions and the upsampling time_conv - each only with Cin % 64 == 0.
        Not covered: conv1 of encoder and decoder (raw, padded input), the downsampling time_conv, the 1x1 convolutions (the ResidualBlock
        shortcut becomes a covered convolution only on frames of >= 16 384 pixels: asserted absent here), norms, attention."""

        def __init__(self, sd, cfg):
            super().__init__(sd, cfg)
            self.covered = 0
            self._wq = {}

        def _q(self, key):
            if key not in self._wq:
                self._wq[key] = _w16(self.sd[key])
            return self._wq[key]

        def _norm_ok(self, key):
            nk = {"residual.2": "residual.0.gamma", "residual.6": "residual.3.gamma", "head.2": "head.0.gamma"}
            for tail, norm in nk.items():
                if key.endswith(tail):
                    g = self.sd[key[:-len(tail)] + norm]
                    return math.sqrt(g.numel()) * float(g.abs().max()) < 6.0e4
            return False                                    # conv1 of encoder / decoder

        def _conv_cached(self, key, x, cache, idx, pad=(1, 1, 1)):
            if x.shape[1] % 64 or not self._norm_ok(key):
                return super()._conv_cached(key, x, cache, idx, pad)
            self.covered += 1
            x = _r16(x)                                     # the ring and the cached frames hold the fp16 values
            i = idx[0]
            c = wan_vae._cache_tail(x, cache[i])
            y = wan_vae.causal_conv3d(x, self._q(key + ".weight"), self.sd[key + ".bias"], pad=pad, cache_x=cache[i])
            cache[i] = c
            idx[0] += 1
            return y

        def _resblock(self, p, x, cache, idx):
            assert x.shape[3] * x.shape[4] < 16384, "the 1x1x1 shortcut is a covered convolution on frames this large: not emulated"
            return super()._resblock(p, x, cache, idx)

        def _resample(self, p, x, mode, cache, idx):
            sd = self.sd
            b, c, t, h, w = x.shape
            if c % 64:
                return super()._resample(p, x, mode, cache, idx)
            if mode == "upsample3d":
                i = idx[0]
                if cache[i] is None:
                    cache[i] = "Rep"
                    idx[0] += 1
                else:
                    cx = x[:, :, -wan_vae.CACHE_T:].clone()                          # the cache keeps the raw f32 rows
                    if cx.shape[2] < 2:
                        cx = torch.cat([torch.zeros_like(cx) if isinstance(cache[i], str) else cache[i][:, :, -1:], cx], dim=2)
                    tw, tb = self._q(p + "time_conv.weight"), sd[p + "time_conv.bias"]
                    self.covered += 1
                    if isinstance(cache[i], str):
                        x = wan_vae.causal_conv3d(_r16(x), tw, tb, pad=(1, 0, 0))
                    else:
                        x = wan_vae.causal_conv3d(_r16(x), tw, tb, pad=(1, 0, 0), cache_x=_r16(cache[i]))
                    cache[i] = cx
                    idx[0] += 1
                    x = x.reshape(b, 2, c, t, h, w)
                    x = torch.stack((x[:, 0], x[:, 1]), 3).reshape(b, c, t * 2, h, w)
            t = x.shape[2]
            y = _r16(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w))
            wk, bk = p + "resample.1.weight", sd[p + "resample.1.bias"]
            self.covered += 1
            if mode in ("upsample2d", "upsample3d"):
                # four 2x2 phase convolutions of the source image, the pre-summed phase weights rounded (each phase under its own scale)
                out = y.new_empty(b * t, sd[wk].shape[0], 2 * h, 2 * w)
                for a_ in (0, 1):
                    for b_ in (0, 1):
                        wp = _w16(_phase_weights(sd[wk].unsqueeze(2), a_, b_)[:, :, 0].to(y.dtype))
                        out[:, :, a_::2, b_::2] = F.conv2d(F.pad(y, (1 - b_, b_, 1 - a_, a_)), wp, bk)
                y = out
            else:
                y = F.conv2d(F.pad(y, (0, 1, 0, 1)), self._q(wk), bk, stride=(2, 2))
            x = y.reshape(b, t, c, y.shape[2], y.shape[3]).permute(0, 2, 1, 3, 4)
            if mode == "downsample3d":
                i = idx[0]
                if cache[i] is None:
                    cache[i] = x.clone()
                    idx[0] += 1
                else:
                    cx = x[:, :, -1:].clone()
                    x = wan_vae.causal_conv3d(torch.cat([cache[i][:, :, -1:], x], 2), sd[p + "time_conv.weight"], sd[p + "time_conv.bias"],
                                              stride=(2, 1, 1))
                    cache[i] = cx
                    idx[0] += 1
            return x

    return _F16Oracle


WIDTHS = {"w64": dict(dim=64, dec_dim=64), "full": {}}


@functools.lru_cache(maxsize=None)
def _refs(width):
    """(cfg, f32 state dict, z, video, dict of truth / emulation outputs of decode (clamped to [-1, 1]) and encode), computed once per width"""
    from oracle import wan_vae
    torch.set_num_threads(min(32, torch.get_num_threads()))
    cfg = dict(wan_vae.FULL_CFG, **WIDTHS[width])
    sd = wan_vae.make_state_dict(cfg, 2)
    sd64 = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(8)
    z = torch.randn(48, 2, 2, 3, generator=g)
    vid = torch.tanh(torch.randn(3, 5, 32, 48, generator=g))
    scale = wan_vae.scale_tensors(F64)
    out = {}
    with torch.no_grad():
        for name, ora in (("truth", wan_vae.WanVAE(sd64, cfg)), ("emu", _make_emulation()(sd64, cfg))):
            out[name, "dec"] = ora.decode(z.double().unsqueeze(0), scale)[0].clamp_(-1, 1)      # Wan2_2_VAE.decode clamps (vae2_2.py:1045)
            out[name, "enc"] = ora.encode(vid.double().unsqueeze(0), scale)[0]
            if name == "emu":
                assert ora.covered > 40, ora.covered
    return cfg, sd, z, vid, out


def _vae(cfg, sd, precision, **kw):
    from univid_amd.wan.vae2_2 import Wan2_2_VAE
    vae = Wan2_2_VAE(c_dim=cfg["dim"], dec_dim=cfg["dec_dim"], device=DEV, precision=precision, **kw)
    vae.model.load_state_dict(sd)
    return vae


def _run(vae, z, vid):
    with torch.no_grad():
        dec = vae.decode([z.to(DEV)])[0]
        enc = vae.encode([vid.to(DEV)])[0]
    return {"dec": dec.cpu(), "enc": enc.cpu()}


# ---------------------------------------------------------------------------------------------------------------
# the four gates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["w64", "full"])
def test_vae_f16_mode_against_emulation_and_truth(width):
    """Gates 1-4 for decode and encode. The measured figures are recorded (and printed) before anything is asserted."""
    cfg, sd, z, vid, ref = _refs(width)
    got = _run(_vae(cfg, sd, "f16"), z, vid)
    x3 = _run(_vae(cfg, sd, "f16x3"), z, vid)
    f32 = _run(_vae(cfg, sd, "fp32"), z, vid)
    m = {}
    for d in ("dec", "enc"):
        truth, emu = ref["truth", d], ref["emu", d]
        assert got[d].shape == truth.shape
        m[d] = dict(rms_vs_truth_f16=_rms(got[d].double() - truth), rms_vs_truth_emulation=_rms(emu - truth),
                    rms_vs_truth_f16x3=_rms(x3[d].double() - truth), rms_vs_truth_fp32=_rms(f32[d].double() - truth),
                    rel_rms_vs_emulation=_rel_rms(got[d], emu), out_rms=_rms(truth), max_abs_err_vs_truth=float((got[d].double() - truth).abs().max()),
                    inside_frac=float(((got[d].double() - truth).abs() <= 1e-4 + 1e-3 * truth.abs()).double().mean()))
        m[d]["truth_ratio"] = m[d]["rms_vs_truth_f16"] / m[d]["rms_vs_truth_emulation"]
        m[d]["price_vs_f16x3"] = m[d]["rms_vs_truth_f16"] / m[d]["rms_vs_truth_f16x3"]
        m[d]["price_vs_fp32"] = m[d]["rms_vs_truth_f16"] / m[d]["rms_vs_truth_fp32"]
        record_margin(f"vae_f16/{width}/{d}", **m[d])
        print(f"vae_f16 {width} {d}: " + ", ".join(f"{k} = {v:.4g}" for k, v in m[d].items()))
    for d in ("dec", "enc"):
        assert bool(torch.isfinite(got[d]).all()), f"{width} {d}: gate 1"
        assert m[d]["truth_ratio"] <= 1.02, f"{width} {d}: gate 2, rms vs truth {m[d]['rms_vs_truth_f16']:.3e} against the emulation's {m[d]['rms_vs_truth_emulation']:.3e}"
        if (width, d) in GATE3:
            assert m[d]["rel_rms_vs_emulation"] <= GATE3[width, d], f"{width} {d}: gate 3, {m[d]['rel_rms_vs_emulation']:.3e}"
        assert m[d]["price_vs_f16x3"] >= 50.0, f"{width} {d}: gate 4, the mode is only {m[d]['price_vs_f16x3']:.1f} x f16x3's distance from the truth"


# ---------------------------------------------------------------------------------------------------------------
# coverage, pass length, arena, range guard
# ---------------------------------------------------------------------------------------------------------------
def _conv_calls(vae, z, vid, monkeypatch):
    """the uv_conv3d_* launches of one decode + one encode: (entry, Cin in f32-row channels, Cout, kt, kh, kw, Tout, Hout, Wout, up)"""
    from univid_amd import _lib
    calls, orig = [], _lib.call

    def spy(name, *a, **k):
        if name.startswith("uv_conv3d_"):
            calls.append((name, a[12], a[13], a[14], a[15], a[16], a[9], a[10], a[11], a[23]))
        return orig(name, *a, **k)
    monkeypatch.setattr(_lib, "call", spy)
    _run(vae, z, vid)
    monkeypatch.setattr(_lib, "call", orig)
    return calls


@pytest.mark.parametrize("dims", [(64, 64), (32, 32)], ids=["w64", "w32"])
def test_vae_f16_covers_exactly_the_three_pass_convolutions_with_whole_64_channel_rows(dims, monkeypatch):
    """The launches of an f16x3 run and of an f16 run, one to one: a uv_conv3d_f16x3 launch becomes uv_conv3d_f16 exactly when its
    Cin % 64 == 0; every other launch (bf16x6 on raw input, f16x3 with 32 / 96 / 160 ... channels) is the same call. With
    c_dim = dec_dim = 32 the 32-channel convolutions stay f16x3 and the 64- and 128-channel ones switch."""
    from oracle import wan_vae
    cfg = dict(wan_vae.FULL_CFG, dim=dims[0], dec_dim=dims[1])
    sd = wan_vae.make_state_dict(cfg, 2)
    g = torch.Generator().manual_seed(8)
    z, vid = torch.randn(48, 2, 2, 3, generator=g), torch.tanh(torch.randn(3, 5, 32, 48, generator=g))
    a = _conv_calls(_vae(cfg, sd, "f16x3"), z, vid, monkeypatch)
    b = _conv_calls(_vae(cfg, sd, "f16"), z, vid, monkeypatch)
    assert len(a) == len(b) and len(a) > 100
    switched = kept = 0
    for ca, cb in zip(a, b):
        assert ca[1:] == cb[1:], (ca, cb)
        if ca[0] == "uv_conv3d_f16x3" and ca[1] % 64 == 0:
            assert cb[0] == "uv_conv3d_f16", (ca, cb)
            switched += 1
        else:
            assert cb[0] == ca[0], (ca, cb)
            kept += ca[0] == "uv_conv3d_f16x3"
    assert switched > 40
    assert {c[0] for c in a} == {"uv_conv3d_f16x3", "uv_conv3d_bf16x6"}
    if dims == (32, 32):
        assert kept > 0 and {c[1] for c in a if c[0] == "uv_conv3d_f16x3"} >= {32, 64, 128}
        assert all(c[1] != 32 for c in b if c[0] == "uv_conv3d_f16")
    else:
        assert kept == 0


def test_vae_f16_pass_length_does_not_change_the_result():
    """frames_per_pass 1 against 4 (and 3, which does not divide the clip) in the mode: bit-identical decode and encode, also for a second
    clip of another shape through the same object (plain rings keyed by format and shape, caches cleared)."""
    from oracle import wan_vae
    cfg = dict(wan_vae.FULL_CFG, dim=64, dec_dim=64)
    sd = wan_vae.make_state_dict(cfg, 3)
    g = torch.Generator().manual_seed(12)
    z = torch.randn(48, 6, 2, 3, generator=g)
    vid = torch.tanh(torch.randn(3, 21, 32, 48, generator=g))
    z2 = torch.randn(48, 3, 3, 2, generator=g)
    ref = _vae(cfg, sd, "f16", frames_per_pass=1)
    with torch.no_grad():
        d1, e1, d1b = ref.decode([z.to(DEV)])[0], ref.encode([vid.to(DEV)])[0], ref.decode([z2.to(DEV)])[0]
    assert d1.shape == (3, 21, 32, 48) and e1.shape == (48, 6, 2, 3)
    for G in (4, 3):
        vae = _vae(cfg, sd, "f16", frames_per_pass=G)
        with torch.no_grad():
            d, e, db = vae.decode([z.to(DEV)])[0], vae.encode([vid.to(DEV)])[0], vae.decode([z2.to(DEV)])[0]
        assert torch.equal(d, d1) and torch.equal(e, e1) and torch.equal(db, d1b), f"f16: {G} frames per pass differs from streaming"


def test_vae_f16_second_call_allocates_nothing_on_the_device():
    """The arena in the mode: after one decode and encode at a clip shape, repeat calls cause no device allocation besides their two
    result tensors, and give the same bits."""
    import gc
    from oracle import wan_vae
    cfg = dict(wan_vae.FULL_CFG, dim=64, dec_dim=64)
    vae = _vae(cfg, wan_vae.make_state_dict(cfg, 3), "f16")
    z = torch.randn(48, 5, 6, 10, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    with torch.no_grad():
        v0 = vae.decode([z])[0]
        e0 = vae.encode([v0])[0]
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        n1 = torch.cuda.memory_stats(DEV)["num_device_alloc"]
        v1 = vae.decode([z])[0]
        e1 = vae.encode([v0])[0]
        torch.cuda.synchronize()
        n2 = torch.cuda.memory_stats(DEV)["num_device_alloc"]
    assert torch.equal(v0, v1) and torch.equal(e0, e1)
    assert n2 - n1 <= 2, f"repeat VAE calls in f16 mode allocated on the device: {n2 - n1} hipMalloc(s) for two result tensors"
    eng = vae.model._eng()
    assert {k[3] for k in eng.scratch} == {0, 3}, "plain and f32-sized rings are separate buffers"
    assert all(r.shape[-1] == (k[2] // 2 if k[3] == 3 else k[2]) for k, r in eng.scratch.items() if r is not None)


def test_vae_f16_norm_outside_fp16_range_keeps_f32_rows():
    """The range guard in the mode: gamma x 1e5 on one norm (its convolution's weights x 1e-5) puts sqrt(C) max|gamma| out of fp16's range:
    THAT norm keeps f32 rows and its convolution runs as bf16x6, the others stay plain fp16. The decode is finite and close to
    precision='fp32' on the same weights: rel rms <= 5e-3. (Where that comes from: a product of two operands rounded to 11 bits carries
    ~2^-11 sqrt(2 / 3) = 4e-4 relative rms error; the ~40 covered convolutions a decoder output depends on add in quadrature to
    ~2.5e-3; twice that. A convolution fed with overflowed fp16 rows would be off by O(1) or not finite.)"""
    from oracle import wan_vae
    cfg = dict(wan_vae.FULL_CFG, dim=64, dec_dim=64)
    sd = wan_vae.make_state_dict(cfg, 2)
    z = torch.randn(48, 2, 2, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    pair = {}
    for prec in ("f16", "fp32"):
        big = _vae(cfg, sd, prec)
        with torch.no_grad():
            big.model.decoder.middle[0].residual[0].gamma.mul_(1e5)
            big.model.decoder.middle[0].residual[2].weight.mul_(1e-5)
        big.model.invalidate()
        with torch.no_grad():
            pair[prec] = big.decode([z])[0]
        if prec == "f16":
            fmts = list(big.model._eng()._fmt.values())
            assert fmts.count(0) == 1 and set(fmts) == {0, 2}, fmts
    assert bool(torch.isfinite(pair["f16"]).all())
    rel = _rel_rms(pair["f16"], pair["fp32"])
    record_margin("vae_f16/range_guard", rel_rms_vs_fp32=rel)
    print(f"vae_f16 range guard: rel rms vs fp32 = {rel:.3e}")
    assert rel <= 5e-3, rel
    assert not torch.equal(pair["f16"], pair["fp32"])


# ---------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------
def test_vae_precision_keyword_reaches_the_vae(tmp_path):
    """Wan2_2_VAE(precision="f16") / WanVAE_.prepare("f16"); WanTI2V(vae_precision=...) on the VAE it builds from the checkpoint directory and
    on an injected one (through prepare), None leaving an injected VAE's mode alone; CrossAttentionConfig(vae_precision=...) handed on."""
    from oracle import wan_vae
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    cfg = dict(wan_vae.FULL_CFG, dim=64, dec_dim=64)
    sd = wan_vae.make_state_dict(cfg, 2)
    z = torch.randn(48, 2, 2, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    direct = _vae(cfg, sd, "f16")
    with torch.no_grad():
        want = direct.decode([z])[0]
    assert direct.model._eng().precision == "f16"
    _, _, dit = _tiny_model(0)

    class Cfg(TI2VConfig):
        vae_kwargs = dict(c_dim=64, dec_dim=64)
    torch.save(sd, tmp_path / "Wan2.2_VAE.pth")
    built = WanTI2V(Cfg, checkpoint_dir=str(tmp_path), model=dit, device=DEV, vae_precision="f16")
    assert built.vae is not None and built.vae.model.precision == "f16"
    with torch.no_grad():
        assert torch.equal(built.vae.decode([z])[0], want)
    default = WanTI2V(Cfg, checkpoint_dir=str(tmp_path), model=dit, device=DEV)
    assert default.vae.model.precision == "f16x3"
    # injected: switched through prepare; None leaves the mode alone - whichever it is
    inj = _vae(cfg, sd, "f16x3")
    with torch.no_grad():
        x3 = inj.decode([z])[0]
    assert WanTI2V(TI2VConfig, model=dit, vae=inj, device=DEV).vae.model.precision == "f16x3"
    pipe = WanTI2V(TI2VConfig, model=dit, vae=inj, device=DEV, vae_precision="f16")
    assert pipe.vae is inj and inj.model.precision == "f16" and inj.model._engine.precision == "f16"
    with torch.no_grad():
        assert torch.equal(inj.decode([z])[0], want) and not torch.equal(want, x3)
    assert WanTI2V(TI2VConfig, model=dit, vae=inj, device=DEV, vae_precision=None).vae.model.precision == "f16"
    with pytest.raises(ValueError, match="'f16'"):
        WanTI2V(TI2VConfig, model=dit, vae=_vae(cfg, sd, "f16x3"), device=DEV, vae_precision="fp16")
    # the pipeline's configuration field
    plain = WanTI2V(TI2VConfig, model=dit, vae=_vae(cfg, sd, "f16x3"), device=DEV)
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(vae_precision="f16", use_lora=False, enable_bagel_extraction=False),
                                         wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.vae_model.model.precision == "f16" and fused.dit_model.ffn_precision == "bf16"
    kept = CrossAttentionFusionPipeline(CrossAttentionConfig(use_lora=False, enable_bagel_extraction=False), wan_pipeline=plain,
                                        context_projector=lambda *a, **k: None)
    assert kept.vae_model.model.precision == "f16"
    # WanVAE_.prepare directly
    m = _vae(cfg, sd, "fp32").model
    assert m.prepare("f16")._engine.precision == "f16" and m.precision == "f16"
