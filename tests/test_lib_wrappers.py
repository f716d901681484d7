"""GPU (the test marked gpu): every wrapper of univid_amd._lib that the product code launches through rejects a too-short output or a wrong-dtype
operand - device tensors of at most 64 x 64 - with a UnividHipError that names the argument, BEFORE anything is launched
(_lib.CALL_COUNT does not move): the faulty pointer never reaches the device. The well-formed calls of the same wrappers are what the
model, sampler, VAE and text-encoder goldens run end to end; the checker's dtype / layout / extent logic itself is covered on the CPU
(tests/test_host_logic.py)."""
import pytest
import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _cases(dev):
    from univid_amd import _lib as L

    def z(*shape, dtype=F32):
        return torch.zeros(*shape, dtype=dtype, device=dev)

    x = z(2, 4, 4)
    short = z(31)
    w1 = z(4, 32)
    px = z(2, 2, 2, 32)                                   # channels-last pixels

    def conv(precision="fp32", src=px, w=w1, out=None, **kw):
        return L.conv3d(precision, src, lambda kind: (w, 1.0), z(4), z(2, 2, 2, 4) if out is None else out, 2, 2, 2, 2, 2, 2, 32, 4, 1, 1, 1, **kw)

    b = lambda *s: z(*s, dtype=BF16)
    return {
        # sampler: flat n
        "cfg_convert.x0": lambda: L.cfg_convert(x, x, x, 3.0, 0.5, None, x.double()),
        "cfg_convert.noise_pred": lambda: L.cfg_convert(x, x, x, 3.0, 0.5, x[:, :, :2], x),
        "unipc_corrector.m_prev": lambda: L.unipc_corrector(x, x, short, x, x, 1., 1., 1., 1., 1., 1., 2),
        "unipc_predictor.m0": lambda: L.unipc_predictor(x, short, None, x, 1., 1., 1., 1., 1),
        "dpmpp_update.m1": lambda: L.dpmpp_update(x, x, x.half(), x, 1., 1., 1., 2),
        # VAE
        "split_weights_bf16x3.out": lambda: L.split_weights_bf16x3(w1, b(2 * 128 - 1)),
        "split_weights_bf16x6.out": lambda: L.split_weights_bf16x6(w1, b(2 * 128)),
        "split_weights_f16x3.out": lambda: L.split_weights_f16x3(w1, b(2 * 128), 1.0),
        "conv3d.out": lambda: conv(out=z(2, 2, 1, 4)),
        "conv3d.src": lambda: conv(src=z(2, 2, 2, 16)),
        "conv3d.resid": lambda: conv(resid=z(2, 2, 2, 2)),
        "conv3d.weights": lambda: conv(precision="f16x3", in_split=2, w=b(2 * 128)),          # the f16x3 entry reads fp16 pieces
        "vae_rms_silu.out": lambda: L.vae_rms_silu(px, z(32), z(2, 2, 1, 32)),
        "vae_rms_silu.gamma": lambda: L.vae_rms_silu(px, z(16), z(2, 2, 2, 32)),
        "vae_split_f16.scale": lambda: L.vae_split_f16(px, z(2, 2, 2, 32), z(1)),
        "softmax_rows.x": lambda: L.softmax_rows(z(4, 8), 5, 8, 1.0),
        "vae_video_in.out": lambda: L.vae_video_in(z(3, 2, 4, 4), z(1, 2, 2, 32), 0, 2),
        "vae_video_out.vid": lambda: L.vae_video_out(z(2, 2, 2, 12), z(1, 3, 2, 4, 4, dtype=F16), 0, 2),
        "vae_latent_in.inv_std": lambda: L.vae_latent_in(z(4, 1, 2, 2), z(4), z(3), z(1, 2, 2, 4)),
        "vae_latent_out.out": lambda: L.vae_latent_out(z(1, 2, 2, 8), z(4), z(4), z(1, 4, 1, 2, 1), 4),
        "vae_avgdown_add.out": lambda: L.vae_avgdown_add(z(2, 4, 4, 8), z(1, 2, 1, 16), 2, 2),
        "vae_dupup_add.out": lambda: L.vae_dupup_add(z(2, 2, 2, 16), z(3, 4, 4, 8), 2, 0),
        "gemm_f32.out": lambda: L.gemm_f32(z(2, 2, 2, 8), z(4, 8), z(4), z(2, 2, 1, 4)),             # channels-last rows
        "gemm_f32.resid": lambda: L.gemm_f32(z(2, 2, 2, 8), z(4, 8), z(4), z(2, 2, 2, 4), resid=b(2, 2, 2, 4)),
        # attention seam
        "cast_f32_to16.out": lambda: L.cast_f32_to16(x, b(31)),
        "cast_16_to_f32.out": lambda: L.cast_16_to_f32(b(2, 4, 4), x.double()),
        "transpose_16.out": lambda: L.transpose_16(b(24, 8), b(8, 64 + 24)[:, 25:], 24, 8, 64),
        # text encoder / projector
        "t5_attention.rel_bias": lambda: L.t5_attention(b(8, 64), b(8, 64), b(8, 64), b(8, 64), 1, z(2 * 8 - 2), 8),
        "add_bf16.y": lambda: L.add_bf16(b(4, 8), z(4, 8), b(4, 8)),
        "t5_gated_gelu.gate": lambda: L.t5_gated_gelu(b(31), b(4, 8), b(4, 8)),
        "gelu_erf.x": lambda: L.gelu_erf(b(31), b(4, 8)),
        "interp_linear_rows.out": lambda: L.interp_linear_rows(b(4, 8), z(6, 8)),
        # DiT glue
        "add_rows.e0": lambda: L.add_rows(z(1, 6, 8), z(1, 48), z(2, 48)),
        "add_rows.mod": lambda: L.add_rows(b(1, 6, 8), z(2, 48), z(2, 48)),
        "add_bf16_resid.y": lambda: L.add_bf16_resid(z(4, 8), b(3, 8), 4, 8),
        "sinusoid.out": lambda: L.sinusoid(z(3), z(2, 16)),
        "linear_rows.W": lambda: L.linear_rows(z(3, 8), b(4, 8), z(4), z(3, 4)),
        "linear_rows.out": lambda: L.linear_rows(z(3, 8), z(4, 8), None, z(2, 4)),
        "patchify.out": lambda: L.patchify(z(4, 1, 2, 4), b(6, 16)[5:], (1, 2, 2)),
        "unpatchify.out": lambda: L.unpatchify(z(2, 16), z(4, 1, 2, 2), (1, 1, 2), (1, 2, 2)),
        "unpatchify.rows": lambda: L.unpatchify(z(2, 16).t(), z(4, 1, 2, 4), (1, 1, 2), (1, 2, 2)),
        "l2_normalize_rows.out": lambda: L.l2_normalize_rows(z(4, 8), z(3, 8)),
    }


def test_every_new_wrapper_is_covered():
    """One case at least for each wrapper the product code was moved onto (and for gemm_f32's channels-last rows); no GPU needed."""
    from univid_amd import _lib as L
    new = ("cfg_convert unipc_corrector unipc_predictor dpmpp_update split_weights_bf16x3 split_weights_bf16x6 split_weights_f16x3 conv3d "
           "vae_rms_silu vae_split_f16 softmax_rows vae_video_in vae_video_out vae_latent_in vae_latent_out vae_avgdown_add vae_dupup_add "
           "cast_f32_to16 cast_16_to_f32 transpose_16 t5_attention add_bf16 t5_gated_gelu gelu_erf interp_linear_rows add_rows add_bf16_resid "
           "sinusoid linear_rows patchify unpatchify l2_normalize_rows gemm_f32").split()
    assert all(callable(getattr(L, n)) for n in new)
    assert {c.split(".")[0] for c in _cases("cpu")} == set(new)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    from univid_amd import _lib as L
    L.init()
    cases = _cases("cuda")
    torch.cuda.synchronize()
    before = L.CALL_COUNT
    for name, run in cases.items():
        with pytest.raises(L.UnividHipError, match=name.replace(".", r"\.") + ": "):
            run()
        assert L.CALL_COUNT == before, f"{name}: a launch went out"
    torch.cuda.synchronize()
