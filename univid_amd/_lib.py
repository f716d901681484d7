"""ctypes binding of libunivid_hip.so (the C ABI declared in include/univid_hip.h).

PyTorch-ROCm tensors in, raw device pointers out: this module is the only place in the package that turns a tensor into
`data_ptr()` + sizes + the current HIP stream. Every launching entry point has ONE plain wrapper function below, and every
pointer argument of every wrapper passes `_check` (dtype, layout, addressed extent against the tensor's storage, device) before
the library is touched; the rest of the package calls the wrappers only. `call` / `ptr` / `stream_ptr` stay public for tests
and tools that drive the C ABI with deliberately odd buffers. There is NO fallback: if the shared library is missing or a
call is rejected, a RuntimeError (UnividHipError) is raised.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libunivid_hip.so")

_c = ctypes
_P, _L, _I, _F = _c.c_void_p, _c.c_long, _c.c_int, _c.c_float

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "uv_version": [],
    "uv_init": [],
    "uv_last_error": [],
    "uv_build_id": [],
    "uv_device_arch": [_c.c_char_p, _I],
    "uv_host_blocking_sync": [_I],
    "uv_set_option": [_I, _I],
    "uv_get_option": [_I, _c.POINTER(_I)],
    "uv_reset_options": [],
    "uv_gemm_bf16_nt": [_P, _L, _P, _L, _P, _I, _I, _I, _I, _P, _L, _P, _P, _L, _I, _P],
    "uv_gemm_bf16_nt_ws": [_P, _L, _P, _L, _P, _I, _I, _I, _I, _P, _L, _P, _P, _L, _I, _P, _L, _P],
    "uv_gemm_splitk_ws_bytes": [_I, _I, _I],
    "uv_gemm_plan": [_I, _I, _I, _I, _L, _I, _I, _L, _c.POINTER(_I), _c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I)],
    "uv_gemm_f16_nt": [_P, _L, _P, _L, _P, _I, _I, _I, _I, _P, _L, _P, _P, _L, _I, _P],
    "uv_mx_quant_bf16": [_P, _L, _P, _L, _P, _L, _I, _I, _P],
    "uv_gemm_mxfp8_nt": [_P, _L, _P, _L, _P, _L, _P, _L, _P, _I, _I, _I, _I, _P, _L, _P, _P, _L, _P],
    "uv_gemm_mxfp8_nt_t": [_P, _L, _P, _L, _P, _L, _P, _L, _P, _I, _I, _I, _P, _L, _P],
    "uv_gemm_mxfp8_nt_ssq": [_P, _L, _P, _L, _P, _L, _P, _L, _P, _I, _I, _I, _P, _L, _P, _L, _P],
    "uv_gemm_f32_nt": [_P, _L, _P, _L, _P, _I, _I, _I, _P, _L, _P, _L, _P],
    "uv_gemm_bf16_nt_ssq": [_P, _L, _P, _L, _P, _I, _I, _I, _P, _L, _P, _L, _I, _P],
    "uv_rms_scale_from_ssq": [_P, _L, _I, _I, _I, _F, _P, _P],
    "uv_lora_down_bf16": [_P, _L, _P, _L, _P, _I, _I, _I, _P, _L, _I, _P],
    "uv_lora_down_seg_bf16": [_P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P, _L, _I, _P],
    "uv_cast_f32_bf16_rows": [_P, _L, _P, _L, _I, _I, _P],
    "uv_flash_attn_bf16_qnorm": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P, _P, _P],
    "uv_flash_attn_bf16": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P],
    "uv_flash_attn_f16": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P],
    "uv_flash_attn_win_bf16": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _I, _I, _P],
    "uv_flash_attn_win_plan": [_I, _I, _I, _I, _I, _I, _c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I), _c.POINTER(_I)],
    "uv_flash_attn_bs_bf16": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _P, _P, _I, _P],
    "uv_flash_attn_bs_plan": [_I, _I, _I, _I, _c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I)],
    "uv_attn_pool_qk": [_P, _L, _P, _L, _P, _P, _I, _I, _I, _I, _P],
    "uv_attn_bs_select": [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P],
    "uv_flash_attn_bs_lists_bf16": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _F, _P, _P, _I, _I, _P],
    "uv_flash_attn_mxqk": [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P],
    "uv_flash_attn_mxqk_plan": [_I, _I, _I, _I, _I, _c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I), _c.POINTER(_I)],
    "uv_vt_mx_quant": [_P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _P],
    "uv_flash_attn_mxpv": [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P],
    "uv_flash_attn_mxpv_plan": [_I, _I, _I, _I, _I, _c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I), _c.POINTER(_I)],
    "uv_flash_attn_kernel_name": [_I, _I, _L, _L, _I, _c.c_char_p, _I],
    "uv_flash_attn_plan": [_I, _I, _I, _I, _I, _L, _L, _I, _c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I), _c.POINTER(_I)],
    "uv_transpose_16": [_P, _L, _P, _L, _I, _I, _I, _P],
    "uv_cast_f32_to16": [_P, _P, _L, _I, _P],
    "uv_cast_16_to_f32": [_P, _P, _L, _I, _P],
    "uv_layernorm_mod": [_P, _L, _P, _L, _I, _I, _F, _I, _P, _L, _I, _I, _P, _P, _P, _I, _I, _P],
    "uv_layernorm_mod_mx": [_P, _L, _P, _L, _P, _L, _I, _I, _F, _I, _P, _L, _I, _I, _P, _P, _P, _I, _P],
    "uv_t5_attention_bf16": [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _P, _I, _P],
    "uv_add_bf16": [_P, _P, _P, _L, _P],
    "uv_t5_gated_gelu_bf16": [_P, _P, _P, _L, _P],
    "uv_gelu_erf_bf16": [_P, _P, _L, _P],
    "uv_interp_linear_rows_bf16": [_P, _L, _P, _L, _I, _I, _I, _P],
    "uv_l2_normalize_rows_f32": [_P, _L, _P, _L, _I, _I, _F, _P],
    "uv_rmsnorm_rope": [_P, _L, _P, _L, _P, _I, _I, _I, _F, _P, _I, _I, _I, _I, _P],
    "uv_rmsnorm_rope_qk_mx": [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _I, _I, _I, _I, _F, _P, _I, _I, _I, _I, _P],
    "uv_rmsnorm_rope_qk": [_P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _I, _I, _F, _P, _I, _I, _I, _I, _P],
    "uv_patchify_bf16": [_P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "uv_unpatchify_f32": [_P, _L, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "uv_sinusoid_f32": [_P, _P, _I, _I, _P],
    "uv_linear_rows_f32": [_P, _L, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "uv_add_rows_f32": [_P, _P, _P, _I, _L, _P],
    "uv_cast_f32_bf16": [_P, _P, _L, _P],
    "uv_add_bf16_resid": [_P, _L, _P, _L, _I, _I, _P],
    "uv_text_weight_rows_bf16": [_P, _L, _P, _L, _I, _I, _I, _F, _P],
    "uv_cfg_convert": [_P, _P, _P, _F, _F, _P, _P, _L, _P],
    "uv_unipc_corrector": [_P, _P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _I, _L, _P],
    "uv_unipc_predictor": [_P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _P],
    "uv_dpmpp_update": [_P, _P, _P, _P, _F, _F, _F, _I, _L, _P],
    "uv_step_cache_update": [_P, _P, _P, _P, _P, _P, _L, _I, _P],
    "uv_step_cache_apply": [_P, _P, _P, _P, _P, _L, _I, _P],
    "uv_rows_rel_l1": [_P, _P, _I, _I, _P],
    "uv_conv3d_f32": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                      _P, _L, _P],
    "uv_conv3d_bf16x6": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                         _P, _L, _P],
    "uv_conv3d_bf16x3": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                         _P, _L, _I, _P],
    "uv_conv3d_f16x3": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                        _P, _L, _F, _P, _P],
    "uv_conv3d_f16": [_P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                      _P, _L, _F, _P, _P],
    "uv_cast_weights_f16": [_P, _P, _L, _F, _P],
    "uv_vae_cast_f16": [_P, _L, _P, _L, _L, _I, _P, _P],
    "uv_conv3d_plan": [_I] * 18 + [_c.c_char_p, _I, _c.POINTER(_I), _c.POINTER(_I)],
    "uv_vae_split_f16": [_P, _L, _P, _L, _L, _I, _P, _P],
    "uv_split_weights_f16x3": [_P, _P, _L, _F, _P],
    "uv_split_weights_bf16x3": [_P, _P, _L, _P],
    "uv_split_weights_bf16x6": [_P, _P, _L, _P],
    "uv_vae_rms_silu": [_P, _L, _P, _P, _L, _L, _I, _I, _I, _P],
    "uv_softmax_rows_f32": [_P, _L, _I, _I, _F, _P],
    "uv_vae_dupup_add": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "uv_vae_avgdown_add": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "uv_vae_latent_in": [_P, _P, _P, _P, _L, _I, _L, _P],
    "uv_vae_latent_out": [_P, _L, _P, _P, _P, _I, _L, _P],
    "uv_vae_video_in": [_P, _P, _L, _I, _I, _I, _I, _I, _P],
    "uv_vae_video_out": [_P, _L, _P, _I, _I, _I, _I, _I, _P],
}
_RESTYPE = {"uv_last_error": _c.c_char_p, "uv_build_id": _c.c_char_p, "uv_gemm_splitk_ws_bytes": _L}

OPT_CONV_HALO, OPT_GEMM_GM, OPT_ATTN_CUT, OPT_ATTN_WIN_FORM = range(4)      # include/univid_hip.h: UV_OPT_*
EPI_BF16, EPI_GELU_BF16, EPI_F32_FROM_BF16, EPI_RESID_F32, EPI_GATE_RESID_F32, EPI_BF16_T = range(6)

_lib = None
_inited = set()        # device indices whose arch check + per-device library state (zero page) are done


class UnividHipError(RuntimeError):
    pass


def load(path=None):
    """Loads the shared library (torch first, so the HIP runtime torch ships is the one both sides use)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise UnividHipError(
            f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `python -m univid_amd.build`). univid_amd has no CPU/eager fallback.")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, _I)
    _check_build_id(lib, path)
    _lib = lib
    return lib


def _check_build_id(lib, path):
    """A stale .so next to newer kernel sources (git pull onto old local objects) would run old kernels behind new ctypes
    signatures: compare the digest compiled into the library with the one of the sources in the tree."""
    if os.path.abspath(path) != LIB_PATH or not os.path.isdir(os.path.join(_HERE, "csrc")):
        return
    from . import build as _build
    have, want = lib.uv_build_id().decode(), _build.source_id()
    if have != want:
        raise UnividHipError(
            f"{path} was built from other kernel sources (library {have}, tree {want}): rebuild with "
            "`python -m univid_amd.build`. univid_amd never runs a stale extension.")


def init(device=None):
    """One-time checks for `device` (index; default = the current one): a HIP device is visible, it is a gfx950, and the
    library's per-device state exists. Called by every entry point with the device of its tensors."""
    lib = load()
    if device is None:
        if not torch.cuda.is_available():
            raise UnividHipError("no HIP device visible: univid_amd's hot path only runs on an MI355X (gfx950)")
        device = torch.cuda.current_device()
    if device not in _inited:
        if not torch.cuda.is_available():
            raise UnividHipError("no HIP device visible: univid_amd's hot path only runs on an MI355X (gfx950)")
        torch.cuda.init()
        with torch.cuda.device(device):
            rc = lib.uv_init()
            if rc != 0:
                raise UnividHipError(f"uv_init failed: {lib.uv_last_error().decode()}")
            buf = ctypes.create_string_buffer(64)
            lib.uv_device_arch(buf, 64)
        arch = buf.value.decode()
        if not arch.startswith("gfx950"):
            raise UnividHipError(f"device {device}: arch {arch!r} is not gfx950: the kernels are built for MI355X only")
        _inited.add(device)
    return lib


def set_option(key, value):
    """uv_set_option: explicit developer switch (A/B tools, tests); the library never reads the environment."""
    lib = load()
    if lib.uv_set_option(int(key), int(value)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())


def get_option(key):
    lib = load()
    v = _I(0)
    if lib.uv_get_option(int(key), ctypes.byref(v)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return v.value


def reset_options():
    load().uv_reset_options()


class _DevPtr(_c.c_void_p):
    """A device pointer that remembers which GPU it lives on, so `call` can make that GPU current for the launch."""
    dev = None


class _Stream:
    """Placeholder for 'the current HIP stream of the device the tensors of this call live on'; resolved in `call`."""


_STREAM = _Stream()


def stream_ptr():
    return _STREAM


def ptr(t):
    if t is None:
        return None
    p = _DevPtr(t.data_ptr())
    p.dev = t.device.index if t.device.type == "cuda" else -1
    return p


# Optional live kernel timing (bench.py): PROFILE = {entry_point: []} times those entry points with HIP events
# recorded on the launch stream; PROFILE_ALL times every entry point. Off (None) in normal use.
PROFILE = None
PROFILE_ALL = False
CALL_COUNT = 0          # entry-point launches since import (bench.py reports launches per step)


def call(name, *args, flops=0):
    """Launches one entry point on the device its pointer arguments live on (all on ONE device, else an error) and on that
    device's current stream: `WanTI2V(device_id=1)` / the reference's manual model placement work without the process ever
    calling torch.cuda.set_device."""
    dev = None
    for a in args:
        if type(a) is _DevPtr:
            if a.dev != dev:
                if dev is not None or a.dev < 0:
                    raise UnividHipError(f"{name}: tensors must live on ONE GPU (got devices {dev} and {a.dev}; -1 = host memory)")
                dev = a.dev
    if dev is None:
        dev = torch.cuda.current_device() if torch.cuda.is_available() else None
    global CALL_COUNT
    lib = init(dev)
    if dev != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return call(name, *args, flops=flops)
    stream = torch.cuda.current_stream(dev)
    args = tuple(_c.c_void_p(stream.cuda_stream) if a is _STREAM else a for a in args)
    prof = PROFILE
    timed = prof is not None and (PROFILE_ALL or name in prof)
    if timed:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
    CALL_COUNT += 1
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise UnividHipError(f"{name} failed ({rc}): {lib.uv_last_error().decode()}")
    if timed:
        e.record(stream)
        prof.setdefault(name, []).append((s, e, flops))


# ---- host-side helpers (no tensors) -------------------------------------------------------------------------------

def host_blocking_sync(on=True, device=None):
    """uv_host_blocking_sync for `device` (default: the current one): a host thread waiting in synchronize sleeps instead of spinning.
    Process-wide policy: the APPLICATION decides (bench.py's ranks and univid_amd.parallel's workers call it; a library import never does)."""
    dev = torch.device("cuda" if device is None else device)
    idx = torch.cuda.current_device() if dev.index is None else dev.index
    lib = load()
    with torch.cuda.device(idx):
        if lib.uv_host_blocking_sync(1 if on else 0) != 0:
            raise UnividHipError(lib.uv_last_error().decode())


def gemm_splitk_ws_bytes(M, N, K, device=None):
    """Bytes of workspace with which gemm_bf16(..., ws=) runs the leftover-row strip of an [M, K] x [N, K]^T projection as one round of
    split-K workgroups (0: this shape has no such strip). The answer depends on the device's CU count."""
    dev = torch.device("cuda" if device is None else device)
    idx = torch.cuda.current_device() if dev.index is None else dev.index
    lib = init(idx)
    with torch.cuda.device(idx):
        return int(lib.uv_gemm_splitk_ws_bytes(int(M), int(N), int(K)))


def gemm_plan(M, N, K, epi=0, ldo=None, tile_cfg=0, f16=False, ws_bytes=0):
    """Launch plan of a gemm_bf16 / gemm_bf16_ssq call of this shape (ldo: the output's leading dimension, default N; ws_bytes: the size
    of the workspace it would pass) on the current device - 256 CUs without one: [dict(kernel=name, m0=first row, rows=count)], one or
    two steps (include/univid_hip.h: uv_gemm_plan)."""
    n, m0, rows = _I(0), (_I * 2)(), (_I * 2)()
    buf = ctypes.create_string_buffer(64)
    lib = load()
    if lib.uv_gemm_plan(int(M), int(N), int(K), int(epi), int(N if ldo is None else ldo), int(tile_cfg), int(f16), int(ws_bytes), ctypes.byref(n),
                        buf, 32, m0, rows) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return [dict(kernel=buf.raw[32 * i:32 * i + 32].split(b"\0", 1)[0].decode(), m0=m0[i], rows=rows[i]) for i in range(n.value)]


# ---- one checked wrapper per launching entry point ----------------------------------------------------------------
# Each takes tensors and scalars, derives sizes / leading dimensions / the stream itself, passes EVERY pointer argument through _check and
# makes the one call(): the C side only sees pointers whose dtype, layout and addressed extent were verified.

F32, BF16, F16, U8, I32 = torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int32
_16 = (BF16, F16)


def _check(fn, *args):
    """The one check of a wrapper's pointer arguments, each given as (tensor, name, dtype, n[, rows[, optional]]): first every tensor's
    dtype, layout and extent, in that order, then every tensor's device - all before the library is touched and from tensor metadata only
    (no sync, no allocation: every wrapper runs inside HIP-graph capture). dtype: one dtype or a tuple of them. rows None / absent: a
    flat kernel reads / writes `n` consecutive elements, so the tensor must be contiguous. Otherwise the kernel addresses `rows` rows of
    `n` elements, stride(-2) apart: the innermost dimension must be contiguous and the leading ones one run of rows. The extent must fit
    between the tensor's first element and the end of its STORAGE, not numel(): a view whose rows are wider than its shape (the LoRA
    slot buf[:, K:], vt[:, col0:], a[j * L:]) is legitimate. optional: None is accepted."""
    args = [(a + (None, False))[:6] for a in args]
    for t, name, dtype, n, rows, optional in args:
        name = f"{fn}.{name}"
        if t is None:
            if optional:
                continue
            raise UnividHipError(f"{name}: a tensor is required, got None")
        if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
            raise UnividHipError(f"{name}: expected {dtype}, got {t.dtype}")
        if rows is None:
            if not t.is_contiguous():
                raise UnividHipError(f"{name}: must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
            need = n
        else:
            if t.dim() < 2:
                raise UnividHipError(f"{name}: rows of a matrix are expected, got shape {tuple(t.shape)}")
            if t.stride(-1) != 1:
                raise UnividHipError(f"{name}: innermost dimension must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
            if any(t.shape[d] != 1 and t.stride(d) != t.stride(d + 1) * t.shape[d + 1] for d in range(t.dim() - 2)):
                raise UnividHipError(f"{name}: leading dimensions must form one run of rows (shape {tuple(t.shape)}, strides {t.stride()})")
            need = (rows - 1) * t.stride(-2) + n if rows > 0 and n > 0 else 0
        have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if need > have:
            raise UnividHipError(f"{name}: the kernel addresses {need} elements, the tensor's storage holds {have} from its first element")
    for t, name, *_ in args:
        if t is not None and t.device.type != "cuda":
            raise UnividHipError(f"{fn}.{name}: tensor must live on the GPU (got {t.device})")


def _epilogue_args(a, bias, out, epi, M, N, gate, gate_tid):
    """bias / out / gate / gate_tid of the GEMMs that share uv_gemm_bf16_nt's epilogues: out's dtype and shape follow the epilogue."""
    half = a.dtype if a.dtype in _16 else BF16
    if epi not in range(6):
        raise UnividHipError(f"gemm: unknown epilogue {epi} (include/univid_hip.h: UV_EPI_*)")
    o = (out, "out", half, M, N) if epi == EPI_BF16_T else (out, "out", half if epi in (EPI_BF16, EPI_GELU_BF16) else F32, N, M)
    return ((bias, "bias", half, N, None, True), o, (gate, "gate", F32, N, 0 if gate is None else gate.shape[0], True),
            (gate_tid, "gate_tid", I32, M, None, True))


# -- DiT: GEMMs --
def gemm_bf16(a, w, bias, out, epi, M=None, gate=None, gate_tid=None, tile_cfg=0, ws=None):
    """a [M,K] bf16, w [N,K] bf16, bias bf16 [N] | None; out per epilogue (see include/univid_hip.h).
    ws: uint8 scratch tensor of >= gemm_splitk_ws_bytes(M, N, K) bytes (uv_gemm_bf16_nt_ws), or None."""
    f16 = a.dtype == F16      # IEEE fp16 operands (SigLIP2 ranker): same kernels, fp16 MFMA / conversions
    M = a.shape[0] if M is None else M
    N, K = w.shape
    _check("gemm_bf16", (a, "a", _16, K, M), (w, "w", a.dtype, K, N), *_epilogue_args(a, bias, out, epi, M, N, gate, gate_tid),
           (ws, "ws", U8, 0 if ws is None else ws.numel(), None, True))
    if ws is not None and not f16:
        call("uv_gemm_bf16_nt_ws", ptr(a), a.stride(-2), ptr(w), w.stride(-2), ptr(bias), M, N, K, epi, ptr(out), out.stride(-2),
             ptr(gate), ptr(gate_tid), 0 if gate is None else gate.stride(-2), tile_cfg, ptr(ws), ws.numel(), stream_ptr(), flops=2 * M * N * K)
        return out
    call("uv_gemm_f16_nt" if f16 else "uv_gemm_bf16_nt", ptr(a), a.stride(-2), ptr(w), w.stride(-2), ptr(bias), M, N, K, epi, ptr(out), out.stride(-2),
         ptr(gate), ptr(gate_tid), 0 if gate is None else gate.stride(-2), tile_cfg, stream_ptr(), flops=2 * M * N * K)
    return out


def mx_quant(x, codes, scales, M=None, K=None):
    """x bf16 [rows, >= K] -> OCP MXFP8: codes uint8 [rows, >= K] (e4m3fn) and scales uint8 [rows, >= K / 32] (one e8m0 byte per 32
    consecutive K elements of a row; include/univid_hip.h states the rule). Quantises the first M rows / K columns (defaults: all of x)."""
    M = x.shape[0] if M is None else M
    K = x.shape[1] if K is None else K
    _check("mx_quant", (x, "x", BF16, K, M), (codes, "codes", U8, K, M), (scales, "scales", U8, K // 32, M))
    if x.dim() != 2 or codes.dim() != 2 or scales.dim() != 2 or M > min(x.shape[0], codes.shape[0], scales.shape[0]) or \
            K > min(x.shape[1], codes.shape[1]) or K > 32 * scales.shape[1]:
        raise UnividHipError(f"mx_quant: x {tuple(x.shape)} / codes {tuple(codes.shape)} / scales {tuple(scales.shape)} do not fit M = {M}, K = {K}")
    call("uv_mx_quant_bf16", ptr(x), x.stride(-2), ptr(codes), codes.stride(-2), ptr(scales), scales.stride(-2), M, K, stream_ptr())
    return codes, scales


def gemm_mxfp8(a, a_scale, w, w_scale, bias, out, epi, M=None, gate=None, gate_tid=None):
    """gemm_bf16 for MXFP8 operands: a [M,K] / w [N,K] uint8 e4m3fn codes with their e8m0 scales [rows, >= K / 32] uint8 (mx_quant);
    bias bf16 [N] | None; out per epilogue, EPI_BF16 ... EPI_GATE_RESID_F32 (see include/univid_hip.h)."""
    M = a.shape[0] if M is None else M
    N, K = w.shape
    _check("gemm_mxfp8", (a, "a", U8, K, M), (a_scale, "a_scale", U8, K // 32, M), (w, "w", U8, K, N), (w_scale, "w_scale", U8, K // 32, N),
           *_epilogue_args(a, bias, out, epi, M, N, gate, gate_tid))
    if a.shape[1] < K or M > min(a.shape[0], a_scale.shape[0]) or a_scale.shape[1] * 32 < K or w_scale.shape[1] * 32 < K or w_scale.shape[0] < N:
        raise UnividHipError(f"gemm_mxfp8: a {tuple(a.shape)} / a_scale {tuple(a_scale.shape)} / w {tuple(w.shape)} / w_scale "
                             f"{tuple(w_scale.shape)} do not fit M = {M}")
    call("uv_gemm_mxfp8_nt", ptr(a), a.stride(-2), ptr(a_scale), a_scale.stride(-2), ptr(w), w.stride(-2), ptr(w_scale), w_scale.stride(-2),
         ptr(bias), M, N, K, epi, ptr(out), out.stride(-2), ptr(gate), ptr(gate_tid), 0 if gate is None else gate.stride(-2), stream_ptr(),
         flops=2 * M * N * K)
    return out


def _mx_operands(fn, a, a_scale, w, w_scale, M, N, K):
    """The shape conditions gemm_mxfp8 puts on its operands beyond _check's extents, for the two entry points beside it."""
    if a.shape[1] < K or M > min(a.shape[0], a_scale.shape[0]) or a_scale.shape[1] * 32 < K or w_scale.shape[1] * 32 < K or w_scale.shape[0] < N:
        raise UnividHipError(f"{fn}: a {tuple(a.shape)} / a_scale {tuple(a_scale.shape)} / w {tuple(w.shape)} / w_scale "
                             f"{tuple(w_scale.shape)} do not fit M = {M}")


def gemm_mxfp8_t(a, a_scale, w, w_scale, bias, out_t, M=None):
    """gemm_mxfp8(EPI_BF16) written transposed: out_t bf16 [N, >= M], out_t[n][m] = the bits gemm_mxfp8 writes at [m][n] (V^T of the
    MXFP8 v projection; include/univid_hip.h: uv_gemm_mxfp8_nt_t)."""
    M = a.shape[0] if M is None else M
    N, K = w.shape
    _check("gemm_mxfp8_t", (a, "a", U8, K, M), (a_scale, "a_scale", U8, K // 32, M), (w, "w", U8, K, N), (w_scale, "w_scale", U8, K // 32, N),
           (bias, "bias", BF16, N, None, True), (out_t, "out_t", BF16, M, N))
    _mx_operands("gemm_mxfp8_t", a, a_scale, w, w_scale, M, N, K)
    call("uv_gemm_mxfp8_nt_t", ptr(a), a.stride(-2), ptr(a_scale), a_scale.stride(-2), ptr(w), w.stride(-2), ptr(w_scale), w_scale.stride(-2),
         ptr(bias), M, N, K, ptr(out_t), out_t.stride(-2), stream_ptr(), flops=2 * M * N * K)
    return out_t


def gemm_mxfp8_ssq(a, a_scale, w, w_scale, bias, out, ssq, M=None):
    """gemm_mxfp8(EPI_BF16) plus ssq[m][g] = the output row's sum of squares over columns [32 g, 32 g + 32) (f32 [M, >= N / 32]), in
    gemm_bf16_ssq's summation order (include/univid_hip.h: uv_gemm_mxfp8_nt_ssq)."""
    M = a.shape[0] if M is None else M
    N, K = w.shape
    _check("gemm_mxfp8_ssq", (a, "a", U8, K, M), (a_scale, "a_scale", U8, K // 32, M), (w, "w", U8, K, N), (w_scale, "w_scale", U8, K // 32, N),
           (bias, "bias", BF16, N, None, True), (out, "out", BF16, N, M), (ssq, "ssq", F32, N // 32, M))
    _mx_operands("gemm_mxfp8_ssq", a, a_scale, w, w_scale, M, N, K)
    call("uv_gemm_mxfp8_nt_ssq", ptr(a), a.stride(-2), ptr(a_scale), a_scale.stride(-2), ptr(w), w.stride(-2), ptr(w_scale), w_scale.stride(-2),
         ptr(bias), M, N, K, ptr(out), out.stride(-2), ptr(ssq), ssq.stride(-2), stream_ptr(), flops=2 * M * N * K)
    return out


def gemm_bf16_ssq(a, w, bias, out, ssq, M=None, tile_cfg=0):
    """out = bf16(a w^T + bias) and ssq[m][g] = the output row's sum of squares over columns [32 g, 32 g + 32) (f32 [M, N / 32])."""
    M = a.shape[0] if M is None else M
    N, K = w.shape
    _check("gemm_bf16_ssq", (a, "a", BF16, K, M), (w, "w", BF16, K, N), (bias, "bias", BF16, N, None, True), (out, "out", BF16, N, M),
           (ssq, "ssq", F32, N // 32, M))
    call("uv_gemm_bf16_nt_ssq", ptr(a), a.stride(-2), ptr(w), w.stride(-2), ptr(bias), M, N, K, ptr(out), out.stride(-2), ptr(ssq), ssq.stride(-2),
         tile_cfg, stream_ptr(), flops=2 * M * N * K)
    return out


def rms_scale_from_ssq(ssq, rs, M, C, eps):
    """rs[m] = 1 / sqrt(sum(ssq[m]) / C + eps): the RMSNorm scale of row m from its per-group sums of squares."""
    _check("rms_scale_from_ssq", (ssq, "ssq", F32, ssq.shape[1], M), (rs, "rs", F32, M))
    call("uv_rms_scale_from_ssq", ptr(ssq), ssq.stride(-2), M, ssq.shape[1], C, float(eps), ptr(rs), stream_ptr())
    return rs


def lora_down(buf, K, A, scale, M=None, Rpad=None):
    """The un-merged LoRA slot of an activation buffer, in place: buf bf16 [rows, >= K + Rpad] holds x in its first K columns;
    columns [K, K + Rpad) of its first M rows become bf16(scale * (x A^T)), zero beyond A's R rows (include/univid_hip.h).
    A bf16 [R, K] (stacked lora_A weights), scale f32 [R]. Rpad defaults to R rounded up to whole 128-column groups."""
    R = A.shape[0]
    M = buf.shape[0] if M is None else M
    Rpad = (R + 127) // 128 * 128 if Rpad is None else Rpad
    _check("lora_down", (buf, "buf", BF16, K + Rpad, M), (A, "A", BF16, K, R), (scale, "scale", F32, R))
    if buf.dim() != 2 or A.dim() != 2 or A.shape[1] != K or scale.numel() != R or buf.shape[1] < K + Rpad or M > buf.shape[0]:
        raise UnividHipError(f"lora_down: buffer {tuple(buf.shape)} / A {tuple(A.shape)} / scale {tuple(scale.shape)} do not fit K = {K}, "
                             f"slot = {Rpad}, M = {M}")
    out = buf[:, K:]
    call("uv_lora_down_bf16", ptr(buf), buf.stride(-2), ptr(A), A.stride(-2), ptr(scale), M, K, R, ptr(out), buf.stride(-2), Rpad, stream_ptr(),
         flops=2 * M * R * K)
    return buf


def lora_down_seg(buf, K, A, scale, seg_rows, M=None, Rpad=None):
    """lora_down with one scale row per segment of `seg_rows` consecutive rows of buf (a stacked sample): scale f32 [nseg, R], rows
    stride(0) apart; row m of buf takes scale[m // seg_rows], and a zero entry gives exactly +0 (uv_lora_down_seg_bf16). The rows of
    `scale` must cover the M rows; the last segment may be partial."""
    R = A.shape[0]
    M = buf.shape[0] if M is None else M
    Rpad = (R + 127) // 128 * 128 if Rpad is None else Rpad
    nseg = scale.shape[0] if scale is not None and scale.dim() == 2 else 0
    _check("lora_down_seg", (buf, "buf", BF16, K + Rpad, M), (A, "A", BF16, K, R), (scale, "scale", F32, R, nseg))
    if buf.dim() != 2 or A.dim() != 2 or A.shape[1] != K or scale.shape[1] != R or buf.shape[1] < K + Rpad or M > buf.shape[0]:
        raise UnividHipError(f"lora_down_seg: buffer {tuple(buf.shape)} / A {tuple(A.shape)} / scale {tuple(scale.shape)} do not fit K = {K}, "
                             f"slot = {Rpad}, M = {M}")
    seg_rows = int(seg_rows)
    if seg_rows < 1 or nseg < 1 or nseg * seg_rows < M:
        raise UnividHipError(f"lora_down_seg: {nseg} scale row(s) for segments of {seg_rows} row(s) do not cover M = {M}")
    out = buf[:, K:]
    call("uv_lora_down_seg_bf16", ptr(buf), buf.stride(-2), ptr(A), A.stride(-2), ptr(scale), scale.stride(-2), seg_rows, nseg, M, K, R,
         ptr(out), buf.stride(-2), Rpad, stream_ptr(), flops=2 * M * R * K)
    return buf


def cast_f32_bf16(x, out, R, C):
    """out[:R, :C] = bf16(x[:R, :C]); the contiguous entry point when neither side has a wider leading dimension."""
    _check("cast_f32_bf16", (x, "x", F32, C, R), (out, "out", BF16, C, R))
    if x.stride(-2) == C and out.stride(-2) == C:
        call("uv_cast_f32_bf16", ptr(x), ptr(out), R * C, stream_ptr())
    else:
        call("uv_cast_f32_bf16_rows", ptr(x), x.stride(-2), ptr(out), out.stride(-2), R, C, stream_ptr())
    return out


def gemm_f32(a, w, bias, out, resid=None, M=None):
    """out = a w^T + bias (+ resid), all f32: a [..., K] (M rows, default every leading dimension: a channels-last [T, H, W, C] view is
    its pixel rows), w [N, K], bias [N] | None, out / resid [..., N]."""
    M = a.numel() // a.shape[-1] if M is None else M
    N, K = w.shape
    _check("gemm_f32", (a, "a", F32, K, M), (w, "w", F32, K, N), (bias, "bias", F32, N, None, True), (out, "out", F32, N, M),
           (resid, "resid", F32, N, M, True))
    call("uv_gemm_f32_nt", ptr(a), a.stride(-2), ptr(w), w.stride(-2), ptr(bias), M, N, K, ptr(out), out.stride(-2),
         ptr(resid), 0 if resid is None else resid.stride(-2), stream_ptr())
    return out


# -- DiT: attention and its operator seam --
def vt_cols(batch, L):
    """Columns of the V^T operand of `flash_attn` for `batch` stacked samples of L keys: sample b's keys are columns [b*L, (b+1)*L), and
    the last sample's run up to its 64-key tile bound. The columns past batch*L are masked by the kernels (P = 0 exactly), so they only
    have to be FINITE."""
    return (batch - 1) * L + (L + 63) // 64 * 64


def flash_attn(q, k, vt, out, Lq, Lk, H, D, scale, batch=1, q_rs=None, q_weight=None):
    """q [batch*Lq, C], k [batch*Lk, C], vt [C, >= vt_cols(batch, Lk)] (sample b = columns b*Lk..), out [batch*Lq, C].
    q_rs / q_weight: q is the RAW projection and the kernel's Q prologue applies norm_q (per-row scale f32 [batch*Lq], weight f32 [C])."""
    f16 = q.dtype == F16
    C, half = H * D, F16 if f16 else BF16
    if f16 and q_rs is not None:      # uv_flash_attn_bf16_qnorm would read the fp16 bits as bf16
        raise UnividHipError("flash_attn: the q-norm prologue (q_rs / q_weight) is built for bf16 only, q is fp16")
    _check("flash_attn", (q, "q", half, C, batch * Lq), (k, "k", half, C, batch * Lk),
           (vt, "vt", half, vt_cols(batch, Lk), C), (out, "out", half, C, batch * Lq),
           (q_rs, "q_rs", F32, batch * Lq, None, True), (q_weight, "q_weight", F32, C, None, q_rs is None))
    if q_rs is not None:
        call("uv_flash_attn_bf16_qnorm", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(vt), vt.stride(-2), ptr(out), out.stride(-2),
             batch, Lq, Lk, H, D, float(scale), ptr(q_rs), ptr(q_weight), stream_ptr(), flops=4 * batch * Lq * Lk * H * D)
        return out
    call("uv_flash_attn_f16" if f16 else "uv_flash_attn_bf16", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(vt), vt.stride(-2), ptr(out), out.stride(-2),
         batch, Lq, Lk, H, D, float(scale), stream_ptr(), flops=4 * batch * Lq * Lk * H * D)
    return out


def attn_kernel_name(Lq, Lk, D, batch=1, H=None, f16=False, ldk=None, ldvt=None):
    """Name of the kernel `flash_attn` dispatches for this geometry. ldk / ldvt: the leading dimensions of k and V^T, default the dense
    ones ([tokens, H*D] rows as the DiT uses them, V^T just wide enough for the batch)."""
    H = H or 1
    buf = ctypes.create_string_buffer(96)
    ldk = H * D if ldk is None else ldk
    ldvt = vt_cols(batch, Lk) if ldvt is None else ldvt
    rc = load().uv_flash_attn_kernel_name(Lk, D, int(ldk), int(ldvt), int(f16), buf, 96)
    if rc != 0:
        raise UnividHipError(load().uv_last_error().decode())
    return buf.value.decode()


def attn_plan(Lq, Lk, D, batch=1, H=1, f16=False, ldk=None, ldvt=None):
    """Launch plan of `flash_attn` for this geometry on the current device - 256 CUs without one - under the current OPT_ATTN_CUT:
    dict(kernel=name, q_blocks=blocks per (sample, head), n12=how many of them own 12 units, grid=workgroups). ldk / ldvt: the leading
    dimensions of k and V^T, default the dense ones ([tokens, H*D] rows, V^T just wide enough for the batch)."""
    buf = ctypes.create_string_buffer(96)
    qb, n12, grid = _I(0), _I(0), _I(0)
    ldk = H * D if ldk is None else ldk
    ldvt = vt_cols(batch, Lk) if ldvt is None else ldvt
    lib = load()
    if lib.uv_flash_attn_plan(batch, Lq, Lk, H, D, int(ldk), int(ldvt), int(f16), buf, 96, ctypes.byref(qb), ctypes.byref(n12), ctypes.byref(grid)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return dict(kernel=buf.value.decode(), q_blocks=qb.value, n12=n12.value, grid=grid.value)


def flash_attn_win(q, k, vt, out, L, H, D, scale, window, batch=1):
    """`flash_attn` for Lq == Lk == L under flash-attn's window_size = (left, right): query i attends keys max(0, i - left) ..
    min(L - 1, i + right) of its sample, -1 = unbounded on that side (causal = right 0). bf16, head_dim 128 only; (-1, -1) visits every key
    and equals `flash_attn` bit for bit."""
    C = H * D
    left, right = (int(w) for w in window)
    _check("flash_attn_win", (q, "q", BF16, C, batch * L), (k, "k", BF16, C, batch * L), (vt, "vt", BF16, vt_cols(batch, L), C),
           (out, "out", BF16, C, batch * L))
    call("uv_flash_attn_win_bf16", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(vt), vt.stride(-2), ptr(out), out.stride(-2), batch, L, H, D,
         float(scale), left, right, stream_ptr(), flops=4 * batch * L * L * H * D)
    return out


def attn_win_plan(L, D=128, batch=1, H=1, window=(-1, -1)):
    """Launch plan of `flash_attn_win` for this geometry and window, as `attn_plan` reports `flash_attn`'s."""
    buf = ctypes.create_string_buffer(96)
    qb, n12, grid = _I(0), _I(0), _I(0)
    lib = load()
    if lib.uv_flash_attn_win_plan(batch, L, H, D, int(window[0]), int(window[1]), buf, 96, ctypes.byref(qb), ctypes.byref(n12),
                                  ctypes.byref(grid)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return dict(kernel=buf.value.decode(), q_blocks=qb.value, n12=n12.value, grid=grid.value)


class PreparedBlockMask:
    """A block mask as `flash_attn_bs` takes it: the key-tile schedule of one sequence length on one device. Immutable; built only by
    `prepare_block_mask`. L: the sequence length; heads: 1 (one mask for all heads) or H; tile_idx int32 [heads, nqb, nkb] (each row's
    visible 64-key tiles ascending, the rest of the row -1, never read) and tile_cnt int32 [heads, nqb] on `device`; mask: the expanded
    bool mask [heads, nqb, nkb] on the CPU; density: the fraction of set tiles."""
    __slots__ = ("L", "heads", "tile_idx", "tile_cnt", "mask", "density")

    def __init__(self, L, heads, tile_idx, tile_cnt, mask, density, _token=None):
        if _token is not _PBM_TOKEN:
            raise TypeError("PreparedBlockMask is built by prepare_block_mask(mask, L, device)")
        for name, v in (("L", L), ("heads", heads), ("tile_idx", tile_idx), ("tile_cnt", tile_cnt), ("mask", mask), ("density", density)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("PreparedBlockMask is immutable: prepare a new mask")

    def __delattr__(self, name):
        raise AttributeError("PreparedBlockMask is immutable: prepare a new mask")

    @property
    def device(self):
        return self.tile_idx.device

    def __repr__(self):
        return f"PreparedBlockMask(L={self.L}, heads={self.heads}, density={self.density:.4f}, device={self.tile_idx.device})"


_PBM_TOKEN = object()
BS_Q_BLOCK, BS_K_BLOCK = 128, 64      # the kernel's tile: 4 x UV_ATT_QW queries, UV_ATT_KV keys


def _expand_block_mask(fn, mask, L, q_block, k_block):
    """A block mask [nqb', nkb'] / [H, nqb', nkb'] of q_block x k_block blocks, checked against L and expanded exactly to the kernel's
    128 x 64 tiles: (bool [heads, nqb, nkb] on the CPU, L). `fn` names the caller in the messages."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise TypeError(f"{fn}: the mask must be a torch.bool tensor, got "
                        f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
    L, q_block, k_block = int(L), int(q_block), int(k_block)
    if L <= 0:
        raise ValueError(f"{fn}: L = {L} must be positive")
    if q_block <= 0 or q_block % BS_Q_BLOCK or k_block <= 0 or k_block % BS_K_BLOCK:
        raise ValueError(f"{fn}: q_block {q_block} must be a multiple of {BS_Q_BLOCK} and k_block {k_block} a multiple of "
                         f"{BS_K_BLOCK} (the kernel's tile is {BS_Q_BLOCK} queries x {BS_K_BLOCK} keys)")
    if mask.dim() not in (2, 3):
        raise ValueError(f"{fn}: the mask must be [nqb, nkb] or [H, nqb, nkb], got shape {tuple(mask.shape)}")
    want = (-(-L // q_block), -(-L // k_block))
    if tuple(mask.shape[-2:]) != want:
        raise ValueError(f"{fn}: mask shape {tuple(mask.shape)} does not belong to L = {L}: {q_block} x {k_block} blocks "
                         f"need [..., {want[0]}, {want[1]}]")
    if mask.dim() == 3 and mask.shape[0] < 1:
        raise ValueError(f"{fn}: a per-head mask needs at least one head")
    m = mask.detach().to("cpu")
    m = m[None] if m.dim() == 2 else m
    nqb, nkb = -(-L // BS_Q_BLOCK), -(-L // BS_K_BLOCK)
    m = m.repeat_interleave(q_block // BS_Q_BLOCK, dim=1)[:, :nqb].repeat_interleave(k_block // BS_K_BLOCK, dim=2)[:, :, :nkb].contiguous()
    return m, L


def prepare_block_mask(mask, L, device, q_block=BS_Q_BLOCK, k_block=BS_K_BLOCK):
    """The schedule of a block mask for `flash_attn_bs` at sequence length L. mask: a bool tensor [ceil(L / q_block), ceil(L / k_block)]
    (all heads) or [H, ...] (per head); query i of head h attends key j iff mask[h][i // q_block][j // k_block] and j < L. q_block any
    multiple of 128, k_block any multiple of 64 (128 x 128: FlexAttention's default block): coarser masks are expanded exactly to the
    kernel's 128 x 64 tiles. Every query block of every head needs at least one set tile (ValueError otherwise: no empty softmax rows
    exist). The lists are built with CPU ops and uploaded: call it once per mask, outside any graph capture."""
    m, L = _expand_block_mask("prepare_block_mask", mask, L, q_block, k_block)
    nqb, nkb = -(-L // BS_Q_BLOCK), -(-L // BS_K_BLOCK)
    cnt = m.sum(dim=2, dtype=torch.int32)
    if bool((cnt == 0).any()):
        hh, qq = (int(v) for v in (cnt == 0).nonzero()[0])
        raise ValueError(f"prepare_block_mask: query block {qq} of mask head {hh} (queries {qq * BS_Q_BLOCK}..) has no key tile: every "
                         f"{BS_Q_BLOCK}-query block of every head must see at least one tile (an empty softmax row has no value)")
    # each row's set tiles first, ascending (a stable sort of "unset" keeps the column order), the rest -1
    order = torch.sort((~m).to(torch.uint8), dim=2, stable=True).indices.to(torch.int32)
    idx = torch.where(torch.arange(nkb, dtype=torch.int32)[None, None, :] < cnt[:, :, None], order, torch.full_like(order, -1)).contiguous()
    dev = torch.device(device)
    return PreparedBlockMask(L, int(m.shape[0]), idx.to(dev), cnt.contiguous().to(dev), m, float(m.double().mean()), _token=_PBM_TOKEN)


def flash_attn_bs(q, k, vt, out, L, H, D, scale, bm, batch=1):
    """`flash_attn` for Lq == Lk == L under the block mask `bm` (a PreparedBlockMask: `prepare_block_mask`): query i of head h attends key j
    iff bm.mask[h or 0][i // 128][j // 64] and j < L; the samples of a stacked launch share the mask. bf16, head_dim 128 only; the all-ones
    mask equals `flash_attn` bit for bit."""
    C = H * D
    if not isinstance(bm, PreparedBlockMask):
        raise UnividHipError(f"flash_attn_bs.bm: a PreparedBlockMask is required (prepare_block_mask), got {type(bm).__name__}")
    if bm.L != L:
        raise UnividHipError(f"flash_attn_bs.bm: the mask was prepared for L = {bm.L}, the launch has L = {L}")
    if bm.heads not in (1, H):
        raise UnividHipError(f"flash_attn_bs.bm: the mask has {bm.heads} heads, the launch {H} (1 = shared by all heads, or H)")
    if bm.tile_idx.device != q.device:
        raise UnividHipError(f"flash_attn_bs.bm: the mask lives on {bm.tile_idx.device}, the tensors on {q.device}")
    nqb, nkb = -(-L // BS_Q_BLOCK), -(-L // BS_K_BLOCK)
    _check("flash_attn_bs", (q, "q", BF16, C, batch * L), (k, "k", BF16, C, batch * L), (vt, "vt", BF16, vt_cols(batch, L), C),
           (out, "out", BF16, C, batch * L), (bm.tile_idx, "bm.tile_idx", I32, bm.heads * nqb * nkb), (bm.tile_cnt, "bm.tile_cnt", I32, bm.heads * nqb))
    call("uv_flash_attn_bs_bf16", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(vt), vt.stride(-2), ptr(out), out.stride(-2), batch, L, H, D,
         float(scale), ptr(bm.tile_idx), ptr(bm.tile_cnt), bm.heads, stream_ptr(), flops=int(4 * batch * L * L * H * D * bm.density))
    return out


def attn_bs_plan(L, D=128, batch=1, H=1):
    """Launch plan of `flash_attn_bs` for this geometry (the mask does not change it), as `attn_plan` reports `flash_attn`'s."""
    buf = ctypes.create_string_buffer(96)
    qb, grid = _I(0), _I(0)
    lib = load()
    if lib.uv_flash_attn_bs_plan(batch, L, H, D, buf, 96, ctypes.byref(qb), ctypes.byref(grid)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return dict(kernel=buf.value.decode(), q_blocks=qb.value, grid=grid.value)


def prepare_keep_mask(mask, L, device, q_block=BS_Q_BLOCK, k_block=BS_K_BLOCK):
    """The static keep mask of `attn_bs_select` at sequence length L: `prepare_block_mask`'s shapes and block expansion, but rows may be
    empty (the selection adds its top-k tiles to every row). Returns (uint8 [heads, nqb, nkb] on `device`, the expanded bool mask on the
    CPU). Built with CPU ops and uploaded: once per mask, outside any graph capture."""
    m, _ = _expand_block_mask("prepare_keep_mask", mask, L, q_block, k_block)
    return m.to(torch.uint8).to(torch.device(device)), m


BS_SELECT_MAX_TILES = 4096      # uv_attn_bs_select sorts a row's key tiles in LDS


def attn_pool_qk(q, k, qbar, kbar, L, H, D, batch=1):
    """The pooled operands of the top-k tile selection: q, k bf16 [batch*L, >= H*D] (after RMSNorm + RoPE, as the attention kernel reads them)
    -> qbar fp32 [batch, H, ceil(L / 128), D] and kbar fp32 [batch, H, ceil(L / 64), D], the fp32 mean of each 128-query block's / 64-key
    tile's valid rows. head_dim 128 only."""
    C = H * D
    nqb, nkb = -(-L // BS_Q_BLOCK), -(-L // BS_K_BLOCK)
    _check("attn_pool_qk", (q, "q", BF16, C, batch * L), (k, "k", BF16, C, batch * L), (qbar, "qbar", F32, batch * H * nqb * D),
           (kbar, "kbar", F32, batch * H * nkb * D))
    call("uv_attn_pool_qk", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(qbar), ptr(kbar), batch, L, H, D, stream_ptr())
    return qbar, kbar


def attn_bs_select(qbar, kbar, keep, top_k, tile_idx, tile_cnt, L, H, batch=1):
    """The key-tile lists of `flash_attn_bs_lists` from pooled scores: per (sample, head, 128-query block) the tiles `keep` marks (uint8
    [1 or H, nqb, nkb] on the device, or None) plus the `top_k` best of the others by s = qbar . kbar (score descending, tile index
    ascending), written ascending into tile_idx int32 [batch, H, nqb, nkb] with their number in tile_cnt int32 [batch, H, nqb]. At most
    BS_SELECT_MAX_TILES key tiles."""
    nqb, nkb = -(-L // BS_Q_BLOCK), -(-L // BS_K_BLOCK)
    keep_heads = 1
    if keep is not None:
        if keep.dim() != 3 or tuple(keep.shape[1:]) != (nqb, nkb):
            raise UnividHipError(f"attn_bs_select.keep: expected uint8 [1 or {H}, {nqb}, {nkb}], got shape {tuple(keep.shape)}")
        keep_heads = int(keep.shape[0])
    _check("attn_bs_select", (qbar, "qbar", F32, batch * H * nqb * 128), (kbar, "kbar", F32, batch * H * nkb * 128),
           (keep, "keep", U8, keep_heads * nqb * nkb, None, True), (tile_idx, "tile_idx", I32, batch * H * nqb * nkb),
           (tile_cnt, "tile_cnt", I32, batch * H * nqb))
    call("uv_attn_bs_select", ptr(qbar), ptr(kbar), ptr(keep), keep_heads, int(top_k), ptr(tile_idx), ptr(tile_cnt), batch, L, H, stream_ptr())
    return tile_idx, tile_cnt


def flash_attn_bs_lists(q, k, vt, out, L, H, D, scale, tile_idx, tile_cnt, mask_heads, mask_samples, batch=1):
    """`flash_attn_bs` under raw lists on the device with a leading sample axis: tile_idx int32 [mask_samples, mask_heads, nqb, nkb],
    tile_cnt int32 [mask_samples, mask_heads, nqb] (`prepare_block_mask`'s format; `attn_bs_select` writes them); mask_samples 1 (shared
    by the samples, `flash_attn_bs` exactly) or batch, mask_heads 1 or H."""
    C = H * D
    nqb, nkb = -(-L // BS_Q_BLOCK), -(-L // BS_K_BLOCK)
    rows = max(int(mask_samples), 0) * max(int(mask_heads), 0) * nqb
    _check("flash_attn_bs_lists", (q, "q", BF16, C, batch * L), (k, "k", BF16, C, batch * L), (vt, "vt", BF16, vt_cols(batch, L), C),
           (out, "out", BF16, C, batch * L), (tile_idx, "tile_idx", I32, rows * nkb), (tile_cnt, "tile_cnt", I32, rows))
    call("uv_flash_attn_bs_lists_bf16", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(vt), vt.stride(-2), ptr(out), out.stride(-2), batch, L,
         H, D, float(scale), ptr(tile_idx), ptr(tile_cnt), int(mask_heads), int(mask_samples), stream_ptr())
    return out


def flash_attn_mxqk(q_codes, q_scales, k_codes, k_scales, vt, out, Lq, Lk, H, D, scale, batch=1):
    """`flash_attn` with MXFP8 q / k (include/univid_hip.h): q_codes uint8 [batch*Lq, >= H*128] / q_scales uint8 [batch*Lq, >= H*4] (head h
    at bytes 128 h / 4 h), k likewise over batch*Lk rows (`rmsnorm_rope_qk_mx` or `mx_quant` write them); vt / out bf16 as for `flash_attn`.
    head_dim 128 only."""
    C = H * D
    _check("flash_attn_mxqk", (q_codes, "q_codes", U8, C, batch * Lq), (q_scales, "q_scales", U8, C // 32, batch * Lq),
           (k_codes, "k_codes", U8, C, batch * Lk), (k_scales, "k_scales", U8, C // 32, batch * Lk),
           (vt, "vt", BF16, vt_cols(batch, Lk), C), (out, "out", BF16, C, batch * Lq))
    call("uv_flash_attn_mxqk", ptr(q_codes), q_codes.stride(-2), ptr(q_scales), q_scales.stride(-2), ptr(k_codes), k_codes.stride(-2),
         ptr(k_scales), k_scales.stride(-2), ptr(vt), vt.stride(-2), ptr(out), out.stride(-2), batch, Lq, Lk, H, D, float(scale), stream_ptr(),
         flops=4 * batch * Lq * Lk * H * D)
    return out


def attn_mxqk_plan(Lq, Lk, D=128, batch=1, H=1):
    """Launch plan of `flash_attn_mxqk` for this geometry, as `attn_plan` reports `flash_attn`'s."""
    buf = ctypes.create_string_buffer(96)
    qb, n12, grid = _I(0), _I(0), _I(0)
    lib = load()
    if lib.uv_flash_attn_mxqk_plan(batch, Lq, Lk, H, D, buf, 96, ctypes.byref(qb), ctypes.byref(n12), ctypes.byref(grid)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return dict(kernel=buf.value.decode(), q_blocks=qb.value, n12=n12.value, grid=grid.value)


def vt_mx_cols(batch, L):
    """Columns of the MXFP8 V^T codes of `flash_attn_mxpv` for `batch` stacked samples of L keys: every sample padded to whole 64-key tiles
    (sample b = columns [b*Lkp, (b+1)*Lkp), Lkp = roundup(L, 64)); the scale array has 4 bytes per column and head."""
    return batch * ((L + 63) // 64 * 64)


def vt_mx_quant(vt, vt_codes, vt_scales, Lk, H, D=128, batch=1):
    """bf16 vt [H*D, >= (batch-1)*Lk + roundup(Lk, 8)] (sample b = columns b*Lk.., as the EPI_BF16_T GEMM writes it) -> vt_codes uint8
    [H*D, >= vt_mx_cols(batch, Lk)] and vt_scales uint8 [H, >= 4 * vt_mx_cols(batch, Lk)] in the V^T format of include/univid_hip.h (keys
    permuted inside their 32-key block, tile-major scales, pads written). head_dim 128 only."""
    C, cols = H * D, vt_mx_cols(batch, Lk)
    _check("vt_mx_quant", (vt, "vt", BF16, (batch - 1) * Lk + (Lk + 7) // 8 * 8, C), (vt_codes, "vt_codes", U8, cols, C),
           (vt_scales, "vt_scales", U8, 4 * cols, H))
    call("uv_vt_mx_quant", ptr(vt), vt.stride(-2), ptr(vt_codes), vt_codes.stride(-2), ptr(vt_scales), vt_scales.stride(-2), batch, Lk, H, D,
         stream_ptr())
    return vt_codes, vt_scales


def flash_attn_mxpv(q_codes, q_scales, k_codes, k_scales, vt_codes, vt_scales, out, Lq, Lk, H, D, scale, batch=1):
    """`flash_attn_mxqk` with the MXFP8 V^T of `vt_mx_quant` (codes uint8 [H*128, >= vt_mx_cols(batch, Lk)], scales uint8 [H, >= 4 x that]) and
    e4m3 softmax weights: P.V on the block-scaled matrix instruction as well (include/univid_hip.h). head_dim 128 only."""
    C, cols = H * D, vt_mx_cols(batch, Lk)
    _check("flash_attn_mxpv", (q_codes, "q_codes", U8, C, batch * Lq), (q_scales, "q_scales", U8, C // 32, batch * Lq),
           (k_codes, "k_codes", U8, C, batch * Lk), (k_scales, "k_scales", U8, C // 32, batch * Lk),
           (vt_codes, "vt_codes", U8, cols, C), (vt_scales, "vt_scales", U8, 4 * cols, H), (out, "out", BF16, C, batch * Lq))
    call("uv_flash_attn_mxpv", ptr(q_codes), q_codes.stride(-2), ptr(q_scales), q_scales.stride(-2), ptr(k_codes), k_codes.stride(-2),
         ptr(k_scales), k_scales.stride(-2), ptr(vt_codes), vt_codes.stride(-2), ptr(vt_scales), vt_scales.stride(-2), ptr(out), out.stride(-2),
         batch, Lq, Lk, H, D, float(scale), stream_ptr(), flops=4 * batch * Lq * Lk * H * D)
    return out


def attn_mxpv_plan(Lq, Lk, D=128, batch=1, H=1):
    """Launch plan of `flash_attn_mxpv` for this geometry, as `attn_plan` reports `flash_attn`'s."""
    buf = ctypes.create_string_buffer(96)
    qb, n12, grid = _I(0), _I(0), _I(0)
    lib = load()
    if lib.uv_flash_attn_mxpv_plan(batch, Lq, Lk, H, D, buf, 96, ctypes.byref(qb), ctypes.byref(n12), ctypes.byref(grid)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return dict(kernel=buf.value.decode(), q_blocks=qb.value, n12=n12.value, grid=grid.value)


def conv_plan(prec, Tout, Hout, Wout, Hin, Win, Cin, Cout, kt, kh, kw, st=1, sh=1, sw=1, ph=0, pw=0, up=0, interleave=0):
    """Launch plan of a uv_conv3d_* call of this geometry on the current device - 256 CUs without one - under the current OPT_CONV_HALO:
    dict(kernel=name, tiles_m=row tiles or pixel patches, tiles_n=output-channel tiles). prec: 0 f32, 1 / 2 bf16x3 without / with
    in_split, 3 bf16x6, 4 f16x3 - and the single-pass 'f16' entry asked with HALF its Cin (it runs the plain-row form of that kernel)."""
    buf = ctypes.create_string_buffer(32)
    tm, tn = _I(0), _I(0)
    lib = load()
    if lib.uv_conv3d_plan(prec, Tout, Hout, Wout, Hin, Win, Cin, Cout, kt, kh, kw, st, sh, sw, ph, pw, up, interleave, buf, 32,
                          ctypes.byref(tm), ctypes.byref(tn)) != 0:
        raise UnividHipError(lib.uv_last_error().decode())
    return dict(kernel=buf.value.decode(), tiles_m=tm.value, tiles_n=tn.value)


def cast_f32_to16(x, out):
    """out (bf16 or IEEE fp16) = x (f32), round to nearest even; contiguous tensors of x.numel() elements."""
    _check("cast_f32_to16", (x, "x", F32, x.numel()), (out, "out", _16, x.numel()))
    call("uv_cast_f32_to16", ptr(x), ptr(out), x.numel(), int(out.dtype == F16), stream_ptr())
    return out


def cast_16_to_f32(x, out):
    """out (f32) = x (bf16 or IEEE fp16), exact; contiguous tensors of x.numel() elements."""
    _check("cast_16_to_f32", (x, "x", _16, x.numel()), (out, "out", F32, x.numel()))
    call("uv_cast_16_to_f32", ptr(x), ptr(out), x.numel(), int(x.dtype == F16), stream_ptr())
    return out


def transpose_16(rows, out, L, C, Lpad):
    """out[c][l] = rows[l][c] for l < L, c < C (16-bit elements); columns L .. Lpad - 1 of out are written as zero."""
    _check("transpose_16", (rows, "rows", _16, C, L), (out, "out", rows.dtype, Lpad, C))
    call("uv_transpose_16", ptr(rows), rows.stride(-2), ptr(out), out.stride(-2), L, C, Lpad, stream_ptr())
    return out


# -- DiT: fused glue --
def layernorm_mod(x, out, L, C, eps, mode=0, tab=None, shift_off=0, scale_off=0, tid=None, w=None, b=None,
                  round_ln=False):
    _check("layernorm_mod", (x, "x", F32, C, L), (out, "out", (F32, BF16, F16), C, L),
           (tab, "tab", F32, max(shift_off, scale_off) + C, 0 if tab is None else tab.shape[0], True), (tid, "tid", I32, L, None, True),
           (w, "w", F32, C, None, True), (b, "b", F32, C, None, True))
    call("uv_layernorm_mod", ptr(x), x.stride(-2), ptr(out), out.stride(-2), L, C, float(eps), mode, ptr(tab),
         0 if tab is None else tab.stride(-2), shift_off, scale_off, ptr(tid), ptr(w), ptr(b), int(round_ln),
         2 if out.dtype == F16 else int(out.dtype == BF16), stream_ptr())
    return out


def layernorm_mod_mx(x, codes, scales, L, C, eps, mode=1, tab=None, shift_off=0, scale_off=0, tid=None, w=None, b=None, round_ln=False):
    """layernorm_mod (mode 1 or 2, bf16 output) stored as OCP MXFP8: codes uint8 [L, >= C] and scales uint8 [L, >= C / 32] hold, bit for
    bit, mx_quant of what layernorm_mod writes into a bf16 `out` for the same inputs (include/univid_hip.h: uv_layernorm_mod_mx)."""
    _check("layernorm_mod_mx", (x, "x", F32, C, L), (codes, "codes", U8, C, L), (scales, "scales", U8, C // 32, L),
           (tab, "tab", F32, max(shift_off, scale_off) + C, 0 if tab is None else tab.shape[0], True), (tid, "tid", I32, L, None, True),
           (w, "w", F32, C, None, True), (b, "b", F32, C, None, True))
    call("uv_layernorm_mod_mx", ptr(x), x.stride(-2), ptr(codes), codes.stride(-2), ptr(scales), scales.stride(-2), L, C, float(eps), mode,
         ptr(tab), 0 if tab is None else tab.stride(-2), shift_off, scale_off, ptr(tid), ptr(w), ptr(b), int(round_ln), stream_ptr())
    return codes, scales


def rmsnorm_rope(x, out, weight, L, C, D, eps, freqs=None, grid=(0, 0, 0), row0=0):
    """freqs: the complex128 [1024, D / 2] RoPE table as float64 (re, im) pairs, or None (no rotary embedding)."""
    _check("rmsnorm_rope", (x, "x", BF16, C, L), (out, "out", BF16, C, L), (weight, "weight", F32, C),
           (freqs, "freqs", torch.float64, 1024 * D, None, True))
    call("uv_rmsnorm_rope", ptr(x), x.stride(-2), ptr(out), out.stride(-2), ptr(weight), L, C, D, float(eps), ptr(freqs),
         int(grid[0]), int(grid[1]), int(grid[2]), int(row0), stream_ptr())
    return out


def rmsnorm_rope_qk(q, k, q_weight, k_weight, L, Ls, C, D, eps, freqs, grid, row0=0):
    """In-place QK RMSNorm + RoPE of q and k (same strides) in one launch; rows = L / Ls stacked samples of Ls tokens."""
    _check("rmsnorm_rope_qk", (q, "q", BF16, C, L), (k, "k", BF16, C, L), (q_weight, "q_weight", F32, C), (k_weight, "k_weight", F32, C),
           (freqs, "freqs", torch.float64, 1024 * D, None, True))
    if q.stride(-2) != k.stride(-2):
        raise UnividHipError("rmsnorm_rope_qk: q and k must have the same row stride")
    call("uv_rmsnorm_rope_qk", ptr(q), ptr(q), ptr(q_weight), ptr(k), ptr(k), ptr(k_weight), q.stride(-2), q.stride(-2), L, Ls, C, D,
         float(eps), ptr(freqs), int(grid[0]), int(grid[1]), int(grid[2]), int(row0), stream_ptr())


def rmsnorm_rope_qk_mx(q, k, q_weight, k_weight, q_codes, q_scales, k_codes, k_scales, L, Ls, C, D, eps, freqs, grid, row0=0):
    """`rmsnorm_rope_qk` with an MXFP8 store: q / k bf16 [L, C] are only READ; codes uint8 [L, >= C] and scales uint8 [L, >= C / 32] receive,
    bit for bit, `mx_quant` of what `rmsnorm_rope_qk` would write. head_dim 128 only."""
    _check("rmsnorm_rope_qk_mx", (q, "q", BF16, C, L), (k, "k", BF16, C, L), (q_weight, "q_weight", F32, C), (k_weight, "k_weight", F32, C),
           (q_codes, "q_codes", U8, C, L), (q_scales, "q_scales", U8, C // 32, L), (k_codes, "k_codes", U8, C, L),
           (k_scales, "k_scales", U8, C // 32, L), (freqs, "freqs", torch.float64, 1024 * D, None, True))
    if q.stride(-2) != k.stride(-2) or q_codes.stride(-2) != k_codes.stride(-2) or q_scales.stride(-2) != k_scales.stride(-2):
        raise UnividHipError("rmsnorm_rope_qk_mx: q / k, their codes and their scales must each share one row stride")
    call("uv_rmsnorm_rope_qk_mx", ptr(q), ptr(q_weight), ptr(q_codes), ptr(q_scales), ptr(k), ptr(k_weight), ptr(k_codes), ptr(k_scales),
         q.stride(-2), q_codes.stride(-2), q_scales.stride(-2), L, Ls, C, D, float(eps), ptr(freqs), int(grid[0]), int(grid[1]), int(grid[2]),
         int(row0), stream_ptr())
    return q_codes, q_scales, k_codes, k_scales


def text_weight_rows(x, out, n_scaled, w):
    """out[r] = bf16(x[r] * bf16(w)) for the first n_scaled rows of one sample's embedded context [R, C] bf16, the other rows copied:
    UniVid's dynamic text weight (model_pipeline.py:1787-1797)."""
    R, C = x.shape
    _check("text_weight_rows", (x, "x", BF16, C, R), (out, "out", BF16, C, R))
    call("uv_text_weight_rows_bf16", ptr(x), x.stride(-2), ptr(out), out.stride(-2), R, int(n_scaled), C, float(w), stream_ptr())
    return out


def patchify(x, out, patch):
    """x f32 [Cin, F, H, W] (contiguous) -> out bf16 [L, Kpad]: the im2col rows of the patch embedding, one per (pt, ph, pw) patch."""
    (Cin, F, H, W), (pt, ph, pw) = x.shape, patch
    _check("patchify", (x, "x", F32, x.numel()), (out, "out", BF16, out.shape[1], F // pt * (H // ph) * (W // pw)))
    call("uv_patchify_bf16", ptr(x), ptr(out), out.stride(-2), Cin, F, H, W, pt, ph, pw, out.shape[1], stream_ptr())
    return out


def unpatchify(rows, out, grid, patch):
    """rows f32 [Fp * Hp * Wp, pt * ph * pw * Cout] (head output) -> out f32 [Cout, Fp * pt, Hp * ph, Wp * pw] (contiguous)."""
    (Fp, Hp, Wp), (pt, ph, pw), Cout = grid, patch, out.shape[0]
    _check("unpatchify", (rows, "rows", F32, pt * ph * pw * Cout, Fp * Hp * Wp), (out, "out", F32, Fp * Hp * Wp * pt * ph * pw * Cout))
    call("uv_unpatchify_f32", ptr(rows), rows.stride(-2), ptr(out), Cout, Fp, Hp, Wp, pt, ph, pw, stream_ptr())
    return out


def sinusoid(t, out):
    """out f32 [n, dim] (contiguous) = sinusoidal_embedding_1d of the n timesteps t (f32)."""
    n, dim = t.numel(), out.shape[1]
    _check("sinusoid", (t, "t", F32, n), (out, "out", F32, n * dim))
    call("uv_sinusoid_f32", ptr(t), ptr(out), n, dim, stream_ptr())
    return out


def linear_rows(x, W, b, out, act_in=0):
    """out[r] = act_in(x[r]) W^T + b, f32, for a few rows: x [R, K], W [N, K] contiguous, b [N] | None, out [R, N]. act_in: 0 none, 1 SiLU."""
    R, (N, K) = x.shape[0], W.shape
    _check("linear_rows", (x, "x", F32, K, R), (W, "W", F32, N * K), (b, "b", F32, N, None, True), (out, "out", F32, N, R))
    call("uv_linear_rows_f32", ptr(x), x.stride(-2), ptr(W), ptr(b), ptr(out), out.stride(-2), R, N, K, int(act_in), stream_ptr())
    return out


def add_rows(mod, e0, out):
    """out[r] = mod + e0[r], f32: mod n elements, e0 / out [R, n], all contiguous."""
    R, n = out.shape
    _check("add_rows", (mod, "mod", F32, n), (e0, "e0", F32, R * n), (out, "out", F32, R * n))
    call("uv_add_rows_f32", ptr(mod), ptr(e0), ptr(out), R, n, stream_ptr())
    return out


def add_bf16_resid(x, y, L, C):
    """x f32 [L, C] += float(y bf16 [L, C])."""
    _check("add_bf16_resid", (x, "x", F32, C, L), (y, "y", BF16, C, L))
    call("uv_add_bf16_resid", ptr(x), x.stride(-2), ptr(y), y.stride(-2), L, C, stream_ptr())
    return x


def l2_normalize_rows(x, out, eps=1e-12):
    """out[r] = x[r] / max(||x[r]||, eps), f32 [R, C]."""
    R, C = x.shape
    _check("l2_normalize_rows", (x, "x", F32, C, R), (out, "out", F32, C, R))
    call("uv_l2_normalize_rows_f32", ptr(x), x.stride(-2), ptr(out), out.stride(-2), R, C, eps, stream_ptr())
    return out


# -- text encoder and ContextProjector (bf16) --
def t5_attention(q, k, v, out, H, rel_bias, span):
    """umT5 attention of one prompt: q, k, v, out bf16 [n, H * 64]; rel_bias f32 [H, 2 * span - 1] (contiguous), span >= n."""
    n = q.shape[0]
    _check("t5_attention", (q, "q", BF16, H * 64, n), (k, "k", BF16, H * 64, n), (v, "v", BF16, H * 64, n), (out, "out", BF16, H * 64, n),
           (rel_bias, "rel_bias", F32, H * (2 * span - 1)))
    call("uv_t5_attention_bf16", ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(v), v.stride(-2), ptr(out), out.stride(-2), n, H,
         ptr(rel_bias), span, stream_ptr())
    return out


def add_bf16(x, y, out):
    """out = x + y: contiguous bf16 tensors of out.numel() elements (out may be x or y)."""
    _check("add_bf16", (x, "x", BF16, out.numel()), (y, "y", BF16, out.numel()), (out, "out", BF16, out.numel()))
    call("uv_add_bf16", ptr(x), ptr(y), ptr(out), out.numel(), stream_ptr())
    return out


def t5_gated_gelu(gate, fc1, out):
    """out = fc1 * GELU(gate) with umT5's op-by-op bf16 roundings: contiguous bf16 tensors of out.numel() elements."""
    _check("t5_gated_gelu", (gate, "gate", BF16, out.numel()), (fc1, "fc1", BF16, out.numel()), (out, "out", BF16, out.numel()))
    call("uv_t5_gated_gelu_bf16", ptr(gate), ptr(fc1), ptr(out), out.numel(), stream_ptr())
    return out


def gelu_erf(x, out):
    """out = exact (erf) GELU of x: contiguous bf16 tensors of out.numel() elements (out may be x)."""
    _check("gelu_erf", (x, "x", BF16, out.numel()), (out, "out", BF16, out.numel()))
    call("uv_gelu_erf_bf16", ptr(x), ptr(out), out.numel(), stream_ptr())
    return out


def interp_linear_rows(x, out):
    """F.interpolate(mode='linear', align_corners=False) along the token axis: x bf16 [Lin, C] -> out bf16 [Lout, C]."""
    (Lin, C), Lout = x.shape, out.shape[0]
    _check("interp_linear_rows", (x, "x", BF16, C, Lin), (out, "out", BF16, C, Lout))
    call("uv_interp_linear_rows_bf16", ptr(x), x.stride(-2), ptr(out), out.stride(-2), Lin, Lout, C, stream_ptr())
    return out


# -- sampler: contiguous f32 latents of out.numel() elements; the older x0 (m_prev / m1) only for order 2 --
def cfg_convert(cond, uncond, sample, guide_scale, sigma, noise_pred, x0):
    """noise_pred (| None) = uncond + guide_scale * (cond - uncond); x0 = sample - sigma * noise_pred."""
    n = x0.numel()
    _check("cfg_convert", (cond, "cond", F32, n), (uncond, "uncond", F32, n), (sample, "sample", F32, n),
           (noise_pred, "noise_pred", F32, n, None, True), (x0, "x0", F32, n))
    call("uv_cfg_convert", ptr(cond), ptr(uncond), ptr(sample), float(guide_scale), float(sigma), ptr(noise_pred), ptr(x0), x0.numel(),
         stream_ptr())
    return x0


def unipc_corrector(x_last, m0, m_prev, model_t, out, r, c1, c2, rho0, rho_last, rk, order):
    """multistep_uni_c_bh_update with host-computed coefficients."""
    n = out.numel()
    _check("unipc_corrector", (x_last, "x_last", F32, n), (m0, "m0", F32, n), (m_prev, "m_prev", F32, n, None, order != 2),
           (model_t, "model_t", F32, n), (out, "out", F32, n))
    call("uv_unipc_corrector", ptr(x_last), ptr(m0), ptr(m_prev), ptr(model_t), ptr(out), r, c1, c2, rho0, rho_last, rk, order, n, stream_ptr())
    return out


def unipc_predictor(x, m0, m_prev, out, r, c1, c2, rk, order):
    """multistep_uni_p_bh_update with host-computed coefficients."""
    n = out.numel()
    _check("unipc_predictor", (x, "x", F32, n), (m0, "m0", F32, n), (m_prev, "m_prev", F32, n, None, order != 2), (out, "out", F32, n))
    call("uv_unipc_predictor", ptr(x), ptr(m0), ptr(m_prev), ptr(out), r, c1, c2, rk, order, out.numel(), stream_ptr())
    return out


def dpmpp_update(x, m0, m1, out, r, c, inv_r0, order):
    """DPM-Solver++ first-order / midpoint second-order update with host-computed coefficients."""
    n = out.numel()
    _check("dpmpp_update", (x, "x", F32, n), (m0, "m0", F32, n), (m1, "m1", F32, n, None, order != 2), (out, "out", F32, n))
    call("uv_dpmpp_update", ptr(x), ptr(m0), ptr(m1), ptr(out), r, c, inv_r0, order, out.numel(), stream_ptr())
    return out


# -- step cache: contiguous f32 buffers of n elements; ctl = [have, k, c1, c2] f32 in device memory; d1 / d2 only where order has them --
STEP_CACHE_GRID_ELEMS = 2048 * 256 * 4      # elements one pass of the largest grid covers (csrc/step_cache.hip: SC_MAX_BLOCKS x SC_THREADS x 4)


def _step_cache_args(fn, d0, d1, d2, ctl, n, order):
    if order not in (0, 1, 2):
        raise UnividHipError(f"{fn}: order must be 0, 1 or 2, got {order!r}")
    if n <= 0:
        raise UnividHipError(f"{fn}: n must be positive, got {n}")
    return ((d0, "d0", F32, n), (d1, "d1", F32, n, None, order < 1), (d2, "d2", F32, n, None, order < 2), (ctl, "ctl", F32, 4))


def step_cache_update(x_out, x_in, d0, d1, d2, ctl, order, n=None):
    """After the blocks of a computed step: r = x_out - x_in, the first / second backward differences over k steps where `have` and
    `order` allow them, then d0 = r, d1 = n1, d2 = n2 (include/univid_hip.h: uv_step_cache_update). Buffers beyond `order` are not
    touched (pass None)."""
    n = x_out.numel() if n is None else int(n)
    _check("step_cache_update", (x_out, "x_out", F32, n), (x_in, "x_in", F32, n), *_step_cache_args("step_cache_update", d0, d1, d2, ctl, n, order))
    call("uv_step_cache_update", ptr(x_out), ptr(x_in), ptr(d0), ptr(d1 if order >= 1 else None), ptr(d2 if order >= 2 else None), ptr(ctl), n,
         int(order), stream_ptr())
    return d0


def step_cache_apply(x, d0, d1, d2, ctl, order, n=None):
    """Instead of the blocks of a skipped step: x += d0 + d1 * c1 + d2 * c2, each term while `have` covers it (include/univid_hip.h:
    uv_step_cache_apply). Buffers beyond `order` are not touched (pass None)."""
    n = x.numel() if n is None else int(n)
    _check("step_cache_apply", (x, "x", F32, n), *_step_cache_args("step_cache_apply", d0, d1, d2, ctl, n, order))
    call("uv_step_cache_apply", ptr(x), ptr(d0), ptr(d1 if order >= 1 else None), ptr(d2 if order >= 2 else None), ptr(ctl), n, int(order),
         stream_ptr())
    return x


def rows_rel_l1(rows, out):
    """out[i] = sum|rows[i + 1] - rows[i]| / sum|rows[i]|: rows f32 [n_rows, K] contiguous, out f32 [n_rows - 1]; fp64 sums in a fixed order."""
    if rows.dim() != 2 or rows.shape[0] < 2 or rows.shape[1] < 1:
        raise UnividHipError(f"rows_rel_l1: at least two rows of at least one column are expected, got shape {tuple(rows.shape)}")
    n_rows, K = rows.shape
    _check("rows_rel_l1", (rows, "rows", F32, n_rows * K), (out, "out", F32, n_rows - 1))
    call("uv_rows_rel_l1", ptr(rows), ptr(out), n_rows, K, stream_ptr())
    return out


# -- VAE (f32, channels-last [T, H, W, C]: rows = pixels, leading dimension = stride(-2)) --
def split_weights_bf16x3(w, out):
    """w f32 [rows, K] -> out bf16, 2 w.numel() elements: hi | lo planes for uv_conv3d_bf16x3."""
    _check("split_weights_bf16x3", (w, "w", F32, w.numel()), (out, "out", BF16, 2 * w.numel()))
    call("uv_split_weights_bf16x3", ptr(w), ptr(out), w.numel(), stream_ptr())
    return out


def split_weights_bf16x6(w, out):
    """w f32 [rows, K] -> out bf16, 3 w.numel() elements: the exact three-way split for uv_conv3d_bf16x6."""
    _check("split_weights_bf16x6", (w, "w", F32, w.numel()), (out, "out", BF16, 3 * w.numel()))
    call("uv_split_weights_bf16x6", ptr(w), ptr(out), w.numel(), stream_ptr())
    return out


def split_weights_f16x3(w, out, scale):
    """w f32 [rows, K] -> out fp16, 2 w.numel() elements: hi | lo pieces of w * scale (a power of two) for uv_conv3d_f16x3."""
    _check("split_weights_f16x3", (w, "w", F32, w.numel()), (out, "out", F16, 2 * w.numel()))
    call("uv_split_weights_f16x3", ptr(w), ptr(out), w.numel(), float(scale), stream_ptr())
    return out


def cast_weights_f16(w, out, scale):
    """w f32 [rows, K] -> out fp16, w.numel() elements: fp16(w * scale) (scale a power of two), the weight matrix of uv_conv3d_f16."""
    _check("cast_weights_f16", (w, "w", F32, w.numel()), (out, "out", F16, w.numel()))
    call("uv_cast_weights_f16", ptr(w), ptr(out), w.numel(), float(scale), stream_ptr())
    return out


# conv3d's entry points: name, and the weight operand's (element dtype, elements per f32 weight)
_CONV = {"f32": ("uv_conv3d_f32", F32, 1), "bf16x6": ("uv_conv3d_bf16x6", BF16, 3), "bf16x3": ("uv_conv3d_bf16x3", BF16, 2),
         "f16x3": ("uv_conv3d_f16x3", F16, 2), "f16": ("uv_conv3d_f16", F16, 1)}


def conv3d(precision, src, weights, bias, out, Tin, Hin, Win, Tout, Hout, Wout, Cin, Cout, kt, kh, kw, st=1, sh=1, sw=1, t_off=0, ph=0, pw=0,
           up=0, interleave=0, resid=None, in_split=0, act_scale=None, flops=0):
    """One causal 3D / 2D convolution (include/univid_hip.h: uv_conv3d_*). The VAE's arithmetic `precision` ('fp32' | 'bf16x6' | 'f16x3' |
    'bf16x3' | 'f16') and `in_split`, the format of src (0 f32 rows, 1 bf16 pieces, 2 fp16 pieces, 3 plain fp16), select the entry: bf16x3
    throughout its mode; in f16x3 and f16 mode, f16x3 where src holds fp16 pieces and bf16x6 where it holds f32 rows; in f16 mode, the
    single-pass f16 entry where src holds plain fp16. weights(kind) -> (the weight operand of entry `kind`: the 'f32' [Cout, kt kh kw Cin]
    matrix, its 'bf16x6' | 'bf16x3' | 'f16x3' split or its 'f16' cast, the power-of-two scale of the two fp16 forms).
    src [Tin, Hin, Win, Cin] - plain fp16 (in_split 3): the f32-typed [Tin, Hin, Win, Cin / 2] tensor whose rows hold the Cin fp16 values;
    out / resid: the output pixels' rows with Cout channels (interleave: Cout / 2 and twice the frames;
    up >= 2: the [Tout, 2 Hout, 2 Wout] image of which this call writes one phase)."""
    if in_split == 3 and precision != "f16":
        raise UnividHipError(f"conv3d: plain fp16 rows (in_split 3) belong to precision 'f16', not {precision!r}")
    kind = "bf16x3" if precision == "bf16x3" else "f16" if in_split == 3 else "f16x3" if precision in ("f16x3", "f16") and in_split == 2 else \
        "bf16x6" if precision in ("bf16x6", "f16x3", "f16") else "f32"
    if kind == "f16" and Cin % 64:
        raise UnividHipError(f"conv3d: the single-pass f16 entry needs Cin % 64 == 0, got {Cin}")
    half = 2 if kind == "f16" else 1         # fp16 channels per f32-sized slot of src
    entry, wdtype, planes = _CONV[kind]
    w, w_scale = weights(kind)
    rows = Tout * Hout * Wout * (2 if interleave else 4 if up >= 2 else 1)
    cols = Cout // 2 if interleave else Cout
    _check("conv3d", (src, "src", F32, Cin // half, Tin * Hin * Win), (w, "weights", wdtype, planes * Cout * kt * kh * kw * Cin),
           (bias, "bias", F32, Cout), (out, "out", F32, cols, rows), (resid, "resid", F32, cols, rows, True),
           (act_scale, "act_scale", F32, 1, None, True))
    tail = (int(in_split == 1),) if kind == "bf16x3" else (w_scale, ptr(act_scale)) if kind in ("f16x3", "f16") else ()
    call(entry, ptr(src), src.stride(-2) * half, Tin, Hin, Win, ptr(w), ptr(bias), ptr(out), out.stride(-2), Tout, Hout, Wout, Cin, Cout, kt, kh, kw,
         st, sh, sw, t_off, ph, pw, up, interleave, ptr(resid), 0 if resid is None else resid.stride(-2), *tail, stream_ptr(), flops=flops)
    return out


def vae_rms_silu(x, gamma, out, silu=True, split=0):
    """RMS_norm (+ SiLU) per pixel: x f32 [..., C] -> out, the same bytes per pixel as f32 rows (split 0) or bf16 / fp16 pieces (1 / 2); split 3:
    plain fp16, the C values of a pixel in the first C / 2 f32-sized slots of its row (C % 64 == 0), so out may be [..., C / 2]."""
    P, C = x.numel() // x.shape[-1], x.shape[-1]
    if split == 3 and C % 64:
        raise UnividHipError(f"vae_rms_silu: plain fp16 output (split 3) needs C % 64 == 0, got {C}")
    _check("vae_rms_silu", (x, "x", F32, C, P), (gamma, "gamma", F32, C), (out, "out", F32, C // 2 if split == 3 else C, P))
    call("uv_vae_rms_silu", ptr(x), x.stride(-2), ptr(gamma), ptr(out), out.stride(-2), P, C, int(silu), int(split), stream_ptr())
    return out


def vae_split_f16(x, out, scale):
    """fp16 pieces of a raw feature map x f32 [..., C] under a device-found power-of-two scale; scale f32 [2] <- (1 / s, work space)."""
    P, C = x.numel() // x.shape[-1], x.shape[-1]
    _check("vae_split_f16", (x, "x", F32, C, P), (out, "out", F32, C, P), (scale, "scale", F32, 2))
    call("uv_vae_split_f16", ptr(x), x.stride(-2), ptr(out), out.stride(-2), P, C, ptr(scale), stream_ptr())
    return out


def vae_cast_f16(x, out, scale):
    """Plain fp16 of a raw feature map x f32 [..., C] (C % 64 == 0) under vae_split_f16's device-found power-of-two scale: out f32-typed
    [..., >= C / 2], the C fp16 values of a pixel at the start of its row; scale f32 [2] <- (1 / s, work space)."""
    P, C = x.numel() // x.shape[-1], x.shape[-1]
    if C % 64:
        raise UnividHipError(f"vae_cast_f16: C must be a multiple of 64, got {C}")
    _check("vae_cast_f16", (x, "x", F32, C, P), (out, "out", F32, C // 2, P), (scale, "scale", F32, 2))
    call("uv_vae_cast_f16", ptr(x), x.stride(-2), ptr(out), out.stride(-2), P, C, ptr(scale), stream_ptr())
    return out


def softmax_rows(x, R, n, scale):
    """In-place softmax of x[:R, :n] * scale, f32."""
    _check("softmax_rows", (x, "x", F32, n, R))
    call("uv_softmax_rows_f32", ptr(x), x.stride(-2), R, n, float(scale), stream_ptr())
    return x


def vae_dupup_add(x, out, ft, drop):
    """out [T * ft - drop, 2 H, 2 W, Cout] += DupUp3D(x [T, H, W, Cin]); contiguous f32."""
    (T, H, W, Cin), Cout = x.shape, out.shape[-1]
    _check("vae_dupup_add", (x, "x", F32, x.numel()), (out, "out", F32, (T * ft - drop) * 2 * H * 2 * W * Cout))
    call("uv_vae_dupup_add", ptr(x), ptr(out), T, H, W, Cin, Cout, ft, drop, stream_ptr())
    return out


def vae_avgdown_add(x, out, ft, fs):
    """out [ceil(T / ft), H / fs, W / fs, Cout] += AvgDown3D(x [T, H, W, Cin]); contiguous f32."""
    (T, H, W, Cin), Cout = x.shape, out.shape[-1]
    _check("vae_avgdown_add", (x, "x", F32, x.numel()), (out, "out", F32, (T + ft - 1) // ft * (H // fs) * (W // fs) * Cout))
    call("uv_vae_avgdown_add", ptr(x), ptr(out), T, H, W, Cin, Cout, ft, fs, stream_ptr())
    return out


def vae_latent_in(z, mean, inv_std, out):
    """z f32 [Z, f, h, w] (contiguous) -> out f32 [f, h, w, >= Z] rows of z / inv_std + mean; mean, inv_std f32 [Z]."""
    Z, P = z.shape[0], z.numel() // z.shape[0]
    _check("vae_latent_in", (z, "z", F32, Z * P), (mean, "mean", F32, Z), (inv_std, "inv_std", F32, Z), (out, "out", F32, Z, P))
    call("uv_vae_latent_in", ptr(z), ptr(mean), ptr(inv_std), ptr(out), out.stride(-2), Z, P, stream_ptr())
    return out


def vae_latent_out(mu, mean, inv_std, out, Z):
    """The first Z channels of the rows mu f32 [f, h, w, >= Z] -> out f32 [Z, f, h, w] (contiguous) of (mu - mean) * inv_std."""
    P = mu.numel() // mu.shape[-1]
    _check("vae_latent_out", (mu, "mu", F32, Z, P), (mean, "mean", F32, Z), (inv_std, "inv_std", F32, Z), (out, "out", F32, Z * P))
    call("uv_vae_latent_out", ptr(mu), mu.stride(-2), ptr(mean), ptr(inv_std), ptr(out), Z, P, stream_ptr())
    return out


def vae_video_in(vid, out, f0, T):
    """Frames [f0, f0 + T) of vid f32 [3, F, H, W] (contiguous) -> the 12 patchified channels of out f32 [T, H / 2, W / 2, >= 12]."""
    _, F, H, W = vid.shape
    _check("vae_video_in", (vid, "vid", F32, 3 * F * H * W), (out, "out", F32, 12, T * (H // 2) * (W // 2)))
    call("uv_vae_video_in", ptr(vid), ptr(out), out.stride(-2), F, H, W, f0, T, stream_ptr())
    return out


def vae_video_out(y, vid, f0, T):
    """The 12 channels of y f32 [T, Hp, Wp, >= 12] -> frames [f0, f0 + T) of vid f32 [3, F, 2 Hp, 2 Wp] (contiguous), clamped to [-1, 1]."""
    F, H, W = vid.shape[-3:]
    _check("vae_video_out", (y, "y", F32, 12, T * (H // 2) * (W // 2)), (vid, "vid", F32, 3 * F * H * W))
    call("uv_vae_video_out", ptr(y), y.stride(-2), ptr(vid), F, H // 2, W // 2, f0, T, stream_ptr())
    return vid
