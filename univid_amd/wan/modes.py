"""The DiT's opt-in forward settings (ffn_precision, proj_precision, attn_precision, attn_window, attn_block_mask) in one place: which
combinations are legal (`validate_modes`, the ONLY guard: a new mode is added there and to its table), which nn.Linears the MXFP8 GEMM
modes cover (`mx_covered`), the resolvers a mask spec normalises to, and the pipelines' rule (`apply_requested`). The state itself is
written by WanAttentionBlock._apply_modes / WanModel._apply_modes (model.py) only."""
import collections
import math

import torch

from .. import _lib
from .attention import TopKBlockMask

FFN_PRECISIONS = ("bf16", "mxfp8")
PROJ_PRECISIONS = ("bf16", "mxfp8")
ATTN_PRECISIONS = ("bf16", "mxfp8_qk", "mxfp8_qk_pv")

# every setting with its default, in the order the pipelines apply them (WanModel.set_<name> each)
MODE_DEFAULTS = dict(ffn_precision="bf16", attn_precision="bf16", attn_window=None, attn_block_mask=None, proj_precision="bf16")


class _MaskResolver:
    """What the two resolvers of a mask spec share: the spec, the model's head count, and the cache of what `resolve` made."""

    def __init__(self, spec, num_heads):
        self.spec, self.num_heads, self._cache = spec, int(num_heads), {}

    def prepared(self):
        """{(grid or L, device): what `resolve` returned} so far (tools report the densities)."""
        return dict(self._cache)

    def prepare(self, grid, device):
        return self.resolve(tuple(int(g) for g in grid), math.prod(int(g) for g in grid), torch.device(device))


class AttnBlockMask(_MaskResolver):
    """set_attn_block_mask's spec as the self-attention launches resolve it: the PreparedBlockMask of a forward's patch grid. spec: a
    PreparedBlockMask or a bool tensor (one fixed L: a forward at another L raises), or a callable f(F, H, W, num_heads) -> bool mask
    [ceil(L / 128), ceil(L / 64)] or [num_heads, ...] with L = F H W, evaluated and prepared ONCE per distinct (grid, device) and cached.
    Preparing builds lists on the CPU and uploads them, which a HIP-graph capture cannot hold: a forward inside a capture whose grid was
    not prepared raises (WanTI2V's eager warm-up forward prepares it before it captures; `prepare(grid, device)` does so by hand)."""

    def resolve(self, grid, L, device):
        spec = self.spec
        if isinstance(spec, _lib.PreparedBlockMask):
            if spec.L != L:
                raise ValueError(f"attn_block_mask was prepared for L = {spec.L}; this forward has L = {L} (patch grid {tuple(grid)})")
            if spec.device != device:
                raise ValueError(f"attn_block_mask lives on {spec.device}; this forward runs on {device}")
            return spec
        key = (L, device) if torch.is_tensor(spec) else (tuple(grid), device)
        bm = self._cache.get(key)
        if bm is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"attn_block_mask: patch grid {tuple(grid)} (L = {L}) was not prepared before this HIP-graph capture - "
                                   f"run one eager forward at this grid, or AttnBlockMask.prepare(grid, device), first")
            mask = spec if torch.is_tensor(spec) else spec(int(grid[0]), int(grid[1]), int(grid[2]), self.num_heads)
            bm = _lib.prepare_block_mask(mask, L, device)      # (a tensor of another L's shape is refused here, naming the shape)
            if bm.heads not in (1, self.num_heads):
                raise ValueError(f"attn_block_mask: a per-head mask needs {self.num_heads} heads, got {bm.heads}")
            self._cache[key] = bm
        return bm


class AttnTopKMask(_MaskResolver):
    """set_attn_block_mask's resolver of a TopKBlockMask (univid_amd.wan.attention): per patch grid the count of non-kept tiles a query
    block lists and the static keep mask on the device. keep's tensor / callable forms resolve and cache exactly as AttnBlockMask's specs
    do - a tensor belongs to one L, a callable is evaluated once per distinct (grid, device), and uploading inside a HIP-graph capture is
    refused (WanTI2V's eager warm-up forward prepares it; `prepare(grid, device)` does so by hand). Without a keep mask nothing is
    uploaded and every grid resolves anywhere. The lists themselves are built on the device in every forward."""

    # one grid's resolved spec: top_k (int), keep (uint8 [1 or H, nqb, nkb] on the device, or None), mask (the expanded bool keep mask on
    # the CPU, or None), L
    Plan = collections.namedtuple("Plan", "top_k keep mask L")

    def resolve(self, grid, L, device):
        spec = self.spec
        key = (tuple(grid), device) if callable(spec.keep) else (L, device)
        plan = self._cache.get(key)
        if plan is None:
            nkb = -(-L // _lib.BS_K_BLOCK)
            if nkb > _lib.BS_SELECT_MAX_TILES:
                raise NotImplementedError(f"attn_block_mask: L = {L} has {nkb} key tiles; the top-k selection kernel sorts at most "
                                          f"{_lib.BS_SELECT_MAX_TILES} (L <= {_lib.BS_SELECT_MAX_TILES * _lib.BS_K_BLOCK})")
            keep = mask = None
            if spec.keep is not None:
                if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(f"attn_block_mask: the keep mask of patch grid {tuple(grid)} (L = {L}) was not prepared before this "
                                       f"HIP-graph capture - run one eager forward at this grid, or AttnTopKMask.prepare(grid, device), first")
                m = spec.keep if torch.is_tensor(spec.keep) else spec.keep(int(grid[0]), int(grid[1]), int(grid[2]), self.num_heads)
                keep, mask = _lib.prepare_keep_mask(m, L, device, spec.q_block, spec.k_block)
                if mask.shape[0] not in (1, self.num_heads):
                    raise ValueError(f"attn_block_mask: a per-head keep mask needs {self.num_heads} heads, got {mask.shape[0]}")
            plan = self._cache[key] = AttnTopKMask.Plan(spec.count(L), keep, mask, L)
        return plan


def mx_covered(owner):
    """{mode: the nn.Linears of `owner` that the mode's "mxfp8" puts on uv_gemm_mxfp8_nt} - the one statement of it. owner: a
    WanAttentionBlock (ffn_precision: ffn.0 / ffn.2) or an attention module (proj_precision: its `_mx_proj`). The MXFP8 GEMM has no
    adapter slot, so the mode and an un-merged LoRA adapter on a covered Linear refuse each other: validate_modes when the mode is set,
    univid_amd.lora when the adapter is attached."""
    covered = {}
    if hasattr(owner, "ffn"):
        covered["ffn_precision"] = [owner.ffn[0], owner.ffn[2]]
    if hasattr(owner, "_mx_proj"):
        covered["proj_precision"] = [getattr(owner, n) for n in owner._mx_proj]
    return covered


# The table; a call's refusals come in the order form, geometry, conflicts. ffn_precision and proj_precision are
# independent of each other and of the three attention settings.
#   setting          values                             refused when                                                                   error
#   ffn_precision    "bf16", "mxfp8"                    "mxfp8" with dim % 256 or ffn_dim % 256                                        ValueError
#                                                       "mxfp8" with an un-merged adapter on ffn.0 / ffn.2                             NotImplementedError
#   proj_precision   "bf16", "mxfp8"                    "mxfp8" with dim % 256                                                         ValueError
#                                                       "mxfp8" with an un-merged adapter on a projection in an attention's _mx_proj   NotImplementedError
#   attn_precision   "bf16", "mxfp8_qk", "mxfp8_qk_pv"  non-bf16 with head_dim other than 128                                          ValueError
#                                                       non-bf16 with a window or a mask                                               NotImplementedError
#   attn_window      (left, right), None, (-1, -1)      malformed                                                                      ValueError
#                                                       non-global with head_dim != 128, attn_precision != "bf16", or beside a mask    NotImplementedError
#   attn_block_mask  see WanModel.set_attn_block_mask   wrong type                                                                     TypeError
#                                                       wrong head count                                                               ValueError
#                                                       non-None with head_dim != 128, attn_precision != "bf16", or beside a window    NotImplementedError
def validate_modes(cand, *, dim, head_dim, num_heads, ffn_dim=0, block=None, attns=()):
    """The guard of every setter and constructor: raises, or returns the complete candidate normalised - the window as (left, right), each
    >= 0 or -1 = unbounded (flash-attn's window_size), or None for global attention (None or (-1, -1)); the mask spec as the AttnBlockMask
    / AttnTopKMask that resolves it (a resolver passed as a spec is reused, with its cache) or None. cand: {setting: value}, a missing one
    is at its default. The rest is one block's geometry and, for the un-merged adapter test over mx_covered, the block and its attentions."""
    c = {**MODE_DEFAULTS, **cand}
    ffn, proj, attn, window, spec = c["ffn_precision"], c["proj_precision"], c["attn_precision"], c["attn_window"], c["attn_block_mask"]
    if ffn not in FFN_PRECISIONS:
        raise ValueError(f"ffn_precision {ffn!r}: one of {FFN_PRECISIONS}")
    if ffn == "mxfp8":
        if dim % 256 or ffn_dim % 256:
            raise ValueError(f"ffn_precision 'mxfp8' needs dim and ffn_dim to be multiples of 256 (dim {dim}, ffn_dim {ffn_dim}): "
                             "uv_gemm_mxfp8_nt takes N % 256 == 0 and K % 128 == 0")
        if block is not None and any(getattr(lin, "_uv_lora", None) for lin in mx_covered(block)["ffn_precision"]):
            raise NotImplementedError(
                "ffn_precision 'mxfp8' and an un-merged LoRA adapter (merge=False) on ffn.0 / ffn.2 cannot be combined: the MXFP8 GEMM has no "
                "adapter slot. Detach the adapter or merge it (merge=True: the merged weights are re-quantised), or keep ffn_precision 'bf16'. "
                "Un-merged adapters on the attention projections work in both modes.")
    if proj not in PROJ_PRECISIONS:
        raise ValueError(f"proj_precision {proj!r}: one of {PROJ_PRECISIONS}")
    if proj == "mxfp8":
        if dim % 256:
            raise ValueError(f"proj_precision 'mxfp8' needs dim to be a multiple of 256 (dim {dim}): uv_gemm_mxfp8_nt takes N % 256 == 0 and "
                             "K % 128 == 0, uv_layernorm_mod_mx C % 256 == 0")
        if any(getattr(lin, "_uv_lora", None) for a in attns for lin in mx_covered(a)["proj_precision"]):
            raise NotImplementedError(
                "proj_precision 'mxfp8' and an un-merged LoRA adapter (merge=False) on self_attn.q / k / v / o or cross_attn.q / o cannot be "
                "combined: the MXFP8 GEMM has no adapter slot. Detach the adapter or merge it (merge=True: the merged weights are "
                "re-quantised), or keep proj_precision 'bf16'. Un-merged adapters on cross_attn.k / v work in both modes.")
    if attn not in ATTN_PRECISIONS:
        raise ValueError(f"attn_precision {attn!r}: one of {ATTN_PRECISIONS}")
    if attn != "bf16" and head_dim != 128:
        raise ValueError(f"attn_precision {attn!r} needs head_dim 128 (one MX scale dword per head and row, two 64-element steps of the "
                         f"block-scaled matrix instruction); this model has head_dim {head_dim}")
    if window is not None:
        try:
            ok = len(window) == 2 and all(int(w) == w and not isinstance(w, bool) for w in window)
        except (TypeError, ValueError):
            ok = False
        if not ok or min(int(w) for w in window) < -1:
            raise ValueError(f"window_size {window!r}: (left, right), two integers, each >= 0 or -1 for unbounded")
        window = (int(window[0]), int(window[1]))
        if window == (-1, -1):
            window = None
        elif head_dim != 128:
            raise NotImplementedError(f"window_size {window}: the windowed attention kernels are built for head_dim 128 (this model has {head_dim})")
    resolver = None
    if spec is not None:
        if isinstance(spec, (AttnBlockMask, AttnTopKMask)):
            resolver, spec = spec, spec.spec
        topk = isinstance(spec, TopKBlockMask)
        if topk:
            heads = spec.keep.shape[0] if torch.is_tensor(spec.keep) and spec.keep.dim() == 3 else 1
        elif torch.is_tensor(spec):
            if spec.dtype != torch.bool or spec.dim() not in (2, 3):
                raise TypeError(f"attn_block_mask: a tensor spec must be torch.bool [nqb, nkb] or [num_heads, nqb, nkb], got {spec.dtype} "
                                f"{tuple(spec.shape)}")
            heads = spec.shape[0] if spec.dim() == 3 else 1
        elif isinstance(spec, _lib.PreparedBlockMask):
            heads = spec.heads
        elif callable(spec):
            heads = 1
        else:
            raise TypeError(f"attn_block_mask: None, a bool tensor, a PreparedBlockMask or a callable f(F, H, W, num_heads), got {type(spec).__name__}")
        if heads not in (1, num_heads):
            raise ValueError(f"attn_block_mask: a per-head mask needs {num_heads} heads (or one mask for all), got {heads}")
        if head_dim != 128:
            raise NotImplementedError(f"attn_block_mask: the block-sparse attention kernel is built for head_dim 128 (this model has {head_dim})")
    # the three attention settings against each other: an MXFP8 mode, a window and a mask are one at a time
    if window is not None and attn != "bf16":
        raise NotImplementedError(f"window_size {window} with attn_precision {attn!r}: the windowed attention kernels are bf16 only "
                                  f"- set_attn_precision('bf16') or set_attn_window(None) first")
    if spec is not None and attn != "bf16":
        raise NotImplementedError(f"attn_block_mask with attn_precision {attn!r}: the block-sparse attention kernel is bf16 only "
                                  f"- set_attn_precision('bf16') or set_attn_block_mask(None) first")
    if spec is not None and window is not None:
        raise NotImplementedError(f"attn_block_mask with window_size {window}: one or the other - set_attn_window(None) first, "
                                  f"or fold the window into the mask")
    if spec is not None and resolver is None:
        resolver = (AttnTopKMask if topk else AttnBlockMask)(spec, num_heads)
    return dict(ffn_precision=ffn, attn_precision=attn, attn_window=window, attn_block_mask=resolver, proj_precision=proj)


def apply_requested(model, asked, injected=False):
    """The pipelines' rule (WanTI2V, CrossAttentionFusionPipeline): of `asked` = {setting: value}, what was asked for and differs from
    the model's mode goes through the model's named setter - one setting at a time in MODE_DEFAULTS' order, so each meets the guards
    under what was applied before it. None keeps the mode the model came with (its checkpoint's config.json for the window; the defaults
    unless it was switched); a mask that is not None is always set. injected: the model arrived inside a pipeline built elsewhere - it
    also keeps its mode where `asked` holds the default, and a DiT object without the setters is left alone."""
    for name, default in MODE_DEFAULTS.items():
        value = asked.get(name)
        if value is None or (injected and ((default is not None and value == default) or not hasattr(model, "set_" + name))):
            continue
        if name == "attn_window":
            differs = tuple(value) != tuple(model.window_size)
        else:
            differs = name == "attn_block_mask" or value != getattr(model, name)
        if differs:
            getattr(model, "set_" + name)(value)
