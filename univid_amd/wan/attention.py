"""`flash_attention` / `attention`: the reference's attention operator seam on the MI355X kernels.

Mirrors /root/reference/models/wan/utils/modules/attention.py (flash_attention :24-130, attention :133-179): the same
signature, argument meaning and result dtype, so its callers (model.py:145-150 self-attention with `k_lens=seq_lens`,
model.py:175 cross-attention, distributed/ulysses.py:37) can import this module instead of the flash-attn wheel:

    q [B, Lq, N, C], k [B, Lk, N, C], v [B, Lk, N, C] in any float dtype -> [B, Lq, N, C] in q's dtype;
    operands that are not fp16/bf16 are cast to `dtype` first (:59-83); sample b attends keys [0, k_lens[b]).

The core is `uv_flash_attn_bf16` / `uv_flash_attn_f16` (csrc/attention.hip) and, under `causal` / `window_size`,
`uv_flash_attn_win_bf16` (csrc/attention_win.hip); this file only arranges memory for it: casts
(`uv_cast_f32_to16`), the V^T operand (`uv_transpose_16`, zero-filled to the 64-key tile), the widening of the result
(`uv_cast_16_to_f32`). The fused DiT path (`univid_amd/wan/model.py`) does not come through here - there V^T is written by
the V projection's GEMM epilogue - so this is the path for code that calls the operator directly.

`causal` / `window_size=(left, right)` (attention.py:113-127, flash-attn's meaning: query i attends keys max(0, i - left) ..
min(Lk - 1, i + right), -1 = unbounded, causal forces right = 0) are built for SELF-attention as `WanModel.forward` runs it:
Lq == Lk, every sample attending all Lk keys (`k_lens` None or all Lk), head size 128, bf16 operands after the cast. Bottom-right
alignment for Lq != Lk, ragged `k_lens`, fp16 tensors and head size 64 under a window raise NotImplementedError naming the limit.

`block_mask=` (a trailing keyword of this port; the reference signature is unchanged without it) runs block-sparse SELF-attention
(`uv_flash_attn_bs_bf16`, csrc/attention_bs.hip): a `_lib.PreparedBlockMask` or a bool tensor [ceil(L / 128), ceil(L / 64)] / [N, ...]
(prepared per call), query i of head h attending key j iff mask[h][i // 128][j // 64]. The window's restrictions apply, each refused with
a message naming the limit: Lq == Lk, full `k_lens`, head size 128, bf16, and not beside `causal` / `window_size`. `video_block_mask`
builds such a mask from a 3-D (frame, row, column) neighbourhood. A `TopKBlockMask(top_k, keep=None)` in its place makes the lists
DATA-DEPENDENT: per call, sample, head and 128-query block the `top_k` key tiles with the highest pooled q.k scores, beside the static
`keep` tiles, are chosen on the device (`uv_attn_pool_qk`, `uv_attn_bs_select`, `uv_flash_attn_bs_lists_bf16`; csrc/attention_sel.hip) -
the same restrictions, no host synchronisation.

What the reference function accepts but UniVid never uses is rejected loudly instead of being computed wrongly:
dropout, `q_scale`, grouped K/V heads, head sizes other than 64 / 128, and `q_lens` that
differ from Lq (the reference itself cannot return those: its `.unflatten(0, (b, lq))` needs every q_len == Lq).
There is no eager fallback: without the HIP extension or a gfx950 device the call raises.
"""
import math

import torch

from .. import _lib

__all__ = ["flash_attention", "attention", "video_block_mask", "TopKBlockMask"]

_HALF = (torch.float16, torch.bfloat16)


def _half(x, dtype):
    """attention.py:59-60: keep fp16 / bf16 tensors, cast everything else to `dtype` (round to nearest even)."""
    if x.dtype in _HALF:
        return x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    if x.numel():
        _lib.cast_f32_to16(x, out)
    return out


def _lens(lens, b, full, name):
    if lens is None:
        return [full] * b
    vals = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(vals) != b or min(vals) < 1 or max(vals) > full:
        raise ValueError(f"flash_attention: {name} must hold {b} lengths in [1, {full}], got {vals}")
    return vals


class TopKBlockMask:
    """The spec of DATA-DEPENDENT block-sparse self-attention (the top-k tile selection of the training-free sparse-attention schemes for
    video DiTs), accepted wherever a block mask is: per forward, sample, head and 128-query block i, the key tiles attended are the ones
    `keep` marks plus the `top_k` best of the others by the pooled score s[i][j] = mean(q rows of block i) . mean(k rows of tile j) (fp32; q
    and k after RMSNorm + RoPE; ties go to the lower tile index); fewer than `top_k` candidates: all of them. Chosen on the device, so it
    runs inside a captured HIP graph and differs between the samples of a stacked forward.

    top_k: an int >= 1, or a float in (0, 1] = that fraction of the sequence's ceil(L / 64) key tiles, rounded up. keep: None, a bool
    tensor [ceil(L / q_block), ceil(L / k_block)] or [num_heads, ...] for ONE sequence length, or a callable f(F, H, W, num_heads) -> such
    a mask for the patch grid (`video_block_mask` builds one); rows may be empty. Immutable."""
    __slots__ = ("top_k", "keep", "q_block", "k_block")

    def __init__(self, top_k, keep=None, *, q_block=128, k_block=64):
        if isinstance(top_k, bool) or not isinstance(top_k, (int, float)):
            raise TypeError(f"TopKBlockMask: top_k must be an int >= 1 or a float in (0, 1], got {type(top_k).__name__}")
        if isinstance(top_k, int) and top_k < 1:
            raise ValueError(f"TopKBlockMask: top_k = {top_k} must be >= 1")
        if isinstance(top_k, float) and not 0.0 < top_k <= 1.0:
            raise ValueError(f"TopKBlockMask: a float top_k is a fraction of the key tiles in (0, 1], got {top_k}")
        if torch.is_tensor(keep):
            if keep.dtype != torch.bool or keep.dim() not in (2, 3):
                raise TypeError(f"TopKBlockMask: a tensor keep must be torch.bool [nqb, nkb] or [num_heads, nqb, nkb], got {keep.dtype} "
                                f"{tuple(keep.shape)}")
        elif keep is not None and not callable(keep):
            raise TypeError(f"TopKBlockMask: keep must be None, a bool tensor or a callable f(F, H, W, num_heads), got {type(keep).__name__}")
        q_block, k_block = int(q_block), int(k_block)
        if q_block <= 0 or q_block % _lib.BS_Q_BLOCK or k_block <= 0 or k_block % _lib.BS_K_BLOCK:
            raise ValueError(f"TopKBlockMask: q_block {q_block} must be a multiple of {_lib.BS_Q_BLOCK} and k_block {k_block} a multiple of "
                             f"{_lib.BS_K_BLOCK}")
        for name, v in (("top_k", top_k), ("keep", keep), ("q_block", q_block), ("k_block", k_block)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TopKBlockMask is immutable: build a new spec")

    def __delattr__(self, name):
        raise AttributeError("TopKBlockMask is immutable: build a new spec")

    def count(self, L):
        """The number of non-kept tiles listed per query block at sequence length L (before the cap at the candidates a row has)."""
        nkb = -(-int(L) // _lib.BS_K_BLOCK)
        if isinstance(self.top_k, int):
            return self.top_k
        return max(1, min(nkb, math.ceil(self.top_k * nkb)))

    def __repr__(self):
        keep = "None" if self.keep is None else (f"tensor{tuple(self.keep.shape)}" if torch.is_tensor(self.keep) else "callable")
        return f"TopKBlockMask(top_k={self.top_k!r}, keep={keep})"


def topk_attention(q, k, vt, out, L, H, D, scale, top_k, keep, batch, scratch=None):
    """The three launches of self-attention under a TopKBlockMask on q / k as the attention kernel reads them (bf16 [batch*L, H*D]): pool,
    select, attend. top_k: the resolved count; keep: uint8 [1 or H, nqb, nkb] on the device or None. scratch(tag, shape, dtype) supplies
    qbar / kbar / the lists (the model: stable per-stream buffers, so a captured graph allocates nothing); default: fresh tensors."""
    nqb, nkb = -(-L // _lib.BS_Q_BLOCK), -(-L // _lib.BS_K_BLOCK)
    if nkb > _lib.BS_SELECT_MAX_TILES:
        raise NotImplementedError(f"TopKBlockMask: L = {L} has {nkb} key tiles; the selection kernel sorts at most {_lib.BS_SELECT_MAX_TILES} "
                                  f"(L <= {_lib.BS_SELECT_MAX_TILES * _lib.BS_K_BLOCK})")
    if scratch is None:
        def scratch(tag, shape, dtype):
            return torch.empty(shape, dtype=dtype, device=q.device)
    qbar = scratch("topk_qbar", (batch, H, nqb, D), torch.float32)
    kbar = scratch("topk_kbar", (batch, H, nkb, D), torch.float32)
    idx = scratch("topk_idx", (batch, H, nqb, nkb), torch.int32)
    cnt = scratch("topk_cnt", (batch, H, nqb), torch.int32)
    _lib.attn_pool_qk(q, k, qbar, kbar, L, H, D, batch=batch)
    _lib.attn_bs_select(qbar, kbar, keep, top_k, idx, cnt, L, H, batch=batch)
    _lib.flash_attn_bs_lists(q, k, vt, out, L, H, D, scale, idx, cnt, H, batch, batch=batch)
    return idx, cnt


def flash_attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
                    window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, version=None, *, block_mask=None):
    """Reference signature (attention.py:24-38). `deterministic` and `version` select nothing here: the kernel is always
    deterministic (no atomics, fixed reduction order) and there is one implementation. `block_mask`: see the module's docstring."""
    assert dtype in _HALF
    if q.device.type != "cuda":
        raise _lib.UnividHipError(f"flash_attention: tensors must live on the GPU (got {q.device}); univid_amd has no CPU path")
    try:
        window = tuple(int(w) for w in window_size)
    except (TypeError, ValueError):
        window = ()
    if len(window) != 2 or min(window) < -1:
        raise ValueError(f"flash_attention: window_size {window_size!r} must be (left, right), each >= 0 or -1 for unbounded")
    if causal:
        window = (window[0], 0)      # flash-attn: causal forces right = 0, whatever window_size[1] says
    windowed = window != (-1, -1)
    masked = block_mask is not None
    if masked and windowed:
        raise NotImplementedError("flash_attention: block_mask combined with causal / window_size is not built: fold the window into the mask")
    topk = isinstance(block_mask, TopKBlockMask)
    if topk and callable(block_mask.keep):
        raise TypeError("flash_attention: a TopKBlockMask whose keep is a callable needs a patch grid, which this call does not carry: pass "
                        "keep as a bool tensor (video_block_mask builds it)")
    if masked and not topk and not isinstance(block_mask, _lib.PreparedBlockMask) and not (torch.is_tensor(block_mask) and block_mask.dtype == torch.bool):
        raise TypeError(f"flash_attention: block_mask must be a PreparedBlockMask or a torch.bool tensor, got "
                        f"{block_mask.dtype if torch.is_tensor(block_mask) else type(block_mask).__name__}")
    if dropout_p:
        raise NotImplementedError("flash_attention: dropout_p > 0 is a training option; the inference kernels have no dropout")
    if q_scale is not None:
        raise NotImplementedError("flash_attention: q_scale is never passed on UniVid's path; fold it into softmax_scale")
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("flash_attention: q, k, v must be [B, L, N, C]")
    b, lq, n, c = q.shape
    lk = k.size(1)
    if k.shape != (b, lk, n, c) or v.shape != (b, lk, n, c):
        raise NotImplementedError(f"flash_attention: k / v must be [B, Lk, {n}, {c}] like q's heads (grouped K/V heads and "
                                  f"C2 != C1 are not built); got k {tuple(k.shape)}, v {tuple(v.shape)}")
    if c not in (64, 128):
        raise NotImplementedError(f"flash_attention: head size {c} (the kernels are built for 64 and 128)")
    if windowed and c != 128:
        raise NotImplementedError(f"flash_attention: causal / window_size with head size {c} is not built (the windowed kernels are head size 128)")
    if windowed and lq != lk:
        raise NotImplementedError(f"flash_attention: causal / window_size with Lq != Lk ({lq} vs {lk}: flash-attn's bottom-right alignment) "
                                  f"is not built, self-attention only")
    if masked and c != 128:
        raise NotImplementedError(f"flash_attention: block_mask with head size {c} is not built (the block-sparse kernel is head size 128)")
    if masked and lq != lk:
        raise NotImplementedError(f"flash_attention: block_mask with Lq != Lk ({lq} vs {lk}) is not built, self-attention only")
    out_dtype = q.dtype
    if any(ql != lq for ql in _lens(q_lens, b, lq, "q_lens")):
        raise ValueError("flash_attention: q_lens other than Lq cannot be returned as [B, Lq, N, C] (attention.py:107,127)")
    kls = _lens(k_lens, b, lk, "k_lens")

    qh, kh, vh = _half(q, dtype), _half(k, dtype), _half(v, dtype)
    if not (qh.dtype == kh.dtype == vh.dtype):          # attention.py:82-83 casts q and k to v's dtype
        raise NotImplementedError("flash_attention: q, k, v of different half dtypes; pass one dtype")
    if windowed and any(kl != lk for kl in kls):
        raise NotImplementedError(f"flash_attention: causal / window_size with ragged k_lens {kls} (Lk = {lk}) is not built: strip the padding "
                                  f"first, as WanModel.forward does")
    if windowed and vh.dtype != torch.bfloat16:
        raise NotImplementedError("flash_attention: causal / window_size with fp16 tensors is not built (the windowed kernels are bf16)")
    if masked and any(kl != lk for kl in kls):
        raise NotImplementedError(f"flash_attention: block_mask with ragged k_lens {kls} (Lk = {lk}) is not built: strip the padding first, "
                                  f"as WanModel.forward does")
    if masked and vh.dtype != torch.bfloat16:
        raise NotImplementedError("flash_attention: block_mask with fp16 tensors is not built (the block-sparse kernel is bf16)")
    if topk:
        keep = None
        if block_mask.keep is not None:
            keep, keep_mask = _lib.prepare_keep_mask(block_mask.keep, lk, q.device, block_mask.q_block, block_mask.k_block)
            if keep_mask.shape[0] not in (1, n):
                raise ValueError(f"flash_attention: the TopKBlockMask's keep has {keep_mask.shape[0]} heads; this call has {n} (1 = shared "
                                 f"by all heads)")
        top_k = block_mask.count(lk)
    elif masked:
        bm = block_mask if isinstance(block_mask, _lib.PreparedBlockMask) else _lib.prepare_block_mask(block_mask, lk, q.device)
        if bm.L != lk or bm.heads not in (1, n):
            raise ValueError(f"flash_attention: block_mask was prepared for L = {bm.L} and {bm.heads} head(s); this call has L = {lk} and "
                             f"{n} heads (1 = shared by all heads)")
    C = n * c
    dev = q.device
    scale = float(softmax_scale) if softmax_scale is not None else c ** -0.5
    out = torch.empty(b, lq, C, dtype=vh.dtype, device=dev)
    q2, k2, v2 = qh.view(b * lq, C), kh.view(b * lk, C), vh.view(b * lk, C)

    def vt_of(rows, L, vt, col0):
        """vt[:, col0 : col0 + roundup(L, 64)] = rows[:L]^T, zero beyond L."""
        _lib.transpose_16(rows, vt[:, col0:], L, C, _lib.vt_cols(1, L))

    if len(set(kls)) == 1 and kls[0] == lk and (b == 1 or lk % 8 == 0):
        # every sample attends all Lk keys: ONE launch over the stacked samples (sample s = V^T columns [s*Lk, (s+1)*Lk))
        vt = torch.empty(C, _lib.vt_cols(b, lk), dtype=vh.dtype, device=dev)
        for s in range(b):      # later samples overwrite the previous sample's zero padding, the last one keeps it
            vt_of(v2[s * lk:(s + 1) * lk], lk, vt, s * lk)
        if windowed:
            _lib.flash_attn_win(q2, k2, vt, out.view(b * lq, C), lq, n, c, scale, window, batch=b)
        elif topk:
            topk_attention(q2, k2, vt, out.view(b * lq, C), lq, n, c, scale, top_k, keep, b)
        elif masked:
            _lib.flash_attn_bs(q2, k2, vt, out.view(b * lq, C), lq, n, c, scale, bm, batch=b)
        else:
            _lib.flash_attn(q2, k2, vt, out.view(b * lq, C), lq, lk, n, c, scale, batch=b)
    else:
        for s in range(b):      # ragged key lengths: one launch per sample on its first k_lens[s] keys
            L = kls[s]
            vt = torch.empty(C, _lib.vt_cols(1, L), dtype=vh.dtype, device=dev)
            vt_of(v2[s * lk:s * lk + L], L, vt, 0)
            if windowed:        # (every k_len == Lk here: Lk % 8 != 0 at batch > 1)
                _lib.flash_attn_win(q2[s * lq:(s + 1) * lq], k2[s * lk:s * lk + L], vt, out[s], lq, n, c, scale, window)
            elif topk:
                topk_attention(q2[s * lq:(s + 1) * lq], k2[s * lk:s * lk + L], vt, out[s], lq, n, c, scale, top_k, keep, 1)
            elif masked:
                _lib.flash_attn_bs(q2[s * lq:(s + 1) * lq], k2[s * lk:s * lk + L], vt, out[s], lq, n, c, scale, bm)
            else:
                _lib.flash_attn(q2[s * lq:(s + 1) * lq], k2[s * lk:s * lk + L], vt, out[s], lq, L, n, c, scale)
    out = out.view(b, lq, n, c)
    if out_dtype == out.dtype:
        return out
    if out_dtype == torch.float32:                                            # attention.py:130
        wide = torch.empty(b, lq, n, c, dtype=torch.float32, device=dev)
        return _lib.cast_16_to_f32(out, wide)
    return out.type(out_dtype)   # fp64 / other-half callers: a dtype view change of the finished result, no arithmetic


def attention(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
              window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, fa_version=None, *, block_mask=None):
    """attention.py:133-179. The reference falls back to `scaled_dot_product_attention` WITHOUT the padding mask when no
    flash-attn wheel is installed; here the kernel is always present, so this is `flash_attention` (mask included)."""
    return flash_attention(q=q, k=k, v=v, q_lens=q_lens, k_lens=k_lens, dropout_p=dropout_p, softmax_scale=softmax_scale,
                           q_scale=q_scale, causal=causal, window_size=window_size, deterministic=deterministic, dtype=dtype,
                           version=fa_version, block_mask=block_mask)


def video_block_mask(grid, frames=(-1, -1), rows=-1, cols=-1, num_heads=None, q_block=128, k_block=64):
    """A block mask [ceil(L / q_block), ceil(L / k_block)] (bool, CPU; [num_heads, ...] with the same mask per head when num_heads is
    given) for a video of grid = (F, H, W) patches flattened as i = (f * H + h) * W + w, L = F H W: block (qb, kb) is set iff SOME query
    token in qb and SOME key token in kb have -before <= f_k - f_q <= after, |h_k - h_q| <= rows and |w_k - w_q| <= cols, with frames =
    (before, after); -1 = unbounded on that axis.

    The result is the BLOCK COVER of that 3-D neighbourhood: attention under it (`flash_attention(block_mask=)`,
    `WanModel.set_attn_block_mask`) computes the function the MASK defines - every query of a block sees every key of each set tile -
    not the element-exact neighbourhood, which it contains. Every query block sees at least its own tokens, so no row is empty."""
    F, H, W = (int(g) for g in grid)
    before, after = (int(f) for f in frames)
    rows, cols = int(rows), int(cols)
    if min(F, H, W) < 1 or min(before, after, rows, cols) < -1:
        raise ValueError(f"video_block_mask: grid {grid!r} must be positive, frames {frames!r} / rows {rows} / cols {cols} >= 0 or -1 = unbounded")
    L = F * H * W
    nqb, nkb = -(-L // q_block), -(-L // k_block)
    i = torch.arange(L)
    f, h, w = i // (H * W), (i // W) % H, i % W

    def near(lo, hi, size):
        """[size, size] bool: lo <= c_k - c_q <= hi, -1 = unbounded."""
        d = torch.arange(size)[None, :] - torch.arange(size)[:, None]
        return ((d >= -lo) if lo >= 0 else torch.ones_like(d, dtype=torch.bool)) & ((d <= hi) if hi >= 0 else torch.ones_like(d, dtype=torch.bool))

    # ONE token pair must meet all three conditions, so the axes cannot be covered separately: per query block, the keys within reach of
    # SOME of its tokens (q_block x L pair tests), then the tiles those keys lie in
    qcell = i // q_block
    kcell = i // k_block
    nf, nh, nw = near(before, after, F), near(rows, rows, H), near(cols, cols, W)
    mask = torch.zeros(nqb, nkb, dtype=torch.bool)
    for qb in range(nqb):
        sel = qcell == qb
        ok = (nf[f[sel]][:, f] & nh[h[sel]][:, h] & nw[w[sel]][:, w]).any(dim=0)       # [L] keys
        mask[qb, kcell[ok].unique()] = True
    return mask if num_heads is None else mask[None].expand(int(num_heads), nqb, nkb).clone()
