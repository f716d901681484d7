"""Wan DiT (`WanModel`) on MI355X: the reference's module tree / parameter names / call signatures over the
hand-written HIP kernels of libunivid_hip.so.

Mirrors /root/reference/models/wan/utils/modules/model.py (WanModel :294-546, WanAttentionBlock :183-259,
WanSelfAttention :101-155, WanCrossAttention :158-180, Head :262-291, WanRMSNorm :69-85, WanLayerNorm :88-98)
so that UniVid's own code keeps working against it: `.blocks` is an nn.ModuleList, cross-attention modules are
instances of a class NAMED `WanCrossAttention` whose `.forward(x, context, context_lens)` can be re-assigned
per instance (models/model_pipeline.py:1745-1807), the nn.Linear children are called
self_attn.{q,k,v,o} / cross_attn.{q,k,v,o} / ffn.0 / ffn.2 (LoRA targets, model_pipeline.py:474-493), and the
state-dict keys equal the reference's, so its checkpoints load.

Numerics contract = UniVid's runtime setting (fp32 parameters, ambient autocast(bf16), fp32 islands; SURVEY.md
Appendix A): parameters stay fp32 nn.Parameters; `prepare()` makes the bf16 copies autocast would make on
every call. Every op runs in a HIP kernel; torch is used for memory, streams and views only. There is no
eager fallback: without the extension or a gfx950 device, forward raises.

Per-token timesteps (`t` of shape [B, seq_len], textimage2video.py:373-378) are handled without materialising
the reference's [L, 6, dim] fp32 modulation tensor (843 MB at L = 11 440): the distinct timestep values
(1 for t2v, 2 for i2v) go through the time MLPs once, and kernels index the resulting rows with a
token -> row map.
"""
import contextlib
import math
from typing import List, Optional

import torch
import torch.nn as nn

from .. import _lib
from .attention import topk_attention
from .modes import ATTN_PRECISIONS, FFN_PRECISIONS, MODE_DEFAULTS, PROJ_PRECISIONS, AttnBlockMask, AttnTopKMask, validate_modes  # noqa: F401
from .._lib import (EPI_BF16, EPI_BF16_T, EPI_F32_FROM_BF16, EPI_GATE_RESID_F32, EPI_GELU_BF16, EPI_RESID_F32)

__all__ = ["WanModel"]

BF16 = torch.bfloat16


def _round_up(x, m):
    return (x + m - 1) // m * m


def rope_params(max_seq_len, dim, theta=10000):
    """complex128 phasor table (model.py:27-35); built once on the host in fp64."""
    ang = torch.outer(torch.arange(max_seq_len),
                      1.0 / torch.pow(theta, torch.arange(0, dim, 2).to(torch.float64).div(dim)))
    return torch.polar(torch.ones_like(ang), ang)


class _Prepared:
    """bf16 weight/bias copies of one nn.Linear (what autocast's weight cache holds in the reference)."""
    __slots__ = ("w", "b")

    def __init__(self, lin: nn.Linear, pad_k: int = 0):
        if hasattr(lin, "base_layer") or hasattr(lin, "lora_A"):
            # PEFT's lora.Linear (what the reference's LoRAManager installs on q/k/v/o/ffn.0/ffn.2, model_pipeline.py:340-380)
            # exposes `.weight` = base_layer.weight: reading it would silently DROP the adapter. The fused kernels consume one
            # dense weight per projection, so the deltas have to be folded in first.
            raise NotImplementedError(
                "a LoRA-wrapped nn.Linear (PEFT lora.Linear) was found in the DiT: the HIP path reads dense weights and would "
                "ignore the adapter. Load the adapter directory with `univid_amd.lora.LoRAManager().load_lora_weights(dir, model)` "
                "(folds it into the dense weights), or fold it in with `peft_model.merge_and_unload()` and call "
                "`WanModel.invalidate()` before the next forward - or, to keep the adapter un-merged and swappable, attach the adapter "
                "directory to the un-wrapped model with `LoRAManager().load_lora_weights(dir, model, merge=False)`.")
        w = lin.weight.detach()
        if pad_k and w.shape[1] % pad_k:
            w = torch.nn.functional.pad(w, (0, pad_k - w.shape[1] % pad_k))
        self.w = w.to(BF16).contiguous()
        self.b = None if lin.bias is None else lin.bias.detach().to(BF16).contiguous()


class _PreparedMx:
    """OCP MXFP8 operand of one nn.Linear for uv_gemm_mxfp8_nt: e4m3fn codes [N, K] and e8m0 scales [N, K / 32] (uint8 both), quantised
    by uv_mx_quant_bf16 from the bf16 copy the bf16 path reads - which is not kept - and the bf16 bias."""
    __slots__ = ("w", "s", "b")

    def __init__(self, lin: nn.Linear):
        p = _Prepared(lin)
        N, K = p.w.shape
        self.w = torch.empty(N, K, dtype=torch.uint8, device=p.w.device)
        self.s = torch.empty(N, K // 32, dtype=torch.uint8, device=p.w.device)
        _lib.mx_quant(p.w, self.w, self.s)
        self.b = p.b


def _mx_act(t, M, K):
    """bf16 activation [>= M, >= K] -> its MXFP8 form (codes, scales) over M rows (uv_mx_quant_bf16): the input of an MXFP8 projection."""
    c = torch.empty(M, K, dtype=torch.uint8, device=t.device)
    sc = torch.empty(M, K // 32, dtype=torch.uint8, device=t.device)
    _lib.mx_quant(t, c, sc, M=M, K=K)
    return c, sc


# ---- un-merged LoRA (univid_amd/lora.py attaches; peft lora/layer.py Linear.forward) ---------------------------------------------
# An attached adapter lives on its nn.Linear as `lin._uv_lora = {adapter name: {"A": [r, in], "B": [out, r], "scaling": s, "weight": w}}`
# and never touches the fp32 master weight. The projections that read ONE activation share one slot of whole 128-column groups behind
# that activation's K columns: uv_lora_down_bf16 writes T = bf16(scale o (x A^T)) there (every adapter's lora_A stacked row-wise), and
# each adapted projection's bf16 operand becomes [W | B | 0] with its lora_B in its own column range of the slot, so the tuned GEMM
# kernels run unchanged with K + S columns and the adapter's contribution lands in the fp32 accumulator in front of the fused epilogue.
LORA_MAX_SLOT = 512     # columns of one activation's slot = the stacked rank of all adapters on all projections reading it, rounded up to 128


class _LoraSlot:
    """Stacked lora_A [R, K] bf16, the per-row scale f32 [R] (scaling x run-time weight) and the slot width S of one activation.
    Under per-sample adapter weights (WanModel.set_adapter_weights) also the scale matrix f32 [samples, R], one row per sample of the
    coming forwards: `seg` on the device, `seg_host` its host copy (None = global weights: the launch is the vector one)."""
    __slots__ = ("A", "scale", "S", "rows", "seg", "seg_host")

    def __init__(self, entries, dev):
        self.rows = [(ad, ad["A"].shape[0]) for ad in entries]
        R = sum(r for _, r in self.rows)
        self.S = _round_up(R, 128)
        if self.S > LORA_MAX_SLOT:
            raise ValueError(f"the adapters on the projections of one input stack to rank {R}: more than the {LORA_MAX_SLOT} slot columns "
                             f"(LORA_MAX_SLOT) an activation buffer carries")
        self.A = torch.cat([ad["A"].to(device=dev, dtype=BF16) for ad in entries]).contiguous()
        self.scale = torch.empty(R, dtype=torch.float32, device=dev)
        self.seg = self.seg_host = None
        self.refresh_scale()

    def refresh_scale(self):
        """Re-reads scaling x weight of every adapter into the device vector, in place (graph-captured launches read the same memory)."""
        host = torch.cat([torch.full((r,), float(ad["scaling"]) * float(ad["weight"]), dtype=torch.float32) for ad, r in self.rows])
        self.scale.copy_(host)
        # per-sample weights: `ad["per_sample"]` holds one weight per sample (None = the adapter's global weight). The device matrix is kept
        # when the model goes back to global weights: a captured graph of that setting reads it again when the setting comes back
        n = max((len(ad["per_sample"]) for ad, _ in self.rows if ad.get("per_sample") is not None), default=0)
        if not n:
            self.seg_host = None
            return
        def w(ad, i):
            ps = ad.get("per_sample")
            return float(ad["weight"] if ps is None or ps[i] is None else ps[i])
        self.seg_host = torch.stack([torch.cat([torch.full((r,), float(ad["scaling"]) * w(ad, i), dtype=torch.float32) for ad, r in self.rows])
                                     for i in range(n)])
        if self.seg is None or self.seg.shape != self.seg_host.shape:
            with torch.inference_mode(False):      # a normal tensor: written in place by later settings, inside or outside inference mode
                self.seg = torch.empty(self.seg_host.shape, dtype=torch.float32, device=self.scale.device)
        self.seg.copy_(self.seg_host)

    def rows_equal(self, s0, n):
        """True when the samples [s0, s0 + n) carry the same scale row (always, under global weights)."""
        h = self.seg_host
        return h is None or bool((h[s0:s0 + n] == h[s0:s0 + 1]).all())


def _prepare_group(lins):
    """({name: _Prepared}, _LoraSlot | None) of the nn.Linears that read the same activation. Without attached adapters: exactly the
    dense operands. With: the adapted projections get [W | B | 0] (the others keep W and ignore the slot)."""
    preps = {n: _Prepared(l) for n, l in lins.items()}
    entries = [(n, ad) for n, l in lins.items() for ad in getattr(l, "_uv_lora", {}).values()]
    if not entries:
        return preps, None
    first = next(iter(preps.values())).w
    K, dev = first.shape[1], first.device
    slot = _LoraSlot([ad for _, ad in entries], dev)
    col = K
    for n, ad in entries:
        p, r = preps[n], ad["A"].shape[0]
        if p.w.shape[1] == K:
            w = torch.zeros(p.w.shape[0], K + slot.S, dtype=BF16, device=dev)
            w[:, :K] = p.w
            p.w = w
        p.w[:, col:col + r] = ad["B"].to(device=dev, dtype=BF16)
        col += r
    return preps, slot


def _act_buf(rows, K, slots, dev):
    """bf16 activation [rows, K + S]: S = the widest slot of the projections that will read it (0 without adapters: the plain buffer)."""
    S = max((s.S for s in slots if s is not None), default=0)
    return torch.empty(rows, K + S, dtype=BF16, device=dev)


def _slotted(t, K, slot, M=None, seg_rows=None, s0=0):
    """The activation `t` (x in its first K columns) as the [W | B] GEMMs of `slot` read it: the slot's down-projection of the first M
    rows written behind the K columns, in place when `t` was allocated with room for it (_act_buf), into a widened copy otherwise.
    Under per-sample adapter weights the M rows are stacked samples of seg_rows rows each (None: one sample), the first of them sample
    s0 of the forward: each takes its own scale row."""
    if slot is None:
        return t
    M = t.shape[0] if M is None else M
    if t.shape[1] < K + slot.S:
        e = torch.empty(t.shape[0], K + slot.S, dtype=BF16, device=t.device)
        e[:M, :K].copy_(t[:M, :K])
        t = e
    if M and slot.seg_host is None:
        _lib.lora_down(t, K, slot.A, slot.scale, M=M, Rpad=slot.S)
    elif M:
        _lib.lora_down_seg(t, K, slot.A, slot.seg[s0:], M if seg_rows is None else seg_rows, M=M, Rpad=slot.S)
    return t


class WanRMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim))


class WanLayerNorm(nn.LayerNorm):
    def __init__(self, dim, eps=1e-6, elementwise_affine=False):
        super().__init__(dim, elementwise_affine=elementwise_affine, eps=eps)


class WanSelfAttention(nn.Module):
    def __init__(self, dim, num_heads, window_size=(-1, -1), qk_norm=True, eps=1e-6):
        assert dim % num_heads == 0
        super().__init__()
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.qk_norm, self.eps = qk_norm, eps
        if not qk_norm:
            raise NotImplementedError("only the TI2V-5B setting (qk_norm) is built")
        # (left, right) of flash-attn's window_size, or None = global attention (WanModel.set_attn_window): instance state
        self.attn_window = self._validate({"attn_window": window_size})["attn_window"]
        self.window_size = self.attn_window or (-1, -1)
        self.attn_block_mask = None      # an AttnBlockMask, or None = global attention (WanModel.set_attn_block_mask): instance state
        self.q = nn.Linear(dim, dim)
        self.k = nn.Linear(dim, dim)
        self.v = nn.Linear(dim, dim)
        self.o = nn.Linear(dim, dim)
        self.norm_q = WanRMSNorm(dim, eps=eps)
        self.norm_k = WanRMSNorm(dim, eps=eps)
        self._prep = None
        self._slots = {}
        self._kv_cache = {}
        self.attn_precision = "bf16"     # WanModel.set_attn_precision: instance state, never a module global
        self.proj_precision = "bf16"     # WanModel.set_proj_precision: likewise

    _groups = {"qkv": ("q", "k", "v"), "o": ("o",)}      # projections by the activation they read (one LoRA slot each)
    _mx_proj = ("q", "k", "v", "o")                      # the projections proj_precision "mxfp8" puts on uv_gemm_mxfp8_nt

    def _validate(self, cand):
        """validate_modes of the settings `cand` on this module alone (its constructor's window, its projections' mode when it prepares)."""
        return validate_modes(cand, dim=self.dim, head_dim=self.head_dim, num_heads=self.num_heads, attns=(self,))

    def prepare(self):
        self._prep, self._slots = {}, {}
        mx = self.proj_precision == "mxfp8"
        if mx:
            self._validate({"proj_precision": "mxfp8"})
        for g, names in self._groups.items():
            if mx and all(n in self._mx_proj for n in names):       # codes + scales; the bf16 operand copies are not kept, no slot
                self._prep.update({n: _PreparedMx(getattr(self, n)) for n in names})
                self._slots[g] = None
                continue
            preps, self._slots[g] = _prepare_group({n: getattr(self, n) for n in names})
            self._prep.update(preps)
        self._kv_cache = {}

    def _qkv(self, h, M, seg_rows, s0, vt):
        """The q / k / v projections of h's first M rows (stacked samples of seg_rows rows, the first of them sample s0 of the forward's
        per-sample adapter weights): the slot's down-projection, then q and k as bf16 [M, C] (returned) and V^T into vt's first M columns
        (sample b = columns b*seg_rows..)."""
        C, p = self.dim, self._prep
        if self.proj_precision == "mxfp8":
            # h = (codes, scales) of the modulated input (uv_layernorm_mod_mx, or mx_quant of a bf16 input): the three GEMMs on MXFP8 operands
            hc, hs = h
            ql = torch.empty(M, C, dtype=BF16, device=hc.device)
            kl = torch.empty(M, C, dtype=BF16, device=hc.device)
            _lib.gemm_mxfp8(hc, hs, p["q"].w, p["q"].s, p["q"].b, ql, EPI_BF16, M=M)
            _lib.gemm_mxfp8(hc, hs, p["k"].w, p["k"].s, p["k"].b, kl, EPI_BF16, M=M)
            _lib.gemm_mxfp8_t(hc, hs, p["v"].w, p["v"].s, p["v"].b, vt, M=M)
            return ql, kl
        h = _slotted(h, C, self._slots["qkv"], M, seg_rows, s0)
        ql = torch.empty(M, C, dtype=BF16, device=h.device)
        kl = torch.empty(M, C, dtype=BF16, device=h.device)
        _lib.gemm_bf16(h, p["q"].w, p["q"].b, ql, EPI_BF16, M=M)
        _lib.gemm_bf16(h, p["k"].w, p["k"].b, kl, EPI_BF16, M=M)
        _lib.gemm_bf16(h, p["v"].w, p["v"].b, vt, EPI_BF16_T, M=M)
        return ql, kl

    def _attn(self, h, L, Lk, grid, freqs, batch, s0):
        """Self-attention of h (bf16 [batch*L, C], samples stacked along the token axis; proj_precision "mxfp8": its (codes, scales)) over
        each sample's first Lk keys (Lk < L: the rest of L is padding; one sample only) -> the attention output (bf16) as the o projection
        reads it (proj_precision "mxfp8": as _o_proj quantises it)."""
        C, H, D = self.dim, self.num_heads, self.head_dim
        M = batch * L
        dev = h[0].device if isinstance(h, tuple) else h.device
        bm = None
        if self.attn_block_mask is not None:
            # the mask counts tokens of the UNPADDED sequence (set_attn_block_mask keeps attn_precision at "bf16" and no window beside it);
            # resolved before the first launch: a refused mask leaves nothing half-computed
            if Lk != L:
                raise NotImplementedError(f"attn_block_mask with padded samples (seq_len {Lk} < {L}) is not built: call WanModel.forward, "
                                          f"which strips the padding")
            bm = self.attn_block_mask.resolve(grid, L, dev)
        vt = _vt_scratch("vt", C, batch, L, dev)
        ql, kl = self._qkv(h, M, L, s0, vt)
        att = _act_buf(M, C, (self._slots["o"],), dev)
        if self.attn_window is not None:
            # the window counts tokens of the UNPADDED sequence (set_attn_window keeps attn_precision at "bf16")
            if Lk != L:
                raise NotImplementedError(f"window_size {self.attn_window} with padded samples (seq_len {Lk} < {L}) is not built: "
                                          f"call WanModel.forward, which strips the padding")
            _lib.rmsnorm_rope_qk(ql, kl, self.norm_q.weight, self.norm_k.weight, M, L, C, D, self.eps, freqs, grid)
            _lib.flash_attn_win(ql, kl, vt, att, L, H, D, 1.0 / math.sqrt(D), self.attn_window, batch=batch)
            return _slotted(att, C, self._slots["o"], M, L, s0)
        if bm is not None:
            _lib.rmsnorm_rope_qk(ql, kl, self.norm_q.weight, self.norm_k.weight, M, L, C, D, self.eps, freqs, grid)
            if isinstance(bm, AttnTopKMask.Plan):
                # the lists of THIS forward's q / k, per sample and head, built on the device into stable scratch: pool, select, attend -
                # no host synchronisation, nothing allocated inside a captured forward
                topk_attention(ql, kl, vt, att, L, H, D, 1.0 / math.sqrt(D), bm.top_k, bm.keep, batch,
                               scratch=lambda tag, shape, dtype: _mx_scratch(tag, shape, dev, dtype))
            else:
                _lib.flash_attn_bs(ql, kl, vt, att, L, H, D, 1.0 / math.sqrt(D), bm, batch=batch)
            return _slotted(att, C, self._slots["o"], M, L, s0)
        if self.attn_precision != "bf16":
            # q and k leave the norm + RoPE pass as MXFP8 codes + scales (fresh buffers: no in-place form), S = K Q^T on the block-scaled
            # matrix instruction; "mxfp8_qk": V^T, P.V and the output stay bf16
            qc, kc = (torch.empty(M, C, dtype=torch.uint8, device=dev) for _ in range(2))
            qs, ks = (torch.empty(M, C // 32, dtype=torch.uint8, device=dev) for _ in range(2))
            _lib.rmsnorm_rope_qk_mx(ql, kl, self.norm_q.weight, self.norm_k.weight, qc, qs, kc, ks, M, L, C, D, self.eps, freqs, grid)
            if self.attn_precision == "mxfp8_qk_pv":
                # the bf16 V^T of the GEMM (un-merged LoRA included) quantised along the keys into stable scratch (every byte, pads
                # included, is rewritten per call), P as e4m3: P.V on the block-scaled instruction too. Lk < L: one sample, its first Lk keys
                cols = _lib.vt_mx_cols(batch, L)
                vc = _mx_scratch("vt_codes", (C, cols), dev)
                vs = _mx_scratch("vt_scales", (H, 4 * cols), dev)
                if Lk == L:
                    _lib.vt_mx_quant(vt, vc, vs, L, H, D, batch=batch)
                else:
                    _lib.vt_mx_quant(vt, vc, vs, Lk, H, D)
                _lib.flash_attn_mxpv(qc, qs, kc, ks, vc, vs, att, L, Lk, H, D, 1.0 / math.sqrt(D), batch=batch)
            else:
                _lib.flash_attn_mxqk(qc, qs, kc, ks, vt, att, L, Lk, H, D, 1.0 / math.sqrt(D), batch=batch)
            return _slotted(att, C, self._slots["o"], M, L, s0)
        # q and k of every stacked sample in one launch (RoPE positions restart with every sample)
        _lib.rmsnorm_rope_qk(ql, kl, self.norm_q.weight, self.norm_k.weight, M, L, C, D, self.eps, freqs, grid)
        _lib.flash_attn(ql, kl, vt, att, L, Lk, H, D, 1.0 / math.sqrt(D), batch=batch)
        return _slotted(att, C, self._slots["o"], M, L, s0)

    def _self_attn(self, h, L, grid, freqs, x_resid, gate, gate_tid, batch=1, sp=None, s0=0):
        """h: bf16 [batch*L, C] modulated input (samples stacked along the token axis). Adds o(attn) * gate into x_resid
        (fp32) in the GEMM epilogue. sp = (SeqParallel, L_total, r0): h holds this rank's token range of every sample.
        s0: the first stacked sample's index among the samples of per-sample adapter weights (WanModel.set_adapter_weights)."""
        if sp is not None:
            return self._self_attn_sp(h, L, grid, freqs, x_resid, gate, gate_tid, batch, sp, s0=s0)
        self._o_proj(self._attn(h, L, L, grid, freqs, batch, s0), x_resid, EPI_GATE_RESID_F32, batch * L, gate=gate, gate_tid=gate_tid)

    def _o_proj(self, att, out, epi, M, gate=None, gate_tid=None):
        """The o projection of the attention output att (bf16, its slot filled) into `out` through epilogue `epi`; proj_precision "mxfp8":
        one quantise pass over att (the attention kernels store bf16), then the MXFP8 GEMM with the same epilogue."""
        p = self._prep["o"]
        if self.proj_precision == "mxfp8":
            ac, asc = _mx_act(att, M, self.dim)
            _lib.gemm_mxfp8(ac, asc, p.w, p.s, p.b, out, epi, M=M, gate=gate, gate_tid=gate_tid)
        else:
            _lib.gemm_bf16(att, p.w, p.b, out, epi, M=M, gate=gate, gate_tid=gate_tid)

    def _self_attn_sp(self, h, n, grid, freqs, x_resid, gate, gate_tid, batch, sp, s0=0):
        """Ulysses form (distributed/sequence_parallel.py:147-176, ulysses.py:9-47): projections, RMSNorm and RoPE on the
        rank's n tokens of each sample; q/k/V^T exchanged to [all tokens, heads/p]; attention over the whole sequence for
        the rank's heads; output exchanged back; o-projection + gated residual on the rank's tokens."""
        if self.attn_window is not None:
            raise NotImplementedError(f"window_size {self.attn_window} is not built for the sequence-parallel forward (the Ulysses attention "
                                      f"runs the dense kernel): set_attn_window(None) or run without sequence parallelism")
        if self.attn_block_mask is not None:
            raise NotImplementedError("attn_block_mask is not built for the sequence-parallel forward (the Ulysses attention runs the dense "
                                      "kernel): set_attn_block_mask(None) or run without sequence parallelism")
        if self.attn_precision != "bf16":
            raise NotImplementedError(f"attn_precision {self.attn_precision!r} is not built for the sequence-parallel forward (the Ulysses "
                                      f"exchange carries bf16 q / k): set_attn_precision('bf16') or run without sequence parallelism")
        if self.proj_precision != "bf16":
            raise NotImplementedError(f"proj_precision {self.proj_precision!r} is not built for the sequence-parallel forward (its projections "
                                      f"read a bf16 activation): set_proj_precision('bf16') or run without sequence parallelism")
        par, Lt, r0 = sp
        C, H, D = self.dim, self.num_heads, self.head_dim
        P = par.size
        if H % P or Lt % 8:
            raise NotImplementedError(f"sequence parallel needs heads % ranks == 0 and tokens % 8 == 0 (H={H}, p={P}, L={Lt})")
        p = self._prep
        dev = h.device
        M = batch * n
        Cp, Hp = C // P, H // P
        vt = torch.zeros(C, _lib.vt_cols(1, max(M, 1)), dtype=BF16, device=dev)      # (the rank's tokens of all samples side by side)
        qf = torch.empty(batch * Lt, Cp, dtype=BF16, device=dev)
        kf = torch.empty(batch * Lt, Cp, dtype=BF16, device=dev)
        vtf = _vt_scratch("vt_sp", Cp, batch, Lt, dev)
        ql, kl = self._qkv(h, M, n, s0, vt) if M else (h.new_empty(0, C), h.new_empty(0, C))
        for b in range(batch):
            rows = slice(b * n, (b + 1) * n)
            if n:
                _lib.rmsnorm_rope(ql[rows], ql[rows], self.norm_q.weight, n, C, D, self.eps, freqs, grid, row0=r0)
                _lib.rmsnorm_rope(kl[rows], kl[rows], self.norm_k.weight, n, C, D, self.eps, freqs, grid, row0=r0)
            par.heads_to_tokens(ql[rows], Lt, qf[b * Lt:(b + 1) * Lt])
            par.heads_to_tokens(kl[rows], Lt, kf[b * Lt:(b + 1) * Lt])
            par.heads_to_tokens_T(vt[:, b * n:(b + 1) * n], Lt, vtf, col0=b * Lt)
        attf = torch.empty(batch * Lt, Cp, dtype=BF16, device=dev)
        _lib.flash_attn(qf, kf, vtf, attf, Lt, Lt, Hp, D, 1.0 / math.sqrt(D), batch=batch)
        att = torch.empty(M, C, dtype=BF16, device=dev)
        for b in range(batch):
            par.tokens_to_heads(attf[b * Lt:(b + 1) * Lt], Lt, att[b * n:(b + 1) * n])
        if M:
            att = _slotted(att, C, self._slots["o"], M, n, s0)
            _lib.gemm_bf16(att, p["o"].w, p["o"].b, x_resid, EPI_GATE_RESID_F32, M=M, gate=gate, gate_tid=gate_tid)

    def forward(self, x, seq_lens, grid_sizes, freqs):
        """Reference signature (model.py:126-155): x [B, L, C] -> [B, L, C] bf16. Keys >= seq_lens[b] are masked,
        which here means: only the first seq_lens[b] tokens are attended (the rest of L is padding)."""
        L = x.size(1)
        if self.attn_window is not None and any(int(s) < L for s in seq_lens):
            raise NotImplementedError(f"window_size {self.attn_window} with padded samples (seq_lens {[int(s) for s in seq_lens]} < {L}) is "
                                      f"not built: call WanModel.forward, which strips the padding")
        if self.attn_block_mask is not None and any(int(s) < L for s in seq_lens):
            raise NotImplementedError(f"attn_block_mask with padded samples (seq_lens {[int(s) for s in seq_lens]} < {L}) is not built: "
                                      f"call WanModel.forward, which strips the padding")
        _ensure_prepared(self)
        outs = []
        fr = _freqs_device(freqs, x.device)
        for b in range(x.size(0)):      # (sample b of the batch takes its own row of per-sample adapter weights)
            xb = x[b].to(BF16).contiguous()
            if self.proj_precision == "mxfp8":
                xb = _mx_act(xb, L, self.dim)
            att = self._attn(xb, L, int(seq_lens[b]), tuple(int(v) for v in grid_sizes[b]), fr, 1, b)
            y = torch.empty(L, self.dim, dtype=BF16, device=x.device)
            self._o_proj(att, y, EPI_BF16, L)
            outs.append(y)
        return torch.stack(outs)


class WanCrossAttention(WanSelfAttention):
    """Text cross-attention (model.py:158-180). The class name and the (x, context, context_lens) signature are
    part of UniVid's contract: Wan22ContextWrapper finds modules by `__class__.__name__ == 'WanCrossAttention'`
    and replaces `module.forward` with a closure that rescales `context` (model_pipeline.py:1745-1807)."""
    _groups = {"q": ("q",), "kv": ("k", "v"), "o": ("o",)}
    _mx_proj = ("q", "o")       # k / v are context-side, computed once per generation: they stay bf16 in proj_precision "mxfp8"
    _s0 = 0     # a re-assigned `forward` (UniVid's closure) calls the original with (x, context, None) and cannot carry the sample offset:
                # the block sets this around THAT call only (WanAttentionBlock._run); every other path takes s0 as an argument

    def _context_kv(self, ctx, Lc, batch, kv_key, out=None, s0=0):
        """k = norm_k(Wk ctx) [batch*Lc, C] and V^T = (Wv ctx)^T of the embedded context (model.py:170-172). They depend on the
        context and this block's weights only, not on the latent or the timestep, so across the steps of a sampling loop they are
        computed ONCE: `kv_key` identifies the (context generation, sample group) WanModel.forward is running; None = no caching
        (the reference-signature forward, a context under UniVid's dynamic text weight - it changes from forward to forward -, or
        out=(k, V^T): the caller's own buffers, written in place - the HIP-graph runner's, which its captured attention launches read)."""
        hit = self._kv_cache.get(kv_key) if kv_key is not None else None
        if hit is not None:
            return hit
        C, D = self.dim, self.head_dim
        p = self._prep
        dev = ctx.device
        if out is not None:
            kl, vt = out
        else:
            kl = torch.empty(batch * Lc, C, dtype=BF16, device=dev)
            if kv_key is None:
                vt = _vt_scratch("cvt", C, batch, Lc, dev)
            else:       # kept in the cache: a tensor of its own
                if batch > 1 and Lc % 8:
                    raise NotImplementedError(f"stacked samples need a context length divisible by 8 (got {Lc})")
                vt = torch.zeros(C, _lib.vt_cols(batch, Lc), dtype=BF16, device=dev)
        ctx = _slotted(ctx, C, self._slots["kv"], batch * Lc, Lc, s0)
        _lib.gemm_bf16(ctx, p["k"].w, p["k"].b, kl, EPI_BF16, M=batch * Lc)
        _lib.gemm_bf16(ctx, p["v"].w, p["v"].b, vt, EPI_BF16_T, M=batch * Lc)
        _lib.rmsnorm_rope(kl, kl, self.norm_k.weight, batch * Lc, C, D, self.eps)
        if kv_key is not None and out is None:
            if self._kv_cache and next(iter(self._kv_cache))[0] != kv_key[0]:
                self._kv_cache.clear()          # a new context generation: the old entries can never hit again
            self._kv_cache[kv_key] = (kl, vt)
        return kl, vt

    def _attend(self, hq, ctx, L, Lc, batch=1, kv_key=None, kv=None, s0=0):
        """hq bf16 [batch*L, C] (normed queries' input; proj_precision "mxfp8": its (codes, scales)), ctx bf16 [batch*Lc, C] -> attention
        output bf16 [batch*L, C].
        kv = (k, V^T) of the stacked contexts in the caller's own buffers (WanModel.forward's context_kv=): ctx is then not read."""
        C, H, D = self.dim, self.num_heads, self.head_dim
        p = self._prep
        mx = self.proj_precision == "mxfp8"
        dev = hq[0].device if mx else hq.device
        M = batch * L
        if not mx:
            hq = _slotted(hq, C, self._slots["q"], M, L, s0)
        ql = torch.empty(M, C, dtype=BF16, device=dev)
        kl, vt = kv if kv is not None else self._context_kv(ctx, Lc, batch, kv_key, s0=s0)
        att = _act_buf(M, C, (self._slots["o"],), dev)
        if mx:
            # the q projection on MXFP8 operands with the sums of squares in its epilogue; norm_q and the attention are the bf16 path's
            ssq = torch.empty(M, C // 32, dtype=torch.float32, device=dev)
            rs = torch.empty(M, dtype=torch.float32, device=dev)
            _lib.gemm_mxfp8_ssq(hq[0], hq[1], p["q"].w, p["q"].s, p["q"].b, ql, ssq, M=M)
            _lib.rms_scale_from_ssq(ssq, rs, M, C, self.eps)
            _lib.flash_attn(ql, kl, vt, att, L, Lc, H, D, 1.0 / math.sqrt(D), batch=batch, q_rs=rs, q_weight=self.norm_q.weight)
            return att
        if C % 32 == 0:
            # norm_q without a pass of its own over q (round 5): the q GEMM's epilogue leaves each output row's sums of squares per 32-column
            # group, a tiny kernel turns them into the row scale 1 / sqrt(mean + eps), and the attention kernel's Q prologue applies scale and
            # weight with WanRMSNorm's rounding points (model.py:82-85) while it loads the raw projection
            ssq = torch.empty(M, C // 32, dtype=torch.float32, device=dev)
            rs = torch.empty(M, dtype=torch.float32, device=dev)
            _lib.gemm_bf16_ssq(hq, p["q"].w, p["q"].b, ql, ssq, M=M)
            _lib.rms_scale_from_ssq(ssq, rs, M, C, self.eps)
            _lib.flash_attn(ql, kl, vt, att, L, Lc, H, D, 1.0 / math.sqrt(D), batch=batch, q_rs=rs, q_weight=self.norm_q.weight)
            return att
        _lib.gemm_bf16(hq, p["q"].w, p["q"].b, ql, EPI_BF16, M=M)
        _lib.rmsnorm_rope(ql, ql, self.norm_q.weight, M, C, D, self.eps)
        _lib.flash_attn(ql, kl, vt, att, L, Lc, H, D, 1.0 / math.sqrt(D), batch=batch)
        return att

    def _cross_fused(self, hq, ctx, L, Lc, x_resid, batch=1, kv_key=None, kv=None, s0=0):
        att = _slotted(self._attend(hq, ctx, L, Lc, batch, kv_key, kv, s0), self.dim, self._slots["o"], batch * L, L, s0)
        self._o_proj(att, x_resid, EPI_RESID_F32, batch * L)

    def forward(self, x, context, context_lens=None):
        """x [B, L1, C], context [B, L2, C] -> [B, L1, C] bf16 (the caller adds it to the residual stream)."""
        if context_lens is not None:
            raise NotImplementedError("context_lens is always None on UniVid's path (model.py:472)")
        _ensure_prepared(self)
        outs = []
        L, Lc = x.size(1), context.size(1)
        for b in range(x.size(0)):
            s0 = self._s0 + b       # (sample b of the batch takes its own row of per-sample adapter weights)
            xb = x[b].to(BF16).contiguous()
            if self.proj_precision == "mxfp8":
                xb = _mx_act(xb, L, self.dim)
            att = _slotted(self._attend(xb, context[b].to(BF16).contiguous(), L, Lc, s0=s0), self.dim, self._slots["o"], s0=s0)
            y = torch.empty(L, self.dim, dtype=BF16, device=x.device)
            self._o_proj(att, y, EPI_BF16, L)
            outs.append(y)
        return torch.stack(outs)


class WanAttentionBlock(nn.Module):
    def __init__(self, dim, ffn_dim, num_heads, window_size=(-1, -1), qk_norm=True, cross_attn_norm=False, eps=1e-6):
        super().__init__()
        self.dim, self.ffn_dim, self.num_heads, self.eps = dim, ffn_dim, num_heads, eps
        self.qk_norm, self.cross_attn_norm = qk_norm, cross_attn_norm
        self.norm1 = WanLayerNorm(dim, eps)
        self.self_attn = WanSelfAttention(dim, num_heads, window_size, qk_norm, eps)
        self.window_size = self.self_attn.window_size
        self.norm3 = WanLayerNorm(dim, eps, elementwise_affine=True) if cross_attn_norm else nn.Identity()
        self.cross_attn = WanCrossAttention(dim, num_heads, (-1, -1), qk_norm, eps)
        self.norm2 = WanLayerNorm(dim, eps)
        self.ffn = nn.Sequential(nn.Linear(dim, ffn_dim), nn.GELU(approximate="tanh"), nn.Linear(ffn_dim, dim))
        self.modulation = nn.Parameter(torch.randn(1, 6, dim) / dim ** 0.5)
        self._prep = None
        self._slots = {}
        self.ffn_precision = "bf16"      # set_ffn_precision: instance state, never a module global
        self.proj_precision = "bf16"     # set_proj_precision: likewise (the attention modules carry their own copy)

    def prepare(self):
        self.self_attn.prepare()
        self.cross_attn.prepare()
        self._prepare_ffn()

    def _validated(self, changes):
        """This block's settings with `changes` ({setting: value}) laid over them, through validate_modes: raises, or returns the complete
        normalised candidate. Changes nothing."""
        sa = self.self_attn
        now = {k: getattr(sa if k.startswith("attn_") else self, k) for k in MODE_DEFAULTS}      # attn_*: the self-attention holds them
        return validate_modes({**now, **changes}, dim=self.dim, ffn_dim=self.ffn_dim, head_dim=sa.head_dim, num_heads=sa.num_heads,
                              block=self, attns=(sa, self.cross_attn))

    def _apply_modes(self, changes):
        """Every block-level setter: validates the candidate, then - and only then - writes the settings and all their mirrors, and drops
        what was prepared under the old value of a changed one. After construction nothing else writes these attributes. The cross-
        attention's window, mask and attn_precision never move; the model's prepared-weights generation is the model-level setters' to move."""
        new = self._validated(changes)
        sa = self.self_attn
        sa.attn_precision, sa.attn_window, sa.attn_block_mask = new["attn_precision"], new["attn_window"], new["attn_block_mask"]
        sa.window_size = self.window_size = new["attn_window"] or (-1, -1)       # (no prepared weight depends on the three above)
        self.ffn_precision = new["ffn_precision"]
        if "ffn_precision" in changes:
            self._prep = None                    # the FFN operands are re-prepared on the next forward
        self.proj_precision = sa.proj_precision = self.cross_attn.proj_precision = new["proj_precision"]
        if "proj_precision" in changes:
            for a in (sa, self.cross_attn):
                a._prep, a._kv_cache = None, {}  # the projections' operands likewise, and no K / V^T of the other mode is served

    def set_ffn_precision(self, mode):
        """"bf16" (default: the reference's arithmetic) or "mxfp8": ffn.0 / ffn.2 on the block-scaled matrix instructions with OCP MXFP8
        operands (uv_gemm_mxfp8_nt) - a labelled fast mode, narrower than the reference. The FFN operands are re-prepared on the next forward."""
        self._apply_modes({"ffn_precision": mode})

    def set_attn_precision(self, mode):
        """"bf16" (default), "mxfp8_qk": this block's self-attention with MXFP8 q / k, or "mxfp8_qk_pv": with an MXFP8 P.V as well
        (WanModel.set_attn_precision states the modes). No prepared weight depends on it."""
        self._apply_modes({"attn_precision": mode})

    def set_attn_window(self, window_size):
        """(left, right) as flash-attn's window_size, or None / (-1, -1) for global attention: this block's self-attention
        (WanModel.set_attn_window states the mode). No prepared weight depends on it."""
        self._apply_modes({"attn_window": window_size})

    def set_attn_block_mask(self, spec):
        """None (global attention), a bool tensor / PreparedBlockMask of one fixed L, a callable f(F, H, W, num_heads) -> bool mask, or an
        AttnBlockMask that resolves one of them: this block's self-attention (WanModel.set_attn_block_mask states the mode). No prepared
        weight depends on it."""
        self._apply_modes({"attn_block_mask": spec})

    def set_proj_precision(self, mode):
        """"bf16" (default: the reference's arithmetic) or "mxfp8": this block's self-attention q / k / v / o and cross-attention q / o on
        uv_gemm_mxfp8_nt, fed by uv_layernorm_mod_mx (WanModel.set_proj_precision states the mode). The projections' operands are
        re-prepared on the next forward."""
        self._apply_modes({"proj_precision": mode})

    def _prepare_ffn(self):
        if self.ffn_precision == "mxfp8":
            self._validated({})      # (an adapter attached by hand since the mode was set)
            self._prep, self._slots = {"ffn0": _PreparedMx(self.ffn[0]), "ffn2": _PreparedMx(self.ffn[2])}, {"ffn0": None, "ffn2": None}
            return
        p0, s0 = _prepare_group({"ffn0": self.ffn[0]})
        p2, s2 = _prepare_group({"ffn2": self.ffn[2]})
        self._prep, self._slots = {**p0, **p2}, {"ffn0": s0, "ffn2": s2}

    def _run(self, x, L, e0_rows, tid, grid, freqs, ctx, first_block, batch=1, sp=None, kv_key=None, twin_rows=False, s0=0, kv=None):
        """x: fp32 [batch*L, C] residual stream (independent samples stacked along the token axis), updated IN PLACE.
        e0_rows: fp32 [n_t, 6C]; tid int32 [batch*L] | None; ctx: bf16 [batch*Lc, C] embedded context(s); kv_key: cache key of
        the context's cross-attention K / V^T (WanCrossAttention._context_kv), None = recompute.
        twin_rows: the stacked samples enter this block with IDENTICAL rows and timesteps (the CFG pair on one latent, before its
        first cross-attention): the self-attention half runs on sample 0 only and its result is copied to the others - unless per-sample
        adapter weights give the samples different scale rows in the self-attention's slots.
        s0: the first stacked sample's index among the samples of per-sample adapter weights (WanModel.set_adapter_weights).
        kv: the caller's own (k, V^T) of the stacked contexts (WanModel.forward's context_kv=): ctx is not read and may be None."""
        C = self.dim
        dev = x.device
        # (an adapter attached or detached since the last forward left exactly its own module un-prepared: univid_amd/lora.py)
        _ensure_prepared(self.self_attn)
        _ensure_prepared(self.cross_attn)
        if self._prep is None:
            self._prepare_ffn()
        n_t = e0_rows.shape[0]
        Ls, L = L, batch * L          # Ls = tokens per sample; L = rows of every row-wise kernel below
        tab = torch.empty(n_t, 6 * C, dtype=torch.float32, device=dev)
        _lib.add_rows(self.modulation, e0_rows, tab)                                               # model.py:239
        # (rows of the block's bf16 activations: L, or L rounded up to whole 256-row tiles for ffn.0 - see below; the pad rows are never
        # written and their products never read, so they need no zeroing and no scratch that outlives the forward)
        Lf = _ffn0_rows(L, self.ffn_dim, dev)
        mxp, mxf = self.proj_precision == "mxfp8", self.ffn_precision == "mxfp8"
        hooked = "forward" in self.cross_attn.__dict__
        # the block's bf16 activation, unless every producer below stores MXFP8 (uv_layernorm_mod_mx: no bf16 copy is written)
        if not (mxp and mxf) or hooked or not self.cross_attn_norm or sp is not None:
            h_full = _act_buf(Lf, C, (self.self_attn._slots["qkv"], self.cross_attn._slots["q"], self._slots["ffn0"]), dev)
            h = h_full[:L]
        if mxp or mxf:
            u8 = torch.uint8
            hq, hs = torch.empty(L, C, dtype=u8, device=dev), torch.empty(L, C // 32, dtype=u8, device=dev)
        # NOTE for consumers of `mid` (ffn.0's output, below): its rows >= L are the GELU of whatever the allocator left in h_full[L:]
        # - UNDEFINED, possibly NaN / Inf. Rows are independent in every kernel of the block and ffn.2 reads L rows only.
        # self-attention (model.py:243-247)
        twin = twin_rows and batch > 1 and sp is None and all(s is None or s.rows_equal(s0, batch) for s in self.self_attn._slots.values())
        # the rows and samples the self-attention half runs on: sample 0's for twins (no views on the common path: a slice costs the host
        # as much as a launch)
        xa, ta, nb = (x[:Ls], None if tid is None else tid[:Ls], 1) if twin else (x, tid, batch)
        if mxp and sp is None:
            # norm1 + modulation stored as MXFP8: the bytes of layernorm_mod followed by mx_quant, without the bf16 round trip
            _lib.layernorm_mod_mx(xa, hq, hs, nb * Ls, C, self.eps, mode=1, tab=tab, shift_off=0, scale_off=C, tid=ta, round_ln=first_block)
            ha = (hq, hs)
        else:       # (the sequence-parallel forward refuses the mode in _self_attn_sp)
            ha = h[:Ls] if twin else h
            _lib.layernorm_mod(xa, ha, nb * Ls, C, self.eps, mode=1, tab=tab, shift_off=0, scale_off=C, tid=ta, round_ln=first_block)
        self.self_attn._self_attn(ha, Ls, grid, freqs, xa, tab[:, 2 * C:], ta, nb, sp, s0=s0)
        for b in range(nb, batch):
            x[b * Ls:(b + 1) * Ls].copy_(x[:Ls])
        # cross-attention (model.py:251)
        hc = h if not mxp or hooked or not self.cross_attn_norm else None
        if hc is None:
            _lib.layernorm_mod_mx(x, hq, hs, L, C, self.eps, mode=2, w=self.norm3.weight, b=self.norm3.bias)
            hc = (hq, hs)
        elif self.cross_attn_norm:
            _lib.layernorm_mod(x, h, L, C, self.eps, mode=2, w=self.norm3.weight, b=self.norm3.bias)
        else:
            _lib.cast_f32_bf16(x, h, L, C)
        if mxp and not hooked and not isinstance(hc, tuple):      # no norm3: the bf16 cast, then one quantise pass
            _lib.mx_quant(h, hq, hs, M=L, K=C)
            hc = (hq, hs)
        Lc = (ctx if kv is None else kv[0]).shape[0] // batch
        if hooked:
            # forward was re-assigned on the instance (UniVid hook): honour it, then add the residual un-fused. The closure calls the original
            # forward(x, context, None), which reads the sample offset from the module: set for this call only
            self.cross_attn._s0 = s0
            try:
                y = self.cross_attn.forward(h[:, :C].view(batch, Ls, C), ctx.view(batch, Lc, C), None)
            finally:
                self.cross_attn._s0 = 0
            y = y.reshape(L, C).contiguous()
            _lib.add_bf16_resid(x, y, L, C)
        else:
            self.cross_attn._cross_fused(hc, ctx, Ls, Lc, x, batch, kv_key, kv, s0)
        # FFN (model.py:252-255)
        # ffn.0 on rows rounded up to whole 256-row tiles where the extra tiles ride in the last, partial round of the persistent GEMM
        # (22 880 rows x 14 336 columns: 19.47 -> 19.69 rounds, both 20) instead of a leftover-row launch behind it: the pad rows of the
        # input hold whatever the buffer held (rows are independent: nothing of them reaches a row that is read), their outputs are never
        # read (ffn.2 runs on L rows); results unchanged (a row's arithmetic is the same in both kernels)
        if mxf:
            # the opt-in fast mode: both projections' operands as OCP MXFP8 (quantised per row: no pad rows, no slot), same fused epilogues.
            # ffn.0's input leaves norm2 + modulation as MXFP8 (uv_layernorm_mod_mx: the bytes of layernorm_mod followed by mx_quant)
            p0, p2, F = self._prep["ffn0"], self._prep["ffn2"], self.ffn_dim
            _lib.layernorm_mod_mx(x, hq, hs, L, C, self.eps, mode=1, tab=tab, shift_off=3 * C, scale_off=4 * C, tid=tid)
            mid = torch.empty(L, F, dtype=BF16, device=dev)
            _lib.gemm_mxfp8(hq, hs, p0.w, p0.s, p0.b, mid, EPI_GELU_BF16, M=L)
            mq, ms = torch.empty(L, F, dtype=u8, device=dev), torch.empty(L, F // 32, dtype=u8, device=dev)
            _lib.mx_quant(mid, mq, ms)
            _lib.gemm_mxfp8(mq, ms, p2.w, p2.s, p2.b, x, EPI_GATE_RESID_F32, M=L, gate=tab[:, 5 * C:], gate_tid=tid)
            return
        _lib.layernorm_mod(x, h, L, C, self.eps, mode=1, tab=tab, shift_off=3 * C, scale_off=4 * C, tid=tid)
        h_full = _slotted(h_full, C, self._slots["ffn0"], L, Ls, s0)
        mid = _act_buf(Lf, self.ffn_dim, (self._slots["ffn2"],), dev)
        _lib.gemm_bf16(h_full, self._prep["ffn0"].w, self._prep["ffn0"].b, mid, EPI_GELU_BF16, M=Lf)
        # ffn.2's leftover rows (1 120 of 22 880) as one round of 256 x 256 tiles x split-K 4 where the library has that strip for the
        # shape (K >= 8192): it needs scratch for the partial tiles (63 MB at this shape; the allocator hands every block the same one)
        mid = _slotted(mid, self.ffn_dim, self._slots["ffn2"], L, Ls, s0)
        nws = _splitk_ws_bytes(L, C, self._prep["ffn2"].w.shape[1], dev)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
        _lib.gemm_bf16(mid, self._prep["ffn2"].w, self._prep["ffn2"].b, x, EPI_GATE_RESID_F32, M=L,
                       gate=tab[:, 5 * C:], gate_tid=tid, ws=ws)

    def forward(self, x, e, seq_lens, grid_sizes, freqs, context, context_lens=None):
        """Reference signature (model.py:219-259): x [B, L, C], e [B, L, 6, C] fp32 -> [B, L, C] fp32.
        Every token carries its own modulation row here (the general case the reference materialises)."""
        assert e.dtype == torch.float32
        _ensure_prepared(self)
        fr = _freqs_device(freqs, x.device)
        outs = []
        for b in range(x.size(0)):
            L = x.size(1)
            if int(seq_lens[b]) != L:
                raise NotImplementedError("padded sequences: call WanModel.forward, which strips the padding")
            xb = x[b].float().contiguous().clone()
            tid = torch.arange(L, dtype=torch.int32, device=x.device)
            self._run(xb, L, e[b].reshape(L, -1).contiguous(), tid, tuple(int(v) for v in grid_sizes[b]), fr,
                      context[b].to(BF16).contiguous(), first_block=(x.dtype == BF16), s0=b)
            outs.append(xb)
        return torch.stack(outs)


class Head(nn.Module):
    def __init__(self, dim, out_dim, patch_size, eps=1e-6):
        super().__init__()
        self.dim, self.out_dim, self.patch_size, self.eps = dim, out_dim, patch_size, eps
        self.norm = WanLayerNorm(dim, eps)
        self.head = nn.Linear(dim, math.prod(patch_size) * out_dim)
        self.modulation = nn.Parameter(torch.randn(1, 2, dim) / dim ** 0.5)

    def _run(self, x, L, e_rows, tid):
        """fp32 island (model.py:286-290): LN -> modulate -> Linear, all fp32. Returns [L, P*Cout] fp32."""
        C = self.dim
        dev = x.device
        n_t = e_rows.shape[0]
        tab = torch.empty(n_t, 2 * C, dtype=torch.float32, device=dev)
        e2 = e_rows.repeat(1, 2).contiguous()       # e.unsqueeze(2) broadcast over the 2 modulation rows
        _lib.add_rows(self.modulation, e2, tab)
        hh = torch.empty(L, C, dtype=torch.float32, device=dev)
        _lib.layernorm_mod(x, hh, L, C, self.eps, mode=1, tab=tab, shift_off=0, scale_off=C, tid=tid)
        out = torch.empty(L, self.head.out_features, dtype=torch.float32, device=dev)
        _lib.gemm_f32(hh, self.head.weight, self.head.bias, out, M=L)
        return out


_zero_cache = {}     # (tag, device, stream) -> (V^T scratch, its last user (batch, L, data pointer)): _vt_scratch


_ncu = {}


_ws_bytes = {}
SPLITK_STRIP = False     # opt-in (bench.py --splitk-strip): ffn.2's leftover rows as one round of 256 x 256 tiles x split-K 4 (uv_gemm_bf16_nt_ws).
# OFF by default: measured -0.35 ... -0.5 ms of a 251 ms step (round 6), and it ends the property every other schedule of the GEMM keeps - a row's
# bits do not depend on which rows it is launched with - so the stacked CFG pair would no longer be bit-identical to two batch-1 forwards


def _splitk_ws_bytes(M, N, K, dev):
    if not SPLITK_STRIP:
        return 0
    key = (M, N, K, str(dev))
    n = _ws_bytes.get(key)
    if n is None:
        n = _ws_bytes[key] = _lib.gemm_splitk_ws_bytes(M, N, K, dev)
    return n


def _ffn0_rows(L, n_cols, dev):
    """Rows to run the first FFN projection on: L, or L rounded up to 256 when the padded row tile does not add a round of 256 x 256 tiles."""
    Lp = _round_up(L, 256)
    if Lp == L or n_cols % 256:
        return L
    ncu = _ncu.get(dev)
    if ncu is None:
        ncu = _ncu[dev] = max(8, torch.cuda.get_device_properties(dev).multi_processor_count & ~7)
    tn = n_cols // 256
    full, padded = (L // 256) * tn, (Lp // 256) * tn
    return Lp if full >= 2 * ncu and -(-padded // ncu) == -(-full // ncu) else L


def _vt_scratch(tag, C, batch, L, device):
    """V^T [C, _lib.vt_cols(batch, L)]: sample b's keys are columns [b*L, (b+1)*L); the tail [batch*L, columns) up to the 64-key tile
    bound is zero. The attention kernels mask the scores of those columns to -inf (P = 0 exactly), so the contract they need is only
    that the tail is FINITE (0 * NaN would poison the row); it is kept zero here: different (batch, L) pairs can give the same
    column count, and then the previous user's V values would sit in the new user's tail - it is re-zeroed on such a change.
    One tensor per key: a new shape replaces the old one (the caching allocator frees it in stream order), so the cache does not grow
    with the resolutions served."""
    if batch > 1 and L % 8:
        raise NotImplementedError(f"stacked samples need a token count divisible by 8 (got {L}); run them one by one")
    cols = _lib.vt_cols(batch, L)
    # one scratch per stream: forwards running concurrently on different streams must not share it
    key = (tag, device, torch.cuda.current_stream(device).cuda_stream)
    t, user = _zero_cache.get(key, (None, None))
    # (a scratch created under torch.inference_mode() cannot be re-zeroed in place outside it - e.g. by a HIP-graph capture, which runs
    # outside inference mode -: such a tensor is replaced)
    if t is None or tuple(t.shape) != (C, cols) or (t.is_inference() and not torch.is_inference_mode_enabled()):
        t = torch.zeros(C, cols, dtype=BF16, device=device)
    if user not in (None, (batch, L, t.data_ptr())) and cols > batch * L:
        t[:, batch * L:].zero_()
    _zero_cache[key] = (t, (batch, L, t.data_ptr()))
    return t


def _mx_scratch(tag, shape, device, dtype=torch.uint8):
    """uint8 scratch of the MXFP8 V^T (codes / scales of attn_precision "mxfp8_qk_pv"): stable per (tag, device, stream) like _vt_scratch, so
    a captured graph keeps reading and writing the same memory; never zeroed (uv_vt_mx_quant writes every byte the attention reads). Also
    the pooled operands and lists of a TopKBlockMask (fp32 / int32; their kernels write everything the next one reads)."""
    key = (tag, device, torch.cuda.current_stream(device).cuda_stream)
    t, _ = _zero_cache.get(key, (None, None))
    if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or (t.is_inference() and not torch.is_inference_mode_enabled()):
        t = torch.empty(shape, dtype=dtype, device=device)
    _zero_cache[key] = (t, None)
    return t


def scratch_snapshot():
    """Identity of every per-stream scratch tensor (before a HIP-graph capture)."""
    return {k: id(t) for k, (t, _) in _zero_cache.items()}


def scratch_take_new(snapshot):
    """Removes - and returns, for the caller to keep alive - the scratch tensors created since `snapshot`: those of a HIP-graph capture
    live in that graph's private memory pool, and torch's capture stream (part of their cache key) is shared by all captures."""
    taken = []
    for k in list(_zero_cache):
        if snapshot.get(k) != id(_zero_cache[k][0]):
            taken.append(_zero_cache.pop(k)[0])
    return taken


def tensor_version(u):
    """`u._version`, or -1 for a tensor created under torch.inference_mode() (no version counter; such a tensor cannot be written
    in place outside inference mode, and inside a `context_cached()` scope the caller vouches for it)."""
    try:
        return u._version
    except RuntimeError:
        return -1


def _ensure_prepared(mod):
    if getattr(mod, "_prep", None) is None:
        mod.prepare()


def _freqs_device(freqs, device):
    """complex128 [1024, D/2] -> float64 [1024, D/2, 2] on the device (cached on the tensor object)."""
    cached = getattr(freqs, "_uv_dev", None)
    if cached is not None and cached.device == device:
        return cached
    fr = torch.view_as_real(freqs.to(torch.complex128)).contiguous().to(device)
    try:
        freqs._uv_dev = fr
    except Exception:
        pass
    return fr


class WanModel(nn.Module):
    """Wan diffusion backbone (reference WanModel, model.py:294-546), HIP-backed."""

    def __init__(self, model_type="t2v", patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=2048, ffn_dim=8192,
                 freq_dim=256, text_dim=4096, out_dim=16, num_heads=16, num_layers=32, window_size=(-1, -1), qk_norm=True,
                 cross_attn_norm=True, eps=1e-6):
        super().__init__()
        assert model_type in ["t2v", "i2v", "ti2v", "s2v"]
        self.model_type = model_type
        self.patch_size = tuple(patch_size)
        self.text_len, self.in_dim, self.dim, self.ffn_dim = text_len, in_dim, dim, ffn_dim
        self.freq_dim, self.text_dim, self.out_dim = freq_dim, text_dim, out_dim
        self.num_heads, self.num_layers = num_heads, num_layers
        self.attn_window = validate_modes({"attn_window": window_size}, dim=dim, ffn_dim=ffn_dim, head_dim=dim // num_heads,
                                          num_heads=num_heads)["attn_window"]     # None = global attention; set_attn_window
        window_size = self.attn_window or (-1, -1)
        self.window_size, self.qk_norm, self.cross_attn_norm, self.eps = window_size, qk_norm, cross_attn_norm, eps
        self.config = dict(model_type=model_type, patch_size=self.patch_size, text_len=text_len, in_dim=in_dim, dim=dim,
                           ffn_dim=ffn_dim, freq_dim=freq_dim, text_dim=text_dim, out_dim=out_dim, num_heads=num_heads,
                           num_layers=num_layers, window_size=window_size, qk_norm=qk_norm,
                           cross_attn_norm=cross_attn_norm, eps=eps)

        self.patch_embedding = nn.Conv3d(in_dim, dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.text_embedding = nn.Sequential(nn.Linear(text_dim, dim), nn.GELU(approximate="tanh"), nn.Linear(dim, dim))
        self.time_embedding = nn.Sequential(nn.Linear(freq_dim, dim), nn.SiLU(), nn.Linear(dim, dim))
        self.time_projection = nn.Sequential(nn.SiLU(), nn.Linear(dim, dim * 6))
        self.blocks = nn.ModuleList([
            WanAttentionBlock(dim, ffn_dim, num_heads, window_size, qk_norm, cross_attn_norm, eps)
            for _ in range(num_layers)
        ])
        self.head = Head(dim, out_dim, self.patch_size, eps)

        assert (dim % num_heads) == 0 and (dim // num_heads) % 2 == 0
        d = dim // num_heads
        if d not in (64, 128):
            raise NotImplementedError(f"head_dim {d}: the attention kernel is built for 64 and 128")
        # plain attribute like the reference (model.py:397-405), so .to() does not change its dtype
        with torch.device("cpu"):  # fp64 host table, also when the module is built under torch.device('cuda')
            self.freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)),
                                    rope_params(1024, 2 * (d // 6))], dim=1)
        self._prep = None
        self._ctx_cache = None   # (key, input tensors kept alive, embedded contexts, generation): see _embedded_context
        self._ctx_gen = 0
        # `_prep_gen`: the identity of "the prepared weights" for cache / graph keys, moved on by prepare(), invalidate(), the LoRA manager
        # (and by anybody who assigns to it). Under per-sample adapter weights (set_adapter_weights) it identifies (prepared weights,
        # setting): a setting that comes back under unchanged weights gets its generation - and its captured graph - back
        self._adapter_weights = None
        self._gen_top = 0        # the highest generation handed out
        self._gen_global = 0     # the generation of the global weights (None: not handed out yet)
        self._gen_settings = {}  # per-sample setting -> its generation
        self._gen = 0
        # Step-constant context work (text_embedding, cross-attention K / V^T) computed once per context. OFF for the bare
        # reference-signature forward: the cache key is tensor identity + version counter, which cannot see writes that bypass the
        # counter (`.data` writes, raw-pointer kernels). A sampling loop that OWNS its context tensors for its duration switches it
        # on around the loop: `with model.context_cached(): ...` (WanTI2V.denoise and bench.py do).
        self.cache_context = False
        self.sp = None   # SeqParallel when Ulysses sequence parallelism is enabled (enable_sequence_parallel)
        self._text_weight = None  # (per-sample weights, rows, layers | None): set_text_weight
        self.ffn_precision = "bf16"  # set_ffn_precision
        self.attn_precision = "bf16"  # set_attn_precision
        self.attn_block_mask = None   # set_attn_block_mask: an AttnBlockMask, or None = global attention
        self.proj_precision = "bf16"  # set_proj_precision
        self.dedup_twins = True   # block 0's self-attention half once for samples that enter with identical rows (the CFG pair); A/B switch
        self.register_load_state_dict_post_hook(lambda m, _k: m.invalidate())

    # ---- weight preparation -------------------------------------------------------------------------------
    @property
    def _prep_gen(self):
        return self._gen

    @_prep_gen.setter
    def _prep_gen(self, value):
        # an assignment says "the prepared weights changed": the value belongs to the present per-sample setting, every other generation
        # (the other settings', the global weights') is forgotten
        self._gen = int(value)
        self._gen_top = max(self._gen_top, self._gen)
        self._gen_global, self._gen_settings = None, {}
        if self._adapter_weights is None:
            self._gen_global = self._gen
        else:
            self._gen_settings[self._adapter_weights] = self._gen

    def _new_generation(self):
        """What was prepared, cached or captured so far can never be served again (weights, adapters or their global strengths changed):
        a generation nobody has seen, for the present per-sample setting; every other setting's generation is forgotten."""
        self._prep_gen = self._gen_top + 1

    def generation_alive(self, gen):
        """True while a per-sample setting (or the global weights) that was given generation `gen` can come back and get it again."""
        return gen == self._gen_global or gen in self._gen_settings.values()

    def invalidate(self):
        """Forget the bf16 weight copies (call after changing parameters in place)."""
        self._prep = None
        self._new_generation()
        self._drop_context()
        for b in self.blocks:
            b._prep = None
            b.self_attn._prep = None
            b.cross_attn._prep = None

    def _drop_context(self):
        """Forgets the embedded context and every block's cross-attention K / V^T of it."""
        self._ctx_cache = None
        for b in self.blocks:
            b.cross_attn._kv_cache = {}

    def _apply_modes(self, changes):
        """Every model-level setter. Every guard first: each block validates its OWN settings (its own setters may have set it apart) with
        `changes` laid over them - a model without blocks its own geometry -, and nothing has changed when one refuses. Then every block
        gets the same normalised values (a mask: one resolver, one cache), the model's mirrors follow and invalidate() moves the generation."""
        new = None
        for b in self.blocks:
            new = b._validated(changes if new is None else {k: new[k] for k in changes})
        if new is None:
            new = validate_modes({**{k: getattr(self, k) for k in MODE_DEFAULTS}, **changes}, dim=self.dim, ffn_dim=self.ffn_dim, head_dim=self.dim // self.num_heads,
                                 num_heads=self.num_heads)
        changes = {k: new[k] for k in changes}
        for b in self.blocks:
            b._apply_modes(changes)
        for k, v in changes.items():
            setattr(self, k, v)
        self.window_size = self.config["window_size"] = self.attn_window or (-1, -1)
        self.invalidate()

    def set_ffn_precision(self, mode):
        """Arithmetic of every block's ffn.0 / ffn.2: "bf16" (default; like for like with the reference) or "mxfp8" - OCP MXFP8 operands
        (e4m3 elements, one power-of-two scale per 32 K elements, activations and weights alike) on the block-scaled matrix instructions,
        fp32 accumulate, same fused epilogues: a labelled FAST mode, narrower than the reference's arithmetic (README). In "mxfp8" the
        blocks hold codes + scales instead of the bf16 weight copies of the two projections. Everything else in the block stays bf16.
        Merged LoRA works (weights are re-quantised after invalidate()); an un-merged adapter on ffn.0 / ffn.2 raises NotImplementedError
        here - and attaching one while the mode is "mxfp8" raises in LoRAManager - before any state changes. Calls invalidate(): the
        prepared-weights generation moves on, so captured HIP graphs (WanTI2V) re-capture."""
        self._apply_modes({"ffn_precision": mode})

    def set_attn_precision(self, mode):
        """Arithmetic of S = Q K^T in every block's SELF-attention: "bf16" (default; like for like with the reference) or "mxfp8_qk" - q and k
        leave the RMSNorm + RoPE pass as OCP MXFP8 (e4m3 elements, one power-of-two scale per 32 head-dim elements) and S runs on the
        block-scaled matrix instruction: a labelled, opt-in mode NARROWER than the reference's arithmetic (README). The softmax, P.V, V^T
        and the output stay bf16 / fp32 as before; cross-attention stays bf16; the sequence-parallel forward raises NotImplementedError in
        this mode. "mxfp8_qk_pv": the same q / k, and in addition V^T as MXFP8 along the key axis (uv_vt_mx_quant of the GEMM's bf16 V^T) and
        the softmax weights P as e4m3 codes of P * 2^7, so that O = P V runs on the block-scaled instruction too (uv_flash_attn_mxpv; format
        and its price: include/univid_hip.h, README); refused by the sequence-parallel forward likewise.
        Needs head_dim 128 (ValueError otherwise, before any state changes). Independent of set_ffn_precision; the two combine.
        Calls invalidate(): the prepared-weights generation moves on, so captured HIP graphs (WanTI2V) re-capture."""
        self._apply_modes({"attn_precision": mode})

    def set_attn_window(self, window_size):
        """Sliding-window / causal SELF-attention in every block: window_size = (left, right) as flash-attn's (the reference's
        WanModel(window_size=...), a key of every checkpoint's config.json) - token i of a sample attends tokens max(0, i - left) ..
        min(L - 1, i + right) of the flattened (frame, row, column) sequence, -1 = unbounded on that side, (-1, 0) = causal; None or
        (-1, -1) = global attention (default, UniVid's configuration). Opt-in: it CHANGES the model's function (exactly - the same softmax
        over fewer keys, uv_flash_attn_win_bf16), it is not an approximation of global attention (README). Cross-attention is untouched.
        Needs head_dim 128 and attn_precision "bf16" (NotImplementedError otherwise; set_attn_precision refuses an MXFP8 mode while a
        window is set); the sequence-parallel forward and the reference-signature WanSelfAttention.forward on padded samples raise
        NotImplementedError while a window is set. Independent of ffn_precision / proj_precision and of un-merged LoRA. Every guard runs
        before any state changes. Calls invalidate(): the prepared-weights generation moves on, so captured HIP graphs (WanTI2V) re-capture."""
        self._apply_modes({"attn_window": window_size})

    def set_attn_block_mask(self, spec):
        """Block-sparse SELF-attention in every block (uv_flash_attn_bs_bf16): token i of head h attends token j of its sample iff
        mask[h][i // 128][j // 64], on the flattened (frame, row, column) sequence - the masks of the training-free sparse-attention
        schemes for video DiTs (univid_amd.wan.attention.video_block_mask builds the block cover of a 3-D neighbourhood). spec: None =
        global attention (default); a bool tensor [ceil(L / 128), ceil(L / 64)] or [num_heads, ...] or a _lib.PreparedBlockMask, for ONE
        sequence length (a forward at another L raises); or a callable f(F, H, W, num_heads) -> such a bool mask for the patch grid
        (F, H, W), evaluated and prepared once per distinct grid and cached - in an eager forward: a forward inside a HIP-graph capture
        at a grid that was not prepared raises (WanTI2V's warm-up forward prepares it); or a univid_amd.wan.attention.TopKBlockMask(top_k,
        keep=None): DATA-DEPENDENT lists - per forward, sample, head and 128-query block the top_k key tiles with the highest pooled q.k
        scores, beside the static keep tiles, chosen on the device (uv_attn_pool_qk, uv_attn_bs_select, uv_flash_attn_bs_lists_bf16: no
        host synchronisation, runs inside a captured HIP graph, differs between the cond and uncond samples). Opt-in: it CHANGES the model's function (exactly -
        the same softmax over fewer keys), it is not an approximation of global attention (README). Cross-attention is untouched.
        Needs head_dim 128, attn_precision "bf16" and no window_size (NotImplementedError otherwise; set_attn_precision refuses an MXFP8
        mode and set_attn_window a window while a mask is set); the sequence-parallel forward and the reference-signature
        WanSelfAttention.forward on padded samples raise NotImplementedError while a mask is set. Independent of ffn_precision /
        proj_precision and of un-merged and per-sample LoRA. Every guard runs before any state changes. Calls invalidate(): the
        prepared-weights generation moves on, so captured HIP graphs (WanTI2V) re-capture."""
        self._apply_modes({"attn_block_mask": spec})

    def set_proj_precision(self, mode):
        """Arithmetic of the attention projections of every block: "bf16" (default; like for like with the reference) or "mxfp8" - the
        self-attention q / k / v / o and the cross-attention q / o Linears on OCP MXFP8 operands (uv_gemm_mxfp8_nt and its V^T / sums-of-
        squares entry points), the activations produced as MXFP8 by the LayerNorm + modulation kernel itself (uv_layernorm_mod_mx; the
        attention outputs by one quantise pass): a labelled, opt-in mode NARROWER than the reference's arithmetic (README). The blocks then
        hold codes + scales instead of the bf16 copies of those six weights. Cross-attention k / v (context side, once per generation),
        the attention cores and everything else are untouched. Merged LoRA works (re-quantised after invalidate()); an un-merged adapter
        on a covered projection raises NotImplementedError here - and attaching one in the mode raises in LoRAManager -, un-merged
        adapters on cross_attn.k / v keep working. Needs dim % 256 == 0 (ValueError otherwise). The sequence-parallel forward raises
        NotImplementedError in the mode. Every guard runs before any state changes. Independent of set_ffn_precision and
        set_attn_precision; all combinations are legal. Calls invalidate(): the prepared-weights generation moves on, so cached
        cross-attention K / V^T and captured HIP graphs (WanTI2V) of the other mode can never be replayed."""
        self._apply_modes({"proj_precision": mode})

    def prepare(self):
        """Materialise the bf16 operand copies autocast would create on every call of the reference."""
        dev = self.patch_embedding.weight.device
        if dev.type != "cuda":
            raise _lib.UnividHipError("WanModel.prepare: parameters must be on the GPU (model.to('cuda')) - there is "
                                      "no CPU path in univid_amd")
        _lib.init()
        pe = nn.Linear(1, 1, bias=True)
        pe.weight = nn.Parameter(self.patch_embedding.weight.detach().flatten(1), requires_grad=False)
        pe.bias = nn.Parameter(self.patch_embedding.bias.detach(), requires_grad=False)
        self._new_generation()
        self._prep = {
            "patch": _Prepared(pe, pad_k=64),
            "text0": _Prepared(self.text_embedding[0], pad_k=64),
            "text2": _Prepared(self.text_embedding[2]),
        }
        for b in self.blocks:
            b.prepare()
        return self

    # ---- pieces of forward --------------------------------------------------------------------------------
    def _time_rows(self, tvals):
        """tvals: fp32 [n_t] distinct timesteps -> (e [n_t, C], e0 [n_t, 6C]) fp32 (model.py:462-469)."""
        n_t = tvals.numel()
        dev = tvals.device
        C = self.dim
        emb = torch.empty(n_t, self.freq_dim, dtype=torch.float32, device=dev)
        _lib.sinusoid(tvals, emb)
        te0, te2, tp = self.time_embedding[0], self.time_embedding[2], self.time_projection[1]
        h1 = torch.empty(n_t, C, dtype=torch.float32, device=dev)
        e = torch.empty(n_t, C, dtype=torch.float32, device=dev)
        e0 = torch.empty(n_t, 6 * C, dtype=torch.float32, device=dev)
        _lib.linear_rows(emb, te0.weight, te0.bias, h1)
        _lib.linear_rows(h1, te2.weight, te2.bias, e, act_in=1)
        _lib.linear_rows(e, tp.weight, tp.bias, e0, act_in=1)
        return e, e0

    def embed_context(self, context: List[torch.Tensor]):
        """text_embedding on the zero-padded prompt embeddings (model.py:472-478) -> bf16 [B, text_len, C]."""
        _ensure_prepared(self)
        dev = self.patch_embedding.weight.device
        Kp = self._prep["text0"].w.shape[1]
        outs = []
        for u in context:
            if u.size(0) > self.text_len:
                raise ValueError(f"context has {u.size(0)} rows > text_len {self.text_len}")
            a = torch.zeros(self.text_len, Kp, dtype=BF16, device=dev)
            a[:u.size(0), :u.size(1)] = u.to(device=dev, dtype=BF16)
            h = torch.empty(self.text_len, self.dim, dtype=BF16, device=dev)
            _lib.gemm_bf16(a, self._prep["text0"].w, self._prep["text0"].b, h, EPI_GELU_BF16)
            c = torch.empty(self.text_len, self.dim, dtype=BF16, device=dev)
            _lib.gemm_bf16(h, self._prep["text2"].w, self._prep["text2"].b, c, EPI_BF16)
            outs.append(c)
        return torch.stack(outs)

    @contextlib.contextmanager
    def context_cached(self):
        """Scope in which the caller guarantees that the context tensors it passes are not written behind the version counter
        (a sampling loop over loop-constant prompt embeddings): text_embedding and the blocks' cross-attention K / V^T are then
        computed once per context. The cache is dropped when the outermost scope ends."""
        prev = self.cache_context
        self.cache_context = True
        try:
            yield self
        finally:
            self.cache_context = prev
            if not prev:
                self._drop_context()

    # ---- UniVid's dynamic text weight, native (models/model_pipeline.py:1699-1810) -----------------------------
    def set_text_weight(self, weights=None, text_len=0, layers=None):
        """The per-layer cross-attention hook of UniVid's Wan22ContextWrapper (model_pipeline.py:1742-1810) as model state instead of
        30 re-assigned `forward` closures: in the blocks of `layers` (None = every block; an iterable of block indices = the wrapper's
        `injection_layers`) the first `text_len` rows of sample i's EMBEDDED context are multiplied by bf16(weights[i]) before that
        block's K / V projections - exactly `context * weight_mask` of :1787-1797 - for every forward until the next call.
        weights: one float per sample of the forward's x / context lists (the CFG pair stacked as [cond, uncond] carries the two
        consecutive values of the wrapper's per-forward counter, :1856-1864); None, or all 1.0, switches it off (the hook's own
        `text_weight_multiplier != 1.0` test): the forward is then the plain one, with its cached context K / V^T.
        Because the rest of the forward is untouched, the stacked CFG pair, block 0's shared self-attention half, the fused
        residual epilogue and (WanTI2V.denoise) the HIP-graph replay all stay in use."""
        if weights is not None:
            weights = tuple(float(w) for w in weights)
            if all(w == 1.0 for w in weights) or int(text_len) <= 0:
                weights = None
        self._text_weight = None if weights is None else (weights, int(text_len), None if layers is None else frozenset(int(i) for i in layers))

    # ---- per-sample adapter weights -------------------------------------------------------------------------
    def _attached_adapters(self):
        """{adapter name: its nn.Linear entries} of the un-merged adapters attached to this model (univid_amd/lora.py)."""
        ads = {}
        for m in self.modules():
            for name, ad in (getattr(m, "_uv_lora", None) or {}).items():
                ads.setdefault(name, []).append(ad)
        return ads

    def set_adapter_weights(self, per_sample=None):
        """Strengths of the un-merged adapters PER SAMPLE of the coming forwards, inside one stacked pass: `per_sample` is a list with one
        `{adapter name: weight}` dict per sample of the forward's x / context lists (the CFG pair stacked as [cond, uncond]: a style adapter
        on the conditional branch only is `[{"style": 1.0}, {"style": 0.0}]`; two requests with different adapters share one stacked
        forward). A name absent from a dict takes the adapter's global weight (LoRAManager.set_adapter_weight); weight 0 switches the
        adapter off for that sample: its slot columns are exactly +0 and the sample's bits are those of a model without it. None restores
        the global weights: the launch is then exactly the global one. Everything is validated before any state changes.
        Like set_adapter_weight, a change drops the cached cross-attention K / V^T and the embedded context and moves `_prep_gen` on, so
        HIP-graph runners re-capture - but a setting that was used before (under unchanged adapters and global weights) gets the
        generation it had, so its captured graph is replayed."""
        key = None
        if per_sample is not None:
            ads = self._attached_adapters()
            rows = []
            for i, d in enumerate(per_sample):
                if not isinstance(d, dict):
                    raise TypeError(f"set_adapter_weights: sample {i}: a dict {{adapter name: weight}} is expected, got {type(d).__name__}")
                row = []
                for name, w in d.items():
                    if name not in ads:
                        raise KeyError(f"set_adapter_weights: sample {i}: no un-merged adapter named {name!r} is attached (attached: {sorted(ads)})")
                    w = float(w)
                    if not math.isfinite(w):
                        raise ValueError(f"set_adapter_weights: sample {i}: weight {w} of adapter {name!r} is not finite")
                    row.append((name, w))
                rows.append(tuple(sorted(row)))
            if not rows:
                raise ValueError("set_adapter_weights: an empty list (pass None for the global weights)")
            key = tuple(rows)
        if key == self._adapter_weights:
            return
        self._install_adapter_weights(key)

    def _install_adapter_weights(self, key):
        # the slots' device matrices are re-allocated when the sample count changes: graphs captured on the old ones must not come back
        n_old = max((len(k) for k in self._gen_settings), default=None)
        if key is not None and n_old is not None and len(key) != n_old:
            self._gen_settings = {}
        for name, entries in self._attached_adapters().items():
            for ad in entries:
                ad["per_sample"] = None if key is None else [dict(row).get(name) for row in key]
        self._adapter_weights = key
        for m in self.modules():
            for slot in (getattr(m, "_slots", None) or {}).values():
                if slot is not None:
                    slot.refresh_scale()
        self._drop_context()
        if key is None:
            if self._gen_global is None:
                self._gen_top += 1
                self._gen_global = self._gen_top
            self._gen = self._gen_global
            return
        if key not in self._gen_settings:
            while len(self._gen_settings) >= 16:      # (the oldest setting's graph is re-captured if it ever comes back)
                del self._gen_settings[next(iter(self._gen_settings))]
            self._gen_top += 1
            self._gen_settings[key] = self._gen_top
        self._gen = self._gen_settings[key]

    def adapter_weights(self):
        """The present per-sample setting as set_adapter_weights takes it (None: global weights)."""
        return None if self._adapter_weights is None else [dict(row) for row in self._adapter_weights]

    def _adapter_rows_differ(self):
        """True when the per-sample setting gives two samples different strengths of some attached adapter."""
        key = self._adapter_weights
        if key is None:
            return False
        for name, entries in self._attached_adapters().items():
            ws = [dict(row).get(name, entries[0]["weight"]) for row in key]
            if any(w != ws[0] for w in ws):
                return True
        return False

    def weighted_context(self, ctx_all, idx, tw):
        """Embedded contexts of the samples `idx` stacked [len(idx) * text_len, C] with sample i's first tw[1] rows scaled by bf16(tw[0][i])."""
        weights, n_scaled, _ = tw
        Lc = ctx_all.shape[1]
        out = torch.empty(len(idx) * Lc, self.dim, dtype=BF16, device=ctx_all.device)
        for j, i in enumerate(idx):
            _lib.text_weight_rows(ctx_all[i], out[j * Lc:(j + 1) * Lc], min(n_scaled, Lc) if weights[i] != 1.0 else 0, weights[i])
        return out

    def _embedded_context(self, context):
        """text_embedding of the prompt embeddings, cached across forwards: in a sampling loop the same context tensors come
        back every step (textimage2video.py:380-385), and neither text_embedding (model.py:472-478) nor the blocks'
        cross-attention K / V projections of it (model.py:170-172) depend on the latent or the timestep. The key is the
        identity AND version counter of every input tensor (an in-place edit bumps `_version`; the tensors are kept referenced
        here so their storage cannot be recycled under the key); parameter changes go through invalidate().
        Returns (embedded contexts [B, text_len, C] bf16, generation id or None when caching is off)."""
        if not self.cache_context:
            return self.embed_context(context), None
        key = tuple((u.data_ptr(), tensor_version(u), tuple(u.shape), u.dtype, u.device) for u in context)
        c = self._ctx_cache
        if c is None or c[0] != key:
            self._ctx_gen += 1
            c = self._ctx_cache = (key, list(context), self.embed_context(context), self._ctx_gen)
        return c[2], c[3]

    def _stacks(self, x):
        """True when the samples x run as ONE stacked pass: one shape, and 16-byte aligned per-sample columns in V^T (token count and
        context length % 8 == 0)."""
        pt, ph, pw = self.patch_size
        _, F0, H0, W0 = x[0].shape
        return len({tuple(u.shape) for u in x}) == 1 and ((F0 // pt) * (H0 // ph) * (W0 // pw)) % 8 == 0 and self.text_len % 8 == 0

    def forward(self, x, t, context, seq_len, y=None, *, t_rows=None, context_kv=None, step_cache=None):
        r"""Same contract as the reference (model.py:410-497).

        x: List[Tensor[C_in, F, H, W]] fp32; t: Tensor[B] or Tensor[B, seq_len]; context: List[Tensor[L<=text_len,
        text_dim]]; seq_len: int. Returns List[Tensor[C_out, F, H, W]] float32.

        t_rows (extension, keyword-only): the caller's own table of the DISTINCT timesteps instead of `t`:
        `(tvals fp32 [n_t] on the device, sorted ascending, tid int32 [B*L] token -> row | None when n_t == 1[, same: bool - every
        sample carries the same token -> row map, which lets identical samples share block 0's self-attention half])`. With it the
        forward contains no device -> host round trip (finding the distinct values of a [B, seq_len] tensor needs one), which
        is what makes it capturable in a HIP graph (WanTI2V.denoise builds the table from the sampler's scalar timestep and
        the i2v mask). Only for equal-shape samples (one stacked group).

        context_kv (extension, keyword-only): one `(k bf16 [B*text_len, C], V^T bf16 [C, _lib.vt_cols(B, text_len)])` pair per block - the
        cross-attention K / V^T of the stacked samples' embedded contexts in the CALLER's buffers (WanCrossAttention._context_kv(out=)
        fills them), which this forward's cross-attention launches read. `context` is then not read (None will do), nothing is embedded
        or cached, and set_text_weight is not consulted: the weights are whatever the caller put into the buffers. One stacked group
        only, and no re-assigned cross-attention forward (a closure takes the context, not its K / V^T).

        step_cache (extension, keyword-only): `(state, "compute" | "skip")` with a univid_amd.wan.step_cache.StepCacheState, whose control
        table the caller has set for this step (StepCacheState.advance). "compute": the forward is the plain one - its output is bit-identical
        - and in addition copies the residual stream after the patch embedding (x_in) into the state and, after the last block, updates the
        state's residual r = x_out - x_in and its backward differences (uv_step_cache_update). "skip": neither the context nor any block is
        touched; the stream becomes x_in + the forecast residual (uv_step_cache_apply) and the head and unpatchify run as always. This
        computes a DIFFERENT function of the same weights (README). The caller allocates the state's buffers (StepCacheState.buffers) before
        the first step; this forward only checks them, so nothing is allocated inside a capture. One stacked group only and no sequence parallelism (NotImplementedError otherwise).
        """
        if self.model_type == "i2v":
            assert y is not None
        if context_kv is not None:
            if len(context_kv) != len(self.blocks):
                raise ValueError(f"context_kv: {len(context_kv)} (k, V^T) pair(s) for {len(self.blocks)} block(s)")
            if not self._stacks(x):
                raise ValueError("context_kv= needs samples of one shape (a single stacked group)")
            if any("forward" in b.cross_attn.__dict__ for b in self.blocks):
                raise NotImplementedError("context_kv= with a re-assigned cross_attn.forward: the closure takes the context, not its K / V^T")
        skip = False
        if step_cache is not None:
            sc_state, sc_kind = step_cache
            if sc_kind not in ("compute", "skip"):
                raise ValueError(f'step_cache: the second entry must be "compute" or "skip", got {sc_kind!r}')
            if self.sp is not None and self.sp.size > 1:
                raise NotImplementedError("step_cache= is not built for sequence-parallel forwards (the cache holds the whole residual stream)")
            if not self._stacks(x):
                raise NotImplementedError("step_cache= needs samples of one shape that run as a single stacked group (token count % 8 == 0)")
            skip = sc_kind == "skip"
        aw = self._adapter_weights
        if aw is not None:
            if len(aw) != len(x):
                raise ValueError(f"set_adapter_weights was given {len(aw)} sample(s); this forward has {len(x)} sample(s)")
            if self.sp is not None and self.sp.size > 1 and self._adapter_rows_differ():
                raise NotImplementedError("set_adapter_weights: per-sample adapter weights that differ between the samples are not built for "
                                          "sequence-parallel forwards (equal rows, or the global weights, are)")
        _ensure_prepared(self)
        dev = self.patch_embedding.weight.device
        if y is not None:
            x = [torch.cat([u, v], dim=0) for u, v in zip(x, y)]
        if t_rows is None and t.dim() == 1:  # one timestep per sample (model.py:460-461)
            t = t.view(-1, 1).expand(-1, seq_len)
        ctx_all, ctx_gen = self._embedded_context(context) if (context_kv is None and not skip) else (None, None)
        fr = _freqs_device(self.freqs, dev)
        pt, ph, pw = self.patch_size
        C = self.dim
        # Samples of identical shape run as ONE stacked pass ([B*L, C] rows: every GEMM / norm kernel sees B*L rows, the
        # attention kernel gets a batch dimension). Row-wise kernels and per-(sample, head) attention do not mix samples,
        # so each sample's result is bit-identical to running it alone; the benefit is occupancy (e.g. CFG's cond + uncond
        # pair: 4320 attention workgroups instead of 2 x 2160 on 512 slots) and weight reuse. Mixed shapes run one by one.
        xs_in = [u.to(device=dev, dtype=torch.float32).contiguous() for u in x]
        groups = [list(range(len(xs_in)))] if self._stacks(xs_in) else [[i] for i in range(len(xs_in))]
        outs = [None] * len(xs_in)
        for idx in groups:
            B = len(idx)
            cin, F, H, W = xs_in[idx[0]].shape
            Fp, Hp, Wp = F // pt, H // ph, W // pw
            L = Fp * Hp * Wp
            assert L <= seq_len, "sequence longer than seq_len (model.py:453)"
            # patch embedding: im2col -> GEMM, bf16 result stored as the fp32 residual stream (model.py:448-451)
            Kp = self._prep["patch"].w.shape[1]
            a = torch.empty(B * L, Kp, dtype=BF16, device=dev)
            for j, i in enumerate(idx):
                _lib.patchify(xs_in[i], a[j * L:], self.patch_size)
            # timesteps: distinct values -> rows; token -> row map (padding tokens beyond L are never computed)
            if t_rows is not None:
                if len(groups) != 1:
                    raise ValueError("t_rows= needs samples of one shape (a single stacked group)")
                tvals, tid = t_rows[0], t_rows[1]
                twin_t = tid is None or (len(t_rows) > 2 and bool(t_rows[2]))     # third entry: every sample has the same token -> row map
                if tid is not None and tid.numel() != B * L:
                    raise ValueError(f"t_rows: tid must hold {B * L} token -> row indices, got {tid.numel()}")
            else:
                tb = torch.cat([t[i].to(device=dev, dtype=torch.float32).flatten()[:L] for i in idx])
                tvals, inv = torch.unique(tb, return_inverse=True)          # device -> host sync (sizes the table)
                tid = None if tvals.numel() == 1 else inv.to(torch.int32).contiguous()
                # (i2v: two timesteps per sample - the samples of a twin pair must also agree token by token)
                twin_t = tid is None or (B > 1 and bool(torch.equal(inv.view(B, L), inv[:L].expand(B, L))))
            e_rows, e0_rows = self._time_rows(tvals.contiguous())
            ctx = None if (context_kv is not None or skip) else ctx_all[idx[0]] if B == 1 else torch.cat([ctx_all[i] for i in idx], 0)
            kv_key = None if ctx_gen is None else (ctx_gen, tuple(idx))
            par = self.sp if (self.sp is not None and self.sp.size > 1) else None
            if par is None:
                n, sp_arg = L, None
            else:
                # sequence parallel (distributed/sequence_parallel.py:116-119): this rank keeps tokens [r0, r1) of every sample
                r0, r1 = par.token_range(L)
                n, sp_arg = r1 - r0, (par, L, r0)
                a = torch.cat([a[j * L + r0:j * L + r1] for j in range(B)], 0)
                if tid is not None:
                    tid = torch.cat([tid[j * L + r0:j * L + r1] for j in range(B)], 0).contiguous()
            xs = torch.empty(B * n, C, dtype=torch.float32, device=dev)
            if B * n:
                _lib.gemm_bf16(a, self._prep["patch"].w, self._prep["patch"].b, xs, EPI_F32_FROM_BF16)
            # The CFG pair of a sampling step is the SAME latent under two prompts (textimage2video.py:380-385): until the first
            # cross-attention the two samples' rows are identical, so block 0's self-attention half (LayerNorm, q/k/v, RoPE,
            # attention, o-projection: 1/60 of a step's attention and projection work) is computed once and copied. Per-sample results do
            # not depend on the stacking (tested), so the output is bit-identical. Detected, not assumed: the same tensor object for
            # every sample of the group and the same token -> timestep map in every sample.
            twin = (self.dedup_twins and B > 1 and par is None and all(xs_in[i] is xs_in[idx[0]] for i in idx) and
                    (tid is None or twin_t))
            # UniVid's dynamic text weight (set_text_weight): the hooked blocks read the row-scaled context, and compute their K / V^T
            # of it in this forward (it changes from forward to forward while the schedule runs; the cache holds the plain one)
            tw = self._text_weight if (context_kv is None and not skip) else None
            if tw is not None and len(tw[0]) != len(xs_in):
                raise ValueError(f"set_text_weight was given {len(tw[0])} weight(s); this forward has {len(xs_in)} sample(s)")
            ctx_w = self.weighted_context(ctx_all, idx, tw) if (tw is not None and any(tw[0][i] != 1.0 for i in idx)) else None
            if step_cache is not None:
                sc = sc_state
                if not sc.holds(B * n, C, dev):
                    raise RuntimeError(f"step_cache: the state holds no buffers for a [{B * n}, {C}] stream on {dev}: call "
                                       f"StepCacheState.buffers(rows, C, device) before the first step")
                if skip:      # the forecast residual instead of the block stack
                    _lib.step_cache_apply(xs, sc.d[0], sc.d[1], sc.d[2], sc.ctl, sc.order)
                else:
                    sc.x_in.copy_(xs)
            for li, blk in enumerate(() if skip else self.blocks):
                hooked = ctx_w is not None and (tw[2] is None or li in tw[2])
                if par is None or n:
                    blk._run(xs, n, e0_rows, tid, (Fp, Hp, Wp), fr, ctx_w if hooked else ctx, first_block=(li == 0), batch=B, sp=sp_arg,
                             kv_key=None if hooked else kv_key, twin_rows=(twin and li == 0), s0=idx[0],
                             kv=None if context_kv is None else context_kv[li])
                else:   # a rank without tokens still takes part in the self-attention exchanges
                    blk.self_attn._self_attn_sp(xs.new_empty(0, C).to(BF16), 0, (Fp, Hp, Wp), fr, xs, None, None, B, sp_arg)
            if step_cache is not None and not skip:
                _lib.step_cache_update(xs, sc.x_in, sc.d[0], sc.d[1], sc.d[2], sc.ctl, sc.order)
            yh = self.head._run(xs, B * n, e_rows, tid) if B * n else xs.new_empty(0, self.head.head.out_features)
            for j, i in enumerate(idx):
                out = torch.empty(self.out_dim, Fp * pt, Hp * ph, Wp * pw, dtype=torch.float32, device=dev)
                yj = yh[j * n:(j + 1) * n]
                if par is not None:
                    yj = par.gather_rows(yj, L).contiguous()     # gather_forward (sequence_parallel.py:139)
                _lib.unpatchify(yj, out, (Fp, Hp, Wp), self.patch_size)
                outs[i] = out
        return outs

    def enable_sequence_parallel(self, group=None):
        """Ulysses sequence parallelism over the ranks of `group` (what the reference's `use_sp=True` installs,
        textimage2video.py:106-118): every rank calls forward with the SAME inputs and gets the full outputs; tokens are
        sharded inside (univid_amd/parallel.py: SeqParallel). Pass group=False to switch it off."""
        from ..parallel import SeqParallel
        self.sp = None if group is False else SeqParallel(group)
        return self

    def unpatchify(self, x, grid_sizes):
        """model.py:499-522, for callers that use it directly."""
        outs = []
        pt, ph, pw = self.patch_size
        for u, v in zip(x, grid_sizes.tolist()):
            u = u[:math.prod(v)].float().contiguous()
            out = torch.empty(self.out_dim, v[0] * pt, v[1] * ph, v[2] * pw, dtype=torch.float32, device=u.device)
            _lib.unpatchify(u, out, v, self.patch_size)
            outs.append(out)
        return outs

    def init_weights(self, seed=0):
        """Deterministic synthetic init (there are no checkpoints offline); see univid_amd.detinit."""
        from .. import detinit
        detinit.init_module_(self, seed)
        self.invalidate()
        return self

    @classmethod
    def from_pretrained(cls, checkpoint_dir, subfolder=None, device="cpu"):
        """diffusers-layout directory (config.json + [sharded] safetensors), as the reference's ModelMixin.from_pretrained
        (models/wan/textimage2video.py:103)."""
        from .checkpoint import load_wan_model
        return load_wan_model(checkpoint_dir, device=device, subfolder=subfolder)

    @classmethod
    def from_config(cls, cfg: dict):
        keys = ("model_type", "patch_size", "text_len", "in_dim", "dim", "ffn_dim", "freq_dim", "text_dim", "out_dim",
                "num_heads", "num_layers", "window_size", "qk_norm", "cross_attn_norm", "eps")
        return cls(**{k: cfg[k] for k in keys if k in cfg})
