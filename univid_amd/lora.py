"""Inference-side LoRA for the HIP DiT: PEFT adapter directories are read and either FOLDED INTO the dense projection weights
(`merge=True`, the default) or ATTACHED UN-MERGED (`merge=False`), the way the reference runs them.

The reference wraps the DiT's `nn.Linear`s (`self_attn.{q,k,v,o}`, `cross_attn.{q,k,v,o}`, `ffn.0`, `ffn.2`) with PEFT
(`LoRAManager`, /root/reference/models/model_pipeline.py:325-835; `inference.py --use_lora`, :198-264) and keeps the adapters
un-merged: y = base(x) + lora_B(lora_A(x)) * scaling (peft==0.17.1, environment.yaml:417; `peft/tuners/lora/layer.py`
`Linear.forward`). The HIP path consumes ONE dense bf16 weight per projection (its GEMM epilogues - GELU, gated residual,
transposed V - are fused behind it), so an adapter is applied the way PEFT's own `merge_and_unload()` applies it
(`Linear.merge` / `get_delta_weight`): W <- W + scaling * (B @ A) on the fp32 master weights, then the bf16 operand copies are
rebuilt (`WanModel.invalidate()`). The merged projection differs from the un-merged one only by bf16 rounding placement (one
rounding of W + dW instead of separate roundings of the two branches); `tests/test_gpu_parity.py::test_lora_adapter_*` gates
it against the un-merged arithmetic restated in `oracle/lora.py`.

Un-merged (`load_lora_weights(dir, model, merge=False, name=..., weight=...)`): the fp32 master weights are never touched and no copy
of them is kept. Each adapted projection's bf16 operand becomes [W | B | 0] and its input buffer carries T = bf16(s o (x A^T)) in a slot
of whole 128-column groups behind its K columns (kernel `uv_lora_down_bf16`, one launch per input: q/k/v of self-attention share one,
k/v of cross-attention share one), so the tuned GEMM kernels and their fused epilogues run unchanged over K + S columns
(`univid_amd/wan/model.py`: `_prepare_group`, `_slotted`). T is rounded to bf16 once like PEFT's `lora_A(x)`, the scale s (lora_alpha / r,
rslora, `rank_pattern` / `alpha_pattern` per module, times the run-time `weight`) is applied in fp32 before that rounding, and base and
low-rank parts are summed in the fp32 accumulator. Several adapters can be attached under different names (their ranks stack in the
slot), `set_adapter_weight` rewrites the scale vector only, `unload(name)` detaches; attaching / detaching re-prepares only the
attention / FFN modules whose projections changed.

Per-sample weights (`set_adapter_weights([{name: weight}, ...])`, `WanTI2V.denoise(..., adapter_weights=)`): one dict per sample of a
stacked forward - the CFG pair's two branches, or requests that share a forward - instead of one strength for all of them. The scale is
then a matrix [samples, R] and the down-projection is `uv_lora_down_seg_bf16`, which looks the scale up per output row; a weight of 0 gives
exact +0 slot columns, so the sample's bits are those of a model without the adapter, and a workgroup whose rows only touch samples
with the adapter off does not read x at all. Each sample is bit-identical to a single-sample forward at those weights set globally.
Which row of the matrix a launch starts at - the index of its first sample among the forward's samples - travels as the `s0` argument of
the block's `_run` and the attention launch methods (a re-assigned `cross_attn.forward` reads it from `WanCrossAttention._s0`, set for
that call only).

On-disk format read here (what `lora_model.save_pretrained(dir)` writes, model_pipeline.py:608-616, and the manual fallback of
:627-640): `adapter_config.json` (r, lora_alpha, use_rslora, use_dora, bias, fan_in_fan_out, target_modules) and
`adapter_model.safetensors` | `adapter_model.bin` | `lora_weights.pt` with keys
`base_model.model.<module path>.lora_A[.default].weight` [r, in] and `...lora_B[.default].weight` [out, r].
Training-side features (applying fresh adapters, gradients, saving) are out of scope.
"""
import json
import math
import os
import re
from typing import Dict, Tuple

import torch
from torch import nn


def read_adapter(load_path) -> Tuple[dict, Dict[str, torch.Tensor]]:
    """(adapter_config dict, raw tensor dict) of a PEFT adapter directory."""
    load_path = str(load_path)
    if not os.path.isdir(load_path):
        raise FileNotFoundError(f"LoRA weights path does not exist: {load_path}")
    cfg = {}
    for name in ("adapter_config.json", "lora_config.json"):       # PEFT's own file first, the reference's side file second
        p = os.path.join(load_path, name)
        if os.path.exists(p):
            with open(p) as f:
                cfg = json.load(f)
            break
    st = os.path.join(load_path, "adapter_model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return cfg, load_file(st)
    for name in ("adapter_model.bin", "lora_weights.pt"):
        p = os.path.join(load_path, name)
        if os.path.exists(p):
            return cfg, torch.load(p, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no adapter_model.safetensors / adapter_model.bin / lora_weights.pt under {load_path}")


_KEY = re.compile(r"^(?:base_model\.model\.)?(?P<mod>.+?)\.lora_(?P<ab>[AB])(?:\.[^.]+)?\.weight$")


def adapter_factors(tensors: Dict[str, torch.Tensor]) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{module path: (A [r, in], B [out, r])} from PEFT state-dict keys (with or without the adapter name)."""
    ab: Dict[str, dict] = {}
    for k, v in tensors.items():
        m = _KEY.match(k)
        if m is None:
            if "lora_" in k:
                raise ValueError(f"unsupported LoRA tensor {k!r} (only lora_A / lora_B weights of Linear layers are handled; "
                                 f"DoRA magnitudes and embedding adapters are not)")
            continue
        ab.setdefault(m.group("mod"), {})[m.group("ab")] = v
    out = {}
    for mod, d in ab.items():
        if "A" not in d or "B" not in d:
            raise ValueError(f"adapter for {mod!r} is missing its lora_{'B' if 'A' in d else 'A'} weight")
        a, b = d["A"], d["B"]
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1]:
            raise ValueError(f"adapter for {mod!r}: lora_A {tuple(a.shape)} and lora_B {tuple(b.shape)} do not form a rank-r pair")
        out[mod] = (a, b)
    return out


def adapter_scaling(cfg: dict, r: int) -> float:
    """peft LoraLayer.update_layer: lora_alpha / r, or lora_alpha / sqrt(r) with use_rslora. The config MUST name lora_alpha: PEFT
    refuses an adapter directory without its config, and guessing alpha (= r, scaling 1) folds the adapter in at the wrong strength."""
    if "lora_alpha" not in cfg and "alpha" not in cfg:
        raise ValueError("the adapter's config (adapter_config.json / lora_config.json) is missing or does not name lora_alpha: "
                         "the merge scaling lora_alpha / r cannot be guessed")
    for pat in ("rank_pattern", "alpha_pattern"):
        if cfg.get(pat):
            raise NotImplementedError(f"adapter config has a non-empty {pat} (per-module rank / alpha): one global scaling would merge "
                                      f"those modules at the wrong strength")
    alpha = cfg.get("lora_alpha", cfg.get("alpha"))
    return alpha / math.sqrt(r) if cfg.get("use_rslora", False) else alpha / r


def _pattern_value(pattern: dict, module: str, default):
    """peft `get_pattern_key`: the first key of a rank_pattern / alpha_pattern that matches the module path as a (regex) suffix."""
    for key, v in (pattern or {}).items():
        if re.match(rf"(.*\.)?({key})$", module):
            return v
    return default


def module_scaling(cfg: dict, module: str, r: int) -> float:
    """Scaling of ONE module (peft LoraLayer.update_layer with the config's rank_pattern / alpha_pattern applied, LoraModel.
    _create_and_replace): lora_alpha / r, or lora_alpha / sqrt(r) with use_rslora, with this module's own alpha and rank."""
    if "lora_alpha" not in cfg and "alpha" not in cfg:
        raise ValueError("the adapter's config (adapter_config.json / lora_config.json) is missing or does not name lora_alpha: "
                         "the scaling lora_alpha / r cannot be guessed")
    want_r = _pattern_value(cfg.get("rank_pattern"), module, cfg.get("r", r))
    if want_r is not None and int(want_r) != r:
        raise ValueError(f"adapter for {module!r} has rank {r}, its config says {want_r}")
    alpha = _pattern_value(cfg.get("alpha_pattern"), module, cfg.get("lora_alpha", cfg.get("alpha")))
    return alpha / math.sqrt(r) if cfg.get("use_rslora", False) else alpha / r


def _refuse_unsupported(cfg: dict, what: str):
    if cfg.get("use_dora", False):
        raise NotImplementedError(f"DoRA adapters (use_dora=True) are not supported: only plain LoRA deltas can be {what}")
    if cfg.get("bias", "none") not in ("none", None):
        raise NotImplementedError(f"LoRA bias mode {cfg.get('bias')!r} is not supported (the reference uses 'none')")


def _owner(model: nn.Module, path: str):
    """The module that prepares the bf16 operand of the nn.Linear at `path` (the nearest ancestor with a `_prep`), or None."""
    parts = path.split(".")
    for n in range(len(parts) - 1, -1, -1):
        m = model.get_submodule(".".join(parts[:n])) if n else model
        if hasattr(m, "_prep") and hasattr(m, "_slots"):
            return m
    return None


def _adapters_changed(model: nn.Module, paths=(), rescale=False):
    """After attach / detach (`paths`: the nn.Linears concerned - only their owners are re-prepared) or a new weight (`rescale`: the
    scale vectors are rewritten in place): whatever was computed with the previous adapters can never be served again - the prepared-
    weights generation (HIP-graph runners key on it) moves on, cached cross-attention K / V^T and the embedded context are dropped."""
    for path in paths:
        own = _owner(model, path)
        if own is not None:
            own._prep = None
    if rescale:
        for m in model.modules():
            for slot in (getattr(m, "_slots", None) or {}).values():
                if slot is not None:
                    slot.refresh_scale()
    if hasattr(model, "_prep_gen"):       # (a WanModel: only its forward fills those caches)
        model._new_generation()
        model._drop_context()


def _check_slots(model: nn.Module):
    """Raises if the adapters now attached stack, on some shared input, to more rank than an activation's slot holds."""
    from .wan.model import LORA_MAX_SLOT
    for mod_name, m in model.named_modules():
        groups = getattr(m, "_groups", None)
        if groups is None and hasattr(m, "ffn") and hasattr(m, "_slots"):
            groups, get = {"ffn.0": (0,), "ffn.2": (2,)}, lambda n: m.ffn[n]
        else:
            get = lambda n: getattr(m, n)
        for g, names in (groups or {}).items():
            R = sum(ad["A"].shape[0] for n in names for ad in getattr(get(n), "_uv_lora", {}).values())
            if -(-R // 128) * 128 > LORA_MAX_SLOT:
                raise ValueError(f"{mod_name}: the adapters on the projections reading one input ({g}) stack to rank {R}; an activation's "
                                 f"slot holds at most {LORA_MAX_SLOT} columns (univid_amd.wan.model.LORA_MAX_SLOT)")


_MX_REFUSAL = {      # attach-time side of the refusals of univid_amd.wan.modes.validate_modes; mx_covered states the Linears
    "ffn_precision": "an un-merged adapter (merge=False) on ffn.0 / ffn.2 cannot be combined with ffn_precision 'mxfp8' (the MXFP8 GEMM "
                     "has no adapter slot). Merge the adapter (merge=True: the merged weights are re-quantised) or call "
                     "set_ffn_precision('bf16') first. Un-merged adapters on the attention projections work in both modes.",
    "proj_precision": "an un-merged adapter (merge=False) on self_attn.q / k / v / o or cross_attn.q / o cannot be combined with "
                      "proj_precision 'mxfp8' (the MXFP8 GEMM has no adapter slot). Merge the adapter (merge=True: the merged weights are "
                      "re-quantised) or call set_proj_precision('bf16') first. Un-merged adapters on cross_attn.k / v work in both modes."}


def attach_adapter_(model: nn.Module, name: str, factors, cfg: dict, weight: float = 1.0):
    """Attaches the adapter UN-MERGED under `name`: every targeted nn.Linear gets its bf16 factors and scaling (`lin._uv_lora[name]`);
    the fp32 weights are not touched. Everything is validated before the first module changes. Returns the module paths."""
    from .wan.modes import mx_covered
    _refuse_unsupported(cfg, "attached")
    if cfg.get("fan_in_fan_out", False):
        raise NotImplementedError("fan_in_fan_out adapters are not supported un-merged (nn.Linear layers never need it)")
    mods = dict(model.named_modules())
    todo = []
    for path, (a, b) in factors.items():
        lin = mods.get(path)
        if not isinstance(lin, nn.Linear):
            raise KeyError(f"adapter targets {path!r}, which is not an nn.Linear of this model")
        if tuple(lin.weight.shape) != (b.shape[0], a.shape[1]):
            raise ValueError(f"adapter for {path!r} is {b.shape[0]} x {a.shape[1]}, the layer is {tuple(lin.weight.shape)}")
        if _owner(model, path) is None:
            raise NotImplementedError(f"{path!r} is not a projection of the DiT blocks (self_attn / cross_attn q, k, v, o, ffn.0, ffn.2): "
                                      f"only those run un-merged")
        if name in getattr(lin, "_uv_lora", {}):
            raise RuntimeError(f"an adapter named {name!r} is already attached to {path!r}")
        own = _owner(model, path)
        for mode, covered in mx_covered(own).items():       # an MXFP8 GEMM mode that is on refuses an adapter on a Linear it covers
            if getattr(own, mode, "bf16") == "mxfp8" and any(lin is c for c in covered):
                raise NotImplementedError(f"{path!r}: " + _MX_REFUSAL[mode])
        todo.append((path, lin, a, b, module_scaling(cfg, path, a.shape[0])))
    for path, lin, a, b, s in todo:
        dev = lin.weight.device
        if not hasattr(lin, "_uv_lora"):
            lin._uv_lora = {}
        lin._uv_lora[name] = {"A": a.detach().to(dev, torch.bfloat16).contiguous(), "B": b.detach().to(dev, torch.bfloat16).contiguous(),
                              "scaling": float(s), "weight": float(weight)}
    try:
        _check_slots(model)
    except ValueError:
        for _, lin, *_ in todo:
            del lin._uv_lora[name]
        raise
    _adapters_changed(model, [t[0] for t in todo])
    return sorted(t[0] for t in todo)


def detach_adapter_(model: nn.Module, name=None):
    """Removes the un-merged adapter `name` (None: every one) from the model's nn.Linears."""
    paths = []
    for path, lin in model.named_modules():
        ads = getattr(lin, "_uv_lora", None)
        if ads and (name is None or name in ads):
            if name is None:
                ads.clear()
            else:
                del ads[name]
            paths.append(path)
    _adapters_changed(model, paths)
    return paths


def merge_adapter_(model: nn.Module, factors, cfg: dict):
    """W += scaling * (B @ A) on the fp32 master weight of every targeted nn.Linear (peft Linear.get_delta_weight).
    Returns {module path: original weight clone} so that the merge can be undone bit-exactly."""
    if cfg.get("use_dora", False):
        raise NotImplementedError("DoRA adapters (use_dora=True) are not supported: only plain LoRA deltas can be folded in")
    if cfg.get("bias", "none") not in ("none", None):
        raise NotImplementedError(f"LoRA bias mode {cfg.get('bias')!r} is not supported (the reference uses 'none')")
    mods = dict(model.named_modules())
    saved = {}
    # validate EVERY (module, shape, scaling) before the first weight is touched: an error must not leave a half-merged model
    for name, (a, b) in factors.items():
        lin = mods.get(name)
        if not isinstance(lin, nn.Linear):
            raise KeyError(f"adapter targets {name!r}, which is not an nn.Linear of this model")
        if tuple(lin.weight.shape) != (b.shape[0], a.shape[1]):
            raise ValueError(f"adapter for {name!r} is {b.shape[0]} x {a.shape[1]}, the layer is {tuple(lin.weight.shape)}")
        adapter_scaling(cfg, a.shape[0])
    with torch.no_grad():
        for name, (a, b) in factors.items():
            lin = mods[name]
            w = lin.weight
            delta = (b.to(w.device, torch.float32) @ a.to(w.device, torch.float32)) * adapter_scaling(cfg, a.shape[0])
            if cfg.get("fan_in_fan_out", False):
                delta = delta.t()
            saved[name] = w.detach().clone()
            w.add_(delta.to(w.dtype))
    if hasattr(model, "invalidate"):
        model.invalidate()          # bf16 operand copies and the cached context K/V are rebuilt from the merged weights
    return saved


class LoRAManager:
    """Inference half of the reference's LoRAManager (model_pipeline.py:325-835): `load_lora_weights(path, model)` and
    `merge_and_unload()` with the same names; the adapter is merged at load (see the module docstring), `unload()` restores the
    base weights bit for bit. `apply_lora_to_dit` (fresh trainable adapters) belongs to training and raises."""

    def __init__(self, config=None, logger=None):
        self.config = config
        self.logger = logger
        self.lora_model = None
        self.original_model = None
        self.lora_config = None
        self.applied_modules = []
        self._saved = {}
        self.attached = {}       # un-merged adapters: name -> (module paths, adapter config), in attach order

    def apply_lora_to_dit(self, dit_model):
        raise NotImplementedError("applying fresh (trainable) LoRA adapters is training-side (SURVEY.md section 2, row 15); "
                                  "for inference call load_lora_weights(adapter_dir, model)")

    def load_lora_weights(self, load_path, model, merge=True, name="default", weight=1.0):
        """model_pipeline.py:724-750. merge=True: returns the model with the adapter folded in. merge=False: the adapter is attached
        un-merged under `name` at strength `weight` (module docstring); more can follow under other names. Errors raise (the reference
        logs them and returns the un-adapted model, which silently generates with the wrong weights)."""
        if not merge:
            return self._attach(load_path, model, name, weight)
        if self.attached:
            raise RuntimeError(f"un-merged adapter(s) {sorted(self.attached)} are attached to this model: call unload() first")
        if self._saved:
            raise RuntimeError("an adapter is already merged into this model: call unload() first")
        cfg, tensors = read_adapter(load_path)
        factors = adapter_factors(tensors)
        if not factors:
            raise ValueError(f"no lora_A / lora_B tensors found under {load_path}")
        self._saved = merge_adapter_(model, factors, cfg)
        self.lora_config = cfg
        self.applied_modules = sorted(factors)
        self.original_model = self.lora_model = model
        if self.logger is not None:
            r = next(iter(factors.values()))[0].shape[0]
            self.logger.info(f"LoRA adapter merged from {load_path}: {len(factors)} layers, rank {r}, "
                             f"scaling {adapter_scaling(cfg, r):g}")
        return model

    def _attach(self, load_path, model, name, weight):
        if self._saved:
            raise RuntimeError("an adapter is merged into this model: call unload() before attaching one un-merged")
        if self.attached and model is not self.lora_model:
            raise RuntimeError("this manager already holds un-merged adapters of another model")
        if name in self.attached:
            raise RuntimeError(f"an adapter named {name!r} is already attached: unload({name!r}) first, or pick another name")
        cfg, tensors = read_adapter(load_path)
        factors = adapter_factors(tensors)
        if not factors:
            raise ValueError(f"no lora_A / lora_B tensors found under {load_path}")
        paths = attach_adapter_(model, name, factors, cfg, weight)
        self.attached[name] = (paths, cfg)
        self.lora_config = cfg
        self.applied_modules = sorted({p for ps, _ in self.attached.values() for p in ps})
        self.original_model = self.lora_model = model
        if self.logger is not None:
            self.logger.info(f"LoRA adapter {name!r} attached un-merged from {load_path}: {len(paths)} layers, weight {weight:g}")
        return model

    def set_adapter_weight(self, name, weight):
        """Run-time strength of the un-merged adapter `name`: only the scale vectors of the down-projections change."""
        if name not in self.attached:
            raise KeyError(f"no un-merged adapter named {name!r} (attached: {sorted(self.attached)})")
        for lin in self.lora_model.modules():
            ad = getattr(lin, "_uv_lora", {}).get(name)
            if ad is not None:
                ad["weight"] = float(weight)
        _adapters_changed(self.lora_model, rescale=True)

    def set_adapter_weights(self, per_sample=None):
        """Per-sample strengths inside one stacked forward: a list with one {adapter name: weight} dict per sample of the coming forwards
        (names left out keep their global weight), or None for the global weights again (WanModel.set_adapter_weights)."""
        if self.lora_model is None or not self.attached:
            if per_sample is None:
                return
            raise RuntimeError("no un-merged adapter is attached: load one with load_lora_weights(dir, model, merge=False)")
        if per_sample is not None:
            for d in per_sample:
                for name in (d if isinstance(d, dict) else ()):
                    if name not in self.attached:
                        raise KeyError(f"no un-merged adapter named {name!r} (attached: {sorted(self.attached)})")
        self.lora_model.set_adapter_weights(per_sample)

    def merge_and_unload(self):
        """model_pipeline.py:752-764: the adapter is already merged; the dense model is returned and the saved base weights dropped."""
        if self.lora_model is None:
            raise RuntimeError("no LoRA model to merge")
        if self.attached:
            raise RuntimeError("un-merged adapters are attached: load the adapter with merge=True to fold it in")
        self._saved = {}
        return self.lora_model

    def unload(self, name=None):
        """Merged: restores the base weights saved at load (bit for bit) and rebuilds the bf16 operands. Un-merged: detaches the adapter
        `name` (None: all of them)."""
        if self.lora_model is None:
            return None
        if self.attached:
            if name is not None and name not in self.attached:
                raise KeyError(f"no un-merged adapter named {name!r} (attached: {sorted(self.attached)})")
            # per-sample weights that name an adapter which goes away go with it
            ps = self.lora_model.adapter_weights() if hasattr(self.lora_model, "adapter_weights") else None
            if ps is not None and (name is None or any(name in d for d in ps)):
                self.lora_model.set_adapter_weights(None)
            detach_adapter_(self.lora_model, name)
            for n in ([name] if name is not None else list(self.attached)):
                del self.attached[n]
            self.applied_modules = sorted({p for ps, _ in self.attached.values() for p in ps})
            model = self.lora_model
            if not self.attached:
                self.lora_model = None
            return model
        mods = dict(self.lora_model.named_modules())
        with torch.no_grad():
            for name, w in self._saved.items():
                mods[name].weight.copy_(w)
        self._saved = {}
        if hasattr(self.lora_model, "invalidate"):
            self.lora_model.invalidate()
        model, self.lora_model, self.applied_modules = self.lora_model, None, []
        return model

    def get_statistics(self):
        """model_pipeline.py:766-800 (the fields that exist without trainable parameters)."""
        if self.lora_model is None:
            return {}
        m = self.applied_modules
        return {
            "mode": "unmerged" if self.attached else "merged",
            "adapters": list(self.attached),
            "per_sample": bool(self.attached) and getattr(self.lora_model, "adapter_weights", lambda: None)() is not None,
            "lora_modules": len(m),
            "module_breakdown": {"cross_attention": sum("cross_attn" in x for x in m), "self_attention": sum("self_attn" in x for x in m),
                                 "ffn": sum("ffn" in x for x in m), "total": len(m)},
            "lora_config": {"rank": self.lora_config.get("r"), "alpha": self.lora_config.get("lora_alpha"),
                            "use_rslora": self.lora_config.get("use_rslora", False), "use_dora": self.lora_config.get("use_dora", False)},
        }
