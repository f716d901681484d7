"""Un-merged LoRA (univid_amd/lora.py, merge=False) measured on the MI355X, one process:

  kernel   uv_lora_down_bf16 alone at the headline rows (M = 2 x 11 440) against the time to stream x once at the HBM rates of
           MI355X_MICROARCH.md (6.29 TB/s measured float4 copy; 8 TB/s spec)
  seg      per-sample adapter weights: uv_lora_down_bf16 against uv_lora_down_seg_bf16 with two segments (the CFG pair), all scales non-zero
           and with the second segment off, at M = 2 x 11 440, K = 3072, R = 64, alternating rounds (`profiles/lora_per_sample_bench.md`)
  block    one TI2V-5B block at M = 2 x 11 440 with a rank-16 adapter on all ten projections: un-merged against the same block with the
           adapter merged, alternating, device events around each run
  swap     a multi-layer TI2V-width model: time to put an adapter in place (load + operand preparation) and the device memory it
           holds, merged load against un-merged attach; time to change only the adapter weight

Writes the numbers as JSON (default profile_out/lora_bench.json) and prints them. `--layers N` sizes the swap model (default 4)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univid_amd import _lib                                                    # noqa: E402
from univid_amd.lora import LoRAManager                                        # noqa: E402
from univid_amd.wan.model import WanAttentionBlock, WanModel, _ensure_prepared, _freqs_device  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
DIM, FFN, HEADS, LC = 3072, 14336, 24, 512
L1, GRID, B = 11440, (13, 22, 40), 2
TARGETS = [f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo"] + ["ffn.0", "ffn.2"]
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def events(fn, iters, rounds):
    """median over `rounds` of (device time of `iters` calls) / iters, in ms; one untimed round first"""
    ts = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ts), min(ts), max(ts)


def write_adapter(path, shapes, r, alpha, seed):
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    t = {}
    for name, (o, i) in shapes.items():
        t[f"base_model.model.{name}.lora_A.weight"] = torch.randn(r, i, generator=g) / i ** 0.5
        t[f"base_model.model.{name}.lora_B.weight"] = torch.randn(o, r, generator=g) * 0.05
    save_file(t, os.path.join(path, "adapter_model.safetensors"))
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(dict(peft_type="LORA", r=r, lora_alpha=alpha, bias="none", use_rslora=False, use_dora=False, fan_in_fan_out=False,
                       target_modules=sorted(shapes)), f)


def target_shapes(prefixes):
    sh = {}
    for pre in prefixes:
        for t in TARGETS:
            sh[pre + t] = (FFN, DIM) if t == "ffn.0" else (DIM, FFN) if t == "ffn.2" else (DIM, DIM)
    return sh


def randomize_(mod, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 1.0 / p.shape[-1] ** 0.5, generator=g)
            elif "norm" in n and n.endswith("weight"):
                p.fill_(1.0)
            else:
                p.normal_(0.0, 0.02, generator=g)


def bench_kernel(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    M = B * L1
    res = []
    for K, R, what in ((DIM, 48, "h -> q/k/v, 3 x rank 16"), (DIM, 16, "att / hq -> one projection, rank 16"), (DIM, 128, "a full 128-rank slot"),
                       (FFN, 16, "mid -> ffn.2, rank 16")):
        buf = torch.empty(M, K + 128, dtype=BF16, device=DEV)
        buf[:, :K] = torch.randn(M, K, device=DEV, generator=g).to(BF16)
        A = (torch.randn(R, K, device=DEV, generator=g) / K ** 0.5).to(BF16)
        s = torch.full((R,), 2.0, device=DEV)
        med, lo, hi = events(lambda: _lib.lora_down(buf, K, A, s), iters=20, rounds=7)
        nbytes = M * K * 2 + M * 128 * 2 + R * K * 2            # x once, the slot written, A once
        row = dict(M=M, K=K, R=R, what=what, us=med * 1e3, us_min=lo * 1e3, us_max=hi * 1e3, bytes=nbytes, GBps=nbytes / med / 1e6,
                   us_at_6p29TBps=nbytes / HBM_MEASURED * 1e6, us_at_8TBps=nbytes / HBM_SPEC * 1e6)
        print(f"lora_down M={M} K={K:5d} R={R:3d} ({what}): {row['us']:.1f} us [{row['us_min']:.1f} .. {row['us_max']:.1f}], "
              f"{row['GBps']:.0f} GB/s; streaming x once: {row['us_at_6p29TBps']:.1f} us at 6.29 TB/s, {row['us_at_8TBps']:.1f} us at 8 TB/s", flush=True)
        res.append(row)
        del buf
    out["kernel"] = res


def bench_seg(out):
    g = torch.Generator(device=DEV).manual_seed(0)
    M, K, R = B * L1, DIM, 64
    buf = torch.empty(M, K + 128, dtype=BF16, device=DEV)
    buf[:, :K] = torch.randn(M, K, device=DEV, generator=g).to(BF16)
    A = (torch.randn(R, K, device=DEV, generator=g) / K ** 0.5).to(BF16)
    s1 = torch.full((R,), 2.0, device=DEV)
    s_on = torch.full((B, R), 2.0, device=DEV)
    s_half = s_on.clone()
    s_half[1] = 0.0
    variants = {"vector": lambda: _lib.lora_down(buf, K, A, s1), "seg_all_on": lambda: _lib.lora_down_seg(buf, K, A, s_on, L1),
                "seg_second_off": lambda: _lib.lora_down_seg(buf, K, A, s_half, L1)}
    ts = {k: [] for k in variants}
    for r in range(10):                     # alternating rounds; the first is warm-up
        for k, fn in variants.items():
            med, _, _ = events(fn, iters=20, rounds=1)
            if r:
                ts[k].append(med * 1e3)
    out["seg"] = {k: dict(M=M, K=K, R=R, us=statistics.median(v), us_min=min(v), us_max=max(v)) for k, v in ts.items()}
    for k, v in out["seg"].items():
        print(f"lora_down {k} M={M} K={K} R={R}: {v['us']:.2f} us [{v['us_min']:.2f} .. {v['us_max']:.2f}]", flush=True)


def bench_block(out, tmp):
    from univid_amd.wan.model import rope_params
    d = DIM // HEADS
    freqs = torch.cat([rope_params(1024, d - 4 * (d // 6)), rope_params(1024, 2 * (d // 6)), rope_params(1024, 2 * (d // 6))], dim=1)
    fr = _freqs_device(freqs, torch.device(DEV))
    write_adapter(os.path.join(tmp, "blk"), target_shapes(["blocks.0."]), 16, 32, 1)
    holders = {}
    for mode in ("base", "merged", "unmerged"):
        with torch.device(DEV):
            h = torch.nn.Module()
            h.blocks = torch.nn.ModuleList([WanAttentionBlock(DIM, FFN, HEADS, cross_attn_norm=True, eps=1e-6)])
        randomize_(h, 7)
        h.eval()
        if mode != "base":
            LoRAManager().load_lora_weights(os.path.join(tmp, "blk"), h, merge=(mode == "merged"))
        h.blocks[0].prepare()
        holders[mode] = h.blocks[0]
    g = torch.Generator(device=DEV).manual_seed(3)
    M = B * L1
    x0 = torch.randn(M, DIM, device=DEV, generator=g)
    e0 = torch.randn(2, 6 * DIM, device=DEV, generator=g) * 0.3
    tid = (torch.arange(M, device=DEV) % L1 >= L1 // 13).to(torch.int32)
    ctx = (torch.randn(B * LC, DIM, device=DEV, generator=g) * 0.5).to(BF16)
    xs = x0.clone()

    def run(blk):
        with torch.no_grad():
            blk._run(xs, L1, e0, tid, GRID, fr, ctx, first_block=False, batch=B)

    outs = {}
    for mode, blk in holders.items():
        xs.copy_(x0)
        n0 = _lib.CALL_COUNT
        run(blk)
        torch.cuda.synchronize()
        outs[mode] = (xs - x0).float().cpu()
        out.setdefault("block", {})[mode + "_launches"] = _lib.CALL_COUNT - n0
    upd = outs["merged"].pow(2).mean().sqrt()
    out["block"]["unmerged_vs_merged_rel_rms_of_update"] = float((outs["unmerged"] - outs["merged"]).pow(2).mean().sqrt() / upd)
    out["block"]["adapter_effect_rel_rms_of_update"] = float((outs["merged"] - outs["base"]).pow(2).mean().sqrt() / upd)
    ts = {m: [] for m in holders}
    for r in range(8):                      # alternating rounds; the first is warm-up
        for mode, blk in holders.items():
            xs.copy_(x0)
            med, _, _ = events(lambda: run(blk), iters=3, rounds=1)
            if r:
                ts[mode].append(med)
    for mode in holders:
        out["block"][mode + "_ms"] = statistics.median(ts[mode])
        out["block"][mode + "_ms_min_max"] = (min(ts[mode]), max(ts[mode]))
    out["block"]["unmerged_over_merged"] = out["block"]["unmerged_ms"] / out["block"]["merged_ms"]
    print("block (M = 2 x 11440, rank 16 on ten projections):", json.dumps(out["block"]), flush=True)


def bench_swap(out, tmp, layers):
    pres = [f"blocks.{i}." for i in range(layers)]
    write_adapter(os.path.join(tmp, "P"), target_shapes(pres), 16, 32, 11)
    write_adapter(os.path.join(tmp, "Q"), target_shapes(pres), 16, 32, 12)
    with torch.device(DEV):
        m = WanModel(model_type="ti2v", patch_size=(1, 2, 2), text_len=LC, in_dim=48, dim=DIM, ffn_dim=FFN, freq_dim=256, text_dim=4096,
                     out_dim=48, num_heads=HEADS, num_layers=layers, cross_attn_norm=True)
    randomize_(m, 5)
    m.eval()

    def ready():
        """every bf16 operand the next forward needs exists"""
        _ensure_prepared(m)
        for blk in m.blocks:
            _ensure_prepared(blk.self_attn)
            _ensure_prepared(blk.cross_attn)
            if blk._prep is None:
                blk._prepare_ffn()
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ready()
        return (time.perf_counter() - t0) * 1e3

    ready()
    res = dict(layers=layers, fp32_parameters=sum(p.numel() for p in m.parameters()))
    mem0 = torch.cuda.memory_allocated()
    mgr = LoRAManager()
    res["merged_load_ms"] = timed(lambda: mgr.load_lora_weights(os.path.join(tmp, "P"), m))
    res["merged_held_MB"] = (torch.cuda.memory_allocated() - mem0) / 2 ** 20
    res["merged_swap_ms"] = timed(lambda: (mgr.unload(), mgr.load_lora_weights(os.path.join(tmp, "Q"), m)))
    res["merged_unload_ms"] = timed(lambda: mgr.unload())
    mem0 = torch.cuda.memory_allocated()
    res["unmerged_attach_ms"] = timed(lambda: mgr.load_lora_weights(os.path.join(tmp, "P"), m, merge=False, name="P"))
    res["unmerged_held_MB"] = (torch.cuda.memory_allocated() - mem0) / 2 ** 20
    res["unmerged_swap_ms"] = timed(lambda: (mgr.unload("P"), mgr.load_lora_weights(os.path.join(tmp, "Q"), m, merge=False, name="Q")))
    res["unmerged_reweight_ms"] = timed(lambda: mgr.set_adapter_weight("Q", 0.5))
    res["unmerged_unload_ms"] = timed(lambda: mgr.unload())
    res["file_read_ms"] = timed(lambda: __import__("univid_amd.lora", fromlist=["read_adapter"]).read_adapter(os.path.join(tmp, "P")))
    out["swap"] = res
    print("swap:", json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profile_out", "lora_bench.json"))
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--only", choices=["kernel", "seg", "block", "swap"], default=None)
    a = ap.parse_args()
    _lib.init()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        if a.only in (None, "kernel"):
            bench_kernel(out)
        if a.only in (None, "seg"):
            bench_seg(out)
        if a.only in (None, "block"):
            bench_block(out, tmp)
        if a.only in (None, "swap"):
            bench_swap(out, tmp, a.layers)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
