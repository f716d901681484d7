"""GEMM micro-benchmark on the DiT's shapes: every tile config, interleaved rounds in ONE process, random operands.

    python tools/gemm_bench.py [--cfgs 0,5,6,7] [--rounds 5] [--check]
    python tools/gemm_bench.py --mxproj      the attention projections' shape (N = K = 3072 at 22 880 and 11 440 rows), bf16 against MXFP8, per epilogue
    python tools/gemm_bench.py --mx          the two FFN shapes, bf16 (tile_cfg 0) against MXFP8 (uv_gemm_mxfp8_nt), quantise passes included

Prints median/min TFLOP/s per (shape, config). `--check` compares each config with an fp64 reference on a row sample.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univid_amd import _lib  # noqa: E402
from univid_amd._lib import EPI_BF16, EPI_GELU_BF16, EPI_GATE_RESID_F32, EPI_BF16_T, EPI_F32_FROM_BF16, EPI_RESID_F32  # noqa: E402

L2 = 22880  # cond+uncond stacked tokens at 704x1280x49 (2 x 11440)
SHAPES = [
    ("q/k (bf16)", L2, 3072, 3072, EPI_BF16),
    ("v (bf16^T)", L2, 3072, 3072, EPI_BF16_T),
    ("o (gate+resid f32)", L2, 3072, 3072, EPI_GATE_RESID_F32),
    ("ffn.0 (gelu)", L2, 14336, 3072, EPI_GELU_BF16),
    ("ffn.2 (gate+resid f32)", L2, 3072, 14336, EPI_GATE_RESID_F32),
    ("single sample q", 11440, 3072, 3072, EPI_BF16),
    ("ctx k/v", 1024, 3072, 3072, EPI_BF16),
    ("ffn.0 without gelu", L2, 14336, 3072, EPI_BF16),
    ("tail strip K=3072", 1120, 3072, 3072, EPI_BF16),
    ("tail strip K=14336", 1120, 3072, 14336, EPI_GATE_RESID_F32),
    ("o-shape, f32 write only", L2, 3072, 3072, EPI_F32_FROM_BF16),
    ("o-shape, f32 resid", L2, 3072, 3072, EPI_RESID_F32),
    ("8192^3", 8192, 8192, 8192, EPI_BF16),
    ("aligned q (89 x 256 rows)", 22784, 3072, 3072, EPI_BF16),
    ("aligned ffn.0 shape", 22784, 14336, 3072, EPI_BF16),
    ("aligned ffn.2 shape", 22784, 3072, 14336, EPI_BF16),
    ("ranker q/k/v/o (64 x 256 tokens)", 16384, 768, 768, EPI_BF16),
    ("ranker fc1", 16384, 3072, 768, EPI_GELU_BF16),
    ("ranker fc2", 16384, 768, 3072, EPI_BF16),
    ("q+k as ONE N=6144 launch", L2, 6144, 3072, EPI_BF16),       # measured 652-654 us against 2 x 327.7 us (shape 0): no gain
    ("q+k+v-sized N=9216 launch", L2, 9216, 3072, EPI_BF16),      # 960 us against 3 x 327.7 (-2.4 %; the V third would need the transposed epilogue)
    ("aligned ffn.0 shape, GELU", 22784, 14336, 3072, EPI_GELU_BF16),   # against shape 14 (plain bf16 epilogue): the GELU epilogue's surcharge
    ("ranker q+k+v as ONE N=2304 launch", 16384, 2304, 768, EPI_BF16),  # round 6, against 3 x shape 16: 576 tiles (2.25 rounds) against 3 x 192 (3 x 0.75)
]


def _median_us(fn, rounds, iters):
    ts = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1) / iters * 1e3)
    return statistics.median(ts)


def bench_mx(rounds, iters):
    """ffn.0 (GELU) and ffn.2 (gated residual) at the CFG pair's 22 880 rows: the bf16 path (tile_cfg 0) against the MXFP8 path, whose
    activation-quantise passes (uv_mx_quant_bf16 of ffn.0's input and of `mid`) are timed separately and counted into the pair time.
    Random operands; one process, the variants interleaved per round by _median_us's caller order."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    M, C, F = L2, 3072, 14336
    u8 = torch.uint8
    h = (torch.rand(M, C, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
    w0 = ((torch.rand(F, C, device=dev, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
    w2 = ((torch.rand(C, F, device=dev, generator=g) * 2 - 1) * 0.02).to(torch.bfloat16)
    b0 = (torch.rand(F, device=dev, generator=g) - 0.5).to(torch.bfloat16)
    b2 = (torch.rand(C, device=dev, generator=g) - 0.5).to(torch.bfloat16)
    x = torch.rand(M, C, device=dev, generator=g)
    gate = torch.rand(2, C, device=dev, generator=g)
    tid = (torch.arange(M, device=dev) * 2 // M).to(torch.int32)
    mid = torch.zeros(M, F, device=dev, dtype=torch.bfloat16)
    q = {n: (torch.empty(t.shape, dtype=u8, device=dev), torch.empty(t.shape[0], t.shape[1] // 32, dtype=u8, device=dev))
         for n, t in (("h", h), ("mid", mid), ("w0", w0), ("w2", w2))}
    _lib.mx_quant(w0, *q["w0"])
    _lib.mx_quant(w2, *q["w2"])
    steps = {
        "bf16 ffn.0 (gelu)": (lambda: _lib.gemm_bf16(h, w0, b0, mid, EPI_GELU_BF16), 2.0 * M * F * C),
        "bf16 ffn.2 (gate+resid)": (lambda: _lib.gemm_bf16(mid, w2, b2, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid), 2.0 * M * F * C),
        "mx quant h [22880 x 3072]": (lambda: _lib.mx_quant(h, *q["h"]), 0),
        "mxfp8 ffn.0 (gelu)": (lambda: _lib.gemm_mxfp8(*q["h"], *q["w0"], b0, mid, EPI_GELU_BF16), 2.0 * M * F * C),
        "mx quant mid [22880 x 14336]": (lambda: _lib.mx_quant(mid, *q["mid"]), 0),
        "mxfp8 ffn.2 (gate+resid)": (lambda: _lib.gemm_mxfp8(*q["mid"], *q["w2"], b2, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid), 2.0 * M * F * C),
    }
    us = {}
    for name, (fn, fl) in steps.items():
        us[name] = _median_us(fn, rounds, iters)
        print(f"{name:30s} {us[name]:8.1f} us" + (f"  {fl / us[name] / 1e6:7.1f} TF/s" if fl else ""), flush=True)
    bf = us["bf16 ffn.0 (gelu)"] + us["bf16 ffn.2 (gate+resid)"]
    mx = sum(v for k, v in us.items() if k.startswith("mx"))
    print(f"pair: bf16 {bf:.1f} us, mxfp8 incl. both quantise passes {mx:.1f} us, ratio bf16 / mxfp8 = {bf / mx:.3f}", flush=True)


def bench_mxproj(rounds, iters):
    """The attention projections (N = K = 3072) at the CFG pair's 22 880 rows and one sample's 11 440: uv_gemm_bf16_nt (tile_cfg 0) /
    uv_gemm_bf16_nt_ssq against uv_gemm_mxfp8_nt / _t / _ssq on pre-quantised operands, per epilogue - BF16 (q / k), T (v), SSQ (cross q),
    GATE_RESID (o). Random operands; one process, bf16 and MXFP8 of an epilogue back to back."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    C, u8, bf = 3072, torch.uint8, torch.bfloat16
    for M in (L2, L2 // 2):
        a = (torch.rand(M, C, device=dev, generator=g) * 2 - 1).to(bf)
        w = ((torch.rand(C, C, device=dev, generator=g) * 2 - 1) * 0.05).to(bf)
        bias = (torch.rand(C, device=dev, generator=g) - 0.5).to(bf)
        ac, asc = torch.empty(M, C, dtype=u8, device=dev), torch.empty(M, C // 32, dtype=u8, device=dev)
        wc, wsc = torch.empty(C, C, dtype=u8, device=dev), torch.empty(C, C // 32, dtype=u8, device=dev)
        _lib.mx_quant(a, ac, asc)
        _lib.mx_quant(w, wc, wsc)
        out = torch.zeros(M, C, device=dev, dtype=bf)
        out_t = torch.zeros(C, (M + 63) // 64 * 64, device=dev, dtype=bf)
        ssq = torch.zeros(M, C // 32, device=dev)
        x = torch.rand(M, C, device=dev, generator=g)
        gate = torch.rand(2, C, device=dev, generator=g)
        tid = (torch.arange(M, device=dev) * 2 // M).to(torch.int32)
        pairs = {
            "BF16": (lambda: _lib.gemm_bf16(a, w, bias, out, EPI_BF16), lambda: _lib.gemm_mxfp8(ac, asc, wc, wsc, bias, out, EPI_BF16)),
            "T": (lambda: _lib.gemm_bf16(a, w, bias, out_t, EPI_BF16_T), lambda: _lib.gemm_mxfp8_t(ac, asc, wc, wsc, bias, out_t)),
            "SSQ": (lambda: _lib.gemm_bf16_ssq(a, w, bias, out, ssq), lambda: _lib.gemm_mxfp8_ssq(ac, asc, wc, wsc, bias, out, ssq)),
            "GATE_RESID": (lambda: _lib.gemm_bf16(a, w, bias, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid),
                           lambda: _lib.gemm_mxfp8(ac, asc, wc, wsc, bias, x, EPI_GATE_RESID_F32, gate=gate, gate_tid=tid)),
        }
        fl = 2.0 * M * C * C
        for name, (f_bf, f_mx) in pairs.items():
            t_bf, t_mx = _median_us(f_bf, rounds, iters), _median_us(f_mx, rounds, iters)
            print(f"M={M:6d} N=K=3072 {name:10s}: bf16 {t_bf:7.1f} us {fl / t_bf / 1e6:7.1f} TF/s | mxfp8 {t_mx:7.1f} us {fl / t_mx / 1e6:7.1f} TF/s | "
                  f"bf16 / mxfp8 = {t_bf / t_mx:.3f}", flush=True)
        t_q = _median_us(lambda: _lib.mx_quant(a, ac, asc), rounds, iters)
        print(f"M={M:6d} mx_quant of the [M x 3072] bf16 activation: {t_q:7.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="0,1,2,5,6")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--ws", action="store_true", help="pass a split-K workspace (tile_cfg 19 / 20; tile_cfg 0's ffn.2 strip)")
    ap.add_argument("--mx", action="store_true", help="ffn.0 + ffn.2: bf16 against MXFP8 (quantise passes timed separately, included in the pair)")
    ap.add_argument("--mxproj", action="store_true", help="the attention projections' shape: bf16 against MXFP8 per epilogue (BF16, T, SSQ, GATE_RESID)")
    a = ap.parse_args()
    if a.mxproj:
        _lib.init()
        return bench_mxproj(a.rounds, a.iters)
    if a.mx:
        _lib.init()
        return bench_mx(a.rounds, a.iters)
    cfgs = [int(c) for c in a.cfgs.split(",")]
    _lib.init()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    sel = [int(s) for s in a.shapes.split(",")] if a.shapes else range(len(SHAPES))
    for si in sel:
        name, M, N, K, epi = SHAPES[si]
        A = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
        W = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
        bias = (torch.rand(N, device=dev, generator=g) - 0.5).to(torch.bfloat16)
        gate = gate_tid = None
        if epi in (EPI_F32_FROM_BF16, EPI_RESID_F32):
            out = torch.rand(M, N, device=dev, generator=g)
        elif epi == EPI_GATE_RESID_F32:
            out = torch.rand(M, N, device=dev, generator=g)
            gate = torch.rand(2, N, device=dev, generator=g)
            gate_tid = (torch.arange(M, device=dev) * 2 // M).to(torch.int32)
        elif epi == EPI_BF16_T:
            out = torch.zeros(N, (M + 63) // 64 * 64, device=dev, dtype=torch.bfloat16)
        else:
            out = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
        times = {c: [] for c in cfgs}
        # split-K configurations (19 / 20) and the automatic choice's split-K strip take a workspace (uv_gemm_bf16_nt_ws)
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        ws = torch.empty(max(4096 + tiles * 4 * 262144 if tiles <= 1024 else 0, _lib.gemm_splitk_ws_bytes(M, N, K), 256), dtype=torch.uint8, device=dev) if a.ws else None
        for r in range(a.rounds + 1):
            for c in cfgs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    _lib.gemm_bf16(A, W, bias, out, epi, gate=gate, gate_tid=gate_tid, tile_cfg=c, ws=ws)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[c].append(e0.elapsed_time(e1) / a.iters)
        fl = 2.0 * M * N * K
        line = f"{name:24s} M={M:6d} N={N:6d} K={K:6d}"
        for c in cfgs:
            med, mn = statistics.median(times[c]), min(times[c])
            line += f" | cfg{c}: {fl / med / 1e9:7.1f} (best {fl / mn / 1e9:7.1f}) TF/s {med * 1e3:7.1f} us"
        print(line, flush=True)
        if a.check:
            rows = torch.randint(0, M, (64,), device=dev, generator=g)
            rows[0], rows[1] = 0, M - 1
            ref = A[rows].double() @ W.double().t() + bias.double()
            for c in cfgs:
                if epi == EPI_GATE_RESID_F32:
                    base = torch.rand(M, N, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
                    o = base.clone()
                    _lib.gemm_bf16(A, W, bias, o, epi, gate=gate, gate_tid=gate_tid, tile_cfg=c)
                    want = base[rows].double() + ref.to(torch.bfloat16).double() * gate[gate_tid[rows].long()].double()
                    err = (o[rows].double() - want).abs().max().item()
                elif epi == EPI_BF16_T:
                    o = torch.zeros_like(out)
                    _lib.gemm_bf16(A, W, bias, o, epi, tile_cfg=c)
                    err = (o[:, rows].t().double() - ref).abs().max().item()
                else:
                    o = torch.zeros_like(out)
                    _lib.gemm_bf16(A, W, bias, o, epi, tile_cfg=c)
                    want = torch.nn.functional.gelu(ref.to(torch.bfloat16).float(), approximate="tanh").double() if epi == EPI_GELU_BF16 else ref
                    err = (o[rows].double() - want).abs().max().item()
                print(f"    check cfg{c}: max abs err {err:.3e} (ref absmax {ref.abs().max().item():.2f})", flush=True)


if __name__ == "__main__":
    main()
