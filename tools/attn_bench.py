"""Attention-only micro benchmark (developer tool): full-size self-attention launches for profiling.   env: L (11440), B (1), LK (L), N (5), ROUNDS (7)
    --qk mxfp8          bf16 against the MXFP8 q / k and q / k + P.V modes, launches and producers alternating in one process
    --window L,R[:L,R...]   the dense launch against uv_flash_attn_win_bf16 under each window (-1 = unbounded; -1,0 = causal), and against (-1,-1)
                        through the same entry - which visits every tile: what the classification costs -, all alternating in one process;
                        --forms: every window also on the 12-wave and on the 4-wave form (OPT_ATTN_WIN_FORM), whatever the plan's rule says
    --block-mask F,H,W  (F H W == L: the patch grid) the dense launch against uv_flash_attn_bs_bf16 under the all-ones mask (what a listed tile
                        costs), video_block_mask of +-2 frames - beside window_size = 2 frames each way through uv_flash_attn_win_bf16 -, of
                        +-1 frame x +-8 rows (no window expresses it) and a per-head mix (spatial heads: the own frame; temporal heads: every
                        frame, +-2 rows x +-4 columns), all alternating in one process
    --attn-topk K[,B,A,R,C]  with --block-mask F,H,W: also the data-dependent lists of TopKBlockMask(K, keep) - K an int or a fraction of the key
                        tiles, keep = video_block_mask(frames=(B, A), rows=R, cols=C) when given: uv_attn_pool_qk, uv_attn_bs_select and
                        uv_flash_attn_bs_lists_bf16 each on its own, beside uv_flash_attn_bs_bf16 under a STATIC mask of the same lists'
                        density (the keep tiles plus the K nearest others), and pooling against its traffic bound (one read of q and k)"""
import math, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univid_amd import _lib
_lib.init()
dev = "cuda"; BF16 = torch.bfloat16
L, H, D = int(os.environ.get("L", 11440)), 24, 128
B = int(os.environ.get("B", 1))     # stacked samples (the CFG pair is B=2)
C = H * D
torch.manual_seed(0)
Lk = int(os.environ.get("LK", L))
q = torch.randn(B * L, C, device=dev).to(BF16); k = torch.randn(B * Lk, C, device=dev).to(BF16)
vt = torch.randn(C, (B - 1) * Lk + (Lk + 63) // 64 * 64, device=dev).to(BF16)
out = torch.empty(B * L, C, dtype=BF16, device=dev)
n = int(os.environ.get("N", 5))
for _ in range(n):
    _lib.flash_attn(q, k, vt, out, L, Lk, H, D, 1 / math.sqrt(D), batch=B)
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(n):
    _lib.flash_attn(q, k, vt, out, L, Lk, H, D, 1 / math.sqrt(D), batch=B)
e.record(); torch.cuda.synchronize()
ms = s.elapsed_time(e) / n
import hashlib
print(f"attention B{B} Lq{L} Lk{Lk}: {ms:.3f} ms {4*B*L*Lk*C/ms/1e9:.1f} TFLOP/s  kernel={_lib.attn_kernel_name(L, Lk, D, B)}  out sha={hashlib.sha1(out.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:12]}")


if "--qk" in sys.argv and sys.argv[sys.argv.index("--qk") + 1] == "mxfp8":
    # bf16 against the MXFP8 q / k mode and the MXFP8 q / k + P.V mode (WanModel.set_attn_precision("mxfp8_qk" / "mxfp8_qk_pv")) on the same
    # random operands, in ONE process: the launches and their producers (rmsnorm_rope_qk / rmsnorm_rope_qk_mx on the raw projections, and for
    # the P.V mode the V^T quantiser vt_mx_quant) alternate round by round, the first round of each is dropped, medians and the spread
    # (min .. max) of the ROUNDS rounds are printed. The figure that counts is launch + ALL producers of the mode.
    import statistics
    rounds = int(os.environ.get("ROUNDS", 7))
    U8 = torch.uint8
    F, Hh, Ww = 1, 1, 1                                         # RoPE grid: the kernels' cost does not depend on the positions
    freqs = torch.view_as_real(torch.polar(torch.ones(1024, D // 2, dtype=torch.float64), torch.rand(1024, D // 2, dtype=torch.float64))).contiguous().to(dev)
    wq, wk = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    q_raw, k_raw = torch.randn(B * L, C, device=dev).to(BF16), torch.randn(B * Lk, C, device=dev).to(BF16)
    qc, kc = torch.empty(B * L, C, dtype=U8, device=dev), torch.empty(B * Lk, C, dtype=U8, device=dev)
    qs, ks = torch.empty(B * L, C // 32, dtype=U8, device=dev), torch.empty(B * Lk, C // 32, dtype=U8, device=dev)
    _lib.mx_quant(q, qc, qs); _lib.mx_quant(k, kc, ks)
    out_mx, out_pv = torch.empty_like(out), torch.empty_like(out)
    vcols = _lib.vt_mx_cols(B, Lk)
    vc, vs = torch.empty(C, vcols, dtype=U8, device=dev), torch.empty(H, 4 * vcols, dtype=U8, device=dev)
    _lib.vt_mx_quant(vt, vc, vs, Lk, H, D, batch=B)
    qn, kn = q_raw.clone(), k_raw.clone()
    assert L == Lk, "the producers run on q and k of one geometry (self-attention)"
    work = {
        "attn bf16": lambda: _lib.flash_attn(q, k, vt, out, L, Lk, H, D, 1 / math.sqrt(D), batch=B),
        "attn mxqk": lambda: _lib.flash_attn_mxqk(qc, qs, kc, ks, vt, out_mx, L, Lk, H, D, 1 / math.sqrt(D), batch=B),
        "prod bf16": lambda: _lib.rmsnorm_rope_qk(qn, kn, wq, wk, B * L, L, C, D, 1e-6, freqs, (F, Hh, Ww)),      # (in place: re-normalises its own output, same cost)
        "attn mxpv": lambda: _lib.flash_attn_mxpv(qc, qs, kc, ks, vc, vs, out_pv, L, Lk, H, D, 1 / math.sqrt(D), batch=B),
        "prod vtq": lambda: _lib.vt_mx_quant(vt, vc, vs, Lk, H, D, batch=B),
        "prod mxqk": lambda: _lib.rmsnorm_rope_qk_mx(q_raw, k_raw, wq, wk, qc, qs, kc, ks, B * L, L, C, D, 1e-6, freqs, (F, Hh, Ww)),
    }
    times = {name: [] for name in work}
    for rnd in range(rounds + 1):
        for name, fn in work.items():
            fn(); torch.cuda.synchronize()
            s.record()
            for _ in range(n):
                fn()
            e.record(); torch.cuda.synchronize()
            if rnd:
                times[name].append(s.elapsed_time(e) / n * 1e3)
    _lib.mx_quant(q, qc, qs); _lib.mx_quant(k, kc, ks)          # (the producer rounds overwrote the codes)
    work["attn mxqk"](); work["attn mxpv"](); torch.cuda.synchronize()
    med = {name: statistics.median(t) for name, t in times.items()}
    flop = 4 * B * L * Lk * C
    for name, t in times.items():
        extra = f"  {flop / med[name] / 1e9:.3f} PFLOP/s" if name.startswith("attn") else ""
        print(f"{name} B{B} L{L}: median {med[name]:.1f} us  (min {min(t):.1f} max {max(t):.1f}, {len(t)} rounds of {n}){extra}")
    tot_b, tot_m = med["attn bf16"] + med["prod bf16"], med["attn mxqk"] + med["prod mxqk"]
    spread = max(times["attn bf16"]) - min(times["attn bf16"]) + max(times["prod bf16"]) - min(times["prod bf16"])
    print(f"launch + producer: bf16 {tot_b:.1f} us, mxfp8_qk {tot_m:.1f} us, ratio {tot_m / tot_b:.3f} (bf16 spread between rounds {spread:.1f} us); "
          f"kernel={_lib.attn_mxqk_plan(L, Lk, D, B, H)['kernel']}; rel rms of the mxqk output against bf16 on the same operands "
          f"{float((out_mx.float() - out.float()).pow(2).mean().sqrt() / out.float().pow(2).mean().sqrt()):.3e}")
    tot_p = med["attn mxpv"] + med["prod mxqk"] + med["prod vtq"]
    print(f"launch + producers (q / k producer and V^T quantiser): mxfp8_qk_pv {tot_p:.1f} us, ratio to bf16 {tot_p / tot_b:.3f}, to mxfp8_qk {tot_p / tot_m:.3f} "
          f"(bf16 spread {spread:.1f} us); kernel={_lib.attn_mxpv_plan(L, Lk, D, B, H)['kernel']}; rel rms of the mxpv output against bf16 on the same "
          f"operands {float((out_pv.float() - out.float()).pow(2).mean().sqrt() / out.float().pow(2).mean().sqrt()):.3e}")


if "--window" in sys.argv:
    # Dense and windowed launches on the same random operands, alternating round by round in ONE process, the first round dropped; medians and
    # the spread (min .. max) of the ROUNDS rounds. Per launch also the 32-query x 64-key tiles the waves COMPUTE (host arithmetic, the kernels'
    # own rule) and the time per computed tile, next to the dense kernel's. plan_attn_win's 12-wave rule is measured with windows on either
    # side of span 2048, e.g. 832,831 (span 2047: the 4-wave form) against 832,832 (2048: the 12-wave form) - the same work to one key.
    import statistics
    assert L == Lk, "windows are built for self-attention (Lq == Lk)"
    rounds = int(os.environ.get("ROUNDS", 7))
    wins = [tuple(int(x) for x in w.split(",")) for w in sys.argv[sys.argv.index("--window") + 1].split(":")]
    wins = [(-1, -1)] + [w for w in wins if w != (-1, -1)]

    def wave_tiles(win):
        le, ri = (L if w < 0 else min(w, L) for w in win)
        return B * H * sum(min(L - 1, min(u * 32 + 31, L - 1) + ri) // 64 - max(0, u * 32 - le) // 64 + 1 for u in range((L + 31) // 32))

    forms = (0, 1, 2) if "--forms" in sys.argv else (0,)
    outs = {(w, f): torch.empty_like(out) for w in wins for f in forms}

    def win_launch(w, f):
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, f)
        _lib.flash_attn_win(q, k, vt, outs[w, f], L, H, D, 1 / math.sqrt(D), w, batch=B)
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, 0)

    work = {"dense": lambda: _lib.flash_attn(q, k, vt, out, L, L, H, D, 1 / math.sqrt(D), batch=B)}
    for key in outs:
        work[key] = (lambda key=key: win_launch(*key))
    times = {name: [] for name in work}
    for rnd in range(rounds + 1):
        for name, fn in work.items():
            fn(); torch.cuda.synchronize()
            s.record()
            for _ in range(n):
                fn()
            e.record(); torch.cuda.synchronize()
            if rnd:
                times[name].append(s.elapsed_time(e) / n * 1e3)
    med = {name: statistics.median(t) for name, t in times.items()}
    dense_tiles = B * H * ((L + 31) // 32) * ((L + 63) // 64)
    print(f"dense B{B} L{L}: median {med['dense']:.1f} us (min {min(times['dense']):.1f} max {max(times['dense']):.1f}, {rounds} rounds of {n}); "
          f"{dense_tiles} wave tiles, {med['dense'] * 1e3 / dense_tiles:.3f} ns per tile; kernel={_lib.attn_plan(L, L, D, B, H)['kernel']}")
    assert all(torch.equal(outs[(-1, -1), f], out) for f in forms), "(-1, -1) through the win entry differs from the dense launch"
    for w, f in outs:
        assert torch.equal(outs[w, f], outs[w, 0]), "the form changes the bits"
        t, tiles, key = times[w, f], wave_tiles(w), (w, f)
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, f)
        plan = _lib.attn_win_plan(L, D, B, H, w)
        _lib.set_option(_lib.OPT_ATTN_WIN_FORM, 0)
        print(f"window {w} form {('auto', '12-wave', '4-wave')[f]} B{B} L{L}: median {med[key]:.1f} us (min {min(t):.1f} max {max(t):.1f}); {med[key] / med['dense']:.4f} x dense, "
              f"dense / window = {med['dense'] / med[key]:.3f}; {tiles} wave tiles ({tiles / dense_tiles:.4f} of dense), {med[key] * 1e3 / tiles:.3f} ns per tile "
              f"({med[key] / tiles / (med['dense'] / dense_tiles):.3f} x the dense kernel's); plan={plan}")


if "--block-mask" in sys.argv:
    # Dense, windowed and block-sparse launches on the same random operands, alternating round by round in ONE process, the first round
    # dropped; medians and the spread (min .. max) of the ROUNDS rounds. Per launch the 128-query x 64-key tiles its workgroups visit (the
    # lists' lengths; dense and windowed: host arithmetic), the density and the time per visited tile next to the dense kernel's.
    import statistics
    from univid_amd.wan.attention import video_block_mask
    assert L == Lk, "block masks are built for self-attention (Lq == Lk)"
    rounds = int(os.environ.get("ROUNDS", 7))
    grid = tuple(int(x) for x in sys.argv[sys.argv.index("--block-mask") + 1].split(","))
    assert len(grid) == 3 and grid[0] * grid[1] * grid[2] == L, f"--block-mask F,H,W must multiply to L = {L}"
    frame = grid[1] * grid[2]
    nqb, nkb = (L + 127) // 128, (L + 63) // 64
    spatial, temporal = video_block_mask(grid, frames=(0, 0)), video_block_mask(grid, frames=(-1, -1), rows=2, cols=4)
    masks = {"ones": torch.ones(nqb, nkb, dtype=torch.bool),
             "frames+-2": video_block_mask(grid, frames=(2, 2)),
             "frames+-1 x rows+-8": video_block_mask(grid, frames=(1, 1), rows=8),
             "per-head mix (spatial | temporal)": torch.stack([spatial if hd % 2 == 0 else temporal for hd in range(H)])}
    bms = {name: _lib.prepare_block_mask(m, L, dev) for name, m in masks.items()}
    win = (2 * frame, 2 * frame)
    outs = {name: torch.empty_like(out) for name in list(masks) + ["window"]}
    work = {"dense": lambda: _lib.flash_attn(q, k, vt, out, L, L, H, D, 1 / math.sqrt(D), batch=B),
            "window": lambda: _lib.flash_attn_win(q, k, vt, outs["window"], L, H, D, 1 / math.sqrt(D), win, batch=B)}
    for name in masks:
        work[name] = (lambda name=name: _lib.flash_attn_bs(q, k, vt, outs[name], L, H, D, 1 / math.sqrt(D), bms[name], batch=B))
    times = {name: [] for name in work}
    for rnd in range(rounds + 1):
        for name, fn in work.items():
            fn(); torch.cuda.synchronize()
            s.record()
            for _ in range(n):
                fn()
            e.record(); torch.cuda.synchronize()
            if rnd:
                times[name].append(s.elapsed_time(e) / n * 1e3)
    med = {name: statistics.median(t) for name, t in times.items()}
    dense_tiles = B * H * nqb * nkb
    per_dense = med["dense"] * 1e3 / dense_tiles
    print(f"dense B{B} L{L} grid {grid}: median {med['dense']:.1f} us (min {min(times['dense']):.1f} max {max(times['dense']):.1f}, {rounds} rounds of {n}); "
          f"{dense_tiles} 128 x 64 tiles, {per_dense:.2f} ns per tile; kernel={_lib.attn_plan(L, L, D, B, H)['kernel']}")
    assert torch.equal(outs["ones"], out), "the all-ones mask differs from the dense launch"
    win_tiles = B * H * sum(min(L - 1, min(b * 128 + 127, L - 1) + win[1]) // 64 - max(0, b * 128 - win[0]) // 64 + 1 for b in range(nqb))
    t = times["window"]
    print(f"window {win} B{B} L{L}: median {med['window']:.1f} us (min {min(t):.1f} max {max(t):.1f}); dense / window = {med['dense'] / med['window']:.3f}; "
          f"{win_tiles} tiles staged per 128 queries ({win_tiles / dense_tiles:.4f} of dense), {med['window'] * 1e3 / win_tiles:.2f} ns per tile "
          f"({med['window'] * 1e3 / win_tiles / per_dense:.3f} x the dense kernel's); plan={_lib.attn_win_plan(L, D, B, H, win)}")
    for name, bm in bms.items():
        t, tiles = times[name], B * (H // bm.heads) * int(bm.tile_cnt.sum())
        print(f"block mask {name} B{B} L{L}: median {med[name]:.1f} us (min {min(t):.1f} max {max(t):.1f}); dense / masked = {med['dense'] / med[name]:.3f}; "
              f"density {bm.density:.4f}, {tiles} tiles visited, {med[name] * 1e3 / tiles:.2f} ns per tile ({med[name] * 1e3 / tiles / per_dense:.3f} x the dense "
              f"kernel's); grid order: XCD-contiguous block ids (flash_attn_fwd3_kernel's); plan={_lib.attn_bs_plan(L, D, B, H)}")

    if "--attn-topk" in sys.argv:
        # The three launches of a TopKBlockMask on the same operands, in the same alternation: pooling, selection, and the attention under the
        # device-built lists - beside the static-mask launch of EQUAL density (every row lists the keep tiles plus the top_k non-kept tiles
        # nearest to its diagonal). Random q / k give scattered lists; real activations are not measured here.
        from univid_amd.wan.attention import TopKBlockMask
        arg = sys.argv[sys.argv.index("--attn-topk") + 1].split(",")
        keep_mask = video_block_mask(grid, frames=(int(arg[1]), int(arg[2])), rows=int(arg[3]), cols=int(arg[4])) if len(arg) == 5 else None
        top_k = TopKBlockMask(float(arg[0]) if "." in arg[0] else int(arg[0])).count(L)
        keep = None if keep_mask is None else _lib.prepare_keep_mask(keep_mask, L, dev)[0]
        kb = torch.zeros(nqb, nkb, dtype=torch.bool) if keep_mask is None else keep_mask
        dist = (torch.arange(nkb)[None, :] - 2 * torch.arange(nqb)[:, None]).abs().double().masked_fill(kb, float("inf"))
        near = torch.zeros_like(kb)
        near.scatter_(1, dist.argsort(dim=1, stable=True)[:, :top_k], True)
        static = _lib.prepare_block_mask(kb | (near & ~kb), L, dev)
        qbar, kbar = torch.empty(B, H, nqb, D, device=dev), torch.empty(B, H, nkb, D, device=dev)
        idx, cnt = torch.empty(B, H, nqb, nkb, dtype=torch.int32, device=dev), torch.empty(B, H, nqb, dtype=torch.int32, device=dev)
        o_topk, o_static = torch.empty_like(out), torch.empty_like(out)
        work = {"dense": work["dense"],
                "static mask": lambda: _lib.flash_attn_bs(q, k, vt, o_static, L, H, D, 1 / math.sqrt(D), static, batch=B),
                "pool": lambda: _lib.attn_pool_qk(q, k, qbar, kbar, L, H, D, batch=B),
                "select": lambda: _lib.attn_bs_select(qbar, kbar, keep, top_k, idx, cnt, L, H, batch=B),
                "top-k lists": lambda: _lib.flash_attn_bs_lists(q, k, vt, o_topk, L, H, D, 1 / math.sqrt(D), idx, cnt, H, B, batch=B)}
        times = {name: [] for name in work}
        for rnd in range(rounds + 1):
            for name, fn in work.items():
                fn(); torch.cuda.synchronize()
                s.record()
                for _ in range(n):
                    fn()
                e.record(); torch.cuda.synchronize()
                if rnd:
                    times[name].append(s.elapsed_time(e) / n * 1e3)
        med = {name: statistics.median(t) for name, t in times.items()}
        tiles_topk, tiles_static = int(cnt.sum()), B * H * int(static.tile_cnt.sum())
        assert tiles_topk == tiles_static or keep_mask is not None, "the static mask of equal density lists another number of tiles"
        gb = (q.numel() + k.numel()) * 2 / 1e9
        for name, t in times.items():
            print(f"top-k {name} B{B} L{L} top_k {top_k} keep {arg[1:] or None}: median {med[name]:.1f} us (min {min(t):.1f} max {max(t):.1f}, {len(t)} rounds of {n})")
        print(f"pool: {gb / med['pool'] * 1e3:.2f} TB/s over one read of q and k ({gb * 1e3:.1f} MB); pool + select = {med['pool'] + med['select']:.1f} us = "
              f"{(med['pool'] + med['select']) / med['top-k lists']:.3f} of the launch under its lists; top-k lists / static mask = "
              f"{med['top-k lists'] / med['static mask']:.3f} at {tiles_topk} vs {tiles_static} tiles ({tiles_topk / dense_tiles:.4f} of dense); "
              f"per listed tile {med['top-k lists'] * 1e3 / tiles_topk:.2f} ns ({med['top-k lists'] * 1e3 / tiles_topk / per_dense:.3f} x the dense kernel's); "
              f"dense / (pool + select + launch) = {med['dense'] / (med['pool'] + med['select'] + med['top-k lists']):.3f}")
