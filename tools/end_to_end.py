"""End-to-end generation time (developer tool): WanTI2V.t2v / i2v with the production model sizes (30-block TI2V-5B DiT, full-width VAE,
random-init weights, synthetic prompt embeddings): 50 UniPC steps with CFG + VAE decode, per stage, for the exact-f32 VAE and the
f32-grade bf16x6 / f16x3 modes - at the bench size (49 frames of 704 x 1280) and at UniVid's own default workload (121 frames of
704 x 1280, inference.py:48-50).   env: STEPS (50), FRAMES ("49,121"), PRECS ("fp32,bf16x6,f16x3"; also bf16x3 and the opt-in narrow f16)
    --vae-ab ROUNDS   instead of the table, and without the DiT: seconds per VAE decode (z [48, 13, 45, 80]) and encode (49 x 720 x 1280) in
                      precision f16x3 and f16, alternating in one process after a warm-up of each; every round is printed
    --ffn-precision bf16|mxfp8   the DiT's FFN projections in the opt-in MXFP8 mode (WanModel.set_ffn_precision)
    --attn-precision bf16|mxfp8_qk|mxfp8_qk_pv   the DiT's self-attention in an opt-in MXFP8 mode (WanModel.set_attn_precision)
    --proj-precision bf16|mxfp8   the DiT's attention projections in the opt-in MXFP8 mode (WanModel.set_proj_precision)
    --proj-ab ROUNDS [--also-with-mx]   instead of the table: ms per denoise step with the attention projections in bf16 and mxfp8, alternating in one
                       process; --also-with-mx repeats the comparison beside ffn_precision mxfp8 + attn_precision mxfp8_qk_pv in the same process
    --attn-window L,R   the DiT's self-attention under flash-attn's window_size = (L, R) tokens (WanModel.set_attn_window; -1 = unbounded)
    --window-ab ROUNDS   instead of the table: ms per denoise step with global attention and with --attn-window, alternating in one process
    --attn-block-mask B,A,R,C   with --window-ab: a third side, the self-attention under video_block_mask(frames=(B, A), rows=R, cols=C) of the
                         latent's patch grid (WanModel.set_attn_block_mask; -1 = unbounded); --attn-window may then be left out
    --attn-topk K[,B,A,R,C]   with --window-ab: one more side, the self-attention under TopKBlockMask(K, keep) - K an int or a fraction of the
                         key tiles, keep = video_block_mask(frames=(B, A), rows=R, cols=C) when given - with lists built on the device per
                         forward, sample and head; the other sides may then be left out
    --attn-ab ROUNDS   instead of the table: ms per denoise step with the self-attention in bf16, mxfp8_qk and mxfp8_qk_pv, alternating in one process
    --step-cache-ab ROUNDS --step-cache SPEC   instead of the table: ms per GENERATION of the denoise loop plain and under the step cache SPEC
                       (comma-separated key=value of StepCache: order, interval | rel_l1_thresh, first_steps, last_steps - "interval=3,order=1"),
                       alternating in one process; the plan's computed fraction and the time of the skipping forward on its own"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from univid_amd import _lib
from univid_amd.wan.model import WanModel
from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
from univid_amd.wan.vae2_2 import Wan2_2_VAE
_lib.init()
dev = "cuda"
steps = int(os.environ.get("STEPS", 50))


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
    return r, time.perf_counter() - t0


if "--vae-ab" in sys.argv:
    # --vae-ab ROUNDS: the VAE alone. One object per mode (each keeps its arena), one untimed decode and encode of each, then ROUNDS rounds of
    # decode f16x3, decode f16, encode f16x3, encode f16; every round printed, then medians, the spread of each and the distance between the
    # two modes' results
    import statistics
    rounds = int(sys.argv[sys.argv.index("--vae-ab") + 1])
    g = torch.Generator(device=dev).manual_seed(7)
    z = torch.randn(48, 13, 45, 80, device=dev, generator=g)
    vid = torch.tanh(torch.randn(3, 49, 720, 1280, device=dev, generator=g))
    vaes = {p: Wan2_2_VAE(device=dev, seed=0, precision=p) for p in ("f16x3", "f16")}
    res, ts = {}, {(w, p): [] for w in ("decode", "encode") for p in vaes}
    with torch.no_grad():
        for p, v in vaes.items():
            res["decode", p], res["encode", p] = v.decode([z])[0], v.encode([vid])[0]
        for rnd in range(rounds):
            for what in ("decode", "encode"):
                for p, v in vaes.items():
                    _, t = clock((lambda: v.decode([z])) if what == "decode" else (lambda: v.encode([vid])))
                    ts[what, p].append(t)
            print(f"round {rnd}: " + ", ".join(f"{w} {p} {ts[w, p][-1]:.4f} s" for w, p in ts), flush=True)
    for what in ("decode", "encode"):
        med = {p: statistics.median(ts[what, p]) for p in vaes}
        spread = {p: max(ts[what, p]) - min(ts[what, p]) for p in vaes}
        a, b = res[what, "f16x3"].double(), res[what, "f16"].double()
        print(f"{what}: f16x3 median {med['f16x3']:.4f} s (spread {spread['f16x3']:.4f}), f16 median {med['f16']:.4f} s (spread {spread['f16']:.4f}); "
              f"gain {med['f16x3'] - med['f16']:.4f} s, f16 / f16x3 = {med['f16'] / med['f16x3']:.4f}; rel rms f16 vs f16x3 "
              f"{float((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()):.3e}, finite {bool(torch.isfinite(res[what, 'f16']).all())}", flush=True)
    sys.exit(0)
with torch.device(dev):
    m = WanModel.from_config(TI2VConfig.dit)
m = m.eval().requires_grad_(False)
m.init_weights(0)
ffn_precision = sys.argv[sys.argv.index("--ffn-precision") + 1] if "--ffn-precision" in sys.argv else "bf16"
m.set_ffn_precision(ffn_precision)
attn_precision = sys.argv[sys.argv.index("--attn-precision") + 1] if "--attn-precision" in sys.argv else "bf16"
m.set_attn_precision(attn_precision)
proj_precision = sys.argv[sys.argv.index("--proj-precision") + 1] if "--proj-precision" in sys.argv else "bf16"
m.set_proj_precision(proj_precision)
attn_window = tuple(int(v) for v in sys.argv[sys.argv.index("--attn-window") + 1].split(",")) if "--attn-window" in sys.argv else None
if "--window-ab" not in sys.argv:
    m.set_attn_window(attn_window)
print(f"ffn_precision {ffn_precision} attn_precision {attn_precision} proj_precision {proj_precision} attn_window {attn_window}", flush=True)
m.prepare()
g = torch.Generator(device=dev).manual_seed(1)
pe = [torch.randn(40, 4096, device=dev, generator=g) * 0.1]
ne = [torch.randn(9, 4096, device=dev, generator=g) * 0.1]


frames = [int(f) for f in os.environ.get("FRAMES", "49,121").split(",")]
precs = os.environ.get("PRECS", "fp32,bf16x6,f16x3").split(",")
if "--window-ab" in sys.argv:
    # --window-ab ROUNDS: the denoise loop alone (t2v, decode=False) at the first FRAMES entry with global attention and with --attn-window,
    # alternating round by round in THIS process (each switch re-captures: its warm-up generation is not timed), the first round dropped;
    # medians and the spread of the rounds. The precision options apply to both sides.
    import statistics
    from univid_amd.wan.attention import video_block_mask
    vm = tuple(int(v) for v in sys.argv[sys.argv.index("--attn-block-mask") + 1].split(",")) if "--attn-block-mask" in sys.argv else None
    tk = sys.argv[sys.argv.index("--attn-topk") + 1].split(",") if "--attn-topk" in sys.argv else None
    assert attn_window is not None or vm is not None or tk is not None, "--window-ab needs --attn-window L,R, --attn-block-mask B,A,R,C or --attn-topk K[,B,A,R,C]"
    rounds, F = int(sys.argv[sys.argv.index("--window-ab") + 1]), frames[0]
    pipe = WanTI2V(model=m, vae=Wan2_2_VAE(device=dev, seed=0, precision="f16x3"), device=dev)
    ms = {None: []}
    if attn_window is not None:
        ms[attn_window] = []
    if vm is not None:
        ms[f"video_block_mask{vm}"] = []
    spec = None if vm is None else (lambda Fg, Hg, Wg, nh: video_block_mask((Fg, Hg, Wg), frames=vm[:2], rows=vm[2], cols=vm[3]))
    specs = {f"video_block_mask{vm}": spec}
    if tk is not None:
        from univid_amd.wan.attention import TopKBlockMask
        kv = tuple(int(v) for v in tk[1:])
        assert len(kv) in (0, 4), "--attn-topk K or K,B,A,R,C"
        ms[f"top_k{tuple(tk)}"] = []
        specs[f"top_k{tuple(tk)}"] = TopKBlockMask(float(tk[0]) if "." in tk[0] else int(tk[0]),
                                                   (lambda Fg, Hg, Wg, nh: video_block_mask((Fg, Hg, Wg), frames=kv[:2], rows=kv[2], cols=kv[3])) if kv else None)
    resolvers = {}
    for rnd in range(rounds + 1):
        for win in ms:
            m.set_attn_block_mask(None)
            m.set_attn_window(None if isinstance(win, str) else win)
            m.set_attn_block_mask(specs[win] if isinstance(win, str) else None)
            resolvers[win] = m.attn_block_mask
            with torch.no_grad():
                pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne, decode=False)
                lat, t = clock(lambda: pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=steps, seed=7, prompt_embeds=pe,
                                                negative_prompt_embeds=ne, decode=False))
            assert bool(torch.isfinite(lat).all())
            if rnd:
                ms[win].append(t / steps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{F} frames, ffn {ffn_precision}, attn {attn_precision}, window {k}: median {med[k]:.2f} ms/step (min {min(v):.2f} max {max(v):.2f}, {len(v)} rounds of "
              f"{steps} steps)", flush=True)
    for k in ms:
        if k is not None:
            print(f"{k} / global = {med[k] / med[None]:.4f}, gain {med[None] - med[k]:.2f} ms/step (global spread {max(ms[None]) - min(ms[None]):.2f} ms)"
                  + ("" if spec is None or k != f"video_block_mask{vm}" else f"; densities {[round(b.density, 4) for b in resolvers[k].prepared().values()]}"),
                  flush=True)
    sys.exit(0)
if "--step-cache-ab" in sys.argv:
    # --step-cache-ab ROUNDS --step-cache SPEC: the denoise loop alone (t2v, decode=False) at the first FRAMES entry, plain and under the step
    # cache SPEC, alternating round by round in THIS process (both runners stay captured: a 2-step warm-up of each side is not timed), the
    # first round dropped; ms per GENERATION, the plan's computed fraction, and the skipping forward on its own (replays of its capture).
    import statistics
    from univid_amd.wan.step_cache import StepCache
    spec = dict(kv.split("=") for kv in sys.argv[sys.argv.index("--step-cache") + 1].split(","))
    num = {"rel_l1_thresh": float}
    pol = StepCache(int(spec.pop("order", 1)), **{k: num.get(k, int)(v) for k, v in spec.items()})
    rounds, F = int(sys.argv[sys.argv.index("--step-cache-ab") + 1]), frames[0]
    pipe = WanTI2V(model=m, vae=None, device=dev)
    gen = lambda n, sc: pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=n, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne, decode=False,
                                 step_cache=sc)
    ms = {"plain": [], "cached": []}
    with torch.no_grad():
        for side, sc in (("plain", False), ("cached", StepCache(pol.order, schedule=[True, False], last_steps=0))):      # captures; the cached side runs a skip too
            gen(2, sc)
        for rnd in range(rounds + 1):
            for side, sc in (("plain", False), ("cached", pol)):
                lat, t = clock(lambda: gen(steps, sc))
                assert bool(torch.isfinite(lat).all())
                if side == "cached":
                    plan = pipe.last_step_plan
                if rnd:
                    ms[side].append(t * 1e3)
                print(f"round {rnd}: {side} {t * 1e3:.1f} ms", flush=True)
        runner = pipe._runner
        assert runner.cache is not None and len(pipe._runners) == 2
        skip = []
        for _ in range(5):
            _, t = clock(lambda: [runner.graph_skip.replay() for _ in range(20)])
            skip.append(t / 20 * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_c = sum(plan)
    for k, v in ms.items():
        print(f"{F} frames, {steps} steps, {k}: median {med[k]:.1f} ms per generation (min {min(v):.1f} max {max(v):.1f}, {len(v)} rounds)", flush=True)
    print(f"{pol}: {n_c} of {steps} steps computed (fraction {n_c / steps:.3f}); cached / plain = {med['cached'] / med['plain']:.4f}; skipping forward "
          f"alone: median {statistics.median(skip):.3f} ms (min {min(skip):.3f} max {max(skip):.3f}); a skipped step in the loop = (cached - computed "
          f"fraction x plain) / skipped steps = {(med['cached'] - n_c / steps * med['plain']) / max(1, steps - n_c):.3f} ms", flush=True)
    sys.exit(0)
if "--attn-ab" in sys.argv:
    # --attn-ab ROUNDS: the denoise loop alone (t2v, decode=False) at the first FRAMES entry with the self-attention in "bf16", "mxfp8_qk" and "mxfp8_qk_pv",
    # alternating round by round in THIS process (each switch re-prepares and re-captures: its warm-up generation is not timed), the first
    # round dropped; medians and the spread of the rounds. --ffn-precision applies to both sides.
    import statistics
    rounds, F = int(sys.argv[sys.argv.index("--attn-ab") + 1]), frames[0]
    pipe = WanTI2V(model=m, vae=Wan2_2_VAE(device=dev, seed=0, precision="f16x3"), device=dev)
    ms = {"bf16": [], "mxfp8_qk": [], "mxfp8_qk_pv": []}
    for rnd in range(rounds + 1):
        for mode in ms:
            m.set_attn_precision(mode)
            with torch.no_grad():
                pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne, decode=False)
                _, t = clock(lambda: pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=steps, seed=7, prompt_embeds=pe,
                                              negative_prompt_embeds=ne, decode=False))
            if rnd:
                ms[mode].append(t / steps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{F} frames, ffn {ffn_precision}, attn {k:11s}: median {med[k]:.2f} ms/step (min {min(v):.2f} max {max(v):.2f}, {len(v)} rounds of {steps} steps)", flush=True)
    print(f"mxfp8_qk / bf16 = {med['mxfp8_qk'] / med['bf16']:.4f}, mxfp8_qk_pv / bf16 = {med['mxfp8_qk_pv'] / med['bf16']:.4f}, mxfp8_qk_pv / mxfp8_qk = "
          f"{med['mxfp8_qk_pv'] / med['mxfp8_qk']:.4f} (bf16 spread {max(ms['bf16']) - min(ms['bf16']):.2f} ms)", flush=True)
    sys.exit(0)
if "--proj-ab" in sys.argv:
    # --proj-ab ROUNDS: the denoise loop alone (t2v, decode=False) at the first FRAMES entry with the attention projections in "bf16" and
    # "mxfp8", alternating round by round in THIS process (each switch re-prepares and re-captures: its warm-up generation is not timed), the
    # first round dropped; medians and the round-to-round spread of each. --ffn-precision / --attn-precision apply to both sides;
    # --also-with-mx runs the comparison a second time beside the other two MXFP8 modes.
    import statistics
    rounds, F = int(sys.argv[sys.argv.index("--proj-ab") + 1]), frames[0]
    pipe = WanTI2V(model=m, vae=Wan2_2_VAE(device=dev, seed=0, precision="f16x3"), device=dev)
    for ffn_p, attn_p in [(ffn_precision, attn_precision)] + ([("mxfp8", "mxfp8_qk_pv")] if "--also-with-mx" in sys.argv else []):
        m.set_ffn_precision(ffn_p)
        m.set_attn_precision(attn_p)
        ms = {"bf16": [], "mxfp8": []}
        for rnd in range(rounds + 1):
            for mode in ms:
                m.set_proj_precision(mode)
                with torch.no_grad():
                    pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne, decode=False)
                    _, t = clock(lambda: pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=steps, seed=7, prompt_embeds=pe,
                                                  negative_prompt_embeds=ne, decode=False))
                if rnd:
                    ms[mode].append(t / steps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            print(f"{F} frames, ffn {ffn_p}, attn {attn_p}, proj {k:5s}: median {med[k]:.2f} ms/step (min {min(v):.2f} max {max(v):.2f}, spread "
                  f"{max(v) - min(v):.2f}, {len(v)} rounds of {steps} steps)", flush=True)
        print(f"ffn {ffn_p}, attn {attn_p}: proj mxfp8 / bf16 = {med['mxfp8'] / med['bf16']:.4f}, gain {med['bf16'] - med['mxfp8']:.2f} ms/step (bf16 spread "
              f"{max(ms['bf16']) - min(ms['bf16']):.2f} ms, mxfp8 spread {max(ms['mxfp8']) - min(ms['mxfp8']):.2f} ms)", flush=True)
    sys.exit(0)
for F in frames:
    for prec in precs:
        vae = Wan2_2_VAE(device=dev, seed=0, precision=prec)
        pipe = WanTI2V(model=m, vae=vae, device=dev, ffn_precision=ffn_precision, attn_precision=attn_precision, proj_precision=proj_precision)
        with torch.no_grad():
            # warm-up of both loops (2 steps each): one-time costs - the VAE's weight preparation, the HIP-graph captures of the t2v and i2v
            # forward pairs (one per latent shape and mode; a NEW PROMPT does not recapture) - stay out of the timed generations
            w = pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=2, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne)
            pipe.i2v("", w[:, 0].clamp(-1, 1).contiguous(), max_area=704 * 1280, frame_num=F, sampling_steps=2, seed=3, prompt_embeds=pe,
                     negative_prompt_embeds=ne)
            del w
            lat, t_den = clock(lambda: pipe.t2v("", size=(1280, 704), frame_num=F, sampling_steps=steps, seed=7, prompt_embeds=pe,
                                                negative_prompt_embeds=ne, decode=False))
            vid, t_dec = clock(lambda: vae.decode([lat])[0])
            img = vid[:, 0].clamp(-1, 1).contiguous()
            _, t_i2v = clock(lambda: pipe.i2v("", img, max_area=704 * 1280, frame_num=F, sampling_steps=steps, seed=3, prompt_embeds=pe,
                                              negative_prompt_embeds=ne))
        print(f"{F:3d} frames, VAE {prec:7s}: t2v {steps} steps {t_den:6.2f} s ({t_den / steps * 1e3:.1f} ms/step) + decode {t_dec:5.2f} s = "
              f"{t_den + t_dec:6.2f} s per {F}-frame 704x1280 clip (latent {list(lat.shape)}); i2v (encode 1 frame + {steps} steps + decode) "
              f"{t_i2v:6.2f} s; finite {bool(torch.isfinite(vid).all())}", flush=True)
        if prec == "f16x3":
            # the same clip through UniVid's OWN entry point (inference.py:311,377 -> CrossAttentionFusionPipeline.generate_video_with_bagel_context,
            # models/model_pipeline.py:2577-2655) with inference.py's dynamic text weight (cosine 1.3 -> 1.0 over the first 40 % of the steps):
            # the native schedule keeps it on the graph-replay path, so it must cost what the plain t2v + decode above cost
            import types
            from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
            bagel = types.SimpleNamespace(extract_semantic_tokens=lambda text, image: torch.zeros(1, 128, 3584, device=dev, dtype=torch.bfloat16))
            ccfg = CrossAttentionConfig(use_lora=False, use_dynamic_text_weight=True, total_sampling_steps=steps)
            fusion = CrossAttentionFusionPipeline(ccfg, wan_pipeline=pipe, bagel_extractor=bagel, context_projector=None)
            kw = dict(steps=steps, guidance_scale=5.0, frames=F, size=(1280, 704), shift=5.0, seed=7, prompt_embeds=pe, negative_prompt_embeds=ne)
            with torch.no_grad():
                (v2, _), t_pipe = clock(lambda: fusion.generate_video_with_bagel_context("", **kw))
                (_, _), t_pipe_i2v = clock(lambda: fusion.generate_video_with_bagel_context("", image=img, **dict(kw, seed=3)))
            print(f"{F:3d} frames, VAE {prec:7s}: through CrossAttentionFusionPipeline (dynamic text weight, native schedule): t2v + decode {t_pipe:6.2f} s, "
                  f"i2v {t_pipe_i2v:6.2f} s; finite {bool(torch.isfinite(v2).all())}", flush=True)
            fusion.cleanup_resources()
            del fusion, v2
        del vae, pipe, vid, lat
        torch.cuda.empty_cache()
