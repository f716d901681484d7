"""Step cache on the GPU: the three kernels bit-exact against their formulas, the cached denoise loop on the tiny DiT (graph == eager,
state reset, capture reuse, the plans of the three rules), its parity against a CPU loop composed from the oracle's pieces, and one case
at TI2V-5B row width.

The arithmetic under test (include/univid_hip.h), every operation one fp32 rounding:
  update: r = x_out - x_in; order >= 1 and have >= 1: n1 = (r - d0) / k; order >= 2 and have >= 2: n2 = (n1 - d1) / k; d0 = r, d1 = n1, d2 = n2
  apply:  rh = d0; have >= 2: rh = rh + d1 * c1; have >= 3: rh = rh + d2 * c2; x = x + rh
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, record_margin
from univid_amd import _lib
from univid_amd.wan.step_cache import StepCache, StepCacheState

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, Fa = True, False
SCHEDULE = [T, T, T, Fa, T, Fa, Fa, T, Fa, T]
SENTINEL = 1234.5
PAD = 4            # sentinel elements in front of and behind every buffer: 4 keeps the buffer 16-byte aligned (the vector path)


# ---- kernels ------------------------------------------------------------------------------------------------------------------------
def _special(n, gen):
    """n fp32 values: random, with +-0, denormals, +-inf and NaN spread over them when there is room."""
    v = torch.randn(n, generator=gen)
    sp = torch.tensor([0.0, -0.0, 1e-40, -3e-42, float("inf"), float("-inf"), float("nan"), 1e-38, 3e38, -3e38])
    if n >= 64:
        idx = torch.randperm(n, generator=gen)[:40]
        v[idx] = sp.repeat(4)
    return v


def _same_bits(got, want, what):
    """Bit for bit; a NaN must be a NaN at the same place (its payload is the hardware's)."""
    got, want = got.cpu(), want.cpu()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ"
    g, w = got.masked_fill(gn, 0).view(torch.int32), want.masked_fill(wn, 0).view(torch.int32)
    bad = (g != w).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at {int(bad[0])}: {got[bad[0]].item()!r} != {want[bad[0]].item()!r}"


class _Buf:
    """A device buffer of n elements at `off` elements into an allocation that holds sentinels around it."""

    def __init__(self, host, off=PAD):
        n = host.numel()
        self.big = torch.full((off + n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.big[off:off + n]
        self.t.copy_(host)
        self.off, self.n = off, n

    def check_sentinels(self, what):
        big = self.big.cpu()
        assert bool((big[:self.off] == SENTINEL).all()) and bool((big[self.off + self.n:] == SENTINEL).all()), f"{what}: wrote outside its buffer"


def ref_update(xo, xi, d, have, k, order):
    d = list(d)
    kt = torch.full_like(xo, float(k))           # (a tensor divisor: a true fp32 division per element)
    r = xo - xi
    if order >= 1 and have >= 1:
        n1 = (r - d[0]) / kt
        if order >= 2 and have >= 2:
            d[2] = (n1 - d[1]) / kt
        d[1] = n1
    d[0] = r
    return d


def ref_apply(x, d, have, c1, c2, order):
    rh = d[0]
    if order >= 1 and have >= 2:
        rh = rh + d[1] * torch.full_like(x, c1)
    if order >= 2 and have >= 3:
        rh = rh + d[2] * torch.full_like(x, c2)
    return x + rh


SIZES = [1, 3, 4, 5, 1024, _lib.STEP_CACHE_GRID_ELEMS + 1]        # the last: one full pass of the largest grid, and one element


def _ctl(have, k=0.0, c1=0.0, c2=0.0):
    return torch.tensor([float(have), k, c1, c2], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_update_kernel_is_bit_exact(order):
    gen = torch.Generator().manual_seed(100 + order)
    for n in SIZES:
        host = [_special(n, gen) for _ in range(5)]          # x_out, x_in, d0, d1, d2
        offs = (PAD,) if n > 1024 else (PAD, 1)              # 1: not 16-byte aligned - the element-by-element path
        for off in offs:
            for have in range(order + 2):
                for k in ((2,) if n > 1024 else (1, 2, 7)):
                    xo, xi = _Buf(host[0], off), _Buf(host[1], off)
                    d = [_Buf(host[2 + j], off) if j <= order else None for j in range(3)]
                    _lib.step_cache_update(xo.t, xi.t, *[b.t if b is not None else None for b in d], _ctl(have, float(k), 99.0, 99.0), order)
                    want = ref_update(host[0], host[1], host[2:5], have, k, order)
                    what = f"update order {order} have {have} k {k} n {n} offset {off}"
                    for j in range(order + 1):               # buffers `have` does not reach equal the input: ref_update leaves them
                        _same_bits(d[j].t, want[j], f"{what}: d{j}")
                        d[j].check_sentinels(f"{what}: d{j}")
                    _same_bits(xo.t, host[0], f"{what}: x_out was written")
                    _same_bits(xi.t, host[1], f"{what}: x_in was written")
                    xo.check_sentinels(what), xi.check_sentinels(what)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_apply_kernel_is_bit_exact(order):
    gen = torch.Generator().manual_seed(200 + order)
    for n in SIZES:
        host = [_special(n, gen) for _ in range(4)]          # x, d0, d1, d2
        offs = (PAD,) if n > 1024 else (PAD, 1)
        for off in offs:
            for have in range(1, order + 2):
                for m in ((2,) if n > 1024 else (1, 2, 7)):
                    c1, c2 = float(m), m * m / 2
                    x = _Buf(host[0], off)
                    d = [_Buf(host[1 + j], off) if j <= order else None for j in range(3)]
                    _lib.step_cache_apply(x.t, *[b.t if b is not None else None for b in d], _ctl(have, 99.0, c1, c2), order)
                    what = f"apply order {order} have {have} m {m} n {n} offset {off}"
                    _same_bits(x.t, ref_apply(host[0], host[1:4], have, c1, c2, order), what)
                    x.check_sentinels(what)
                    for j in range(order + 1):
                        _same_bits(d[j].t, host[1 + j], f"{what}: d{j} was written")
                        d[j].check_sentinels(f"{what}: d{j}")


@pytest.mark.parametrize("K", [1, 7, 256, 18432])
@pytest.mark.parametrize("n_rows", [2, 50])
def test_rows_rel_l1_within_one_ulp_and_reproducible(n_rows, K):
    """fp64 sums of at most 18 432 fp32 terms carry a relative error below 18 432 * 2^-53 = 2e-12, the fp64 quotient 2^-53 more: the fp32
    rounding of that is the correctly rounded exact value or its neighbour - 1 fp32 ulp (derived, not measured)."""
    gen = torch.Generator().manual_seed(K * 100 + n_rows)
    rows = torch.randn(n_rows, K, generator=gen) * 3.0
    dev = rows.to(DEV)
    out1 = torch.full((n_rows + 3,), SENTINEL, dtype=torch.float32, device=DEV)
    out2 = torch.full((n_rows + 3,), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.rows_rel_l1(dev, out1[2:n_rows + 1])
    _lib.rows_rel_l1(dev, out2[2:n_rows + 1])
    a = rows.numpy().astype(np.float64)
    exact = np.abs(a[1:] - a[:-1]).sum(1) / np.abs(a[:-1]).sum(1)
    got = out1[2:n_rows + 1].cpu().numpy()
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - exact) / ulp
    print(f"rows_rel_l1 n_rows {n_rows} K {K}: max error {err.max():.3f} ulp")
    assert err.max() <= 1.0
    assert torch.equal(out1, out2), "two launches differ"
    assert bool((out1[:2] == SENTINEL).all()) and bool((out1[n_rows + 1:] == SENTINEL).all()), "wrote outside out"


def test_rows_rel_l1_zero_row_gives_inf_or_nan():
    rows = torch.randn(5, 33, generator=torch.Generator().manual_seed(5))
    rows[1] = 0.0
    rows[3] = 0.0
    rows[4] = 0.0
    out = torch.empty(4, dtype=torch.float32, device=DEV)
    _lib.rows_rel_l1(rows.to(DEV), out)
    got = out.cpu()
    # pairs (0,1): finite = 1 exactly (|0 - a| / |a|); (1,2): x / 0 = inf; (2,3): 1; (3,4): 0 / 0 = NaN
    assert got[0] == 1.0 and got[2] == 1.0 and torch.isinf(got[1]) and got[1] > 0 and torch.isnan(got[3])


# ---- the tiny DiT -------------------------------------------------------------------------------------------------------------------
class _Tiny:
    def __init__(self):
        from test_gpu_parity import _tiny_model
        from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
        g = self.g = load_golden("sampler_tiny")
        self.cfg, self.sd, self.m = _tiny_model(g["seed"], num_heads=2)
        self.pipe = WanTI2V(TI2VConfig, model=self.m, device=DEV)
        self.steps = 10
        self._plain = {}

    def run(self, pipe=None, z=False, ctx=None, **kw):
        g = self.g
        with torch.no_grad():
            return (pipe or self.pipe).denoise(g["noise"].to(DEV), [(g["ctx"] if ctx is None else ctx).to(DEV).clone()], [g["ctx_null"].to(DEV).clone()],
                                               self.steps, g["shift"], g["guide_scale"], z=g["z"].to(DEV) if z else None, **kw).clone()

    def plain(self, z=False):
        """The uncached loop's result (graph; the existing suite shows graph == eager), computed once and shared."""
        if z not in self._plain:
            self._plain[z] = self.run(z=z, graph=True, step_cache=False)
        return self._plain[z]


@pytest.fixture(scope="module")
def tiny():
    t = _Tiny()
    yield t
    t.pipe._runner = None


@pytest.mark.parametrize("order", [0, 2])
def test_all_true_schedule_equals_the_plain_loop(tiny, order):
    """(a) A computed step's output is bit-identical to the plain forward: with every step computed the cached loop IS the plain loop."""
    pol = StepCache(order, schedule=[T] * tiny.steps)
    plain = tiny.plain()
    for graph in (False, True):
        got = tiny.run(graph=graph, step_cache=pol)
        assert tiny.pipe.last_step_plan == (True,) * tiny.steps
        assert torch.equal(got, plain), f"order {order}, graph {graph}"


@pytest.mark.parametrize("mode", ["t2v", "i2v"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_scheduled_skips_graph_equals_eager_and_state_resets(tiny, order, mode):
    """(b) Under a schedule with single and double skips: graph == eager bit for bit, a second call on the same pipeline equals the first
    (`have` restarts at 0: nothing of the previous generation leaks), the result is not the plain loop's, i2v keeps its first frame."""
    z = mode == "i2v"
    pol = StepCache(order, schedule=SCHEDULE)
    eager = tiny.run(z=z, graph=False, step_cache=pol)
    assert tiny.pipe.last_step_plan == tuple(SCHEDULE)
    graph = tiny.run(z=z, graph=True, step_cache=pol)
    assert torch.equal(graph, eager), "graph != eager"
    assert torch.equal(tiny.run(z=z, graph=True, step_cache=pol), graph), "second graph call differs: state of the first call leaked"
    assert torch.equal(tiny.run(z=z, graph=False, step_cache=pol), eager), "second eager call differs: state of the first call leaked"
    assert torch.isfinite(graph).all() and not torch.equal(graph, tiny.plain(z))
    if z:
        assert torch.equal(graph[:, 0].cpu(), tiny.g["z"][:, 0]), "i2v must keep the first latent frame pinned to z"


def test_orders_differ_from_each_other(tiny):
    """The three orders forecast differently under the same plan (an order that silently ran as another would pass everything else)."""
    outs = [tiny.run(graph=True, step_cache=StepCache(o, schedule=SCHEDULE)) for o in (0, 1, 2)]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[2])


def test_skipped_forward_is_head_of_x_in_plus_forecast(tiny):
    """(c) Three computed forwards (steps 0, 1, 2) fill d0, d1, d2; the skipped forward of step 5 (m = 3: c1 = 3, c2 = 4.5) must equal the
    model's own head and unpatchify applied to x_in + rh, rh formed with torch fp32 operations from the state's buffers."""
    m, g = tiny.m, tiny.g
    gen = torch.Generator().manual_seed(11)
    noise = g["noise"]
    L = noise.shape[1] * noise.shape[2] * noise.shape[3] // 4
    ctx = [g["ctx"].to(DEV), g["ctx_null"].to(DEV)]
    state = StepCacheState(2).buffers(2 * L, m.dim, DEV)

    def fwd(lat, t, st, kind):
        tvec = torch.full((2, L), t, device=DEV)
        return m([lat, lat], t=tvec, context=ctx, seq_len=L, step_cache=(st, kind))

    with torch.no_grad():
        for i, t in enumerate((900.0, 800.0, 650.0)):
            lat = (noise + 0.3 * i * torch.randn(noise.shape, generator=gen)).to(DEV)
            state.advance(i, True)
            got = fwd(lat, t, state, "compute")
            want = m([lat, lat], t=torch.full((2, L), t, device=DEV), context=ctx, seq_len=L)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"computed step {i} differs from the plain forward"
        assert (state.have, state.last) == (3, 2)
        d = [b.cpu().clone() for b in state.d]
        assert all(bool(b.abs().sum() > 0) for b in d)
        lat5 = (noise + torch.randn(noise.shape, generator=gen)).to(DEV)
        state.advance(5, False)
        assert state.ctl.cpu().tolist() == [3.0, 1.0, 3.0, 4.5]
        got = fwd(lat5, 400.0, state, "skip")
        for j in range(3):
            assert torch.equal(state.d[j].cpu(), d[j]), "a skipped step wrote the cache"
        probe = StepCacheState(0).buffers(2 * L, m.dim, DEV)          # x_in of the skipped step: what a computing forward saves
        probe.advance(0, True)
        fwd(lat5, 400.0, probe, "compute")
        x_in = probe.x_in.cpu()
        rh = d[0]
        rh = rh + d[1] * torch.full_like(rh, 3.0)
        rh = rh + d[2] * torch.full_like(rh, 4.5)
        xs = (x_in + rh).to(DEV)
        e_rows, _ = m._time_rows(torch.tensor([400.0], device=DEV))
        yh = m.head._run(xs, 2 * L, e_rows, None)
        grid = (noise.shape[1], noise.shape[2] // 2, noise.shape[3] // 2)
        for j in range(2):
            out = torch.empty_like(got[j])
            _lib.unpatchify(yh[j * L:(j + 1) * L], out, grid, m.patch_size)
            assert torch.equal(got[j], out), f"sample {j}"
        assert not torch.equal(got[0], got[1]), "each sample of the pair keeps its own cache"


def test_prompt_change_reuses_both_captures_and_off_is_the_plain_loop(tiny):
    """(d) One runner - two captures - per (shape, mode, weights, order) serves every prompt; False switches the cache off for a call."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    pipe = WanTI2V(TI2VConfig, model=tiny.m, device=DEV, step_cache=StepCache(1, schedule=SCHEDULE))
    try:
        a = tiny.run(pipe, graph=True)                                        # the pipeline's setting
        assert pipe.last_step_plan == tuple(SCHEDULE) and len(pipe._runners) == 1
        r = pipe._runner
        assert r.cache is not None and r.graph_skip is not None and r.key[-1] == ("step_cache", 1)
        other = tiny.g["ctx"] * -0.5
        b = tiny.run(pipe, graph=True, ctx=other)
        assert pipe._runner is r and len(pipe._runners) == 1, "a new prompt must not cost a recapture"
        assert not torch.equal(a, b) and torch.equal(b, tiny.run(pipe, graph=False, ctx=other))
        assert torch.equal(tiny.run(pipe, graph=True), a)
        off = tiny.run(pipe, graph=True, step_cache=False)
        assert pipe.last_step_plan is None and torch.equal(off, tiny.plain()), "step_cache=False is not the plain loop"
        assert pipe._runner is not r and pipe._runner.cache is None and len(pipe._runners) == 2      # the plain runner is another one; both stay
        assert torch.equal(tiny.run(pipe, graph=True), a) and pipe._runner is r
    finally:
        pipe._runner = None


def test_rel_l1_thresholds_through_last_step_plan(tiny):
    """(e) rel_l1_thresh = 0 computes every step (acc < 0 never holds) and equals the plain loop; a threshold above any sum computes only
    the common-rule steps; both indicators give distances the plan can use."""
    n = tiny.steps
    out = tiny.run(graph=True, step_cache=StepCache(1, rel_l1_thresh=0.0))
    assert tiny.pipe.last_step_plan == (True,) * n and torch.equal(out, tiny.plain())
    for ind in ("e0", "e"):
        out = tiny.run(graph=True, step_cache=StepCache(1, rel_l1_thresh=1e30, indicator=ind, first_steps=2, last_steps=2))
        assert tiny.pipe.last_step_plan == (T, T) + (Fa,) * (n - 4) + (T, T) and torch.isfinite(out).all()
    # in between: the distances are finite positive numbers, so some threshold skips some free steps but not all of them
    some = tiny.run(graph=True, step_cache=StepCache(1, rel_l1_thresh=1e30, last_steps=n - 3))
    assert tiny.pipe.last_step_plan == (T, Fa, Fa) + (T,) * (n - 3) and torch.isfinite(some).all()


# ---- against the oracle -------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _oracle_in_fp32():
    """The oracle with every bf16 rounding removed, as test_gpu_parity._truth_forward does it."""
    from oracle import lora as ora_lora, wan_dit
    old = wan_dit.BF16
    wan_dit.BF16 = ora_lora.BF16 = torch.float32
    try:
        yield
    finally:
        wan_dit.BF16 = ora_lora.BF16 = old


def _oracle_loop(sd, cfg, g, plan, order):
    """oracle.sampler.denoise's t2v loop (UniPC) with the CFG pair as one two-sample forward; under `plan` the skipped steps apply the
    step cache's arithmetic in fp32 to hidden[-1] - x_in and the oracle's head expressions (oracle/wan_dit.py: dit_forward's tail).
    Returns [(noise_pred, latent)] per step."""
    from oracle import sampler, unipc, wan_dit
    sched = unipc.FlowUniPC(num_train_timesteps=1000, shift=1)
    timesteps = sched.set_timesteps(int(g["steps"]), shift=g["shift"])
    latent = g["noise"]
    ctx = [g["ctx"], g["ctx_null"]]
    seq_len = sampler.seq_len_of(latent.shape, cfg["patch_size"])
    ps, dim, eps = tuple(cfg["patch_size"]), cfg["dim"], cfg["eps"]
    d, have, last = [None, None, None], 0, None
    rec = []
    for i, t in enumerate(timesteps):
        tvec = torch.full((2, seq_len), float(t))
        pw, pb = sd["patch_embedding.weight"], sd["patch_embedding.bias"]
        conv = F.conv3d(latent.unsqueeze(0).to(wan_dit.BF16), pw.to(wan_dit.BF16), pb.to(wan_dit.BF16), stride=ps)        # wan_dit.py: dit_forward
        x_in = conv.flatten(2).transpose(1, 2).float().expand(2, -1, -1)
        if plan is None or plan[i]:
            out, hidden, _ = wan_dit.dit_forward(sd, cfg, [latent, latent], tvec, ctx, seq_len, return_hidden=True)
            if plan is not None:
                r = hidden[-1].float() - x_in
                if have:
                    k = torch.full_like(r, float(i - last))
                    if order >= 1 and have >= 1:
                        n1 = (r - d[0]) / k
                        if order >= 2 and have >= 2:
                            d[2] = (n1 - d[1]) / k
                        d[1] = n1
                d[0] = r
                have, last = min(have + 1, order + 1), i
        else:
            m = float(i - last)
            rh = d[0]
            if have >= 2:
                rh = rh + d[1] * m
            if have >= 3:
                rh = rh + d[2] * (m * m / 2)
            xt = x_in + rh
            emb = wan_dit.sinusoidal_embedding_1d(cfg["freq_dim"], tvec.flatten()).unflatten(0, (2, seq_len)).float()
            e = F.linear(F.silu(F.linear(emb, sd["time_embedding.0.weight"], sd["time_embedding.0.bias"])),
                         sd["time_embedding.2.weight"], sd["time_embedding.2.bias"])
            eh = (sd["head.modulation"].unsqueeze(0) + e.unsqueeze(2)).chunk(2, dim=2)
            xh = F.linear(wan_dit.layer_norm(xt, eps) * (1 + eh[1].squeeze(2)) + eh[0].squeeze(2), sd["head.head.weight"], sd["head.head.bias"])
            grid = torch.tensor([conv.shape[2:]] * 2, dtype=torch.long)
            out = [u.float() for u in wan_dit.unpatchify(xh, grid, ps, cfg["out_dim"])]
        cond, uncond = out
        noise_pred = uncond + g["guide_scale"] * (cond - uncond)
        latent = sched.step(noise_pred.unsqueeze(0), t, latent.unsqueeze(0)).squeeze(0)
        rec.append((noise_pred.clone(), latent.clone()))
    return rec


def _rms(a, b):
    return float((a.double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def test_cached_loop_tracks_the_oracle_as_well_as_the_plain_loop(tiny):
    """The 10-step t2v loop under SCHEDULE at order 2, HIP against a CPU loop composed from the oracle's pieces (bf16 arithmetic), both
    measured against the same loop without any bf16 rounding (the truth): ratio = rms(hip - truth) / rms(oracle - truth) for every step's
    noise prediction and for the final latent. The bound is not a number chosen here: the UNCACHED loop - the parent's behaviour - is
    measured the same way in this test, g = the largest of its ratios, and every ratio of the cached loop must be <= 1.2 * max(1, g)
    (1.2: the project's ratchet margin). The cache adds only exact fp32 elementwise arithmetic, so it should amplify the two
    implementations' bf16 noise alike."""
    order = 2
    ratios = {}
    for name, plan in (("uncached", None), ("cached", tuple(SCHEDULE))):
        hip = []
        tiny.run(graph=True, record=hip, step_cache=False if plan is None else StepCache(order, schedule=SCHEDULE))
        ref = _oracle_loop(tiny.sd, tiny.cfg, tiny.g, plan, order)
        with _oracle_in_fp32():
            truth = _oracle_loop(tiny.sd, tiny.cfg, tiny.g, plan, order)
        r = {f"noise_pred_step{i}": _rms(hip[i][0], truth[i][0]) / _rms(ref[i][0], truth[i][0]) for i in range(len(truth))}
        r["final_latent"] = _rms(hip[-1][1], truth[-1][1]) / _rms(ref[-1][1], truth[-1][1])
        ratios[name] = r
        for k, v in r.items():
            print(f"step cache parity, {name}: {k} e_hip / e_oracle = {v:.4f}")
    g_un, g_c = max(ratios["uncached"].values()), max(ratios["cached"].values())
    bound = 1.2 * max(1.0, g_un)
    print(f"uncached max ratio {g_un:.4f}, cached max ratio {g_c:.4f}, bound {bound:.4f}")
    record_margin("step cache: 10-step t2v (tiny DiT, order 2) e_hip / e_oracle vs fp32 truth", uncached_max_ratio=g_un, cached_max_ratio=g_c,
                  bound=bound, **{f"uncached_{k}": v for k, v in ratios["uncached"].items()}, **{f"cached_{k}": v for k, v in ratios["cached"].items()})
    for k, v in ratios["cached"].items():
        assert v <= bound, f"cached loop, {k}: e_hip / e_oracle = {v:.4f} > {bound:.4f} (uncached loop: at most {g_un:.4f})"


# ---- production row width -----------------------------------------------------------------------------------------------------------
def test_production_width_graph_equals_eager():
    """dim 3072, 24 heads, one block, 48 tokens: computed, computed, skipped at order 1 - the buffers at TI2V-5B row width
    (2 x 48 rows of 3072 fp32), graph == eager bit for bit, and the skipped step changes the result."""
    from test_gpu_parity import _tiny_model
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    cfg, sd, m = _tiny_model(3, dim=3072, num_heads=24, num_layers=1, ffn_dim=1024)
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    gen = torch.Generator().manual_seed(7)
    noise = torch.randn(48, 3, 8, 8, generator=gen).to(DEV)
    ctx, ctxn = [torch.randn(9, cfg["text_dim"], generator=gen).to(DEV)], [torch.randn(4, cfg["text_dim"], generator=gen).to(DEV)]
    pol = StepCache(1, schedule=[T, T, Fa], last_steps=0)
    try:
        with torch.no_grad():
            eager = pipe.denoise(noise, ctx, ctxn, 3, 5.0, 5.0, graph=False, step_cache=pol).clone()
            assert pipe.last_step_plan == (T, T, Fa)
            st = pipe._step_state
            assert st.key[:3] == (96, 3072, 1) and (st.have, st.last) == (2, 1) and st.d[2] is None
            assert bool(st.d[0].abs().sum() > 0) and bool(st.d[1].abs().sum() > 0)
            graph = pipe.denoise(noise, ctx, ctxn, 3, 5.0, 5.0, graph=True, step_cache=pol).clone()
            plain = pipe.denoise(noise, ctx, ctxn, 3, 5.0, 5.0, graph=True)
        assert torch.equal(graph, eager) and torch.isfinite(graph).all() and not torch.equal(graph, plain)
    finally:
        pipe._runner = None
