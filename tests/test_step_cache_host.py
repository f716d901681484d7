"""Step cache, host side (no GPU): the policy object's plans, the pipeline's refusals and plumbing, the wrappers' argument checks."""
import pytest
import torch

from univid_amd import _lib
from univid_amd.wan.step_cache import StepCache, StepCacheState

T, F = True, False
NAN, INF = float("nan"), float("inf")


def _set(plan):
    return {i for i, c in enumerate(plan) if c}


def test_interval_rule_is_the_reference_counter():
    """interval=k: the counter is 0 after every computed step and a free step is computed iff it stands at k - 1; first_steps defaults
    to 5 (first_enhance), last_steps to 1. k = 3, n = 50 -> {0..4, 7, 10, ..., 49}."""
    p = StepCache(interval=3).plan(50)
    assert isinstance(p, tuple) and len(p) == 50 and all(type(c) is bool for c in p)
    assert _set(p) == set(range(5)) | set(range(7, 50, 3))
    assert _set(StepCache(interval=2, first_steps=0, last_steps=0).plan(7)) == {0, 2, 4, 6}       # step 0 is computed whatever first_steps says
    assert _set(StepCache(interval=4, first_steps=1, last_steps=0).plan(10)) == {0, 4, 8}
    assert StepCache(interval=3).plan(0) == () and StepCache(interval=3).plan(1) == (True,)


PLAN_CASES = {
    # name: (constructor keywords, n_steps, plan keywords, computed set)
    "first and last overlap": (dict(interval=2, first_steps=4, last_steps=4), 6, {}, {0, 1, 2, 3, 4, 5}),
    "first and last meet": (dict(interval=3, first_steps=2, last_steps=2), 8, {}, {0, 1, 4, 6, 7}),
    "last_steps beyond n": (dict(interval=3, first_steps=1, last_steps=99), 4, {}, {0, 1, 2, 3}),
    "forced resets the counter": (dict(interval=3, first_steps=1, last_steps=0), 10, dict(forced=(2,)), {0, 2, 5, 8}),
    "forced on a computed step": (dict(interval=3, first_steps=1, last_steps=0), 7, dict(forced=[0, 3]), {0, 3, 6}),
    "schedule or-ed with the common rules": (dict(schedule=[F, F, T, F, F, F], first_steps=2), 6, {}, {0, 1, 2, 5}),
    "schedule with forced": (dict(schedule=[T, F, F, F, F], last_steps=0), 5, dict(forced={3}), {0, 3}),
    "all-true schedule": (dict(schedule=[T] * 4), 4, {}, {0, 1, 2, 3}),
    # acc: step 1 0.3 (skip), step 2 0.6 (skip), step 3 1.0 -> computed, reset; step 4 0.5 skip; step 5 NaN -> computed; step 6 0.2 skip;
    # step 7 inf -> computed; step 8 0.9 skip; step 9 is the last step
    "rel_l1 hand-made": (dict(rel_l1_thresh=1.0), 10, dict(distances=[NAN, 0.3, 0.3, 0.4, 0.5, NAN, 0.2, INF, 0.9, 0.0]), {0, 3, 5, 7, 9}),
    "rel_l1 exact threshold computes": (dict(rel_l1_thresh=0.5, last_steps=0), 4, dict(distances=[0, 0.25, 0.25, 0.25]), {0, 2}),
    "rel_l1 forced resets acc": (dict(rel_l1_thresh=1.0, last_steps=0), 6, dict(distances=[0, 0.6, 0.6, 0.6, 0.6, 0.6], forced=(2,)), {0, 2, 4}),
    "rel_l1 threshold above every sum": (dict(rel_l1_thresh=1e30, first_steps=2, last_steps=2), 9, dict(distances=[1e3] * 9), {0, 1, 7, 8}),
    "rel_l1 zero threshold": (dict(rel_l1_thresh=0.0), 5, dict(distances=[0.0] * 5), {0, 1, 2, 3, 4}),
    # polyval, highest power first: 2 d^2 + 1 -> d = 0.5: 1.5 per step against 2.9: skip (1.5), compute (3.0), skip, compute
    "rel_l1 polynomial": (dict(rel_l1_thresh=2.9, coefficients=(2.0, 0.0, 1.0), last_steps=0), 5, dict(distances=[0.5] * 5), {0, 2, 4}),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_table(case):
    kw, n, pkw, want = PLAN_CASES[case]
    p = StepCache(**kw).plan(n, **pkw)
    assert len(p) == n and _set(p) == want, (case, p)


def test_policy_refuses_bad_arguments_and_is_immutable():
    for bad in (dict(), dict(interval=3, schedule=[T]), dict(interval=3, rel_l1_thresh=0.1), dict(schedule=[T], rel_l1_thresh=0.1),
                dict(interval=1), dict(interval=2.5), dict(interval=True), dict(rel_l1_thresh=-1.0), dict(rel_l1_thresh=NAN),
                dict(interval=2, order=3), dict(interval=2, order=-1), dict(interval=2, order=True), dict(interval=2, indicator="t"),
                dict(interval=2, first_steps=-1), dict(interval=2, last_steps=-1), dict(rel_l1_thresh=0.1, coefficients=()),
                dict(rel_l1_thresh=0.1, coefficients=(INF,))):
        with pytest.raises(ValueError):
            StepCache(**bad)
    with pytest.raises(TypeError):
        StepCache(1, 3)                                    # the rule is keyword-only
    with pytest.raises(ValueError, match="schedule has 3 entries, the loop has 4"):
        StepCache(schedule=[T, F, T]).plan(4)
    with pytest.raises(ValueError, match="needs distances"):
        StepCache(rel_l1_thresh=0.1).plan(4)
    with pytest.raises(ValueError, match="3 distances for 4 steps"):
        StepCache(rel_l1_thresh=0.1).plan(4, [0.0, 0.1, 0.1])
    c = StepCache(2, interval=3)
    assert (c.order, c.interval, c.first_steps, c.last_steps, c.indicator, c.coefficients) == (2, 3, 5, 1, "e0", (1.0, 0.0))
    assert StepCache(rel_l1_thresh=0.2).first_steps == 1 and StepCache(interval=2).order == 1
    with pytest.raises(AttributeError):
        c.order = 1
    with pytest.raises(AttributeError):
        del c.interval
    assert c == StepCache(2, interval=3) and hash(c) == hash(StepCache(2, interval=3)) and c != StepCache(1, interval=3)
    assert "interval=3" in repr(c)
    # plan is a pure function of its arguments
    assert c.plan(20) == c.plan(20)


def test_state_counters_follow_the_arithmetic_contract():
    """have = min(have + 1, order + 1) and last = i after a computed step; a skipped step changes neither; nothing can be skipped before
    the first computed step. (The control table lives on the device: here only the counters.)"""
    for order in (0, 1, 2):
        s = StepCacheState(order)
        s.ctl = torch.zeros(4)                             # a host stand-in for the device table
        seen = []
        for i, c in enumerate([T, T, F, T, F, F, T]):
            s.advance(i, c)
            seen.append((s.have, s.last, s.ctl.tolist()))
        assert [h for h, _, _ in seen] == [min(n, order + 1) for n in (1, 2, 2, 3, 3, 3, 4)]
        assert [l for _, l, _ in seen] == [0, 1, 1, 3, 3, 3, 6]
        # ctl = [have before the step, k, c1, c2]: step 3 is computed 2 steps after step 1, step 6 3 steps after step 3
        assert seen[3][2][:2] == [float(min(2, order + 1)), 2.0] and seen[6][2][:2] == [float(min(3, order + 1)), 3.0]
        if order == 2:                                     # step 5 is skipped with m = 2: c1 = 2, c2 = 2 * 2 / 2
            assert seen[5][2] == [3.0, 2.0, 2.0, 2.0]
        s.reset()
        assert (s.have, s.last) == (0, None)
        with pytest.raises(RuntimeError, match="no step was computed yet"):
            s.advance(0, False)
    with pytest.raises(ValueError):
        StepCacheState(3)


def _model(**over):
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG, **over)
    m = WanModel.from_config(dict(cfg, model_type="ti2v"))
    m.load_state_dict(wan_dit.make_state_dict(cfg, 0))
    return m.eval()


class _CountingSchedule:
    layers = None

    def __init__(self):
        self.drawn = 0

    def rows(self, n):
        return 4

    def next_pair(self):
        self.drawn += 1
        return 1.0, 1.0


@pytest.mark.parametrize("limit", ["cfg parallel", "sequence parallel", "foreign model forward", "foreign cross-attention forward", "no stacking"])
def test_pipeline_refuses_before_anything_runs(limit):
    """The step cache needs the plain loop. Under CFG parallelism, sequence parallelism, a re-assigned forward or a token count that does
    not stack, denoise raises NotImplementedError before anything runs (no GPU here: anything that ran would fail differently) and the
    pipeline's state is as it was: the setting, the last plan, the runners, the text-weight schedule's counter."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    pol = StepCache(interval=2)
    pipe = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", step_cache=pol)
    assert pipe.step_cache is pol and pipe.last_step_plan is None
    pipe.last_step_plan = "kept"
    sched = pipe.text_weight_schedule = _CountingSchedule()
    noise = torch.zeros(48, 2, 8, 8)
    if limit == "cfg parallel":
        pipe.cfgp = object()
    elif limit == "sequence parallel":
        pipe.sp_size = 2
    elif limit == "foreign model forward":
        pipe.model.forward = lambda *a, **k: pytest.fail("the forward ran")
    elif limit == "foreign cross-attention forward":
        pipe.model.blocks[1].cross_attn.forward = lambda *a, **k: pytest.fail("the forward ran")
    else:
        noise = torch.zeros(48, 1, 6, 6)                   # 9 tokens
    ctx = [torch.zeros(5, 64)]
    for kw in ({}, dict(step_cache=StepCache(schedule=[T] * 4)), dict(graph=False)):
        with pytest.raises(NotImplementedError, match="step_cache= needs"):
            pipe.denoise(noise, ctx, ctx, 4, 5.0, 5.0, **kw)
    assert pipe.step_cache is pol and pipe.last_step_plan == "kept" and not pipe._runners and pipe._step_state is None and sched.drawn == 0
    with pytest.raises(TypeError, match="StepCache"):
        pipe.denoise(noise, ctx, ctx, 4, 5.0, 5.0, step_cache=3)
    with pytest.raises(TypeError, match="StepCache"):
        WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", step_cache="interval")


def test_forward_keyword_names_its_limits():
    """WanModel.forward(step_cache=): a bad kind, a sequence-parallel model and samples that do not stack are refused before any kernel."""
    m = _model(num_heads=2)
    st = StepCacheState(1)
    x = [torch.zeros(48, 1, 8, 8)] * 2
    with pytest.raises(ValueError, match='"compute" or "skip"'):
        m(x, torch.zeros(2), [torch.zeros(5, 64)] * 2, 16, step_cache=(st, "forecast"))
    with pytest.raises(NotImplementedError, match="single stacked group"):
        m([torch.zeros(48, 1, 6, 6)] * 2, torch.zeros(2), [torch.zeros(5, 64)] * 2, 9, step_cache=(st, "compute"))

    class _SP:
        size = 2
    m.sp = _SP()
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        m(x, torch.zeros(2), [torch.zeros(5, 64)] * 2, 16, step_cache=(st, "skip"))
    assert st.key is None and st.ctl is None


def test_config_keyword_reaches_the_pipeline():
    """CrossAttentionConfig.step_cache defaults to None, is handed to an injected WanTI2V that has the attribute, and - like a mode's
    default - None leaves an injected pipeline's own setting alone. It is not a model mode."""
    from univid_amd.model_pipeline import CrossAttentionConfig, CrossAttentionFusionPipeline
    from univid_amd.wan.modes import MODE_DEFAULTS
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    assert CrossAttentionConfig().step_cache is None and "step_cache" not in MODE_DEFAULTS
    pol, own = StepCache(2, interval=3), StepCache(schedule=[T, F, T])
    base = dict(use_lora=False, enable_bagel_extraction=False)
    plain = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu")
    fused = CrossAttentionFusionPipeline(CrossAttentionConfig(step_cache=pol, **base), wan_pipeline=plain, context_projector=lambda *a, **k: None)
    assert fused.wan_pipeline.step_cache is pol
    kept = WanTI2V(TI2VConfig, model=_model(num_heads=2), device="cpu", step_cache=own)
    CrossAttentionFusionPipeline(CrossAttentionConfig(**base), wan_pipeline=kept, context_projector=lambda *a, **k: None)
    assert kept.step_cache is own
    with pytest.raises(TypeError, match="StepCache"):
        CrossAttentionFusionPipeline(CrossAttentionConfig(step_cache=3, **base), wan_pipeline=plain, context_projector=lambda *a, **k: None)

    class _Duck:                                           # an injected pipeline without the attribute is left alone
        model, vae, text_encoder = _model(num_heads=2), None, None
    duck = _Duck()
    CrossAttentionFusionPipeline(CrossAttentionConfig(step_cache=pol, **base), wan_pipeline=duck, context_projector=lambda *a, **k: None)
    assert not hasattr(duck, "step_cache")


def test_wrappers_check_arguments_before_the_library_is_touched(monkeypatch):
    """step_cache_update / step_cache_apply / rows_rel_l1 on CPU tensors: dtype, layout and extent of every pointer argument, n, order, the
    buffers an order needs and the row count are checked from metadata - each failure names wrapper and argument - and a well-formed call
    fails only for living on the CPU. Nothing is launched or loaded."""
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a rejected call reached the library"))
    E = _lib.UnividHipError
    z = torch.zeros
    n = 24
    xo, xi, d0, d1, d2, ctl = z(4, 6), z(4, 6), z(4, 6), z(4, 6), z(4, 6), z(4)
    with pytest.raises(E, match=r"step_cache_update\.x_out: tensor must live on the GPU"):
        _lib.step_cache_update(xo, xi, d0, d1, d2, ctl, 2)
    with pytest.raises(E, match=r"step_cache_apply\.x: tensor must live on the GPU"):
        _lib.step_cache_apply(xo, d0, d1, d2, ctl, 2)
    for order, bufs in ((0, (d0, None, None)), (1, (d0, d1, None))):      # absent buffers stay absent
        with pytest.raises(E, match="must live on the GPU"):
            _lib.step_cache_update(xo, xi, *bufs, ctl, order)
        with pytest.raises(E, match="must live on the GPU"):
            _lib.step_cache_apply(xo, *bufs, ctl, order)
    for order in (-1, 3, 1.5, None):
        with pytest.raises(E, match="step_cache_update: order must be 0, 1 or 2"):
            _lib.step_cache_update(xo, xi, d0, d1, d2, ctl, order)
        with pytest.raises(E, match="step_cache_apply: order must be 0, 1 or 2"):
            _lib.step_cache_apply(xo, d0, d1, d2, ctl, order)
    with pytest.raises(E, match=r"step_cache_update\.d1: a tensor is required"):
        _lib.step_cache_update(xo, xi, d0, None, None, ctl, 1)
    with pytest.raises(E, match=r"step_cache_update\.d2: a tensor is required"):
        _lib.step_cache_update(xo, xi, d0, d1, None, ctl, 2)
    with pytest.raises(E, match=r"step_cache_apply\.d2: a tensor is required"):
        _lib.step_cache_apply(xo, d0, d1, None, ctl, 2)
    with pytest.raises(E, match=r"step_cache_apply\.d0: a tensor is required"):
        _lib.step_cache_apply(xo, None, None, None, ctl, 0)
    for bad_n in (0, -4):
        with pytest.raises(E, match="step_cache_update: n must be positive"):
            _lib.step_cache_update(xo, xi, d0, d1, d2, ctl, 2, n=bad_n)
        with pytest.raises(E, match="step_cache_apply: n must be positive"):
            _lib.step_cache_apply(xo, d0, d1, d2, ctl, 2, n=bad_n)
    with pytest.raises(E, match="step_cache_apply: n must be positive"):
        _lib.step_cache_apply(z(0), z(0), None, None, ctl, 0)
    upd = dict(x_out=0, x_in=1, d0=2, d1=3, d2=4, ctl=5)
    for name, i in upd.items():
        args = [xo, xi, d0, d1, d2, ctl]
        args[i] = args[i].to(torch.float64)
        with pytest.raises(E, match=rf"step_cache_update\.{name}: expected"):
            _lib.step_cache_update(*args, 2)
        if name != "ctl":
            args[i] = z(6, 4).t()
            with pytest.raises(E, match=rf"step_cache_update\.{name}: must be contiguous"):
                _lib.step_cache_update(*args, 2)
            args[i] = z(n - 1)                              # one element short of the n the call states
            with pytest.raises(E, match=rf"step_cache_update\.{name}: the kernel addresses 24 elements, the tensor's storage holds 23"):
                _lib.step_cache_update(*args, 2, n=n)
    for name, i in dict(x=0, d0=1, d1=2, d2=3, ctl=4).items():
        args = [xo, d0, d1, d2, ctl]
        args[i] = args[i].to(torch.bfloat16)
        with pytest.raises(E, match=rf"step_cache_apply\.{name}: expected"):
            _lib.step_cache_apply(*args, 2)
        if name != "ctl":
            args[i] = z(n - 1)
            with pytest.raises(E, match=rf"step_cache_apply\.{name}: the kernel addresses 24 elements, the tensor's storage holds 23"):
                _lib.step_cache_apply(*args, 2, n=n)
    with pytest.raises(E, match=r"step_cache_apply\.ctl: the kernel addresses 4 elements, the tensor's storage holds 3"):
        _lib.step_cache_apply(xo, d0, d1, d2, z(3), 2)
    with pytest.raises(E, match=r"step_cache_update\.x_in: the kernel addresses 32 elements"):      # n larger than a buffer
        _lib.step_cache_update(z(32), xi, z(32), None, None, ctl, 0, n=32)
    # rows_rel_l1
    rows, out = z(5, 7), z(4)
    with pytest.raises(E, match=r"rows_rel_l1\.rows: tensor must live on the GPU"):
        _lib.rows_rel_l1(rows, out)
    for bad in (z(1, 7), z(0, 7), z(7), z(2, 0), z(2, 3, 4)):
        with pytest.raises(E, match="rows_rel_l1: at least two rows"):
            _lib.rows_rel_l1(bad, out)
    with pytest.raises(E, match=r"rows_rel_l1\.rows: expected"):
        _lib.rows_rel_l1(rows.double(), out)
    with pytest.raises(E, match=r"rows_rel_l1\.rows: must be contiguous"):
        _lib.rows_rel_l1(z(7, 5).t(), out)
    with pytest.raises(E, match=r"rows_rel_l1\.rows: must be contiguous"):
        _lib.rows_rel_l1(z(5, 8)[:, :7], out)
    with pytest.raises(E, match=r"rows_rel_l1\.out: the kernel addresses 4 elements, the tensor's storage holds 3"):
        _lib.rows_rel_l1(rows, z(3))
    with pytest.raises(E, match=r"rows_rel_l1\.out: expected"):
        _lib.rows_rel_l1(rows, out.double())


def test_entry_points_are_declared_with_their_contracts():
    """The three entry points: in the signature table, and declared in the public header under a comment that states the contract."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "univid_hip.h")).read()
    for name in ("uv_step_cache_update", "uv_step_cache_apply", "uv_rows_rel_l1"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert "[have, k, c1, c2]" in hdr and _lib.SIGNATURES["uv_rows_rel_l1"][2:4] == [_lib._I, _lib._I]
