"""Per-sample adapter weights inside one stacked forward: the segmented down-projection kernel uv_lora_down_seg_bf16 (one scale row per
segment of rows, looked up per output row; a zero scale is exact +0 and lets a workgroup skip the pass), WanModel.set_adapter_weights,
WanTI2V.denoise(adapter_weights=) on the eager stacked pair and on the HIP-graph path, and the guards. Every test here needs the new
entry point or the new interfaces."""
import math

import pytest
import torch

from conftest import load_golden
from test_gpu_parity import _lora_factors, _tiny_model, _write_adapter, assert_bf16_kernel
from test_lora_unmerged import LT, NAMES18, SENTINEL, _down_problem

gpu = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(autouse=True)
def _default_options(request):
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    from univid_amd import _lib
    _lib.init()
    _lib.reset_options()
    yield
    _lib.reset_options()


def L():
    from univid_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------------------
#          seg_rows, nseg, M, K, R, Rpad
SHAPES = [(8, 3, 24, 64, 8, 128),          # three segments in one workgroup, two in one wave tile
          (40, 3, 100, 192, 16, 128),      # boundaries mid-tile, partial last segment
          (104, 2, 208, 320, 17, 128),     # K tail of the 256 chunk, NT = 2
          (1, 5, 5, 64, 40, 128),          # one-row segments, NT = 4
          (33, 4, 132, 256, 130, 256)]     # odd segment length, two passes, <8,128>


def _scale_matrix(nseg, R, zeros=True):
    """Distinct values, none a power of two; with `zeros`: the last segment's row all zero, and some zero entries (a -0 among them: the
    rule is `== 0`) in the first row - which is a different row whenever there is more than one segment."""
    sc = (0.37 + 0.0131 * torch.arange(R).float())[None, :] + 0.173 * torch.arange(nseg).float()[:, None]
    if zeros:
        sc[nseg - 1] = 0.0
        row = 0 if nseg > 1 else None
        if row is not None:
            sc[row, ::3] = 0.0
            sc[row, 0] = -0.0
    return sc.contiguous()


def _seg_of_rows(M, seg_rows):
    return torch.arange(M) // seg_rows


def _buffer(x, M, K, Rpad, extra=0):
    buf = torch.full((M + 1, K + Rpad + extra), SENTINEL, dtype=BF16)
    buf[:M, :K] = x
    return buf


@gpu
@pytest.mark.parametrize("seg_rows,nseg,M,K,R,Rpad", SHAPES)
def test_lora_down_seg_vs_double_precision_in_place(seg_rows, nseg, M, K, R, Rpad):
    """K1: scale[s] * (x A^T) in double precision rounded once, under the gate of the un-segmented kernel's K1, in its sentinel layout: the
    activation's own columns, the row below M and the columns beyond K + Rpad keep the sentinel, columns [K + R, K + Rpad) are +0."""
    x, A, _ = _down_problem(M, K, R, M + K + R)
    sc = _scale_matrix(nseg, R)
    buf = _buffer(x, M, K, Rpad, extra=8)
    ref = (sc[_seg_of_rows(M, seg_rows)].double() * (x.double() @ A.double().t())).to(BF16)
    dbuf = buf.to(DEV)
    L().lora_down_seg(dbuf, K, A.to(DEV), sc.to(DEV), seg_rows, M=M, Rpad=Rpad)
    got = dbuf.cpu()
    assert torch.equal(got[:, :K], buf[:, :K]), "the activation's own columns were written"
    assert torch.equal(got[M], buf[M]), "the row below M was written"
    assert torch.equal(got[:, K + Rpad:], buf[:, K + Rpad:]), "columns beyond K + Rpad were written"
    assert (got[:M, K + R:K + Rpad].view(torch.int16) == 0).all(), "slot columns beyond R must be exactly +0"
    assert got[:M, K:K + R].float().abs().sum() > 0
    assert_bf16_kernel(got[:M, K:K + R], ref, name=f"lora_down_seg {seg_rows}x{nseg} M={M} K={K} R={R}")


@gpu
@pytest.mark.parametrize("seg_rows,nseg,M,K,R,Rpad", SHAPES)
def test_zero_scale_is_plus_zero(seg_rows, nseg, M, K, R, Rpad):
    """K2: every element whose scale is zero (a -0 scale included) has all-zero bits."""
    x, A, _ = _down_problem(M, K, R, M + K + R)
    sc = _scale_matrix(nseg, R)
    dbuf = _buffer(x, M, K, Rpad).to(DEV)
    L().lora_down_seg(dbuf, K, A.to(DEV), sc.to(DEV), seg_rows, M=M, Rpad=Rpad)
    got = dbuf.cpu()[:M, K:K + R]
    off = sc[_seg_of_rows(M, seg_rows)] == 0
    assert off.any() and (~off).any()
    assert (got.view(torch.int16)[off] == 0).all(), "a zero scale must give +0 bits"
    assert (got.float()[~off] != 0).float().mean() > 0.99


@gpu
def test_inf_in_an_off_segment_stays_out():
    """K2: Inf in the x rows of the fully-off segment - those rows of the slot are still +0 (whether the workgroup skipped the pass or
    shared it with live rows), and every other row is bit-identical to the run without the Inf."""
    seg_rows, nseg, M, K, R, Rpad = 40, 3, 100, 192, 16, 128
    x, A, _ = _down_problem(M, K, R, 5)
    sc = _scale_matrix(nseg, R)
    clean = _buffer(x, M, K, Rpad).to(DEV)
    L().lora_down_seg(clean, K, A.to(DEV), sc.to(DEV), seg_rows, M=M, Rpad=Rpad)
    xi = x.clone()
    xi[(nseg - 1) * seg_rows:] = float("inf")
    dirty = _buffer(xi, M, K, Rpad).to(DEV)
    L().lora_down_seg(dirty, K, A.to(DEV), sc.to(DEV), seg_rows, M=M, Rpad=Rpad)
    off0 = (nseg - 1) * seg_rows
    assert (dirty[off0:M, K:].view(torch.int16) == 0).all(), "the off segment's slot rows must be +0 whatever x holds"
    assert torch.equal(dirty[:off0, K:], clean[:off0, K:]), "rows of the other segments changed"
    assert torch.isfinite(clean[:M, K:].float()).all()


@gpu
def test_one_segment_equals_the_unsegmented_entry():
    """K3 (a): nseg = 1, all scales non-zero, bit for bit."""
    for M, K, R, Rpad in ((100, 192, 16, 128), (132, 256, 130, 256)):
        x, A, scale = _down_problem(M, K, R, 9)
        a = _buffer(x, M, K, Rpad).to(DEV)
        b = a.clone()
        L().lora_down(a, K, A.to(DEV), scale.to(DEV), M=M, Rpad=Rpad)
        L().lora_down_seg(b, K, A.to(DEV), scale.to(DEV)[None, :], M, M=M, Rpad=Rpad)
        assert torch.equal(a, b)
        assert a[:M, K:K + R].float().abs().sum() > 0


@gpu
@pytest.mark.parametrize("seg_rows,nseg,M,K,R,Rpad", [SHAPES[1], SHAPES[4]])
def test_segmented_launch_equals_per_segment_launches(seg_rows, nseg, M, K, R, Rpad):
    """K3 (b): a segmented launch against the concatenation of per-segment launches of uv_lora_down_bf16, each with its own scale row."""
    x, A, _ = _down_problem(M, K, R, 13)
    sc = _scale_matrix(nseg, R, zeros=False).to(DEV)
    assert (sc != 0).all()
    whole = _buffer(x, M, K, Rpad).to(DEV)
    parts = whole.clone()
    L().lora_down_seg(whole, K, A.to(DEV), sc, seg_rows, M=M, Rpad=Rpad)
    for s in range(nseg):
        r0, r1 = s * seg_rows, min((s + 1) * seg_rows, M)
        L().lora_down(parts[r0:r1], K, A.to(DEV), sc[s], M=r1 - r0, Rpad=Rpad)
    assert torch.equal(whole, parts)


@gpu
def test_lora_down_seg_rejects_bad_arguments_and_writes_nothing():
    """K4."""
    from univid_amd._lib import UnividHipError, call, ptr, stream_ptr
    seg_rows, nseg, M, K, R, Rpad = 8, 3, 20, 128, 8, 128
    x, A, _ = _down_problem(M, K, R, 1)
    buf = torch.full((M, K + 256), SENTINEL, dtype=BF16, device=DEV)
    buf[:, :K] = x.to(DEV)
    keep = buf.clone()
    Ad, sd = A.to(DEV), _scale_matrix(nseg, R, zeros=False).to(DEV)
    out = buf[:, K:]

    def go(s_=sd, ld_=R, seg_rows_=seg_rows, nseg_=nseg):
        call("uv_lora_down_seg_bf16", ptr(buf), buf.stride(0), ptr(Ad), Ad.stride(0), ptr(s_), ld_, seg_rows_, nseg_, M, K, R, ptr(out),
             buf.stride(0), Rpad, stream_ptr())

    for bad in (dict(seg_rows_=0), dict(nseg_=0), dict(nseg_=2), dict(ld_=R - 1), dict(s_=None)):
        with pytest.raises(UnividHipError):
            go(**bad)
    # the wrapper refuses the same before the library is touched
    with pytest.raises(UnividHipError):
        L().lora_down_seg(buf, K, Ad, sd[:2], seg_rows, M=M, Rpad=Rpad)
    with pytest.raises(UnividHipError):
        L().lora_down_seg(buf, K, Ad, sd, 0, M=M, Rpad=Rpad)
    with pytest.raises(UnividHipError):
        L().lora_down_seg(buf, K, Ad, None, seg_rows, M=M, Rpad=Rpad)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep), "a rejected call wrote something"
    go()                                                   # the same call with good arguments runs
    torch.cuda.synchronize()
    assert not torch.equal(buf, keep)


# ---------------------------------------------------------------------------------------------------------------
# model and loop (tiny DiT, two adapters a and b on NAMES18)
# ---------------------------------------------------------------------------------------------------------------
def _manager():
    from univid_amd.lora import LoRAManager
    return LoRAManager()


def _attach_ab(tmp_path, cfg, m, names=NAMES18):
    _write_adapter(str(tmp_path / "a"), _lora_factors(cfg, names, 8, 61, b_std=0.2), 8, 16)
    _write_adapter(str(tmp_path / "b"), _lora_factors(cfg, names, 8, 62, b_std=0.2), 8, 16)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "a"), m, merge=False, name="a")
    mgr.load_lora_weights(str(tmp_path / "b"), m, merge=False, name="b")
    return mgr


@gpu
def test_stacked_samples_take_their_own_adapter_weights(tmp_path):
    """M1: three stacked samples with their own mixes, each bit-identical to a single-sample forward with those values set globally (the
    forwards test_unmerged_adapter_tiny_model_vs_unmerged_oracle gates against the oracle); the all-off sample is the base model.
    The same for the ways a sample's offset into the weights reaches the launches: stacked (an argument of one pass), a mixed-shape batch
    (one pass per sample), block 0's cross_attn.forward re-assigned to a closure (the one call that cannot carry an argument), and both."""
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    x0, t, c0 = g["x"].to(DEV), g["t_one"].to(DEV), g["ctx"].to(DEV)
    xs = [x0, (x0 * 0.5).contiguous(), (x0 + 0.1).contiguous()]
    cs = [c0, (c0 * 0.5).contiguous(), (c0 * 0.8).contiguous()]
    mixes = [{"a": 1.0, "b": 0.0}, {"a": 0.0, "b": 0.5}, {"a": 0.0, "b": 0.0}]
    small = torch.randn(48, 2, 8, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    mixed = [xs[0], small, xs[2]]            # not one shape: the samples run one by one, each at its own offset into the per-sample weights
    ca = m.blocks[0].cross_attn
    original = ca.forward

    def closure(x, context, context_lens=None):      # UniVid's hook reduced to its call of the original bound forward
        return original(x, context, context_lens)
    with torch.no_grad():
        base = [m([xs[i]], t, [cs[i]], LT)[0] for i in range(3)]
        mgr = _attach_ab(tmp_path, cfg, m)
        singles = []
        for i, mix in enumerate(mixes):
            for name, w in mix.items():
                mgr.set_adapter_weight(name, w)
            singles.append(m([xs[i]], t, [cs[i]], LT)[0])
            if i == 1:
                small_single = m([small], t, [cs[1]], LT)[0]
        mgr.set_adapter_weight("a", 1.0)
        mgr.set_adapter_weight("b", 1.0)
        mgr.set_adapter_weights(mixes)
        assert mgr.get_statistics()["per_sample"] is True
        got = m(xs, torch.cat([t, t, t]), cs, LT)
        again = m(xs, torch.cat([t, t, t]), cs, LT)
        got_mixed = m(mixed, torch.cat([t, t, t]), cs, LT)
        ca.forward = closure
        try:
            got_hooked = m(xs, torch.cat([t, t, t]), cs, LT)
            got_mixed_hooked = m(mixed, torch.cat([t, t, t]), cs, LT)
        finally:
            del ca.forward
    for i in range(3):
        assert torch.equal(got[i], singles[i]), f"sample {i} differs from the single-sample forward at its weights"
        assert torch.equal(again[i], got[i])
        want_mixed = small_single if i == 1 else singles[i]
        assert torch.equal(got_mixed[i], want_mixed), f"mixed shapes: sample {i} differs from the single-sample forward at its weights"
        assert torch.equal(got_hooked[i], got[i]), f"re-assigned cross_attn.forward: sample {i} differs from the un-hooked forward"
        assert torch.equal(got_mixed_hooked[i], want_mixed), f"mixed shapes + re-assigned cross_attn.forward: sample {i}"
    assert torch.equal(got[2], base[2]), "a sample with every adapter off must be the base model bit for bit"
    assert not torch.equal(got[0], base[0]) and not torch.equal(got[1], base[1])
    # names left out take the adapter's global weight (a = b = 1 here)
    with torch.no_grad():
        mgr.set_adapter_weights([{}, {"b": 1.0}, {"a": 1.0}])
        full = m(xs, torch.cat([t, t, t]), cs, LT)
        mgr.set_adapter_weights(None)
        assert mgr.get_statistics()["per_sample"] is False
        want = m(xs, torch.cat([t, t, t]), cs, LT)
    assert all(torch.equal(full[i], want[i]) for i in range(3))
    # unloading an adapter that the per-sample weights name clears them
    mgr.set_adapter_weights(mixes)
    mgr.unload("b")
    assert m.adapter_weights() is None and mgr.get_statistics()["per_sample"] is False


@gpu
def test_cfg_pair_with_branch_weights_eager_graph_and_separate_forwards(tmp_path):
    """M2."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    mgr = _attach_ab(tmp_path, cfg, m)
    mgr.set_adapter_weight("b", 0.0)
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    args = (3, g["shift"], g["guide_scale"])
    fresh = []
    runner_for = pipe._runner_for

    def spy(key, make):
        r, f = runner_for(key, make)
        fresh.append(f)
        return r, f
    pipe._runner_for = spy
    with torch.no_grad():
        noise = g["noise"].to(DEV)
        ctx, ctxn = [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()]

        def run(graph, aw=None):
            out = pipe.denoise(noise, ctx, ctxn, *args, graph=graph, adapter_weights=aw).clone()
            assert m.adapter_weights() is None, "the model must be back at global weights after the call"
            return out

        # the reference loop: cond and uncond as two separate forwards, the branch's weight set globally in front of each
        def separate(w_cond, w_uncond):
            n = [0]
            plain = m.forward

            def two_calls(*a, **k):
                mgr.set_adapter_weight("a", w_cond if n[0] % 2 == 0 else w_uncond)
                n[0] += 1
                return plain(*a, **k)
            m.forward = two_calls
            try:
                out = pipe.denoise(noise, ctx, ctxn, *args).clone()
            finally:
                del m.forward
                mgr.set_adapter_weight("a", 1.0)
            assert n[0] == 2 * args[0]
            return out

        # (first: set_adapter_weight moves the prepared-weights generation on, which rightly forgets every captured setting)
        want, want_off, want_half = separate(1.0, 0.0), separate(0.0, 0.0), separate(1.0, 0.5)
        global_on = run(False)
        pair = ({"a": 1.0}, {"a": 0.0})
        eager = run(False, pair)
        assert not fresh
        graphed = run(True, pair)
        assert fresh == [True]
        assert torch.equal(eager, graphed), "eager and graph-replayed pair differ"
        assert torch.equal(eager, want), "the stacked pair differs from two separate forwards (block 0's shared half must not be taken)"
        assert not torch.equal(eager, global_on)
        assert not torch.equal(eager, want_off)
        # a second identical request replays the capture; other weights re-capture; the first ones still replay theirs
        assert torch.equal(run(True, pair), graphed) and fresh == [True, False]
        other = run(True, ({"a": 1.0}, {"a": 0.5}))
        assert fresh == [True, False, True] and not torch.equal(other, graphed)
        assert torch.equal(other, want_half)
        assert torch.equal(run(True, pair), graphed) and fresh == [True, False, True, False]
        # equal branches: today's global-weight run, by one dict or by a pair of them, eager and graph
        assert torch.equal(run(False, ({"a": 1.0}, {"a": 1.0})), global_on)
        assert torch.equal(run(True, {"a": 1.0}), global_on)
        assert torch.equal(run(True), global_on)
        assert mgr.get_statistics()["per_sample"] is False
        pipe._runner = None


@gpu
def test_context_kv_cache_follows_the_per_sample_weights(tmp_path):
    """M3: an adapter on the cross-attention k / v only; between two forwards of the same cached context its per-sample weights change.
    A stale K / V^T cache would give the first result again."""
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    names = [f"blocks.{i}.cross_attn.{p}" for i in range(2) for p in "kv"]
    _write_adapter(str(tmp_path / "kv"), _lora_factors(cfg, names, 8, 71, b_std=0.2), 8, 16)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "kv"), m, merge=False, name="kv")
    x, t, c = [g["x"].to(DEV)], g["t_one"].to(DEV), [g["ctx"].to(DEV)]
    with torch.no_grad():
        on = m(x, t, c, LT)[0]
        mgr.set_adapter_weight("kv", 0.0)
        off = m(x, t, c, LT)[0]
        mgr.set_adapter_weight("kv", 1.0)
        assert not torch.equal(on, off)
        with m.context_cached():
            m.set_adapter_weights([{"kv": 1.0}])
            assert torch.equal(m(x, t, c, LT)[0], on) and torch.equal(m(x, t, c, LT)[0], on)
            m.set_adapter_weights([{"kv": 0.0}])
            assert torch.equal(m(x, t, c, LT)[0], off), "stale K / V^T across a change of per-sample weights"
            m.set_adapter_weights(None)
            assert torch.equal(m(x, t, c, LT)[0], on), "stale K / V^T across the return to global weights"


# ---- guards: everything that is decided without a device runs without one ---------------------------------------------
def _cpu_model_with_adapter(tmp_path):
    from oracle import wan_dit
    from univid_amd.wan.model import WanModel
    cfg = dict(wan_dit.TINY_CFG)
    m = WanModel.from_config(dict(cfg, model_type="ti2v")).eval()
    _write_adapter(str(tmp_path / "a"), _lora_factors(cfg, NAMES18, 8, 81), 8, 16)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "a"), m, merge=False, name="a")
    return cfg, m, mgr


def test_set_adapter_weights_validates_before_any_state_changes(tmp_path):
    """M4: unknown adapter name, non-finite weight, wrong list length - nothing changes, `_prep_gen` included."""
    cfg, m, mgr = _cpu_model_with_adapter(tmp_path)
    gen = m._prep_gen
    for who in (m, mgr):
        with pytest.raises(KeyError, match="nope"):
            who.set_adapter_weights([{"a": 1.0}, {"a": 0.0, "nope": 1.0}])
    for bad in (float("nan"), float("inf"), -math.inf):
        with pytest.raises(ValueError, match="finite"):
            m.set_adapter_weights([{"a": 1.0}, {"a": bad}])
    with pytest.raises(TypeError):
        m.set_adapter_weights([{"a": 1.0}, 0.5])
    assert m.adapter_weights() is None and m._prep_gen == gen and mgr.get_statistics()["per_sample"] is False
    assert all(ad.get("per_sample") is None for lin in m.modules() for ad in getattr(lin, "_uv_lora", {}).values())
    # the list length is checked against the forward's sample count, before anything runs (no device is needed to get there)
    m.set_adapter_weights([{"a": 1.0}, {"a": 0.0}])
    assert m._prep_gen != gen and m.adapter_weights() == [{"a": 1.0}, {"a": 0.0}] and mgr.get_statistics()["per_sample"] is True
    x = torch.zeros(cfg["in_dim"], 4, 16, 16)
    with pytest.raises(ValueError, match=r"2 sample\(s\); this forward has 1 sample"):
        m([x], torch.zeros(1), [torch.zeros(4, cfg["text_dim"])], LT)
    # a setting that comes back gets its generation back; the global weights get theirs
    g2 = m._prep_gen
    m.set_adapter_weights(None)
    assert m._prep_gen == gen and m.adapter_weights() is None
    m.set_adapter_weights([{"a": 1.0}, {"a": 0.0}])
    assert m._prep_gen == g2
    m.set_adapter_weights([{"a": 1.0}, {"a": 0.25}])
    assert m._prep_gen not in (gen, g2)
    mgr.set_adapter_weight("a", 0.5)             # new global strengths: no earlier generation may come back
    g3 = m._prep_gen
    assert g3 not in (gen, g2)
    m.set_adapter_weights(None)
    assert m._prep_gen not in (gen, g2, g3)
    assert not m.generation_alive(g2) and m.generation_alive(m._prep_gen)


def test_sequence_parallel_refuses_differing_rows_before_anything_runs(tmp_path):
    """M4: sequence parallel + per-sample weights that differ -> NotImplementedError naming the setting; equal rows pass the guard."""
    cfg, m, mgr = _cpu_model_with_adapter(tmp_path)

    class TwoRanks:
        size = 2
    m.sp = TwoRanks()
    x = torch.zeros(cfg["in_dim"], 4, 16, 16)
    fwd = lambda: m([x, x], torch.zeros(2), [torch.zeros(4, cfg["text_dim"])] * 2, LT)
    m.set_adapter_weights([{"a": 1.0}, {"a": 0.0}])
    with pytest.raises(NotImplementedError, match="set_adapter_weights"):
        fwd()
    m.set_adapter_weights([{"a": 1.0}, {}])       # the name left out takes the global weight, 1.0: equal rows
    from univid_amd._lib import UnividHipError
    with pytest.raises(UnividHipError):           # past the guard: the forward gets as far as "parameters must be on the GPU"
        fwd()


def test_pipeline_adapter_weights_argument_is_validated_and_restored(tmp_path):
    """M4: WanTI2V.denoise(adapter_weights=) - a bad value raises before the model changes, and the previous setting is restored when the
    loop raises."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    cfg, m, mgr = _cpu_model_with_adapter(tmp_path)
    pipe = WanTI2V(TI2VConfig, model=m, device="cpu")
    gen = m._prep_gen
    noise = torch.zeros(cfg["in_dim"], 4, 16, 16)
    c = [torch.zeros(4, cfg["text_dim"])]
    for bad, err in ((({"a": 1.0}, {"nope": 0.0}), KeyError), (({"a": 1.0}, {"a": float("nan")}), ValueError), (0.5, TypeError),
                     (({"a": 1.0},), TypeError)):
        with pytest.raises(err):
            pipe.denoise(noise, c, c, 2, 5.0, 5.0, graph=False, adapter_weights=bad)
        assert m.adapter_weights() is None and m._prep_gen == gen
    m.set_adapter_weights([{"a": 0.5}, {"a": 0.5}])
    with pytest.raises(Exception):                # no device: the loop itself cannot run - what matters is what it leaves behind
        pipe.denoise(noise, c, c, 2, 5.0, 5.0, graph=False, adapter_weights=({"a": 1.0}, {"a": 0.0}))
    assert m.adapter_weights() == [{"a": 0.5}, {"a": 0.5}]
