"""The three opt-in MXFP8 settings of the DiT COMBINED - ffn_precision x attn_precision x proj_precision, 2 x 3 x 2 = 12 arithmetic
configurations of WanAttentionBlock._run - on every forward path of univid_amd/wan/model.py (-m gpu). The kernels behind the settings are
pinned bit for bit in test_mxfp8 / test_mxproj / test_attn_mxqk / test_attn_mxpv; what is checked here is the host code that wires them
together: which buffer, which operand, which row map goes into which launch. tests/test_mx_mode_matrix_host.py checks the composed oracle
itself without a GPU. The emulations, models, truth run and adapter builders are the other files' (imported, not restated).

1  oracle      emulated(ffn, attn, proj): the single-mode emulations nested; the P.V core extended to masked keys and to b > 1
2  matrix      each of the 11 non-default settings on the small model - t2v (256 tokens), i2v (two timesteps per sample), the 90-token odd
               grid - and the all-on TI2V-5B-width block, against that oracle: gate (a) rms(hip - truth) <= 1.02 rms(emulated - truth)
               (settings with "mxfp8_qk_pv": measured x 1.2, as GATE_BLOCK of test_attn_mxpv - that emulation rounds P against the true row
               maximum, the kernel against the running one), gate (b) rel_rms(hip, emulated) <= measured x 1.2
               (profiles/mx_mode_matrix_margins.json); every setting's output differs from every other's
3  relations   bit identities of the bf16 suite carried into every setting: t_rows, sequence padding, stacking, twins, mixed shapes, the
               order and history of the three set_*_precision calls, per-sample adapter weights, and the all-on denoise (graph == eager,
               native text-weight schedule == closures)
4  modules     the reference-signature forwards of WanSelfAttention (keys masked inside a V^T block), WanCrossAttention and
               WanAttentionBlock (one modulation row per token; a block without norm3) in the settings"""
import contextlib
import itertools
import json
import logging
import os

import pytest
import torch

from conftest import ROOT, load_golden, record_margin
from test_attn_mxpv import emulated_ref, vt_dequant, vt_ref
from test_attn_mxqk import _block_3072, _small_model, emulated_mxqk
from test_gpu_parity import _lora_factors, _rel_rms, _truth_forward, _write_adapter
from test_mxfp8 import _rms, emulated_mxfp8_ffn
from test_mxproj import emulated_mxfp8_proj

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
MARGINS = os.path.join(ROOT, "profiles", "mx_mode_matrix_margins.json")
FFN, ATTN, PROJ = ("bf16", "mxfp8"), ("bf16", "mxfp8_qk", "mxfp8_qk_pv"), ("bf16", "mxfp8")
DEFAULT = ("bf16", "bf16", "bf16")
SETTINGS = [s for s in itertools.product(FFN, ATTN, PROJ) if s != DEFAULT]           # the 11 non-default (ffn, attn, proj)
ALL_ON = ("mxfp8", "mxfp8_qk_pv", "mxfp8")
LT = 256


def sid(s):
    return "ffn_{}-attn_{}-proj_{}".format(*s)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from univid_amd import _lib
    _lib.init()
    yield


@pytest.fixture(autouse=True)
def _default_options():
    from univid_amd import _lib
    _lib.reset_options()
    yield
    _lib.reset_options()


# ---------------------------------------------------------------------------------------------------------------
# 1. the composed emulated oracle
# ---------------------------------------------------------------------------------------------------------------
def mxpv_core(q, k, v, k_lens):
    """The P.V format's core (emulated_ref's arithmetic per head, V quantised-dequantised along the keys, bf16 result) of q, k, v
    [b, l, n, d] with sample i attending its first k_lens[i] keys: the keys at and beyond k_lens[i] are dropped BEFORE V is quantised, so
    that the last 32-key block follows the rule over its keys and zeros (include/univid_hip.h) - a masked key's V never reaches a valid
    key's block scale. Sample by sample."""
    b, lq, n, d = q.shape
    outs = []
    for i in range(b):
        kl = min(int(k_lens[i]), k.shape[1])
        qd, kd = q[i].to(BF16).double().reshape(lq, n * d), k[i, :kl].to(BF16).double().reshape(kl, n * d)
        vd = vt_dequant(*vt_ref(v[i, :kl].to(BF16).reshape(kl, n * d), 1, kl), 1, kl)
        outs.append(emulated_ref(qd, kd, vd, d ** -0.5, 1, n, lq, kl).to(BF16).reshape(lq, n, d))
    return torch.stack(outs).type(q.dtype)


@contextlib.contextmanager
def emulated_mxpv_masked():
    """emulated_mxpv (tests/test_attn_mxpv.py) with the self-attention's core replaced by mxpv_core: masked keys and b > 1."""
    from oracle import wan_dit
    orig = wan_dit.attention_core
    wan_dit.attention_core = lambda q, k, v, k_lens=None: orig(q, k, v) if k_lens is None else mxpv_core(q, k, v, k_lens)
    try:
        with emulated_mxqk():
            yield
    finally:
        wan_dit.attention_core = orig


_PARTS = {"ffn": {"bf16": None, "mxfp8": emulated_mxfp8_ffn},
          "attn": {"bf16": None, "mxfp8_qk": emulated_mxqk, "mxfp8_qk_pv": emulated_mxpv_masked},
          "proj": {"bf16": None, "mxfp8": emulated_mxfp8_proj}}


@contextlib.contextmanager
def emulated(ffn, attn, proj, order=("ffn", "attn", "proj")):
    """The oracle in the setting (ffn, attn, proj): the single-mode emulations nested in `order`. The two `lin` patches fall through to the
    `lin` they captured for keys that are not theirs and the attention patches touch other functions, so every order is the same oracle
    (asserted in tests/test_mx_mode_matrix_host.py). Everything is undone on exit, in reverse order."""
    chosen = dict(ffn=_PARTS["ffn"][ffn], attn=_PARTS["attn"][attn], proj=_PARTS["proj"][proj])
    assert sorted(order) == ["attn", "ffn", "proj"]
    with contextlib.ExitStack() as stack:
        for name in order:
            if chosen[name] is not None:
                stack.enter_context(chosen[name]())
        yield


@contextlib.contextmanager
def fp32_oracle():
    """The oracle's module functions with every bf16 rounding removed: the truth of the module-level cases."""
    from oracle import wan_dit
    old, wan_dit.BF16 = wan_dit.BF16, torch.float32
    try:
        yield
    finally:
        wan_dit.BF16 = old


# ---------------------------------------------------------------------------------------------------------------
# the gates
# ---------------------------------------------------------------------------------------------------------------
def _margin(name, key):
    with open(MARGINS) as f:
        return float(json.load(f)[name][key])


def _check(name, setting, hip, emu, truth):
    """Records and prints the figures, then gates: (a) rms(hip - truth) <= 1.02 rms(emulated oracle - truth) - with "mxfp8_qk_pv" the ratio
    measured on the MI355X x 1.2, as GATE_BLOCK of tests/test_attn_mxpv.py and for its reason: emulated_ref rounds P against the true row
    maximum, the kernel against the running one - and (b) rel_rms(hip, emulated oracle) <= measured x 1.2."""
    e_hip, e_emu = _rms(hip, truth), _rms(emu, truth)
    rel = _rel_rms(hip, emu)
    m = dict(rel_rms_vs_emulated_oracle=rel, truth_ratio=e_hip / e_emu, rms_vs_truth_hip=e_hip, rms_vs_truth_emulated_oracle=e_emu,
             truth_rms=truth.float().pow(2).mean().sqrt().item())
    record_margin("mx_mode_matrix " + name, **m)
    print("mx_mode_matrix " + name, json.dumps(m))
    assert torch.isfinite(hip).all()
    gate_a = 1.2 * _margin(name, "truth_ratio") if setting[1] == "mxfp8_qk_pv" else 1.02
    assert e_hip <= gate_a * e_emu, f"{name}: rms vs truth {e_hip:.4e}, the emulated oracle's {e_emu:.4e} (gate {gate_a:.4f})"
    gate_b = 1.2 * _margin(name, "rel_rms_vs_emulated_oracle")
    assert rel <= gate_b, f"{name}: rel rms vs the emulated oracle {rel:.4e} > gate {gate_b:.4e}"


# ---------------------------------------------------------------------------------------------------------------
# 2. every combination against the oracle
# ---------------------------------------------------------------------------------------------------------------
def _apply(m, setting):
    m.set_ffn_precision(setting[0]), m.set_attn_precision(setting[1]), m.set_proj_precision(setting[2])
    return m


_models, _cases, _truths, _hips = {}, {}, {}, {}


def _model(setting):
    """(cfg, sd, model in the setting): one per setting, shared by the tests that only read it."""
    if setting not in _models:
        cfg, sd, m = _small_model(load_golden("dit_tiny")["seed"])
        _models[setting] = (cfg, sd, m if setting == DEFAULT else _apply(m, setting))          # (the default model never switched)
    return _models[setting]


def cases():
    """name -> (x, t, context, seq_len) on the CPU: the dit_tiny golden inputs with one and with two timesteps per sample, and the
    (3, 5, 6) grid of test_dit_head_dim_128_and_odd_grid: 90 tokens, no multiple of 4, 8, 32 or 64."""
    if not _cases:
        g = load_golden("dit_tiny")
        gen = torch.Generator().manual_seed(11)
        x90, ctx90 = torch.randn(48, 3, 10, 12, generator=gen), torch.randn(32, 64, generator=gen)
        assert g["t_two"].unique().numel() == 2 and g["t_one"].unique().numel() == 1
        _cases.update(t2v=(g["x"], g["t_one"], g["ctx"], LT), i2v=(g["x"], g["t_two"], g["ctx"], LT),
                      odd90=(x90, torch.full((1, 90), 500.0), ctx90, 90))
    return _cases


def _truth(case, cfg, sd):
    if case not in _truths:
        x, t, ctx, n = cases()[case]
        with torch.no_grad():
            _truths[case] = _truth_forward(sd, cfg, [x], t, [ctx], n)[0]
    return _truths[case]


def _hip(setting, case):
    if (setting, case) not in _hips:
        x, t, ctx, n = cases()[case]
        with torch.no_grad():
            _hips[(setting, case)] = _model(setting)[2]([x.to(DEV)], t.to(DEV), [ctx.to(DEV)], n)[0]
    return _hips[(setting, case)]


@pytest.mark.parametrize("case", ["t2v", "i2v", "odd90"])
@pytest.mark.parametrize("setting", SETTINGS, ids=sid)
def test_setting_against_the_composed_oracle(setting, case):
    from oracle import wan_dit
    cfg, sd, _ = _model(setting)
    x, t, ctx, n = cases()[case]
    got = _hip(setting, case)
    with torch.no_grad(), emulated(*setting):
        emu = wan_dit.dit_forward(sd, cfg, [x], t, [ctx], n)[0]
    _check(f"{sid(setting)} {case}", setting, got, emu, _truth(case, cfg, sd))


def test_every_setting_differs_from_every_other():
    """Two settings with equal bits would mean a switch that does nothing; with the oracle's settings pairwise different too (host file),
    the gates above cannot be met by the wrong setting's arithmetic by accident of equality."""
    outs = {s: _hip(s, "t2v") for s in [DEFAULT] + SETTINGS}
    for a, b in itertools.combinations(outs, 2):
        assert not torch.equal(outs[a], outs[b]), f"{sid(a)} and {sid(b)} give the same bits"


def test_all_on_block_ti2v5b_width():
    """One TI2V-5B-width block (dim 3072, 24 heads, ffn 14336) at 48 tokens through _run with the golden token -> row map, everything on."""
    from oracle import wan_dit
    from univid_amd.wan.model import _freqs_device
    g = load_golden("dit_block_3072")
    blk, sdc = _block_3072(g["seed"])
    heads, d, Lt = 24, 128, 48
    blk.set_ffn_precision(ALL_ON[0]), blk.set_attn_precision(ALL_ON[1]), blk.set_proj_precision(ALL_ON[2])
    fr = _freqs_device(wan_dit.rope_table(d), torch.device(DEV))
    x = g["x"][0].to(DEV).clone()
    with torch.no_grad():
        blk._run(x, Lt, g["e_rows"].reshape(2, -1).to(DEV), g["tid"].to(torch.int32).to(DEV), (2, 4, 6), fr, g["ctx"][0].to(DEV), first_block=False)
    args = (sdc, "blocks.0.", g["x"], g["e_rows"][g["tid"]].unsqueeze(0), torch.tensor([Lt]), g["grid"], wan_dit.rope_table(d))
    with torch.no_grad(), emulated(*ALL_ON):
        emu = wan_dit.block_forward(*args, g["ctx"], heads, 1e-6)[0]
    with torch.no_grad(), fp32_oracle():
        truth = wan_dit.block_forward(*args, g["ctx"].float(), heads, 1e-6)[0]
    _check(f"{sid(ALL_ON)} block 3072 L48", ALL_ON, x, emu, truth)


# ---------------------------------------------------------------------------------------------------------------
# 3. bit-identity relations, in every setting
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=sid)
def test_forward_paths_are_bit_identical(setting):
    g = load_golden("dit_tiny")
    cfg, sd, m = _model(setting)
    gen = torch.Generator().manual_seed(5)
    xa, xb = g["x"].to(DEV), torch.randn(48, 4, 16, 16, generator=gen).to(DEV)
    ca, cb = g["ctx"].to(DEV), torch.randn(7, cfg["text_dim"], generator=gen).to(DEV)
    small = torch.randn(48, 4, 8, 8, generator=gen).to(DEV)                    # 4 x 4 x 4 = 64 tokens
    t1, t2, tb = g["t_one"].to(DEV), g["t_two"].to(DEV), torch.full((1, LT), 321.0, device=DEV)
    with torch.no_grad():
        one, two = _hip(setting, "t2v"), _hip(setting, "i2v")
        # the caller's own table of distinct timesteps instead of the per-token tensor
        tvals, inv = torch.unique(t2.flatten(), return_inverse=True)
        rows = m([xa], None, [ca], LT, t_rows=(tvals.float().contiguous(), inv.to(torch.int32).contiguous(), True))[0]
        assert torch.equal(rows, two), "t_rows= differs from t [1, seq_len]"
        # a padded sequence: seq_len 300, the timesteps of the 44 padding tokens a third value
        pad = m([xa], torch.cat([t2, torch.full((1, 44), 55.0, device=DEV)], 1), [ca], 300)[0]
        assert torch.equal(pad, two), "sequence padding changed the valid tokens"
        # two different samples stacked
        b = m([xb], tb, [cb], LT)[0]
        both = m([xa, xb], torch.cat([t2, tb]), [ca, cb], LT)
        assert torch.equal(both[0], two) and torch.equal(both[1], b) and not torch.equal(two, b), "the stacked pair differs from single forwards"
        # the CFG pair on one latent: block 0's shared self-attention half
        c2 = (ca * 0.5).contiguous()
        for t, single in ((t1, one), (t2, two)):
            other = m([xa], t, [c2], LT)[0]
            m.dedup_twins = True
            on = m([xa, xa], torch.cat([t, t]), [ca, c2], LT)
            m.dedup_twins = False
            try:
                off = m([xa, xa], torch.cat([t, t]), [ca, c2], LT)
            finally:
                m.dedup_twins = True
            assert torch.equal(on[0], single) and torch.equal(on[1], other) and not torch.equal(single, other), "twins (dedup on) differ from single forwards"
            assert torch.equal(off[0], single) and torch.equal(off[1], other), "twins (dedup off) differ from single forwards"
        # mixed shapes run one by one
        s_alone = m([small], tb, [cb], LT)[0]
        mixed = m([xa, small], torch.cat([t2, tb]), [ca, cb], LT)
        assert torch.equal(mixed[0], two) and torch.equal(mixed[1], s_alone) and torch.isfinite(s_alone).all(), "the mixed-shape pair differs from single forwards"


@pytest.mark.parametrize("setting", SETTINGS, ids=sid)
def test_order_and_history_of_the_switches_do_not_matter(setting):
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("dit_tiny")
    x, t, ctx = g["x"].to(DEV), g["t_two"].to(DEV), g["ctx"].to(DEV)
    want, base = _hip(setting, "i2v"), _hip(DEFAULT, "i2v")
    calls = dict(ffn=("set_ffn_precision", setting[0]), attn=("set_attn_precision", setting[1]), proj=("set_proj_precision", setting[2]))
    with torch.no_grad():
        cfg, sd, m = _small_model(g["seed"])
        for order in itertools.permutations(calls):
            for name in order:
                gen = m._prep_gen
                getattr(m, calls[name][0])(calls[name][1])
                assert m._prep_gen > gen, f"{calls[name][0]} did not move _prep_gen on"
            assert (m.ffn_precision, m.attn_precision, m.proj_precision) == setting
            assert torch.equal(m([x], t, [ctx], LT)[0], want), f"order {order} gives other bits"
            # ... and back to the default, in the same order: a model that never switched
            for name in order:
                gen = m._prep_gen
                getattr(m, calls[name][0])("bf16")
                assert m._prep_gen > gen
            assert torch.equal(m([x], t, [ctx], LT)[0], base), f"bf16 after a round trip through {sid(setting)} (order {order}) differs from a model that never switched"
        pipe = WanTI2V(TI2VConfig, model=_small_model(g["seed"])[2], device=DEV, ffn_precision=setting[0], attn_precision=setting[1],
                       proj_precision=setting[2])
        assert (pipe.model.ffn_precision, pipe.model.attn_precision, pipe.model.proj_precision) == setting
        assert torch.equal(pipe.model([x], t, [ctx], LT)[0], want), "the constructor path gives other bits"


@pytest.mark.parametrize("setting", SETTINGS, ids=sid)
def test_per_sample_adapter_weights_on_the_context_projections(setting, tmp_path):
    """An un-merged adapter on cross_attn.k / v - the projections where un-merged is legal in every setting - with per-sample weights
    [1, 0] on a stacked pair: sample 0 is the single forward with the adapter, sample 1 the model without it."""
    from univid_amd.lora import LoRAManager
    g = load_golden("dit_tiny")
    cfg, sd, m = _small_model(g["seed"])
    _apply(m, setting)
    names = [f"blocks.{i}.cross_attn.{p}" for i in range(cfg["num_layers"]) for p in "kv"]
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, names, 8, 71, b_std=0.2), 8, 16)
    gen = torch.Generator().manual_seed(5)
    xa, xb = g["x"].to(DEV), torch.randn(48, 4, 16, 16, generator=gen).to(DEV)
    ca, cb = g["ctx"].to(DEV), torch.randn(7, cfg["text_dim"], generator=gen).to(DEV)
    t = g["t_two"].to(DEV)
    mgr = LoRAManager()
    with torch.no_grad():
        plain_a, plain_b = m([xa], t, [ca], LT)[0], m([xb], t, [cb], LT)[0]
        assert torch.equal(plain_a, _hip(setting, "i2v"))
        mgr.load_lora_weights(str(tmp_path / "A"), m, merge=False, name="A")
        with_a = m([xa], t, [ca], LT)[0]
        assert not torch.equal(with_a, plain_a) and torch.isfinite(with_a).all()
        m.set_adapter_weights([{"A": 1.0}, {"A": 0.0}])
        pair = m([xa, xb], torch.cat([t, t]), [ca, cb], LT)
        assert torch.equal(pair[0], with_a), "the weight-1 sample of the stacked pair differs from the single forward with the adapter"
        assert torch.equal(pair[1], plain_b), "the weight-0 sample of the stacked pair differs from the model without the adapter"
        m.set_adapter_weights(None)
        mgr.unload("A")
        assert torch.equal(m([xa], t, [ca], LT)[0], plain_a), "unload does not restore the bits"


def test_all_on_i2v_denoise_text_weight_graph_eager_and_closures():
    """Everything on, 2 steps of the i2v loop (z=) under UniVid's dynamic text weight: the HIP-graph replay, the eager loop and the
    reference's closure path (`forward` re-assigned on every cross-attention) give the same bits."""
    from univid_amd.model_pipeline import CrossAttentionConfig, Wan22ContextWrapper
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    cfg, sd, m = _small_model(g["seed"])
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV, ffn_precision=ALL_ON[0], attn_precision=ALL_ON[1], proj_precision=ALL_ON[2])
    args = ([g["ctx"].to(DEV)], [g["ctx_null"].to(DEV)], 2, g["shift"], g["guide_scale"])

    def gen(native, graph):
        ccfg = CrossAttentionConfig(use_dynamic_text_weight=True, total_sampling_steps=8, text_weight_transition_ratio=0.5)
        wr = Wan22ContextWrapper(pipe, None, logging.getLogger("test_mx_mode_matrix"), ccfg, native=native)
        wr.set_bagel_context(torch.zeros(1, 4, 8))
        assert native or all("forward" in b.cross_attn.__dict__ for b in m.blocks)
        try:
            with torch.no_grad(), wr.scheduled():
                return pipe.denoise(g["noise"].to(DEV), *args, z=g["z"].to(DEV), graph=graph).clone()
        finally:
            wr.restore_original_methods()

    graphed = gen(True, True)
    assert pipe._runner is not None and torch.isfinite(graphed).all()
    assert torch.equal(graphed, gen(True, False)), "graph != eager with everything on"
    assert torch.equal(graphed, gen(False, None)), "the closure path differs from the native schedule with everything on"
    with torch.no_grad():
        plain = pipe.denoise(g["noise"].to(DEV), *args, z=g["z"].to(DEV), graph=True).clone()
        t2v = pipe.denoise(g["noise"].to(DEV), *args, graph=True).clone()
    assert not torch.equal(plain, graphed), "the text weight must change the result"
    assert not torch.equal(plain, t2v), "z= must change the result"
    pipe._runner = None


# ---------------------------------------------------------------------------------------------------------------
# 4. the reference-signature module forwards, in the settings
# ---------------------------------------------------------------------------------------------------------------
DIM, HEADS, EPS = 256, 2, 1e-6
GRIDS, LENS, ROWS = [(2, 5, 7), (2, 5, 6)], [70, 60], 76           # 70 and 60 keys inside 76 rows: the last V^T block holds keys and pad


def _module(cls, prefix, seed=4, **kw):
    """(module on the GPU, its state dict on the CPU), weights from detinit - and then every Linear weight multiplied by a power of two
    (1/2, 1, 2, 4) that moves with the output row (groups of 16), the 32-column block and the projection. detinit gives all projections of
    this size one magnitude, so that all their MX scale bytes agree: a GEMM wired to ANOTHER projection's scales (q's for k) computed the
    same values, and a uniform difference would vanish in norm_q / norm_k anyway."""
    from univid_amd import detinit
    with torch.device(DEV):
        mod = cls(**kw)
    sd = {prefix + k: v for k, v in mod.state_dict(keep_vars=True).items()}
    detinit.init_state_dict_(sd, seed)
    lins = sorted(k for k, v in sd.items() if k.endswith(".weight") and v.dim() == 2)
    with torch.no_grad():
        for i, k in enumerate(lins):
            n, kk = sd[k].shape
            e = (torch.arange(n).view(-1, 1) // 16 + 2 * (torch.arange(kk).view(1, -1) // 32) + i) % 4 - 1
            sd[k].mul_(torch.exp2(e.float()).to(sd[k].device))
    mod._prep = None
    return mod.eval(), {k: v.detach().cpu() for k, v in sd.items()}


def _module_inputs():
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, ROWS, DIM, generator=g)
    ctx = (torch.randn(2, 32, DIM, generator=g) * 0.5).to(BF16)
    return x, ctx


def _valid(t, lens):
    return torch.cat([t[b, :n].float().cpu() for b, n in enumerate(lens)])


@pytest.mark.parametrize("attn", ["mxfp8_qk", "mxfp8_qk_pv"])
@pytest.mark.parametrize("proj", PROJ)
def test_self_attention_forward_with_masked_keys(attn, proj):
    from oracle import wan_dit
    from univid_amd.wan.model import WanSelfAttention
    mod, sdc = _module(WanSelfAttention, "blocks.0.self_attn.", dim=DIM, num_heads=HEADS, window_size=(-1, -1), qk_norm=True, eps=EPS)
    mod.attn_precision, mod.proj_precision, mod._prep = attn, proj, None
    x, _ = _module_inputs()
    freqs = wan_dit.rope_table(DIM // HEADS)
    lens, grids = torch.tensor(LENS), torch.tensor(GRIDS)
    setting = ("bf16", attn, proj)
    with torch.no_grad():
        got = mod(x.to(DEV), lens, grids, freqs)
        with emulated(*setting):
            emu = wan_dit.self_attention(sdc, "blocks.0.self_attn.", x, lens, grids, freqs, HEADS, EPS)
        with fp32_oracle():
            truth = wan_dit.self_attention(sdc, "blocks.0.self_attn.", x, lens, grids, freqs, HEADS, EPS)
        # the padding rows of x replaced by other finite values, far larger than any valid row: a masked key's V that reached a valid
        # key's V^T block scale - or a masked key that was attended - would move the valid rows
        x2 = x.clone()
        for b, n in enumerate(LENS):
            x2[b, n:] = 40.0 * torch.randn(ROWS - n, DIM, generator=torch.Generator().manual_seed(b))
        got2 = mod(x2.to(DEV), lens, grids, freqs)
    assert got.dtype == BF16 and got.shape == emu.shape
    for b, n in enumerate(LENS):
        assert torch.equal(got2[b, :n], got[b, :n]), f"sample {b}: the valid rows depend on the padding rows"
    _check(f"{sid(setting)} self_attn.forward 70/60 of 76", setting, _valid(got, LENS), _valid(emu, LENS), _valid(truth, LENS))


def test_cross_attention_forward_proj_mxfp8():
    from oracle import wan_dit
    from univid_amd.wan.model import WanCrossAttention
    mod, sdc = _module(WanCrossAttention, "blocks.0.cross_attn.", dim=DIM, num_heads=HEADS, window_size=(-1, -1), qk_norm=True, eps=EPS)
    mod.proj_precision, mod._prep = "mxfp8", None
    x, ctx = _module_inputs()
    setting = ("bf16", "bf16", "mxfp8")
    with torch.no_grad():
        got = mod(x.to(DEV), ctx.to(DEV), None)
        with emulated(*setting):
            emu = wan_dit.cross_attention(sdc, "blocks.0.cross_attn.", x, ctx, HEADS, EPS)
        with fp32_oracle():
            truth = wan_dit.cross_attention(sdc, "blocks.0.cross_attn.", x, ctx.float(), HEADS, EPS)
    assert got.dtype == BF16 and got.shape == emu.shape
    assert mod._prep["q"].w.dtype == torch.uint8 and mod._prep["o"].w.dtype == torch.uint8 and mod._prep["k"].w.dtype == BF16
    _check(f"{sid(setting)} cross_attn.forward", setting, got.float().cpu(), emu.float(), truth.float())


def _block(cross_attn_norm=True):
    from univid_amd.wan.model import WanAttentionBlock
    return _module(WanAttentionBlock, "blocks.0.", seed=3, dim=DIM, ffn_dim=512, num_heads=HEADS, window_size=(-1, -1), qk_norm=True,
                   cross_attn_norm=cross_attn_norm, eps=EPS)


def test_block_forward_one_modulation_row_per_token_all_on():
    """WanAttentionBlock.forward(x, e [B, L, 6, C], ...): tid = arange(L) goes into uv_layernorm_mod_mx and the MX GEMM's gated epilogue. 70
    tokens (no multiple of 4), two samples."""
    from oracle import wan_dit
    from univid_amd.wan.model import _freqs_device
    blk, sdc = _block()
    blk.set_ffn_precision(ALL_ON[0]), blk.set_attn_precision(ALL_ON[1]), blk.set_proj_precision(ALL_ON[2])
    Lt, grid = 70, (2, 5, 7)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, Lt, DIM, generator=g)
    e = torch.randn(2, Lt, 6, DIM, generator=g) * 0.3
    ctx = (torch.randn(2, 32, DIM, generator=g) * 0.5).to(BF16)
    freqs = wan_dit.rope_table(DIM // HEADS)
    lens, grids = torch.tensor([Lt, Lt]), torch.tensor([grid, grid])
    with torch.no_grad():
        got = blk(x.to(DEV), e.to(DEV), lens, grids, freqs, ctx.to(DEV))
        with emulated(*ALL_ON):
            emu = wan_dit.block_forward(sdc, "blocks.0.", x, e, lens, grids, freqs, ctx, HEADS, EPS)
        with fp32_oracle():
            truth = wan_dit.block_forward(sdc, "blocks.0.", x, e, lens, grids, freqs, ctx.float(), HEADS, EPS)
        assert got.dtype == torch.float32 and got.shape == emu.shape
        fr = _freqs_device(freqs, torch.device(DEV))
        tid = torch.arange(Lt, dtype=torch.int32, device=DEV)
        for b in range(2):
            xb = x[b].to(DEV).clone()
            blk._run(xb, Lt, e[b].reshape(Lt, -1).to(DEV).contiguous(), tid, grid, fr, ctx[b].to(DEV), first_block=False, s0=b)
            assert torch.equal(xb, got[b]), f"sample {b}: forward differs from _run on the same per-token table"
        # the same modulation values as a 3-row table with a token -> row map: other rows of another table, the same bits
        e_rows = torch.randn(3, 6 * DIM, generator=g) * 0.3
        tmap = (torch.arange(Lt) * 7 % 3).to(torch.int32)
        tok = blk(x[:1].to(DEV), e_rows[tmap.long()].reshape(1, Lt, 6, DIM).to(DEV), lens[:1], grids[:1], freqs, ctx[:1].to(DEV))[0]
        xr = x[0].to(DEV).clone()
        blk._run(xr, Lt, e_rows.to(DEV), tmap.to(DEV), grid, fr, ctx[0].to(DEV), first_block=False)
        assert torch.equal(xr, tok) and not torch.equal(tok, got[0]), "a row map into a 3-row table differs from one row per token"
    _check(f"{sid(ALL_ON)} block.forward per-token e L70", ALL_ON, got, emu, truth)


def test_block_without_norm3_proj_mxfp8():
    """cross_attn_norm=False: the cross-attention's input is the fp32 stream cast to bf16 and then quantised (uv_cast_f32_bf16 + uv_mx_quant_bf16)
    instead of uv_layernorm_mod_mx. The oracle's block_forward always applies norm3: its layer_norm returns x unchanged for the one call
    that carries a weight, for the duration."""
    from oracle import wan_dit
    blk, sdc = _block(cross_attn_norm=False)
    assert isinstance(blk.norm3, torch.nn.Identity) and "blocks.0.norm3.weight" not in sdc
    sdc = dict(sdc, **{"blocks.0.norm3.weight": torch.ones(DIM), "blocks.0.norm3.bias": torch.zeros(DIM)})
    setting = ("bf16", "bf16", "mxfp8")
    blk.set_proj_precision("mxfp8")
    Lt, grid = 70, (2, 5, 7)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(1, Lt, DIM, generator=g)
    e = torch.randn(1, Lt, 6, DIM, generator=g) * 0.3
    ctx = (torch.randn(1, 32, DIM, generator=g) * 0.5).to(BF16)
    freqs = wan_dit.rope_table(DIM // HEADS)
    lens, grids = torch.tensor([Lt]), torch.tensor([grid])
    orig = wan_dit.layer_norm
    wan_dit.layer_norm = lambda x_, eps, weight=None, bias=None: x_ if weight is not None else orig(x_, eps)
    try:
        with torch.no_grad():
            got = blk(x.to(DEV), e.to(DEV), lens, grids, freqs, ctx.to(DEV))
            with emulated(*setting):
                emu = wan_dit.block_forward(sdc, "blocks.0.", x, e, lens, grids, freqs, ctx, HEADS, EPS)
            with fp32_oracle():
                truth = wan_dit.block_forward(sdc, "blocks.0.", x, e, lens, grids, freqs, ctx.float(), HEADS, EPS)
    finally:
        wan_dit.layer_norm = orig
    _check(f"{sid(setting)} block without norm3 L70", setting, got, emu, truth)
