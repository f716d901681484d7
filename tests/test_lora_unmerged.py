"""Un-merged LoRA on the GEMM path (univid_amd/lora.py, `merge=False`): the down-projection kernel uv_lora_down_bf16, the GEMM property
it relies on (zero weight columns behind K change no bit), and the model / manager behaviour - parity with the un-merged oracle
(oracle/lora.py), per-module rank / alpha patterns, stacking, swapping, the stacked CFG pair, the HIP-graph runner and the guards."""
import pytest
import torch

from conftest import load_golden, record_margin
from test_gpu_parity import (_lora_factors, _rel_rms, _sd_with_adapter, _tiny_model, _truth_forward, _write_adapter, assert_bf16_kernel,
                             assert_model_close)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
SENTINEL = 3.0


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


def L():
    from univid_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------------------
def _down_problem(M, K, R, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(BF16)
    A = (torch.randn(R, K, generator=g) / K ** 0.5).to(BF16)
    scale = (0.37 + 0.0131 * torch.arange(R)).float()             # distinct, none a power of two
    return x, A, scale


@pytest.mark.parametrize("M,K,R,Rpad", [(1, 64, 8, 128), (63, 192, 16, 128), (257, 3072, 40, 128), (1014, 3072, 128, 128),
                                        (300, 14336, 48, 128), (130, 256, 136, 256)])
def test_lora_down_vs_double_precision_in_place(M, K, R, Rpad):
    """K1: out = x + K (the slot behind the activation's own columns), one spare row below M; everything outside [0, M) x [K, K + Rpad)
    keeps the sentinel, columns [K + R, K + Rpad) are exactly 0, the rest is the double-precision product rounded once."""
    x, A, scale = _down_problem(M, K, R, M + K + R)
    buf = torch.full((M + 1, K + Rpad), SENTINEL, dtype=BF16)
    buf[:M, :K] = x
    ref = (scale.double() * (x.double() @ A.double().t())).to(BF16)
    dbuf = buf.to(DEV)
    L().lora_down(dbuf, K, A.to(DEV), scale.to(DEV), M=M, Rpad=Rpad)
    got = dbuf.cpu()
    assert torch.equal(got[:, :K], buf[:, :K]), "the activation's own columns were written"
    assert torch.equal(got[M], buf[M]), "the row below M was written"
    assert (got[:M, K + R:].view(torch.int16) == 0).all(), "slot columns beyond R must be exactly +0"
    assert_bf16_kernel(got[:M, K:K + R], ref, name=f"lora_down {M}x{K} R={R}")


def test_lora_down_rows_do_not_depend_on_the_launch():
    """K2: rows [100, 200) of an M = 700 launch against a launch on those rows alone."""
    M, K, R = 700, 3072, 16
    x, A, scale = _down_problem(M, K, R, 7)
    big = torch.zeros(M, K + 128, dtype=BF16, device=DEV)
    big[:, :K] = x.to(DEV)
    small = big[100:200].clone()
    L().lora_down(big, K, A.to(DEV), scale.to(DEV))
    L().lora_down(small, K, A.to(DEV), scale.to(DEV))
    assert torch.equal(big[100:200], small)
    assert big[:, K:K + R].float().abs().sum() > 0


def test_lora_down_rejects_bad_arguments_and_writes_nothing():
    """K3."""
    from univid_amd._lib import UnividHipError, call, ptr, stream_ptr
    M, K, R, Rpad = 20, 128, 8, 128
    x, A, scale = _down_problem(M, K, R, 1)
    buf = torch.full((M, K + 256), SENTINEL, dtype=BF16, device=DEV)
    keep = buf.clone()
    Ad, sd = A.to(DEV), scale.to(DEV)
    out = buf[:, K:]

    def go(x_=buf, A_=Ad, s_=sd, out_=out, K_=K, R_=R, Rpad_=Rpad):
        call("uv_lora_down_bf16", ptr(x_), buf.stride(0), ptr(A_), Ad.stride(0), ptr(s_), M, K_, R_, ptr(out_), buf.stride(0), Rpad_, stream_ptr())

    for bad in (dict(K_=96), dict(R_=129), dict(Rpad_=64), dict(Rpad_=192), dict(R_=0), dict(x_=None), dict(A_=None), dict(s_=None),
                dict(out_=None)):
        with pytest.raises(UnividHipError):
            go(**bad)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep), "a rejected call wrote something"
    go()                                                   # the same call with good arguments runs
    torch.cuda.synchronize()
    assert not torch.equal(buf, keep)


@pytest.mark.parametrize("M,N,K", [(257, 3072, 3072), (300, 512, 256)])
def test_gemm_zero_weight_columns_behind_k_change_no_bit(M, N, K):
    """K4: uv_gemm_bf16_nt over K + 128 columns with lda = ldw = K + 128, the extra weight columns zero and the extra activation columns
    finite garbage, against the plain K launch - the property that lets [x | T] . [W | B | 0]^T leave un-adapted bits alone."""
    from univid_amd._lib import EPI_BF16, EPI_BF16_T, EPI_GATE_RESID_F32, EPI_GELU_BF16
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(BF16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16).to(DEV)
    ae = torch.cat([a, (torch.randn(M, 128, generator=g) * 7).to(BF16).to(DEV)], 1).contiguous()
    we = torch.cat([w, torch.zeros(N, 128, dtype=BF16, device=DEV)], 1).contiguous()
    x0 = torch.randn(M, N, generator=g).to(DEV)
    gate = torch.randn(3, N, generator=g).to(DEV)
    tid = torch.randint(0, 3, (M,), generator=g, dtype=torch.int32).to(DEV)
    Mp = (M + 63) // 64 * 64
    for epi, name in ((EPI_BF16, "BF16"), (EPI_GELU_BF16, "GELU_BF16"), (EPI_BF16_T, "BF16_T"), (EPI_GATE_RESID_F32, "GATE_RESID_F32")):
        outs = []
        for aa, ww in ((a, w), (ae, we)):
            if epi == EPI_BF16_T:
                out = torch.zeros(N, Mp, dtype=BF16, device=DEV)
            elif epi == EPI_GATE_RESID_F32:
                out = x0.clone()
            else:
                out = torch.zeros(M, N, dtype=BF16, device=DEV)
            kw = dict(gate=gate, gate_tid=tid) if epi == EPI_GATE_RESID_F32 else {}
            L().gemm_bf16(aa, ww, bias, out, epi, **kw)
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), f"{name}: K + 128 launch differs from the plain one"


# ---------------------------------------------------------------------------------------------------------------
# model and interface (tiny DiT)
# ---------------------------------------------------------------------------------------------------------------
LT = 256
NAMES18 = [f"blocks.{i}.{a}.{p}" for i in range(2) for a in ("cross_attn", "self_attn") for p in "qkvo"] + ["blocks.1.ffn.0", "blocks.0.ffn.2"]
NAMES20 = [f"blocks.{i}.{a}.{p}" for i in range(2) for a in ("cross_attn", "self_attn") for p in "qkvo"] + \
          [f"blocks.{i}.ffn.{j}" for i in range(2) for j in (0, 2)]


def _setup():
    g = load_golden("dit_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    args = ([g["x"].to(DEV)], g["t_one"].to(DEV), [g["ctx"].to(DEV)], LT)
    return g, cfg, sd, m, args


def _fwd(m, args):
    with torch.no_grad():
        return m(*args)[0]


def _manager():
    from univid_amd.lora import LoRAManager
    return LoRAManager()


def test_zero_adapter_and_zero_weight_are_the_base_model(tmp_path):
    """M1."""
    g, cfg, sd, m, args = _setup()
    base = _fwd(m, args)
    zero = {n: (a, torch.zeros_like(b)) for n, (a, b) in _lora_factors(cfg, NAMES20, 8, 3).items()}
    _write_adapter(str(tmp_path / "zero"), zero, 8, 16)
    _write_adapter(str(tmp_path / "live"), _lora_factors(cfg, NAMES20, 8, 5, b_std=0.2), 8, 16)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "zero"), m, merge=False)
    assert m.blocks[0]._prep is None and m.blocks[0].self_attn._prep is None       # re-prepared by the next forward
    assert torch.equal(_fwd(m, args), base), "an adapter with lora_B = 0 changed the output"
    assert m.blocks[0].self_attn._slots["qkv"].S == 128 and m.blocks[1]._prep["ffn2"].w.shape[1] == cfg["ffn_dim"] + 128
    mgr.unload()
    mgr.load_lora_weights(str(tmp_path / "live"), m, merge=False, weight=0.0)
    assert torch.equal(_fwd(m, args), base), "an adapter at weight 0 changed the output"
    mgr.set_adapter_weight("default", 1.0)
    assert not torch.equal(_fwd(m, args), base)


def _check_vs_oracle(got, base, g, cfg, sd_l, name):
    from oracle import wan_dit
    with torch.no_grad():
        ref = wan_dit.dit_forward(sd_l, cfg, [g["x"]], g["t_one"], [g["ctx"]], LT)[0]
        truth = _truth_forward(sd_l, cfg, [g["x"]], g["t_one"], [g["ctx"]], LT)[0]
    effect = _rel_rms(ref, g["out_one"])
    assert effect > 0.05, f"the test adapter must move the output well above the bf16 noise floor (moved it by {effect:.3f})"
    d_hip, d_ref = (got - base).cpu(), ref - g["out_one"]
    rel = float((d_hip - d_ref).pow(2).mean().sqrt() / d_ref.pow(2).mean().sqrt())
    record_margin(f"{name}: error of the adapter's effect (rel rms)", effect_rel_rms=rel, effect_size=effect)
    print(f"{name}: adapter effect {effect:.4f}, its error {rel:.4e}")
    assert_model_close(got, ref, truth, frac=0.55, max_rel=1.5e-3, truth_ratio=1.05, name=name)
    assert rel < 1.2e-2, f"adapter effect off by {rel:.3e}"


def test_unmerged_adapter_tiny_model_vs_unmerged_oracle(tmp_path):
    """M2: the adapter of test_lora_adapter_directory_tiny_model_vs_unmerged_oracle attached un-merged, under that test's gates."""
    g, cfg, sd, m, args = _setup()
    r, alpha = 8, 16
    factors = _lora_factors(cfg, NAMES18, r, 3, b_std=0.2)
    _write_adapter(str(tmp_path / "best"), factors, r, alpha, with_adapter_name=True)
    base = _fwd(m, args)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "best"), m, merge=False)
    got = _fwd(m, args)
    _check_vs_oracle(got, base, g, cfg, _sd_with_adapter(sd, factors, alpha / r), "tiny DiT + LoRA (un-merged on HIP vs un-merged oracle)")
    st = mgr.get_statistics()
    assert st["mode"] == "unmerged" and st["adapters"] == ["default"] and st["lora_modules"] == len(NAMES18)
    assert st["module_breakdown"]["cross_attention"] == 8 and st["lora_config"]["rank"] == r


def test_unmerged_adapter_ti2v5b_width_block_vs_unmerged_oracle(tmp_path):
    """M3: one TI2V-5B block (L = 1014), rank 16 on the nine targets of test_lora_adapter_ti2v5b_width_block_vs_unmerged_oracle, its gates."""
    from oracle import lora as ora_lora, wan_dit
    from univid_amd.lora import LoRAManager
    from univid_amd.wan.model import WanAttentionBlock, _freqs_device
    cfg = wan_dit.TI2V_5B_CFG
    dim, heads = cfg["dim"], cfg["num_heads"]
    sd = wan_dit.make_state_dict(dict(cfg, num_layers=1), 11)
    sd = {k: v for k, v in sd.items() if k.startswith("blocks.0.")}
    names = [f"blocks.0.{a}.{p}" for a in ("cross_attn", "self_attn") for p in "qkvo"] + ["blocks.0.ffn.0"]
    r, alpha = 16, 32
    factors = _lora_factors(cfg, names, r, 4)
    _write_adapter(str(tmp_path / "ad"), factors, r, alpha)
    gen = torch.Generator().manual_seed(23)
    Lt, grid = 1014, (3, 13, 26)
    x = torch.randn(1, Lt, dim, generator=gen)
    e_rows = torch.randn(2, 6, dim, generator=gen) * 0.3
    tid = (torch.arange(Lt) >= 338).long()
    ctx = (torch.randn(1, 512, dim, generator=gen) * 0.5).to(BF16)
    e0 = e_rows[tid].unsqueeze(0)
    freqs = wan_dit.rope_table(dim // heads)
    sd_l = _sd_with_adapter(sd, factors, alpha / r)
    with torch.no_grad():
        ref = wan_dit.block_forward(sd_l, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        ref_base = wan_dit.block_forward(sd, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        wan_dit.BF16 = ora_lora.BF16 = torch.float32
        try:
            truth = wan_dit.block_forward(sd_l, "blocks.0.", x, e0, torch.tensor([Lt]), torch.tensor([grid]), freqs, ctx, heads, 1e-6)
        finally:
            wan_dit.BF16 = ora_lora.BF16 = BF16
    holder = torch.nn.Module()
    holder.blocks = torch.nn.ModuleList([WanAttentionBlock(dim, cfg["ffn_dim"], heads, cross_attn_norm=True, eps=1e-6)])
    holder.load_state_dict(sd)
    holder = holder.to(DEV).eval()
    w0 = holder.blocks[0].self_attn.q.weight.detach().clone()
    LoRAManager().load_lora_weights(str(tmp_path / "ad"), holder, merge=False)
    blk = holder.blocks[0]
    xs = x[0].to(DEV).contiguous()
    with torch.no_grad():
        blk.prepare()
        blk._run(xs, Lt, e_rows.reshape(2, -1).to(DEV), tid.to(torch.int32).to(DEV), grid, _freqs_device(freqs, torch.device(DEV)),
                 ctx[0].to(DEV), first_block=False)
    assert torch.equal(blk.self_attn.q.weight, w0) and blk.self_attn._prep["q"].w.shape[1] == dim + 128
    effect = _rel_rms(ref[0] - x[0], ref_base[0] - x[0])
    assert effect > 0.05, f"adapter effect on the block's update only {effect:.3f}"
    assert_model_close(xs, ref[0], truth[0], frac=0.51, max_rel=3.2e-3, truth_ratio=1.05, name="TI2V-5B block + LoRA r16 (un-merged on HIP vs un-merged oracle)")


def test_rank_and_alpha_patterns_per_module(tmp_path):
    """M4: rank_pattern / alpha_pattern adapters run un-merged with each module's own scaling; merged they are still refused."""
    g, cfg, sd, m, args = _setup()
    r, alpha = 8, 16
    rank_pattern = {"blocks.0.self_attn.q": 4, "blocks.1.ffn.0": 24}
    alpha_pattern = {"blocks.0.cross_attn.k": 24}
    factors = {}
    for i, n in enumerate(NAMES18):
        factors.update(_lora_factors(cfg, [n], rank_pattern.get(n, r), 100 + i, b_std=0.2))
    _write_adapter(str(tmp_path / "pat"), factors, r, alpha, rank_pattern=rank_pattern, alpha_pattern=alpha_pattern)
    sd_l = dict(sd)
    for n, (a, b) in factors.items():
        sd_l[n + ".lora_A.weight"], sd_l[n + ".lora_B.weight"] = a, b
        sd_l[n + ".lora_scaling"] = alpha_pattern.get(n, alpha) / rank_pattern.get(n, r)
    base = _fwd(m, args)
    mgr = _manager()
    with pytest.raises(NotImplementedError):
        mgr.load_lora_weights(str(tmp_path / "pat"), m, merge=True)
    assert torch.equal(_fwd(m, args), base)
    mgr.load_lora_weights(str(tmp_path / "pat"), m, merge=False)
    got = _fwd(m, args)
    _check_vs_oracle(got, base, g, cfg, sd_l, "tiny DiT + LoRA with rank / alpha patterns (un-merged)")


def test_stacked_adapters_equal_their_concatenation(tmp_path):
    """M5."""
    g, cfg, sd, m, args = _setup()
    P = _lora_factors(cfg, NAMES20, 8, 11, b_std=0.2)
    Q = _lora_factors(cfg, NAMES20, 16, 12, b_std=0.2)
    PQ = {n: (torch.cat([P[n][0], Q[n][0]], 0), torch.cat([P[n][1], Q[n][1]], 1)) for n in NAMES20}
    _write_adapter(str(tmp_path / "P"), P, 8, 16)
    _write_adapter(str(tmp_path / "Q"), Q, 16, 32)
    _write_adapter(str(tmp_path / "PQ"), PQ, 24, 48)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "P"), m, merge=False, name="P")
    only_p = _fwd(m, args)
    mgr.load_lora_weights(str(tmp_path / "Q"), m, merge=False, name="Q")
    assert mgr.get_statistics()["adapters"] == ["P", "Q"]
    both = _fwd(m, args)
    mgr.unload("Q")
    assert torch.equal(_fwd(m, args), only_p), "detaching Q must leave P alone"
    mgr.unload()
    mgr.load_lora_weights(str(tmp_path / "PQ"), m, merge=False)
    assert torch.equal(_fwd(m, args), both) and not torch.equal(both, only_p)
    # the slot limit is named when one input's stacked rank outgrows it (q / k / v of one attention share a slot)
    from univid_amd.wan.model import LORA_MAX_SLOT
    assert LORA_MAX_SLOT >= 256
    big = _lora_factors(cfg, NAMES20[:8], LORA_MAX_SLOT // 3 + 1, 13)
    _write_adapter(str(tmp_path / "big"), big, LORA_MAX_SLOT // 3 + 1, 16)
    before = _fwd(m, args)
    with pytest.raises(ValueError, match="LORA_MAX_SLOT"):
        mgr.load_lora_weights(str(tmp_path / "big"), m, merge=False, name="big")
    assert torch.equal(_fwd(m, args), before) and mgr.get_statistics()["adapters"] == ["default"]


def test_swap_unload_and_context_cache(tmp_path):
    """M6."""
    g, cfg, sd, m, args = _setup()
    P = _lora_factors(cfg, NAMES18, 8, 21, b_std=0.2)
    Q = _lora_factors(cfg, NAMES20, 8, 22, b_std=0.2)
    _write_adapter(str(tmp_path / "P"), P, 8, 16)
    _write_adapter(str(tmp_path / "Q"), Q, 8, 16)
    params = {k: v.detach().clone() for k, v in m.named_parameters()}
    base = _fwd(m, args)
    _, _, fresh = _tiny_model(g["seed"])
    _manager().load_lora_weights(str(tmp_path / "Q"), fresh, merge=False)
    want_q = _fwd(fresh, args)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "P"), m, merge=False, name="P")
    got_p = _fwd(m, args)
    mgr.unload("P")
    mgr.load_lora_weights(str(tmp_path / "Q"), m, merge=False, name="Q")
    assert torch.equal(_fwd(m, args), want_q) and not torch.equal(got_p, want_q)
    mgr.unload()
    assert mgr.get_statistics() == {} and torch.equal(_fwd(m, args), base), "unload() must give the base model bit for bit"
    # a context-cached loop across the swap: cached cross-attention K / V^T of P must not serve Q
    with m.context_cached():
        mgr.load_lora_weights(str(tmp_path / "P"), m, merge=False, name="P")
        assert torch.equal(_fwd(m, args), got_p) and torch.equal(_fwd(m, args), got_p)
        mgr.unload("P")
        mgr.load_lora_weights(str(tmp_path / "Q"), m, merge=False, name="Q")
        assert torch.equal(_fwd(m, args), want_q), "stale K / V^T across an adapter swap"
        mgr.set_adapter_weight("Q", 0.0)
        assert torch.equal(_fwd(m, args), base), "stale K / V^T across a rescale"
    mgr.unload()
    for k, v in m.named_parameters():
        assert torch.equal(v, params[k]), f"{k}: the fp32 master weights must never be touched"


def test_cfg_pair_with_adapter_is_bit_identical_to_single_forwards(tmp_path):
    """M7."""
    g, cfg, sd, m, args = _setup()
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, NAMES20, 8, 31, b_std=0.2), 8, 16)
    _manager().load_lora_weights(str(tmp_path / "A"), m, merge=False)
    x, t, ctx = args[0][0], args[1], args[2][0]
    ctx2 = (ctx * 0.5).contiguous()
    with torch.no_grad():
        a = m([x], t, [ctx], LT)[0]
        b = m([x], t, [ctx2], LT)[0]
        pair = m([x, x], torch.cat([t, t]), [ctx, ctx2], LT)
    assert torch.equal(pair[0], a) and torch.equal(pair[1], b) and not torch.equal(a, b)


def test_hip_graph_denoise_with_adapter_and_rescale(tmp_path):
    """M8."""
    from univid_amd.wan.textimage2video import TI2VConfig, WanTI2V
    g = load_golden("sampler_tiny")
    cfg, sd, m = _tiny_model(g["seed"])
    _write_adapter(str(tmp_path / "A"), _lora_factors(cfg, NAMES20, 8, 41, b_std=0.2), 8, 16)
    mgr = _manager()
    mgr.load_lora_weights(str(tmp_path / "A"), m, merge=False)
    pipe = WanTI2V(TI2VConfig, model=m, device=DEV)
    args = (3, g["shift"], g["guide_scale"])
    with torch.no_grad():
        noise = g["noise"].to(DEV)
        ctx, ctxn = [g["ctx"].to(DEV).clone()], [g["ctx_null"].to(DEV).clone()]
        a_graph = pipe.denoise(noise, ctx, ctxn, *args, graph=True).clone()
        assert pipe._runner is not None
        a_eager = pipe.denoise(noise, ctx, ctxn, *args, graph=False).clone()
        assert torch.equal(a_graph, a_eager)
        mgr.set_adapter_weight("default", 0.5)
        b_graph = pipe.denoise(noise, ctx, ctxn, *args, graph=True).clone()
        b_eager = pipe.denoise(noise, ctx, ctxn, *args, graph=False).clone()
        assert torch.equal(b_graph, b_eager), "the graph replayed the previous adapter weight"
        assert not torch.equal(b_graph, a_graph)
        pipe._runner = None


def test_guards(tmp_path):
    """M9."""
    g, cfg, sd, m, args = _setup()
    f = _lora_factors(cfg, NAMES18, 8, 51)
    _write_adapter(str(tmp_path / "ok"), f, 8, 16)
    _write_adapter(str(tmp_path / "dora"), f, 8, 16, use_dora=True)
    _write_adapter(str(tmp_path / "bias"), f, 8, 16, bias="all")
    _write_adapter(str(tmp_path / "fifo"), f, 8, 16, fan_in_fan_out=True)
    mgr = _manager()
    for bad in ("dora", "bias", "fifo"):
        with pytest.raises(NotImplementedError):
            mgr.load_lora_weights(str(tmp_path / bad), m, merge=False)
    mgr.load_lora_weights(str(tmp_path / "ok"), m)                      # merged
    with pytest.raises(RuntimeError):
        mgr.load_lora_weights(str(tmp_path / "ok"), m, merge=False)
    mgr.unload()
    mgr.load_lora_weights(str(tmp_path / "ok"), m, merge=False)
    with pytest.raises(RuntimeError):
        mgr.load_lora_weights(str(tmp_path / "ok"), m)                  # merged on top of an attached adapter
    with pytest.raises(RuntimeError):
        mgr.load_lora_weights(str(tmp_path / "ok"), m, merge=False)     # the name is taken
    with pytest.raises(KeyError):
        mgr.set_adapter_weight("nope", 1.0)
    mgr.unload()
