"""The composed emulated oracle of tests/test_mx_mode_matrix.py, checked without a GPU: the default setting patches nothing, the nesting
order of the single-mode emulations does not change a bit, the masked-key P.V core equals the existing core on the cut operands, every patch
is undone on exit (after an exception too), and the 12 settings are pairwise different on the small model's forward - two settings the oracle
cannot tell apart would make the GPU gates of that file vacuous."""
import itertools

import pytest
import torch

from conftest import load_golden
from test_attn_mxpv import emulated_mxpv
from test_mx_mode_matrix import ALL_ON, DEFAULT, LT, SETTINGS, emulated, fp32_oracle, mxpv_core, sid
from test_mxfp8 import emulated_mxfp8_ffn
from test_mxproj import emulated_mxfp8_proj

pytestmark = []          # (test_mx_mode_matrix is imported for its oracle only; nothing here carries its gpu mark)

_small, _outs = {}, {}


def small():
    """(golden inputs, cfg, sd) of the small model of the GPU file: the tiny configuration with 2 heads of 128."""
    if not _small:
        from oracle import wan_dit
        g = load_golden("dit_tiny")
        cfg = dict(wan_dit.TINY_CFG, num_heads=2)
        _small.update(g=g, cfg=cfg, sd=wan_dit.make_state_dict(cfg, g["seed"]))
    return _small["g"], _small["cfg"], _small["sd"]


def forward():
    """The i2v forward (two timesteps per sample) of the small model under whatever is patched at the moment."""
    from oracle import wan_dit
    g, cfg, sd = small()
    with torch.no_grad():
        return wan_dit.dit_forward(sd, cfg, [g["x"]], g["t_two"], [g["ctx"]], LT)[0]


def out(setting):
    if setting not in _outs:
        with emulated(*setting):
            _outs[setting] = forward()
    return _outs[setting]


def _patched():
    from oracle import wan_dit
    return wan_dit.lin, wan_dit.rope_apply, wan_dit.attention_core, wan_dit.layer_norm, wan_dit.BF16


def test_the_default_setting_is_the_unpatched_oracle():
    before = _patched()
    plain = forward()
    with emulated(*DEFAULT):
        assert _patched() == before, "the default setting patched something"
        assert torch.equal(forward(), plain)
    assert torch.equal(out(DEFAULT), plain)


def test_nesting_order_does_not_change_a_bit():
    from oracle import wan_dit
    g, cfg, sd = small()
    for setting in (ALL_ON, ("mxfp8", "mxfp8_qk", "mxfp8")):
        for order in itertools.permutations(("ffn", "attn", "proj")):
            with emulated(*setting, order=order):
                assert torch.equal(forward(), out(setting)), f"{sid(setting)}: order {order} is another oracle"
    # the two `lin` patches on their own: a key of neither reaches the unpatched lin, a key of one reaches that one, in either order
    x = torch.randn(5, 256, generator=torch.Generator().manual_seed(1))
    keys = ("blocks.0.cross_attn.k", "blocks.1.self_attn.v", "blocks.0.cross_attn.q", "blocks.1.ffn.0")
    plain = {k: wan_dit.lin(sd, k, x) for k in keys}
    with emulated_mxfp8_ffn():
        ffn = {k: wan_dit.lin(sd, k, x) for k in keys}
    with emulated_mxfp8_proj():
        proj = {k: wan_dit.lin(sd, k, x) for k in keys}
    assert torch.equal(ffn[keys[0]], plain[keys[0]]) and torch.equal(proj[keys[0]], plain[keys[0]])
    assert torch.equal(ffn[keys[1]], plain[keys[1]]) and not torch.equal(proj[keys[1]], plain[keys[1]])
    assert torch.equal(ffn[keys[2]], plain[keys[2]]) and not torch.equal(proj[keys[2]], plain[keys[2]])
    assert not torch.equal(ffn[keys[3]], plain[keys[3]]) and torch.equal(proj[keys[3]], plain[keys[3]])
    want = {keys[0]: plain[keys[0]], keys[1]: proj[keys[1]], keys[2]: proj[keys[2]], keys[3]: ffn[keys[3]]}
    for a, b in ((emulated_mxfp8_ffn, emulated_mxfp8_proj), (emulated_mxfp8_proj, emulated_mxfp8_ffn)):
        with a(), b():
            for k in keys:
                assert torch.equal(wan_dit.lin(sd, k, x), want[k]), (a.__name__, b.__name__, k)


def test_masked_key_core_equals_the_existing_core_on_the_cut_operands():
    from oracle import wan_dit
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(1, 76, 2, 128, generator=g) for _ in range(3))
    v = v * torch.exp2(torch.linspace(-4, 4, 76)).view(1, 76, 1, 1)           # V's magnitude moves along the keys: the block scales matter
    v[:, 70:] *= 64.0                                                          # ... and the masked keys would own their block's scale
    res = {}
    for kl in (60, 70):
        got = mxpv_core(q, k, v, torch.tensor([kl]))
        with emulated_mxpv():
            want = wan_dit.attention_core(q, k[:, :kl], v[:, :kl], k_lens=torch.tensor([kl]))
        assert got.dtype == want.dtype and torch.equal(got, want), f"{kl} of 76 keys"
        res[kl] = got
    assert not torch.equal(res[60], res[70])
    # a V quantised BEFORE the cut would differ: the masked keys 70..75 share the block 64..95 with the valid keys 64..69
    with emulated_mxpv():
        whole = wan_dit.attention_core(q, k, v, k_lens=torch.tensor([76]))
    assert not torch.equal(whole, res[70])
    # b > 1: sample by sample, each with its own key count
    q2, k2, v2 = (torch.cat([t, t.flip(1)]) for t in (q, k, v))
    both = mxpv_core(q2, k2, v2, torch.tensor([70, 60]))
    assert torch.equal(both[0], res[70][0]) and torch.equal(both[1], mxpv_core(q2[1:], k2[1:], v2[1:], torch.tensor([60]))[0])
    # without lens the patched core is the oracle's own (the cross-attention's call)
    plain = wan_dit.attention_core(q, k, v)
    with emulated("bf16", "mxfp8_qk_pv", "bf16"):
        assert torch.equal(wan_dit.attention_core(q, k, v), plain)
        assert torch.equal(wan_dit.attention_core(q, k, v, k_lens=torch.tensor([70])), res[70])


def test_every_patch_is_undone_on_exit_and_after_an_exception():
    before = _patched()
    for setting in [DEFAULT] + SETTINGS:
        with emulated(*setting):
            changed = _patched() != before
        assert changed == (setting != DEFAULT) and _patched() == before, sid(setting)
        with pytest.raises(RuntimeError, match="inside"):
            with emulated(*setting):
                raise RuntimeError("inside")
        assert _patched() == before, sid(setting)
    with pytest.raises(RuntimeError, match="inside"):
        with fp32_oracle(), emulated(*ALL_ON, order=("proj", "attn", "ffn")):
            raise RuntimeError("inside")
    assert _patched() == before


def test_the_oracle_tells_every_setting_from_every_other():
    outs = {s: out(s) for s in [DEFAULT] + SETTINGS}
    assert len(outs) == 12
    for a, b in itertools.combinations(outs, 2):
        assert not torch.equal(outs[a], outs[b]), f"the composed oracle gives the same bits in {sid(a)} and {sid(b)}"
    assert all(torch.isfinite(o).all() for o in outs.values())
