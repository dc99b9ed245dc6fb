"""Timestep STDP without a GPU: the NumPy restatement of the rule (tests/stdp_rule.py) against answers known by hand,
a split over T with carried traces, and the host-side argument checks of ``ops.stdp_update`` / ``Synapsis.stdp_update``
(every one raised before the library is touched)."""
import inspect

import numpy as np
import pytest
import torch

from tests import stdp_rule as R


def _one_pair(t_pre, t_post, B=4, T=8, I=8, O=8, i=3, o=5):
    pre = np.zeros((B, T, I), np.float32)
    post = np.zeros((B, T, O), np.float32)
    pre[1, t_pre, i] = 1.0
    post[1, t_post, o] = 1.0
    return pre, post


# ------------------------------------------------------------------------------------- the rule's own known answers
def test_pre_before_post_is_potentiated_by_the_decayed_trace():
    lp, lq, ap, am = 0.9, 0.8, 0.75, 0.6
    dw, s, _, _ = R.rule(*_one_pair(2, 5), lp, lq, ap, am)
    want = float(np.float32(ap)) * float(np.float32(lp)) ** 3 / 4
    assert np.count_nonzero(dw) == 1 and dw[5, 3] > 0
    assert abs(dw[5, 3] - want) <= 2 * np.spacing(np.float32(want))     # the fp32 trace is two roundings from lambda^3
    assert np.count_nonzero(s) == 1 and s[5, 3] == dw[5, 3]


def test_post_before_pre_is_depressed_by_the_decayed_trace():
    lp, lq, ap, am = 0.9, 0.8, 0.75, 0.6
    dw, _, _, _ = R.rule(*_one_pair(5, 2), lp, lq, ap, am)
    want = -float(np.float32(am)) * float(np.float32(lq)) ** 3 / 4
    assert np.count_nonzero(dw) == 1
    assert abs(dw[5, 3] - want) <= 2 * np.spacing(np.float32(abs(want)))


def test_the_same_step_is_potentiation_only():
    dw, _, _, _ = R.rule(*_one_pair(4, 4), 0.9, 0.8, 0.75, 0.6)
    assert np.count_nonzero(dw) == 1 and dw[5, 3] == float(np.float32(0.75)) / 4


def test_traces_are_the_two_rounding_recursion():
    rng = np.random.default_rng(0)
    pre = rng.standard_normal((2, 6, 4)).astype(np.float32)
    post = R.spikes(rng, (2, 6, 4), 0.5)
    xs, yb, xf, yf = R.traces(pre, post, 0.7, 0.6)
    lp = np.float32(0.7)
    x = np.float32(0.0)
    for t in range(6):
        x = np.float32(np.float32(lp * x) + pre[1, t, 2])
        assert xs[1, t, 2] == x
    assert xf[1, 2] == x and np.all(yb[:, 0] == 0) and xs.dtype == yb.dtype == np.float32
    # y_before is the first rounding of y's own step
    _, yb2, _, _ = R.traces(pre, post, 0.7, 0.6, y0=yf)
    assert np.array_equal(yb2[:, 0], np.float32(0.6) * yf) and np.array_equal(yb[:, 5] + post[:, 5], yf)


def test_a_split_over_T_with_carried_traces_is_the_same_update():
    rng = np.random.default_rng(1)
    B, T, I, O = 3, 12, 8, 12
    pre, post = R.spikes(rng, (B, T, I), 0.3), R.spikes(rng, (B, T, O), 0.2)
    x0 = rng.random((B, I)).astype(np.float32)
    y0 = rng.random((B, O)).astype(np.float32)
    dw, s, xf, yf = R.rule(pre, post, 0.9, 0.8, 0.01, 0.012, x0, y0)
    dw_sum, x, y = np.zeros_like(dw), x0, y0
    for lo, hi in ((0, 5), (5, 6), (6, 12)):
        d, _, x, y = R.rule(pre[:, lo:hi], post[:, lo:hi], 0.9, 0.8, 0.01, 0.012, x, y)
        dw_sum += d
    assert np.array_equal(x, xf) and np.array_equal(y, yf)
    assert np.max(np.abs(dw_sum - dw)) <= 1e-12 * max(1.0, float(np.max(np.abs(dw))))


def test_bf16_rounding_helper_matches_torch():
    rng = np.random.default_rng(2)
    a = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(R.to_bf16_exact(a), torch.from_numpy(a).bfloat16().float().numpy())


# ------------------------------------------------------------------------------------- ops: argument checks
KW = dict(lambda_pre=0.9, lambda_post=0.9, a_plus=0.01, a_minus=0.012, lr=0.5, w_min=-1.0, w_max=1.0)


def test_ops_refuses_cpu_tensors():
    from aura_snn_rag_amd import ops
    pre, post, w = torch.zeros(2, 3, 8), torch.zeros(2, 3, 12), torch.zeros(12, 8)
    with pytest.raises(ops.AuraDeviceError):
        ops.stdp_update(pre, post, None, None, w, **KW)
    with pytest.raises(ops.AuraDeviceError):
        ops.stdp_update(pre[:, 0].contiguous(), post, None, None, None, torch.zeros(12, 8), pre_time_invariant=True, **KW)


def test_ops_raises_value_errors_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    pre, post, w = torch.zeros(2, 3, 8), torch.zeros(2, 3, 12), torch.zeros(12, 8)
    bad = [
        (dict(pre=pre[0]), "rank"),                                              # [T, I]
        (dict(post=post[:, 0]), "rank"),
        (dict(pre=torch.zeros(3, 3, 8)), "B"),
        (dict(pre=torch.zeros(2, 4, 8)), "T"),
        (dict(pre=torch.zeros(2, 3, 6), weight=torch.zeros(12, 6)), "I % 4"),
        (dict(post=torch.zeros(2, 3, 10), weight=torch.zeros(10, 8)), "O % 4"),
        (dict(pre=pre.bfloat16()), "mixed dtypes"),
        (dict(pre=torch.zeros(2, 3, 6).bfloat16(), post=post.bfloat16(), weight=torch.zeros(12, 6)), "I % 4, bf16"),
        (dict(pre=pre.double(), post=post.double()), "fp64"),
        (dict(pre=torch.zeros(2, 3, 16)[:, :, ::2]), "non-contiguous pre"),
        (dict(post=torch.zeros(2, 12, 3).transpose(1, 2)), "non-contiguous post"),
        (dict(weight=torch.zeros(8, 12).t()), "non-contiguous weight"),
        (dict(weight=torch.zeros(8, 12)), "weight shape"),
        (dict(weight=w.bfloat16()), "bf16 weight"),
        (dict(x_trace=torch.zeros(2, 12)), "x_trace shape"),
        (dict(y_trace=torch.zeros(3, 12)), "y_trace shape"),
        (dict(weight=None), "neither weight nor dw_out"),
        (dict(dw_out=torch.zeros(12, 4)), "dw_out shape"),
    ]
    for change, why in bad:
        args = dict(pre=pre, post=post, x_trace=None, y_trace=None, weight=w, dw_out=None)
        args.update(change)
        with pytest.raises(ValueError):
            ops.stdp_update(args["pre"], args["post"], args["x_trace"], args["y_trace"], args["weight"],
                            args["dw_out"], **KW)
            pytest.fail(f"accepted: {why}")
    with pytest.raises(ValueError):                                              # a time-invariant pre is [B, I]
        ops.stdp_update(pre, post, None, None, w, pre_time_invariant=True, **KW)
    with pytest.raises(ValueError):
        ops.stdp_update(pre, post, None, None, w, **dict(KW, w_min=2.0))
    # a valid call gets as far as the device check, still without the library
    with pytest.raises(ops.AuraDeviceError):
        ops.stdp_update(pre, post, torch.zeros(2, 8), torch.zeros(2, 12), w, torch.zeros(12, 8), **KW)


# ------------------------------------------------------------------------------------- modules
def test_a_disabled_synapsis_returns_none_and_launches_nothing(monkeypatch):
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.language_zone.synapsis import Synapsis
    monkeypatch.setattr(ops, "stdp_update", lambda *a, **k: pytest.fail("an op was called"))
    syn = Synapsis(8, 12)
    w, version = syn.weight.detach().clone(), syn.weight._version
    assert syn.stdp_update(torch.zeros(2, 3, 8), torch.zeros(2, 3, 12)) == (None, None)
    assert torch.equal(syn.weight, w) and syn.weight._version == version


def test_the_new_keywords_come_after_the_existing_ones():
    from aura_snn_rag_amd.core.language_zone.snn_ffn import SNNFFN
    from aura_snn_rag_amd.core.language_zone.synapsis import StdpState, Synapsis
    names = list(inspect.signature(Synapsis.__init__).parameters)
    assert names[:8] == ["self", "in_features", "out_features", "enable_plasticity", "stdp_lr", "trace_decay",
                         "target_firing_rate", "bias"]
    p = inspect.signature(Synapsis.__init__).parameters
    assert (p["stdp_a_plus"].default, p["stdp_a_minus"].default, p["stdp_tau_decay"].default,
            p["stdp_bounds"].default) == (1.0, 1.05, None, (-10.0, 10.0))
    assert Synapsis(8, 8, trace_decay=0.9).stdp_decays() == (0.9, 0.9)
    assert Synapsis(8, 8, stdp_tau_decay=(0.8, 0.7)).stdp_decays() == (0.8, 0.7)
    assert StdpState._fields == ("x", "y")
    names = list(inspect.signature(SNNFFN.__init__).parameters)
    assert names[-1] == "plasticity" and inspect.signature(SNNFFN.__init__).parameters["plasticity"].default is False
    plain, plastic = SNNFFN(8, 16), SNNFFN(8, 16, plasticity=True)
    assert list(plain.state_dict()) == list(plastic.state_dict())
    assert plastic.syn1.enable_plasticity and plastic.syn2.enable_plasticity and not plain.syn1.enable_plasticity


def test_a_bf16_weight_is_refused_with_the_way_out():
    from aura_snn_rag_amd.core.language_zone.synapsis import Synapsis
    syn = Synapsis(8, 8, enable_plasticity=True).bfloat16()
    with pytest.raises(TypeError, match="fp32 master weights"):
        syn.stdp_update(torch.zeros(2, 3, 8), torch.zeros(2, 3, 8))
