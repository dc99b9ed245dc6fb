"""The row linear op and the fused decoding step without a GPU: the NumPy rule (tests/row_linear_rule.py) against answers
known by hand and its fp32 restatement against its own fp64 bounds; the host-side refusals of ``ops.row_linear``, of the
library's entry point and of the modules' ``fused=True`` (every one raised before a device is touched); the
``state_dict`` surface; and ``step(fused=True)`` on CPU stand-ins of the two ops (tests/cpu_stub_row_linear.py,
tests/cpu_stub_decode_attention.py): it equals ``step()`` and ``forward`` at every stepped position.

Tolerance of the stub comparisons: both sides are torch fp32 evaluations of the same formula that differ in how the ops
are grouped, as the stepped and the whole-sequence forward of tests/test_host_decode_attention.py do; the same
``2e-5 max(1, max|out|)`` applies (a wrong sub-stage is orders of magnitude beyond it)."""
import math
import types

import numpy as np
import pytest
import torch

from tests import cpu_stub_decode_attention as DSTUB
from tests import cpu_stub_row_linear as STUB
from tests import row_linear_rule as R

ATT_KEYS = sorted(f"{m}.{p}" for m in ("q_proj", "k_proj", "v_proj", "o_proj", "prosody_gate", "memory_gate")
                  for p in ("weight", "bias"))
LAYER_KEYS = sorted(["attention_norm.weight", "attention_norm.bias", "ffn_norm.weight", "ffn_norm.bias", "ffn.0.weight",
                     "ffn.0.bias", "ffn.2.weight", "ffn.2.bias"] + ["attention." + k for k in ATT_KEYS])
MODEL_KEYS = ['pos_encoder.theta_phase_offsets', 'pos_encoder.gamma_phase_offsets', 'pos_encoder.amplitude_modulation',
              'semantic_encoder.token_embedding.weight', 'semantic_encoder.semantic_projection.weight',
              'semantic_encoder.semantic_projection.bias', 'semantic_encoder.place_to_semantic.weight',
              'semantic_encoder.place_to_semantic.bias', 'layer_norm.weight', 'layer_norm.bias', 'output_head.weight']


def _config(D=96, H=2, dropout=0.0):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=dropout, intermediate_size=2 * D)


def _rng(seed=0):
    rng = np.random.default_rng(seed)
    return lambda *s: rng.standard_normal(s).astype(np.float32)


RULES = [lambda *a, **k: R.linear64(*a, **k)["y"], lambda *a, **k: R.linear32(*a, **k)["y"]]


# ------------------------------------------------------------------------------------- the rule's own known answers
@pytest.mark.parametrize("rule", RULES, ids=["fp64", "fp32"])
def test_an_identity_weight_with_the_prologue_gives_layer_norm(rule):
    f = _rng(1)
    x, g, b = f(3, 96) * 2 + 1, f(96), f(96)
    y = rule(x, [np.eye(96, dtype=np.float32)], norm=(g, b), eps=1e-5)[0]
    want = torch.nn.functional.layer_norm(torch.from_numpy(x).double(), (96,), torch.from_numpy(g).double(),
                                          torch.from_numpy(b).double(), 1e-5).numpy()
    assert np.max(np.abs(y - want)) <= 2e-5
    xh32 = R.linear32(x, [np.eye(96, dtype=np.float32)], norm=(g, b))
    assert np.array_equal(xh32["y"][0], xh32["xh"]), "a dot with one non-zero weight of 1 is exact"


@pytest.mark.parametrize("rule", RULES, ids=["fp64", "fp32"])
def test_a_constant_row_gives_beta(rule):
    f = _rng(2)
    g, b = f(256), f(256)
    x = np.full((2, 256), 0.75, dtype=np.float32)                       # 256 copies of 0.75 add up exactly in fp32
    y = rule(x, [np.eye(256, dtype=np.float32)], norm=(g, b), eps=1e-5)[0]
    assert np.array_equal(np.asarray(y, dtype=np.float32), np.broadcast_to(b, (2, 256)))
    _, mu, rstd = R.norm32(x, g, b, 1e-5)
    assert np.all(mu == np.float32(0.75)) and np.all(rstd == np.float32(1.0) / np.sqrt(np.float32(1e-5)))


@pytest.mark.parametrize("rule", RULES, ids=["fp64", "fp32"])
def test_gelu_against_math_erf(rule):
    t = np.array([[0.0, 1.0, -1.0, 6.0, -6.0, 0.5, -0.5, 3.0]], dtype=np.float32)
    y = rule(t, [np.eye(8, dtype=np.float32)], gelu=True)[0][0]
    want = [0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0))) for v in t[0].tolist()]
    assert y[0] == 0.0
    assert np.max(np.abs(y - np.array(want))) <= (1e-15 if rule is RULES[0] else 4e-7)
    assert abs(y[3] - 6.0) <= 1e-6 and abs(y[4]) <= 1e-6


@pytest.mark.parametrize("rule", RULES, ids=["fp64", "fp32"])
def test_a_zero_weight_leaves_the_residual(rule):
    f = _rng(3)
    x, res = f(4, 12), f(4, 5)
    y = rule(x, [np.zeros((5, 12), dtype=np.float32)], residual=res)[0]
    assert np.array_equal(np.asarray(y, dtype=np.float32), res)
    b = f(5)
    y = rule(x, [np.zeros((5, 12), dtype=np.float32)], [b], residual=res)[0]
    assert np.array_equal(np.asarray(y, dtype=np.float32), (b[None, :] + res).astype(np.float32))


def test_the_row_sum_order_is_the_lane_pattern():
    # 2^24 in lane 0's first slot absorbs a 1 that follows it in the same lane, and not one from another lane
    v = np.zeros(520, dtype=np.float32)
    v[0] = 2.0 ** 24
    v[256] = 1.0                                                        # (256 / 4) mod 64 == 0: lane 0 again
    assert R.row_sum32(v[None])[0] == np.float32(2.0 ** 24)
    v[256], v[4], v[12] = 0.0, 1.0, 1.0                                 # lanes 1 and 3 meet at xor 2, lane 0 at xor 1
    assert R.row_sum32(v[None])[0] == np.float32(2.0 ** 24 + 2.0)
    v[12], v[8] = 0.0, 1.0                                              # lane 2 meets lane 0 at xor 2, lane 1 after it
    assert R.row_sum32(v[None])[0] == np.float32(2.0 ** 24)


def test_the_fp32_restatement_is_within_the_derived_bounds_of_fp64():
    worst = 0.0
    for seed, (Rr, K, N, norm, gelu, res, kind) in enumerate([
            (3, 96, 5, True, False, False, "random"), (3, 100, 33, True, True, False, "offset"),
            (5, 260, 17, False, True, True, "random"), (2, 2048, 9, True, True, True, "offset"),
            (2, 8192, 3, False, False, True, "random"), (1, 4, 1, False, False, False, "random")]):
        f = _rng(20 + seed)
        x = f(Rr, K) + (np.float32(1e3) if kind == "offset" else np.float32(0))
        W, b = (f(N, K) / np.sqrt(K)).astype(np.float32), f(N)
        kw = dict(norm=(f(K), f(K)) if norm else None, gelu=gelu, residual=f(Rr, N) if res else None)
        want, got = R.linear64(x, [W], [b], **kw), R.linear32(x, [W], [b], **kw)
        share = np.abs(got["y"][0] - want["y"][0]) / want["bound"][0]
        assert np.all(share <= 1.0), (Rr, K, N, float(share.max()))
        if norm:
            assert np.all(np.abs(got["xh"] - want["xh"]) <= want["xh_bound"])
        if kind == "random":
            # outputs are O(1); the worst-case (K + 8) u sum|x w| reaches 0.03 at K = 8192 and 1e-4 at K = 260
            assert float(want["bound"][0].max()) < (0.05 if K > 2048 else 1e-3), "far below a wiring error"
        worst = max(worst, float(share.max()))
    print(f"worst used share of the bound: {worst:.3f}")


# ------------------------------------------------------------------------------------- host-side refusals
def _args(R_=3, K=16, N=(5,), norm=False, res=False):
    z = torch.zeros
    single = len(N) == 1
    a = dict(x=z(R_, K), weights=z(N[0], K) if single else tuple(z(n, K) for n in N),
             biases=z(N[0]) if single else tuple(z(n) for n in N), kw=dict())
    if norm:
        a["kw"]["norm"] = (z(K), z(K))
    if res:
        a["kw"]["residual"] = z(R_, N[0])
    return a


def test_the_op_refuses_bad_arguments_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    z = torch.zeros
    assert (ops.ROW_LINEAR_MAX_ROWS, ops.ROW_LINEAR_MAX_K) == (32, 8192)
    bad = [
        (_args(R_=33), {}, ValueError, "R = 33"),
        (_args(R_=0), {}, ValueError, "R = 0"),
        (_args(K=18), {}, ValueError, "K % 4"),
        (_args(K=8196), {}, ValueError, "K = 8196"),
        (_args(K=2052, norm=True), {}, ValueError, "prologue with K = 2052"),
        (_args(), dict(x=z(3, 16).half()), TypeError, "fp16 input"),
        (_args(), dict(weights=z(5, 16).bfloat16()), TypeError, "bf16 weight"),
        (_args(N=(5, 5, 5, 5)), {}, ValueError, "four weights"),
        (_args(), dict(weights=()), ValueError, "no weight"),
        (_args(N=(5, 6, 7)), dict(kw=dict(residual=z(3, 5))), ValueError, "residual with three weights"),
        (_args(), dict(x=z(16)), ValueError, "x rank"),
        (_args(), dict(x=z(3, 32)[:, ::2]), ValueError, "non-contiguous x"),
        (_args(), dict(x=None), ValueError, "missing x"),
        (_args(), dict(weights=z(5, 12)), ValueError, "weight K"),
        (_args(), dict(weights=z(0, 16), biases=None), ValueError, "N = 0"),
        (_args(), dict(weights=z(5, 16, 1)), ValueError, "weight rank"),
        (_args(), dict(biases=z(6)), ValueError, "bias length"),
        (_args(N=(5, 6)), dict(biases=z(5)), ValueError, "one bias for two weights"),
        (_args(N=(5, 6)), dict(biases=(z(5),)), ValueError, "bias count"),
        (_args(), dict(weights=[z(5, 16), None], biases=None), ValueError, "a missing weight"),
        (_args(), dict(weights=[z(5, 16), [1.0]], biases=None), TypeError, "a weight that is no tensor"),
        (_args(), dict(kw=dict(norm=(z(16),))), ValueError, "norm without beta"),
        (_args(), dict(kw=dict(norm=(z(16), None))), ValueError, "norm with beta None"),
        (_args(), dict(kw=dict(norm=(z(12), z(16)))), ValueError, "gamma length"),
        (_args(norm=True), dict(kw=dict(norm=(z(16), z(16)), eps=-1.0)), ValueError, "negative eps"),
        (_args(norm=True), dict(kw=dict(norm=(z(16), z(16)), eps=float("nan"))), ValueError, "NaN eps"),
        (_args(), dict(kw=dict(return_normed=True)), ValueError, "return_normed without norm"),
        (_args(), dict(kw=dict(activation="tanh")), ValueError, "unknown activation"),
        (_args(), dict(kw=dict(residual=z(3, 6))), ValueError, "residual shape"),
        (_args(), dict(kw=dict(residual=z(3, 5).double())), TypeError, "fp64 residual"),
        (_args(), dict(kw=dict(out=z(3, 6))), ValueError, "out shape"),
        (_args(), dict(kw=dict(out=z(3, 5).half())), TypeError, "fp16 out"),
        (_args(N=(5, 6)), dict(kw=dict(out=z(3, 5))), ValueError, "one out for two weights"),
    ]
    for a, change, exc, why in bad:
        a.update(change)
        with pytest.raises(exc):
            ops.row_linear(a["x"], a["weights"], a["biases"], **a["kw"])
            pytest.fail(f"accepted: {why}")
    # valid calls get as far as the device check, still without the library: CPU tensors are refused
    for a in (_args(), _args(N=(5, 6, 7), norm=True), _args(res=True), _args(R_=32, K=8192), _args(K=2048, norm=True)):
        with pytest.raises(ops.AuraDeviceError):
            ops.row_linear(a["x"], a["weights"], a["biases"], **a["kw"])


def test_the_library_refuses_bad_geometry_and_pointers_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 0x10000                                           # never dereferenced: every call below returns on the host

    def call(R_=3, K=16, N=(5, 0, 0), eps=1e-5, gelu=0, **ptr):
        p = dict(x=P, W0=P, b0=P, y0=P, W1=None, b1=None, y1=None, W2=None, b2=None, y2=None, gamma=None, beta=None,
                 xh=None, res=None)
        p.update(ptr)
        return lib.aura_row_linear(p["x"], R_, K, p["W0"], p["b0"], p["y0"], N[0], p["W1"], p["b1"], p["y1"], N[1],
                                   p["W2"], p["b2"], p["y2"], N[2], p["gamma"], p["beta"], eps, p["xh"], gelu, p["res"],
                                   0, None)
    INVAL, ALIGN = -1, -3
    three = dict(W1=P, y1=P, W2=P, y2=P)
    for kw in (dict(R_=0), dict(R_=33), dict(K=0), dict(K=18), dict(K=8196), dict(x=None), dict(W0=None), dict(y0=None),
               dict(N=(0, 0, 0)), dict(N=(5, 6, 0)), dict(W1=P, y1=P), dict(W1=P, N=(5, 6, 0)), dict(W2=P, y2=P, N=(5, 0, 7)),
               dict(b1=P), dict(y2=P), dict(N=(5, 6, 0), **three), dict(N=(2 ** 31, 0, 0)),
               dict(N=(2 ** 30, 2 ** 30, 2 ** 30), **three), dict(gamma=P), dict(beta=P),
               dict(gamma=P, beta=P, K=2052), dict(gamma=P, beta=P, eps=-1.0), dict(gamma=P, beta=P, eps=float("nan")),
               dict(xh=P), dict(res=P, N=(5, 6, 7), **three)):
        assert call(**kw) == INVAL, kw
    for name in ("x", "W0"):
        assert call(**{name: P + 4}) == ALIGN, name
    for name in ("gamma", "beta", "xh"):
        assert call(**dict(dict(gamma=P, beta=P), **{name: P + 4})) == ALIGN, name
    for name in ("W1", "W2"):
        assert call(**dict(dict(N=(5, 6, 7), **three), **{name: P + 4})) == ALIGN, name
    for name in ("b0", "y0", "res"):
        assert call(**{name: P + 2}) == ALIGN, name


def _layer(D=96, H=2, dropout=0.0, seed=0):
    from aura_snn_rag_amd import HippocampalTransformerLayer
    torch.manual_seed(seed)
    return HippocampalTransformerLayer(_config(D, H, dropout), object()).eval()


def test_the_modules_refuse_what_the_fused_step_does_not_cover(monkeypatch):
    ops = STUB.install(monkeypatch)
    DSTUB.install(monkeypatch)
    hidden = torch.randn(3, 8, 96)
    training = _layer(dropout=0.1).train()
    cache = training.new_cache(3, 12)
    training.prefill(hidden[:, :4], cache=cache)
    with pytest.raises(RuntimeError, match="dropout"):
        training.step(hidden[:, 4], cache=cache, fused=True)
    training.eval().step(hidden[:, 4], cache=cache, fused=True)         # the same layer in eval mode steps
    assert STUB.CALLS["row_linear"] == 4
    tanh = _layer()
    tanh.ffn[1] = torch.nn.GELU(approximate="tanh")
    relu = _layer()
    relu.ffn[1] = torch.nn.ReLU()
    for layer in (tanh, relu):
        cache = layer.new_cache(3, 12)
        layer.prefill(hidden[:, :4], cache=cache)
        with pytest.raises(ValueError, match="GELU"):
            layer.step(hidden[:, 4], cache=cache, fused=True)
        layer.step(hidden[:, 4], cache=cache)                           # the unfused step takes any activation
    assert STUB.CALLS["row_linear"] == 4 and DSTUB.CALLS["step"] == 3
    wide = _layer(D=16, H=2)
    cache = wide.new_cache(33, 4)
    wide.prefill(torch.randn(33, 2, 16), cache=cache)
    with pytest.raises(ValueError, match="32"):
        wide.step(torch.randn(33, 16), cache=cache, fused=True)
    with pytest.raises(ValueError, match="32"):
        wide.attention.step(torch.randn(33, 16), cache=cache, fused=True)
    assert STUB.CALLS["row_linear"] == 4 and DSTUB.CALLS["step"] == 3, "refused before any op"
    att = wide.attention
    small = att.new_cache(2, 4)
    with pytest.raises(ValueError, match="fused"):
        att.step(torch.randn(2, 16), cache=small, residual=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="fused"):
        att.step(torch.randn(2, 16), cache=small, norm=wide.attention_norm)
    with pytest.raises(TypeError):
        att.step(torch.randn(2, 16), cache=small, fused=True, norm=(torch.ones(16), torch.zeros(16)))
    assert ops.ROW_LINEAR_MAX_ROWS == 32


def test_a_fused_step_refuses_cpu_tensors_without_the_stubs():
    from aura_snn_rag_amd import ops
    layer = _layer(D=16, H=2)
    cache = layer.new_cache(1, 4)
    with pytest.raises(ops.AuraDeviceError):
        layer.step(torch.zeros(1, 16), cache=cache, fused=True)
    with pytest.raises(ops.AuraDeviceError):
        layer.attention.step(torch.zeros(1, 16), cache=cache, fused=True)


# ------------------------------------------------------------------------------------- the modules on the stubs
@pytest.mark.parametrize("variant", ["prosody", "no_prosody", "no_memory"])
def test_the_fused_layer_step_equals_the_step_and_forward_at_every_position(monkeypatch, variant):
    STUB.install(monkeypatch)
    DSTUB.install(monkeypatch)
    layer = _layer(D=96, H=2, seed=3)
    with torch.no_grad():                                               # norms that are not the identity
        for n in (layer.attention_norm, layer.ffn_norm):
            n.weight.add_(0.3 * torch.randn(96))
            n.bias.add_(0.3 * torch.randn(96))
    B, P, n_new, D = 3, 7, 6, 96
    S = P + n_new
    hidden, prosody = torch.randn(B, S, D), 1.5 * torch.randn(B, S, 4)
    pro = (lambda a, b: None) if variant == "no_prosody" else (lambda a, b: prosody[:, a:b])
    mem = variant != "no_memory"
    with torch.no_grad():
        full = layer(hidden, prosody=pro(0, S), use_memory=mem)
        plain, fused = layer.new_cache(B, 16), layer.new_cache(B, 16)
        layer.prefill(hidden[:, :P], prosody=pro(0, P), use_memory=mem, cache=plain)
        layer.prefill(hidden[:, :P], prosody=pro(0, P), use_memory=mem, cache=fused)
        for t in range(P, S):
            step_in = hidden[:, t:t + 1] if t % 2 else hidden[:, t]     # [B, 1, D] and [B, D]
            a = layer.step(step_in, prosody=pro(t, t + 1), use_memory=mem, cache=plain)
            before = STUB.CALLS["row_linear"], DSTUB.CALLS["step"]
            b = layer.step(step_in, prosody=pro(t, t + 1), use_memory=mem, cache=fused, fused=True)
            assert (STUB.CALLS["row_linear"] - before[0], DSTUB.CALLS["step"] - before[1]) == (4, 1)
            tol = 2e-5 * max(1.0, float(full.abs().max()))
            assert b.shape == (B, D) and float((b - a).abs().max()) <= tol, t
            assert float((b - full[:, t]).abs().max()) <= tol, t
    assert DSTUB.LAST["prosody"] == (variant != "no_prosody") and DSTUB.LAST["memory"] == mem
    assert fused.lengths.tolist() == [S] * B and fused.max_length == S
    assert float((fused.k - plain.k).abs().max()) <= 2e-5 and float((fused.v - plain.v).abs().max()) <= 2e-5
    # the last row_linear of a step is ffn.2 with the residual
    assert STUB.LAST["residual"] and STUB.LAST["N"] == (D,) and STUB.LAST["K"] == 2 * D and not STUB.LAST["norm"]


def test_the_fused_attention_step_alone_takes_a_normed_row(monkeypatch):
    STUB.install(monkeypatch)
    DSTUB.install(monkeypatch)
    layer = _layer(D=32, H=4, seed=4)
    att = layer.attention
    hidden = torch.randn(2, 6, 32)
    with torch.no_grad():
        a, b = att.new_cache(2, 8), att.new_cache(2, 8)
        att.prefill(hidden[:, :5], cache=a)
        att.prefill(hidden[:, :5], cache=b)
        want = att.step(hidden[:, 5], cache=a)
        got = att.step(hidden[:, 5], cache=b, fused=True)
        assert float((got - want).abs().max()) <= 2e-5 and STUB.CALLS["row_linear"] == 2
        assert not STUB.LAST["norm"] and not STUB.LAST["residual"]


def test_a_retired_row_keeps_its_cache_in_the_fused_step(monkeypatch):
    STUB.install(monkeypatch)
    DSTUB.install(monkeypatch)
    layer = _layer(D=32, H=4, seed=5)
    hidden = torch.randn(3, 7, 32)
    with torch.no_grad():
        cache = layer.new_cache(3, 10)
        layer.prefill(hidden[:, :5], cache=cache)
        cache.retire([1])
        k0, v0 = cache.k.clone(), cache.v.clone()
        out = layer.step(hidden[:, 5], cache=cache, fused=True)
        assert torch.equal(cache.k[1], k0[1]) and torch.equal(cache.v[1], v0[1]) and not torch.equal(cache.k[0], k0[0])
        assert cache.lengths.tolist() == [6, -1, 6]
        assert float((out[0] - layer(hidden[:, :6])[0, 5]).abs().max()) <= 2e-5


def test_the_model_passes_the_switch_down(monkeypatch):
    from aura_snn_rag_amd import HippocampalTransformer
    STUB.install(monkeypatch)
    DSTUB.install(monkeypatch)
    lm = HippocampalTransformer(types.SimpleNamespace(
        vocab_size=257, embedding_dim=96, num_heads=4, num_layers=2, intermediate_size=192, n_place_cells=200,
        max_seq_len=32, dropout=0.0, theta_frequency=8.0, gamma_frequency=40.0), None).eval()
    seen = []
    for i, layer in enumerate(lm.layers):
        monkeypatch.setattr(layer, "step", lambda h, _i=i, **kw: seen.append((_i, kw["fused"], kw["advance"])) or h)
    monkeypatch.setattr("aura_snn_rag_amd.core.language_zone.hippocampal_transformer.embed_tokens",
                        lambda tokens, *a, **kw: (torch.zeros(tokens.shape[0], 1, 96), None))
    state = lm.new_state(2, 8)
    tokens = torch.zeros(2, dtype=torch.int64)
    lm.step(tokens, state=state, fused=True)
    lm.step(tokens, state=state)
    assert seen == [(0, True, False), (1, True, True), (0, False, False), (1, False, True)]
    with pytest.raises(ValueError, match="32"):
        lm.step(torch.zeros(33, dtype=torch.int64), state=lm.new_state(33, 8), fused=True)
    with pytest.raises(ValueError, match="32"):
        lm.generate(torch.zeros(33, 4, dtype=torch.int64), max_new_tokens=2, fused_step=True)


def test_the_state_dict_keys_are_unchanged():
    from aura_snn_rag_amd import HippocampalProsodyAttention, HippocampalTransformer
    assert sorted(HippocampalProsodyAttention(_config(), object()).state_dict()) == ATT_KEYS and len(ATT_KEYS) == 12
    assert sorted(_layer().state_dict()) == LAYER_KEYS and len(LAYER_KEYS) == 20
    lm = HippocampalTransformer(types.SimpleNamespace(
        vocab_size=257, embedding_dim=96, num_heads=4, num_layers=2, intermediate_size=192, n_place_cells=200,
        max_seq_len=32, dropout=0.0, theta_frequency=8.0, gamma_frequency=40.0), None)
    want = MODEL_KEYS + [f"layers.{i}.{k}" for i in range(2) for k in LAYER_KEYS]
    assert sorted(lm.state_dict()) == sorted(want) and len(want) == 51
