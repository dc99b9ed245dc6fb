"""The fused ``cross_attention`` injection on the CPU: the host-side refusals of ``ops.memory_attend`` and of the library's
entry point, ``MemoryAugmentedLayer.fold_memory`` (the tables against their fp64 values and, through the CPU stand-in of the
op, against ``inject_cross_attention``), the fused step of a ``cross_attention`` layer and ``generate(fused_step=True)`` of
a ``cross_attention`` model on the stand-ins of the ops (tests/cpu_stub_*.py).

Tolerances.  ``2e-5 max(1, |out|)`` is the one ``tests/test_host_memory_layer.py`` holds two fp32 evaluations of the layer's
formula to.  A table element is an fp64 value rounded once to fp32: within ``2^-24`` of it relatively; the test allows
``2^-23`` (its own fp64 evaluation sums in another order, ``1e-13`` relatively at these sizes)."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_memory_attend as ATTEND
from tests import cpu_stub_decode_attention as DECODE
from tests import cpu_stub_extend_attention as EXTEND
from tests import cpu_stub_row_linear as ROWLIN
from tests import cpu_stub_row_linear_epilogue as GATE
from tests import memory_attend_rule as RULE
from tests import test_host_memory_layer as BASE

SHAPES = [(96, 4), (16, 2)]


def _stubs(monkeypatch):
    for stub in (ROWLIN, DECODE, GATE, ATTEND):
        stub.install(monkeypatch)


def _cross(D=96, H=4, snn=False, seed=4, dropout=0.0):
    layer = BASE._layer("cross_attention", snn=snn, bank=object(), D=D, H=H, seed=seed, dropout=dropout)
    with torch.no_grad():                                               # norms and biases that are not the identity
        for n in (layer.attention_norm, layer.memory_norm, layer.ffn_norm):
            n.weight.add_(0.3 * torch.randn(D))
            n.bias.add_(0.3 * torch.randn(D))
        layer.memory_attention.in_proj_bias.add_(0.5 * torch.randn(3 * D))
        layer.memory_attention.out_proj.bias.add_(0.5 * torch.randn(D))
    return layer


def _pinned(layer, ctx, B=3):
    cache = layer.new_cache(B, 16)
    layer._pin(cache, ctx)
    return cache


# ------------------------------------------------------------------------------------------------ refusals on the host
def _args(R=3, D=16, H=2, M=5):
    z = torch.zeros
    return dict(x=z(R, D), norm=(torch.ones(D), z(D)), G=z(R, H, M, D), s0=z(R, H, M), U=z(R, H, M, D), bias=z(D),
                eps=1e-5, out=None)


def _attend(ops, a):
    return ops.memory_attend(a["x"], a["norm"], a["G"], a["s0"], a["U"], a["bias"], eps=a["eps"], out=a["out"])


def test_memory_attend_refuses_bad_arguments_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    z = torch.zeros
    bad = [
        (dict(x=z(33, 16), G=z(33, 2, 5, 16), s0=z(33, 2, 5), U=z(33, 2, 5, 16)), ValueError, "R = 33"),
        (dict(x=z(0, 16), G=z(0, 2, 5, 16), s0=z(0, 2, 5), U=z(0, 2, 5, 16)), ValueError, "R = 0"),
        (dict(x=z(3, 18), norm=(z(18), z(18)), G=z(3, 2, 5, 18), U=z(3, 2, 5, 18), bias=z(18)), ValueError, "D % 4"),
        (dict(x=z(3, 2052), norm=(z(2052), z(2052)), G=z(3, 1, 1, 2052), s0=z(3, 1, 1), U=z(3, 1, 1, 2052),
              bias=None), ValueError, "D = 2052"),
        (dict(x=z(3, 16).half()), TypeError, "fp16 x"),
        (dict(x=z(16)), ValueError, "x rank"),
        (dict(x=None), ValueError, "missing x"),
        (dict(x=z(3, 32)[:, ::2]), ValueError, "non-contiguous x"),
        (dict(norm=None), ValueError, "missing norm"),
        (dict(norm=(torch.ones(16), None)), ValueError, "a norm without bias"),
        (dict(norm=(torch.ones(12), z(12))), ValueError, "gamma length"),
        (dict(norm=(torch.ones(16).double(), z(16))), TypeError, "fp64 gamma"),
        (dict(eps=-1.0), ValueError, "negative eps"),
        (dict(eps=float("nan")), ValueError, "NaN eps"),
        (dict(eps="1e-5"), ValueError, "an eps that is no number"),
        (dict(G=None), ValueError, "missing G"),
        (dict(G=z(3, 10, 16)), ValueError, "G rank"),
        (dict(G=z(2, 2, 5, 16)), ValueError, "G rows"),
        (dict(G=z(3, 2, 5, 12)), ValueError, "G width"),
        (dict(G=z(3, 2, 5, 16).bfloat16()), TypeError, "bf16 G"),
        (dict(G=z(3, 2, 5, 32)[..., ::2]), ValueError, "non-contiguous G"),
        (dict(G=z(3, 2, 33, 16), s0=z(3, 2, 33), U=z(3, 2, 33, 16)), ValueError, "M = 33"),
        (dict(G=z(3, 2, 0, 16), s0=z(3, 2, 0), U=z(3, 2, 0, 16)), ValueError, "M = 0"),
        (dict(G=z(3, 33, 32, 16), s0=z(3, 33, 32), U=z(3, 33, 32, 16)), ValueError, "H M = 1056"),
        (dict(G=z(3, 0, 5, 16), s0=z(3, 0, 5), U=z(3, 0, 5, 16)), ValueError, "H = 0"),
        (dict(s0=None), ValueError, "missing s0"),
        (dict(s0=z(3, 2, 4)), ValueError, "s0 shape"),
        (dict(s0=z(3, 2, 5).double()), TypeError, "fp64 s0"),
        (dict(U=None), ValueError, "missing U"),
        (dict(U=z(3, 2, 4, 16)), ValueError, "U shape"),
        (dict(U=z(3, 2, 5, 16).half()), TypeError, "fp16 U"),
        (dict(bias=z(12)), ValueError, "bias length"),
        (dict(bias=z(16).double()), TypeError, "fp64 bias"),
        (dict(out=z(3, 12)), ValueError, "out shape"),
        (dict(out=z(3, 16).half()), TypeError, "fp16 out"),
    ]
    for change, exc, why in bad:
        a = _args()
        a.update(change)
        with pytest.raises(exc):
            _attend(ops, a)
            pytest.fail(f"accepted: {why}")
    # valid calls get as far as the device check, still without the library: CPU tensors are refused
    for a in (_args(), dict(_args(), bias=None), _args(R=32, D=2048, H=1, M=32), _args(R=1, D=4, H=32, M=32),
              dict(_args(), out=z(3, 16))):
        with pytest.raises(ops.AuraDeviceError):
            _attend(ops, a)
    a = _args()
    assert ops._memory_attend_args(a["x"], a["norm"], a["G"], a["s0"], a["U"], a["bias"], 1e-5, None)[:4] == (3, 16, 2, 5)


def test_the_library_refuses_bad_attend_geometry_and_pointers_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 0x10000                                           # never dereferenced: every call below returns on the host

    def call(R=3, D=16, H=2, M=5, eps=1e-5, **ptr):
        p = dict(x=P, gamma=P, beta=P, G=P, s0=P, U=P, bo=P, y=P)
        p.update(ptr)
        return lib.aura_memory_attend(p["x"], R, D, p["gamma"], p["beta"], eps, p["G"], p["s0"], p["U"], H, M, p["bo"],
                                      p["y"], None)
    INVAL, ALIGN = -1, -3
    for kw in (dict(R=0), dict(R=33), dict(D=0), dict(D=18), dict(D=2052), dict(H=0), dict(M=0), dict(M=33),
               dict(H=33, M=32), dict(H=2 ** 40, M=1), dict(eps=-1.0), dict(eps=float("nan")), dict(x=None),
               dict(gamma=None), dict(beta=None), dict(G=None), dict(s0=None), dict(U=None), dict(y=None)):
        assert call(**kw) == INVAL, kw
    for name in ("x", "gamma", "beta", "G", "U", "bo", "y"):
        assert call(**{name: P + 4}) == ALIGN, name
    assert call(s0=P + 2) == ALIGN


# ------------------------------------------------------------------------------------------------ the rule's own bound
@pytest.mark.parametrize("kind", ["random", "uniform", "onehot", "offset"])
def test_the_rule_in_fp32_stays_within_half_the_derived_bound(kind):
    """The NumPy restatement in fp32 against the one in fp64: the bound is derived, and this is its first customer."""
    for n, (R, D, H, M) in enumerate(((1, 4, 1, 1), (3, 96, 4, 5), (3, 100, 5, 3), (2, 768, 7, 3), (1, 64, 32, 32))):
        rng = np.random.default_rng(10 * n + 1)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        x, gamma, beta = f(R, D), (1.0 + 0.3 * f(D)).astype(np.float32), (0.3 * f(D)).astype(np.float32)
        G, s0, U, bo = (f(R, H, M, D) / np.sqrt(D)).astype(np.float32), f(R, H, M), f(R, H, M, D), f(D)
        if kind == "uniform":
            G[:], s0[:] = 0.0, f(R, H, 1)
        elif kind == "onehot":
            G[:] = 0.0
            s0[:, :, M // 2] = np.float32(201.0)
        elif kind == "offset":
            x = (np.float32(1e3) + x).astype(np.float32)
        want = RULE.attend64(x, gamma, beta, G, s0, U, bo)
        got = RULE.attend32(x, gamma, beta, G, s0, U, bo)
        share = np.abs(got["y"].astype(np.float64) - want["y"]) / want["bound"]
        assert bool(np.isfinite(want["bound"]).all()) and share.max() <= 0.5, (kind, (R, D, H, M), share.max())
        assert bool(np.all(np.abs(got["p"].astype(np.float64) - want["p"]) <= 0.5 * want["dp"]))
        if kind == "uniform" and M & (M - 1) == 0:
            assert bool(np.all(got["p"] == np.float32(1.0 / M)))
        if kind == "onehot":
            assert bool(np.all(got["p"][:, :, M // 2] == 1.0)) and float(got["p"].sum()) == R * H


# ------------------------------------------------------------------------------------------------ the fold
def _tables64(layer, features):
    """The tables of the rule in fp64, one head and memory at a time: another order of evaluation than the layer's."""
    att = layer.memory_attention
    B, M, D = features.shape
    H = att.num_heads
    dh = D // H
    W, b = att.in_proj_weight.detach().double(), att.in_proj_bias.detach().double()
    Wo = att.out_proj.weight.detach().double()
    G, s0, U = torch.zeros(B, H, M, D, dtype=torch.float64), torch.zeros(B, H, M, dtype=torch.float64), \
        torch.zeros(B, H, M, D, dtype=torch.float64)
    for h in range(H):
        rows = slice(h * dh, (h + 1) * dh)
        Wq, bq = W[:D][rows], b[:D][rows]
        Wk, bk = W[D:2 * D][rows], b[D:2 * D][rows]
        Wv, bv = W[2 * D:][rows], b[2 * D:][rows]
        for bi in range(B):
            for m in range(M):
                mem = features[bi, m].double()
                k, v = Wk @ mem + bk, Wv @ mem + bv
                G[bi, h, m] = (Wq.T @ k) / dh ** 0.5
                s0[bi, h, m] = (bq @ k) / dh ** 0.5
                U[bi, h, m] = Wo[:, rows] @ v
    return G, s0, U


@pytest.mark.parametrize("D,H", SHAPES)
def test_every_table_element_is_one_rounding_from_its_fp64_value(D, H):
    from aura_snn_rag_amd import FoldedMemory
    layer = _cross(D, H)
    ctx = BASE._context(D=D)
    cache = _pinned(layer, ctx)
    fold = layer.fold_memory(cache)
    assert isinstance(fold, FoldedMemory) and cache.fold is fold and cache.c is None and cache.u is None
    assert fold.G.shape == (3, H, 5, D) and fold.s0.shape == (3, H, 5) and fold.U.shape == (3, H, 5, D)
    for got, want in zip(fold, _tables64(layer, ctx.features)):
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())
        assert float(want.abs().max()) > 1e-2


@pytest.mark.parametrize("D,H", SHAPES)
def test_fold_and_attend_equal_inject_cross_attention(monkeypatch, D, H):
    from aura_snn_rag_amd.core.language_zone.memory_ops import inject_cross_attention
    ops = ATTEND.install(monkeypatch)
    layer = _cross(D, H)
    ctx = BASE._context(D=D)
    fold = layer.fold_memory(_pinned(layer, ctx))
    hidden = 2.0 * torch.randn(3, D) + 0.5
    with torch.no_grad():
        want = inject_cross_attention(hidden[:, None], ctx.features, layer.memory_norm, layer.memory_attention,
                                      layer.dropout)[:, 0]
        mn = layer.memory_norm
        got = ops.memory_attend(hidden, (mn.weight, mn.bias), fold.G, fold.s0, fold.U,
                                layer.memory_attention.out_proj.bias, eps=mn.eps)
    assert ATTEND.CALLS["memory_attend"] == 1 and ATTEND.LAST == dict(R=3, D=D, H=H, M=5, bias=True, eps=mn.eps)
    assert float((want - hidden).abs().max()) > 1e-2, "the memories reach the output"
    assert float((got - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    # the NumPy rule is the same function
    rule = RULE.attend64(hidden.numpy(), mn.weight.detach().numpy(), mn.bias.detach().numpy(), fold.G.numpy(),
                         fold.s0.numpy(), fold.U.numpy(), layer.memory_attention.out_proj.bias.detach().numpy(), mn.eps)
    assert float(np.abs(rule["y"] - want.double().numpy()).max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    assert bool(np.all(rule["bound"] > 0)) and float(rule["bound"].max()) < 1e-3


def test_fold_memory_is_idempotent_cleared_by_a_pin_and_none_where_nothing_folds():
    layer = _cross()
    ctx = BASE._context()
    cache = _pinned(layer, ctx)
    assert cache.fold is None, "a pin folds nothing"
    fold = layer.fold_memory(cache)
    assert layer.fold_memory(cache) is fold, "a second call returns the tables it holds"
    layer._pin(cache, BASE._context(seed=10))
    assert cache.fold is None, "a new pin drops the tables of the old one"
    assert layer.fold_memory(cache) is not fold
    layer._pin(cache, None)
    assert layer.fold_memory(cache) is None and cache.fold is None, "nothing pinned"
    for inj in ("gate", "concat"):
        other = BASE._layer(inj, bank=object())
        held = _pinned(other, ctx)
        assert other.fold_memory(held) is None and held.fold is None, inj
    with pytest.raises(TypeError):
        layer.fold_memory(layer.attention.new_cache(3, 4))
    # empty slots are zero rows and are folded like any memory: G and U hold what the biases make of them
    from aura_snn_rag_amd import MemoryContext
    zero = _pinned(layer, MemoryContext(torch.zeros(3, 5, 96), torch.zeros(3, 5), None))
    for got, want in zip(layer.fold_memory(zero), _tables64(layer, torch.zeros(3, 5, 96))):
        assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())
    big = _pinned(layer, BASE._context(k=33))
    with pytest.raises(ValueError, match="limits"):
        layer.fold_memory(big)


# ------------------------------------------------------------------------------------------------ the layer on the stubs
def _counts():
    return (ROWLIN.CALLS["row_linear"], DECODE.CALLS["step"], ATTEND.CALLS["memory_attend"],
            GATE.CALLS["row_linear_gate"], GATE.CALLS["row_linear_gif"])


@pytest.mark.parametrize("D,H", SHAPES)
def test_the_fused_cross_attention_step_is_one_more_launch_and_equals_forward(monkeypatch, D, H):
    _stubs(monkeypatch)
    layer = _cross(D, H)
    B, P, n_new = 3, 7, 6
    S = P + n_new
    hidden, prosody = torch.randn(B, S, D), 1.5 * torch.randn(B, S, 4)
    ctx = BASE._context(D=D)
    with torch.no_grad():
        full = layer(hidden, prosody=prosody, memory=ctx)
        tol = 2e-5 * max(1.0, float(full.abs().max()))
        cache = layer.new_cache(B, 16)
        before = _counts()
        layer.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=cache, memory=ctx)
        assert _counts() == before and cache.fold is None, "prefill makes the launches it made and folds nothing"
        assert cache.c is None and cache.u is None
        with pytest.raises(ValueError, match="cross_attention.*fold_memory"):
            layer.step(hidden[:, P], prosody=prosody[:, P], cache=cache, fused=True)
        assert _counts() == before, "refused before any op"
        layer.fold_memory(cache)
        for t in range(P, S):
            step_in = hidden[:, t:t + 1] if t % 2 else hidden[:, t].contiguous()
            before = _counts()
            got = layer.step(step_in, prosody=prosody[:, t], cache=cache, fused=True)
            assert tuple(y - x for x, y in zip(before, _counts())) == (4, 1, 1, 0, 0)
            assert got.shape == (B, D) and float((got - full[:, t]).abs().max()) <= tol, t
        assert ATTEND.LAST == dict(R=B, D=D, H=H, M=5, bias=True, eps=layer.memory_norm.eps)
        assert cache.lengths.tolist() == [S] * B
        # use_memory=False, and a cache that pins nothing, step fused and inject nothing
        plain = layer(hidden, prosody=prosody, use_memory=False)
        for pin in (True, False):
            off = layer.new_cache(B, 16)
            layer.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=off, memory=ctx, use_memory=pin)
            assert (off.memory is not None) == pin and off.fold is None
            before = _counts()
            got = layer.step(hidden[:, P].contiguous(), prosody=prosody[:, P], cache=off, use_memory=False, fused=True)
            assert tuple(y - x for x, y in zip(before, _counts())) == (4, 1, 0, 0, 0)
            assert float((got - plain[:, P]).abs().max()) <= tol


def test_the_fused_hybrid_cross_attention_step_is_eleven_launches(monkeypatch):
    _stubs(monkeypatch)
    layer = _cross(snn=True, seed=6)
    B, P, D = 3, 4, 96
    hidden, ctx = torch.randn(B, P + 1, D), BASE._context()
    with torch.no_grad():
        cache = layer.new_cache(B, 8)
        layer.attention.prefill(layer.attention_norm(hidden[:, :P]), cache=cache.attention)
        layer._pin(cache, ctx)
        layer.fold_memory(cache)
        before = _counts()
        layer.step(hidden[:, P].contiguous(), cache=cache, fused=True)
        # row_linear: q/k/v, o_proj, mlp.0, mlp.2, syn1, syn2; the decode step is two launches: eleven in all
        assert tuple(y - x for x, y in zip(before, _counts())) == (6, 1, 1, 0, 2)


def test_the_fused_cross_attention_step_refuses_what_it_does_not_cover(monkeypatch):
    _stubs(monkeypatch)
    hidden, ctx = torch.randn(3, 96), BASE._context()

    def folded(layer):
        cache = _pinned(layer, ctx)
        layer.fold_memory(cache)
        return cache
    before = _counts()
    training = _cross()
    training.memory_attention.dropout = 0.1
    cache = folded(training)
    with pytest.raises(RuntimeError, match="dropout"):
        training.train().step(hidden, cache=cache, fused=True)
    plain_norm = _cross()
    plain_norm.memory_norm = torch.nn.LayerNorm(96, elementwise_affine=False)
    cache = folded(plain_norm)
    with pytest.raises(ValueError, match="memory_norm"):
        plain_norm.step(hidden, cache=cache, fused=True)
    appended = _cross()
    cache = folded(appended)
    appended.memory_attention.bias_k = torch.nn.Parameter(torch.zeros(1, 1, 96))
    appended.memory_attention.bias_v = torch.nn.Parameter(torch.zeros(1, 1, 96))
    with pytest.raises(ValueError, match="bias_k"):
        appended.step(hidden, cache=cache, fused=True)
    with pytest.raises(ValueError, match="bias_k"):
        appended.fold_memory(_pinned(appended, ctx))
    split = _cross()
    cache = folded(split)
    split.memory_attention._qkv_same_embed_dim = False
    with pytest.raises(ValueError, match="in_proj_weight"):
        split.step(hidden, cache=cache, fused=True)
    zero_attn = _cross()
    cache = folded(zero_attn)
    zero_attn.memory_attention.add_zero_attn = True
    with pytest.raises(ValueError, match="add_zero_attn"):
        zero_attn.step(hidden, cache=cache, fused=True)
    wide = _cross(D=16, H=2)
    cache = wide.new_cache(33, 4)
    wide._pin(cache, BASE._context(B=33, D=16))
    wide.fold_memory(cache)
    with pytest.raises(ValueError, match="32"):
        wide.step(torch.randn(33, 16), cache=cache, fused=True)
    assert _counts() == before, "refused before any op"


def test_a_fused_cross_attention_step_refuses_cpu_tensors_without_the_stubs():
    from aura_snn_rag_amd import ops
    layer = _cross(D=16, H=2)
    cache = _pinned(layer, BASE._context(B=1, D=16), B=1)
    layer.fold_memory(cache)
    with pytest.raises(ops.AuraDeviceError):
        layer.step(torch.zeros(1, 16), cache=cache, fused=True)


# ------------------------------------------------------------------------------------------------ the model on the stubs
def test_generate_with_fused_steps_returns_the_tokens_of_the_unfused_loop(monkeypatch):
    bank = BASE.StandInBank(torch.randn(40, 96, generator=torch.Generator().manual_seed(1)))
    m = BASE._model(monkeypatch, bank, memory_injection="cross_attention")
    ATTEND.install(monkeypatch)
    EXTEND.install(monkeypatch)
    ids = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(1))
    kw = dict(max_new_tokens=9, temperature=0.0, repetition_penalty=1.0)
    unfused, state = m.generate(ids, fused_step=False, return_state=True, capacity=40, **kw)
    assert ATTEND.CALLS["memory_attend"] == 0 and all(c.fold is None for c in state.caches)
    assert bank.recalls == 2
    fused, fstate = m.generate(ids, fused_step=True, return_state=True, capacity=40, **kw)
    assert fused.dtype == torch.int64 and torch.equal(fused, unfused)
    assert ATTEND.CALLS["memory_attend"] == 2 * 8 and all(c.fold is not None for c in fstate.caches)
    assert bank.recalls == 4, "one recall per layer and generation; the fold retrieves nothing"
    # a second turn on the state of an unfused first turn folds on demand
    more = torch.randint(0, 61, (3, 2), generator=torch.Generator().manual_seed(2))
    kw2 = dict(max_new_tokens=4, temperature=0.0, repetition_penalty=1.0)
    second = m.generate(more, state=state, fused_step=True, **kw2)
    assert all(c.fold is not None for c in state.caches) and ATTEND.CALLS["memory_attend"] == 2 * 8 + 2 * 3
    again = m.generate(more, state=fstate, fused_step=False, **kw2)
    assert torch.equal(second, again) and bank.recalls == 4
    # the ragged path folds too: right-padded prompts, fused against unfused
    from tests import cpu_stub_ragged_extend as RAGGED
    RAGGED.install(monkeypatch)
    calls = ATTEND.CALLS["memory_attend"]
    rkw = dict(max_new_tokens=5, temperature=0.0, repetition_penalty=1.0, prompt_lengths=[5, 2, 4])
    ragged = m.generate(ids, fused_step=True, **rkw)
    assert ATTEND.CALLS["memory_attend"] == calls + 2 * 4
    assert torch.equal(ragged, m.generate(ids, fused_step=False, **rkw))
    # the model's fold_memory: one entry per layer, idempotent
    folds = m.fold_memory(state)
    assert len(folds) == 2 and all(f is c.fold for f, c in zip(folds, state.caches))
    gate = BASE._model(monkeypatch, bank, memory_injection="gate")
    st = gate.new_state(3, 16)
    gate.prefill(ids, state=st)
    assert gate.fold_memory(st) == [None, None]
