"""Host side of the multi-token cached step and the resumable ``generate``, on the CPU stand-ins: the modules'
``extend`` (attention, both layer kinds, the three injections, the models), per-row positions and
``generate(.., state=, return_state=, capacity=)``.  The kernel's bits are the GPU tests' business
(tests/test_gpu_extend_attention.py); here the plumbing is held to the modules' own ``forward``."""
import types

import pytest
import torch

from tests import cpu_stub_decode_attention as DECODE
from tests import cpu_stub_extend_attention as EXTEND
from tests import cpu_stub_place_code as PLACE
from tests import cpu_stub_row_linear as ROWLIN
from tests import cpu_stub_row_linear_epilogue as GATE
from tests import cpu_stub_sampling as SAMPLE
from tests import cpu_stub_theta_gamma as THETA
from tests.test_host_memory_layer import StandInBank

INJECTIONS = ("cross_attention", "concat", "gate")
D = 96


def _config(H=4, **kw):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D, **kw)


def _shake_norms(layer):
    with torch.no_grad():                                               # norms that are not the identity
        for n in (layer.attention_norm, layer.ffn_norm):
            n.weight.add_(0.3 * torch.randn(D))
            n.bias.add_(0.3 * torch.randn(D))


def _layer(kind):
    from aura_snn_rag_amd import HippocampalTransformerLayer, MemoryAugmentedLayer
    torch.manual_seed(3)
    if kind == "plain":
        layer = HippocampalTransformerLayer(_config(), object()).eval()
    else:
        bank = StandInBank(torch.randn(40, D, generator=torch.Generator().manual_seed(1)))
        layer = MemoryAugmentedLayer(_config(), bank, use_snn_ffn=False, memory_injection=kind).eval()
    _shake_norms(layer)
    return layer


# ------------------------------------------------------------------------------------------------------ the op's checks
def _op_args(B=2, m=3, H=2, dh=8, cap=20):
    Dm = H * dh
    f = lambda *s: torch.zeros(*s)
    return dict(q=f(B, m, Dm), k_new=f(B, m, Dm), v_new=f(B, m, Dm), x=f(B, m, Dm), prosody=f(B, m, 4), Wp=f(H, 4),
                bp=f(H), wm=f(1, Dm), bm=f(1), lengths=torch.zeros(B, dtype=torch.int32), k_cache=f(B, H, cap, dh),
                v_cache=f(B, H, cap, dh), workspace=f(B * m * H * (4 + 1 * (4 + dh))))


def test_the_op_refuses_bad_arguments_before_touching_a_device():
    from aura_snn_rag_amd import ops
    assert ops.DECODE_EXTEND_MAX == 32
    assert ops.attn_decode_extend_workspace_floats(2, 3, 2, 8, 1) == 2 * 3 * 2 * (4 + 12)
    assert ops.attn_decode_extend_workspace_floats(5, 1, 2, 8, 3) == ops.attn_decode_workspace_floats(5, 2, 8, 3)
    call = lambda **kw: ops.attn_decode_extend(**{**_op_args(), **kw})
    bad = [dict(q=torch.zeros(2, 0, 16)), dict(q=torch.zeros(2, 33, 16)), dict(q=torch.zeros(2, 16)),
           dict(k_new=torch.zeros(2, 2, 16)), dict(prosody=torch.zeros(2, 4)), dict(x=torch.zeros(2, 16)),
           dict(workspace=torch.zeros(10)), dict(n_chunks=2), dict(wm=None), dict(lengths=torch.zeros(3, dtype=torch.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(TypeError):
        call(lengths=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(q=torch.zeros(2, 3, 16, dtype=torch.float64))
    with pytest.raises(ops.AuraDeviceError):                            # everything else in order: CPU tensors
        call()


def test_the_library_refuses_bad_extend_geometry_and_pointers_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 1 << 20                                                         # never dereferenced: every call below is refused
    assert lib.aura_attn_decode_extend_workspace_bytes(2, 3, 2, 8, 1) == 4 * 2 * 3 * 2 * 16
    for bad in ((2, 0, 2, 8, 1), (2, 33, 2, 8, 1), (2, 3, 2, 6, 1), (1 << 28, 32, 4, 8, 1)):
        assert lib.aura_attn_decode_extend_workspace_bytes(*bad) == -1, bad

    def call(m=3, B=2, H=2, dh=8, cap=20, nc=1, q=P, ws=P, wbytes=1 << 20, wm=P, bm=P, x=P, lengths=P):
        return lib.aura_attn_decode_extend(q, P, P, x, P, P, P, wm, bm, lengths, P, P, B, m, H, dh, cap, nc, 1, ws,
                                           wbytes, P, None, None)
    for kw in (dict(m=0), dict(m=33), dict(dh=6), dict(cap=0), dict(nc=2), dict(q=None), dict(wbytes=16), dict(bm=None),
               dict(x=None), dict(B=1 << 28, m=32, H=4, wbytes=1 << 62)):
        assert call(**kw) == -1, kw                                     # AURA_E_INVAL
    for kw in (dict(q=P + 4), dict(ws=P + 8), dict(lengths=P + 2)):
        assert call(**kw) == -3, kw                                     # AURA_E_ALIGN
    assert call(B=0) == 0                                               # launches nothing


# ------------------------------------------------------------------------------------------------------ the layers
@pytest.mark.parametrize("kind", ("plain",) + INJECTIONS)
def test_prefill_extend_and_a_step_equal_forward(monkeypatch, kind):
    for stub in (DECODE, EXTEND):
        stub.install(monkeypatch)
    layer = _layer(kind)
    B, P, m = 3, 7, 5
    S = P + m + 1
    hidden, prosody = torch.randn(B, S, D), 1.5 * torch.randn(B, S, 4)
    with torch.no_grad():
        cache = layer.new_cache(B, 16)
        first = layer.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=cache)
        if kind == "plain":
            full = layer(hidden, prosody=prosody)
        else:
            assert cache.memory is not None
            full = layer(hidden, prosody=prosody, memory=cache.memory)
        tol = 2e-5 * max(1.0, float(full.abs().max()))                  # the bound of test_host_memory_layer.py
        assert float((first - full[:, :P]).abs().max()) <= tol
        mid = layer.extend(hidden[:, P:P + m], prosody=prosody[:, P:P + m], cache=cache)
        assert mid.shape == (B, m, D) and float((mid - full[:, P:P + m]).abs().max()) <= tol
        assert cache.lengths.tolist() == [P + m] * B and cache.max_length == P + m
        last = layer.step(hidden[:, S - 1], prosody=prosody[:, S - 1], cache=cache)
        assert float((last - full[:, S - 1]).abs().max()) <= tol
        assert EXTEND.CALLS["extend"] == 1 and DECODE.CALLS["step"] == 1
        assert EXTEND.LAST["shapes"][:2] == (B, m) and EXTEND.LAST["prosody"]
        quiet = layer.new_cache(B, 16)
        layer.prefill(hidden[:, :P], cache=quiet)
        layer.extend(hidden[:, P:P + m], cache=quiet, advance=False)
        assert quiet.lengths.tolist() == [P] * B and not EXTEND.LAST["prosody"]


def test_extend_refuses_a_cache_that_may_overflow_and_bad_arguments_before_any_op(monkeypatch):
    from aura_snn_rag_amd import HippocampalProsodyAttention, ops
    for stub in (DECODE, EXTEND):
        stub.install(monkeypatch)
    torch.manual_seed(0)
    att = HippocampalProsodyAttention(_config(), object()).eval()
    cache = att.new_cache(2, 10)
    att.prefill(torch.randn(2, 6, D), cache=cache)
    with pytest.raises(RuntimeError, match="fit"):
        att.extend(torch.randn(2, 5, D), cache=cache)
    with pytest.raises(ValueError, match="m=0"):
        att.extend(torch.randn(2, 0, D), cache=cache)
    with pytest.raises(ValueError, match="m=33"):
        att.extend(torch.randn(2, 33, D), cache=att.new_cache(2, 64))
    with pytest.raises(ValueError, match="prosody"):
        att.extend(torch.randn(2, 3, D), prosody=torch.randn(2, 4), cache=cache)
    with pytest.raises(ValueError, match="prosody"):
        att.extend(torch.randn(2, 3, D), prosody=torch.randn(2, 2, 4), cache=cache)
    with pytest.raises(ValueError, match="hidden"):
        att.extend(torch.randn(2, D), cache=cache)
    with pytest.raises(TypeError):
        att.extend(torch.randn(2, 3, D).double(), cache=cache)
    with pytest.raises(ValueError, match="cache"):
        att.extend(torch.randn(3, 3, D), cache=cache)
    assert EXTEND.CALLS["extend"] == 0 and cache.max_length == 6 and cache.extend_workspace is None
    att.extend(torch.randn(2, 4, D), cache=cache)                       # exactly full
    assert cache.max_length == 10 and cache.lengths.tolist() == [10, 10]
    ws = cache.extend_workspace
    assert ws.numel() == ops.attn_decode_extend_workspace_floats(2, 4, 4, D // 4, 1)
    with pytest.raises(RuntimeError, match="fit"):
        att.extend(torch.randn(2, 1, D), cache=cache)
    cache.max_length = 8                                                # (the workspace is kept while it is large enough)
    cache.lengths.fill_(8)
    att.extend(torch.randn(2, 2, D), cache=cache)
    assert cache.extend_workspace is ws


def test_extend_refuses_cpu_tensors_without_the_stubs():
    from aura_snn_rag_amd import HippocampalProsodyAttention, ops
    att = HippocampalProsodyAttention(_config(), object()).eval()
    with pytest.raises(ops.AuraDeviceError):
        att.extend(torch.zeros(1, 2, D), cache=att.new_cache(1, 4))


# ------------------------------------------------------------------------------------------------------ the models
def _model_config(V=61):
    return types.SimpleNamespace(vocab_size=V, embedding_dim=D, num_heads=2, num_layers=2, intermediate_size=2 * D,
                                 n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                 gamma_frequency=40.0)


def _model(monkeypatch, which):
    for stub in (PLACE, THETA, DECODE, EXTEND, SAMPLE, ROWLIN, GATE):
        stub.install(monkeypatch)
    from aura_snn_rag_amd import HippocampalTransformer, SNNRAGTransformer
    torch.manual_seed(0)
    if which == "plain":
        m = HippocampalTransformer(_model_config(), None).eval()
    else:
        bank = StandInBank(torch.randn(40, D, generator=torch.Generator().manual_seed(1)))
        m = SNNRAGTransformer(_model_config(), bank, snn_layers=[], memory_injection="gate").eval()
    with torch.no_grad():
        m.semantic_encoder.token_embedding.weight.mul_(3.0)              # logits of order 1: decisive argmaxes
    return m


def _forward(m, ids, pinned):
    with torch.no_grad():
        return (m(ids) if pinned is None else m(ids, memory=pinned))[0]


def _pinned(m, state):
    return m.pinned_memory(state) if hasattr(m, "pinned_memory") else None


@pytest.mark.parametrize("which", ["plain", "rag"])
def test_the_models_extend_of_70_tokens_is_three_calls_a_layer(monkeypatch, which):
    m = _model(monkeypatch, which)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 61, (2, 76), generator=g)
    state = m.new_state(2, 80)
    with torch.no_grad():
        m.prefill(ids[:, :5], state=state)
        logits = m.extend(ids[:, 5:75], state=state)
        full = _forward(m, ids, _pinned(m, state))
        tol = 2e-5 * max(1.0, float(full.abs().max())) * 4              # four sublayers deep instead of one
        assert logits.shape == (2, 70, 61) and float((logits - full[:, 5:75]).abs().max()) <= tol
        assert EXTEND.CALLS["extend"] == 3 * 2 and EXTEND.LAST["shapes"][1] == 70 - 64
        assert state.position == 75 and state.lengths.tolist() == [75, 75]
        assert all(c.max_length == 75 for c in state.caches)
        seen = torch.zeros(2, 61, dtype=torch.uint8).scatter_(1, ids[:, :75], 1)
        assert torch.equal(state.seen, seen)
        before = DECODE.CALLS["step"], EXTEND.CALLS["extend"]
        last = m.step(ids[:, 75], state=state)
        assert float((last - full[:, 75]).abs().max()) <= tol
        assert DECODE.CALLS["step"] - before[0] == 2 and EXTEND.CALLS["extend"] == before[1]
    with pytest.raises(RuntimeError, match="fit"):
        m.extend(ids[:, :5], state=state)
    with pytest.raises(ValueError):
        m.extend(ids[:, :0], state=state)
    with pytest.raises(ValueError, match="prosody"):
        m.extend(ids[:, :2], prosody=torch.zeros(2, 4), state=state)


def test_a_state_that_is_not_ragged_steps_with_the_calls_it_made(monkeypatch):
    """The scalar position path is the parent's: ``embed_tokens(.., start=position)`` and one decode call a layer; no
    positions tensor is built.  A ragged state takes the positions from the device lengths instead."""
    m = _model(monkeypatch, "plain")
    import aura_snn_rag_amd.core.language_zone.hippocampal_transformer as HT
    calls = []
    real = HT.embed_tokens
    snap = lambda k: {n: v.clone() if isinstance(v, torch.Tensor) else v for n, v in k.items()}   # (views of the lengths)
    monkeypatch.setattr(HT, "embed_tokens", lambda *a, **k: calls.append(snap(k)) or real(*a, **k))
    ids = torch.randint(0, 61, (3, 6), generator=torch.Generator().manual_seed(2))
    state = m.new_state(3, 12)
    assert state.ragged is False and state.pending is None
    with torch.no_grad():
        m.prefill(ids[:, :4], state=state)
        calls.clear()
        m.step(ids[:, 4], state=state)
        assert DECODE.CALLS["step"] == 2 and EXTEND.CALLS["extend"] == 0
        assert calls == [dict(start=4, dense=False)] and state.position == 5
        # rows at different lengths: the same tokens at the rows' own positions
        state.lengths.copy_(torch.tensor([5, 3, -1], dtype=torch.int32))
        state.ragged = True
        calls.clear()
        m.step(ids[:, 5], state=state)
        assert list(calls[0]) == ["dense", "positions"] and calls[0]["positions"].tolist() == [[5], [3], [-1]]
        assert state.lengths.tolist() == [6, 4, -1]
        calls.clear()
        m.extend(ids[:, :3], state=state)
        assert calls[0]["positions"].tolist() == [[6, 7, 8], [4, 5, 6], [-1, 0, 1]]
        assert state.lengths.tolist() == [9, 7, -1]


# ------------------------------------------------------------------------------------------------------ generate
def _recompute(m, rows, n, pinned_of=None):
    """Greedy, row by row (B = 1): ``rows`` the histories; returns the continuations and the smallest argmax margin."""
    outs, gap = [], float("inf")
    for b, row in enumerate(rows):
        out = row[None].clone()
        pinned = None if pinned_of is None else [None if c is None else type(c)(c.features[b:b + 1], c.scores[b:b + 1],
                                                                                 None) for c in pinned_of]
        for _ in range(n):
            lg = _forward(m, out, pinned)[:, -1]
            top2 = torch.topk(lg, 2, dim=-1).values
            gap = min(gap, float(top2[0, 0] - top2[0, 1]))
            out = torch.cat([out, lg.argmax(-1, keepdim=True)], dim=1)
        outs.append(out[0, row.shape[0]:])
    return outs, gap


def _histories(ids, got, eos):
    rows = []
    for b in range(ids.shape[0]):
        new = got[b, ids.shape[1]:]
        hit = (new == eos).nonzero()
        rows.append(torch.cat([ids[b], new[:int(hit[0, 0]) + 1] if len(hit) else new]))
    return rows


@pytest.mark.parametrize("which", ["plain", "rag"])
def test_a_generation_continues_where_every_row_stood(monkeypatch, which):
    m = _model(monkeypatch, which)
    ids = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(1))
    kw = dict(temperature=0.0, repetition_penalty=1.0)
    free = m.generate(ids, max_new_tokens=7, **kw)
    again = m.generate(ids, max_new_tokens=7, **kw)
    assert torch.equal(free, again)
    eos = int(free[1, 5 + 2])                                           # row 1 finishes by its third token
    got, state = m.generate(ids, max_new_tokens=7, eos_token_id=eos, return_state=True, capacity=40, **kw)
    rows = _histories(ids, got, eos)
    assert len({len(r) for r in rows}) > 1 and any(int(r[-1]) != eos for r in rows), "ragged, and one row unfinished"
    assert state.ragged and state.finished.tolist() == [0, 0, 0] and state.capacity == 40
    assert state.lengths.tolist() == [len(r) - 1 for r in rows]
    assert state.pending.tolist() == [int(r[-1]) for r in rows]
    # turn 2: every row equals a from-scratch greedy generation over its own history and reply
    new_ids = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(8))
    pinned = _pinned(m, state)
    want, gap = _recompute(m, [torch.cat([r, new_ids[b]]) for b, r in enumerate(rows)], 6, pinned)
    assert gap > 1e-4, "the fixed seed must leave no argmax open"
    calls = EXTEND.CALLS["extend"]
    turn2, state2 = m.generate(new_ids, max_new_tokens=6, state=state, return_state=True, eos_token_id=None, **kw)
    assert state2 is state and EXTEND.CALLS["extend"] == calls + 2 and EXTEND.LAST["shapes"][1] == 6
    assert turn2.shape == (3, 11) and torch.equal(turn2[:, :5], new_ids)
    for b in range(3):
        assert torch.equal(turn2[b, 5:], want[b]), b
    assert state.lengths.tolist() == [len(r) + 5 + 6 - 1 for r in rows]
    # a third turn, then one that cannot fit: refused on the host before any op
    turn3 = m.generate(new_ids[:, :2], max_new_tokens=3, state=state, return_state=True, eos_token_id=None, **kw)[0]
    assert turn3.shape == (3, 5)
    calls = EXTEND.CALLS["extend"], DECODE.CALLS["step"]
    with pytest.raises(RuntimeError, match="capacity"):
        m.generate(new_ids, max_new_tokens=20, state=state, **kw)
    assert (EXTEND.CALLS["extend"], DECODE.CALLS["step"]) == calls
    with pytest.raises(ValueError, match="return_state"):
        m.generate(new_ids, max_new_tokens=2, state=m.new_state(3, 40), **kw)
    with pytest.raises(ValueError, match="capacity"):
        m.generate(ids, max_new_tokens=7, capacity=11, **kw)


def test_a_sampled_continuation_repeats_with_its_state_and_the_old_path_is_unchanged(monkeypatch):
    m = _model(monkeypatch, "plain")
    ids = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(1))
    new_ids = torch.randint(0, 61, (3, 4), generator=torch.Generator().manual_seed(5))
    kw = dict(temperature=0.9, top_k=20, top_p=0.95, seed=7)
    old = m.generate(ids, max_new_tokens=6, **kw)
    first = [m.generate(ids, max_new_tokens=6, return_state=True, capacity=30, **kw) for _ in range(2)]
    assert torch.equal(first[0][0], old) and torch.equal(first[1][0], old), "return_state and capacity change no token"
    assert first[0][1].step == 6 and first[0][1].seed == 7
    second = [m.generate(new_ids, max_new_tokens=5, state=s, temperature=0.9, top_k=20, top_p=0.95) for _, s in first]
    assert torch.equal(second[0], second[1]) and second[0].shape[1] <= 9
    assert first[0][1].step == 6 + (second[0].shape[1] - 4) or first[0][1].step == 11
