"""Host side of the ragged batches, on the CPU stand-ins: ``ops.attn_decode_extend(.., counts=)``'s refusals, the
modules' ``extend(counts=)`` and ``prefill(lengths=)`` (attention through both layer kinds, the three injections, both
models), the masked retrieval mean, the cutting of counts into pieces of 32 and ``generate(.., prompt_lengths=,
new_lengths=)``.  The kernel's bits are tests/test_gpu_ragged_extend.py's business; here the plumbing is held to the
modules' own ``forward`` over each row's unpadded tokens."""
import pytest
import torch

from tests import cpu_stub_decode_attention as DECODE
from tests import cpu_stub_extend_attention as EXTEND
from tests import cpu_stub_ragged_extend as RAGGED
from tests.test_host_extend import D, INJECTIONS, _forward, _layer, _model, _op_args, _pinned, _recompute

JUNK = 50.0                                                             # what the padding holds: large, finite, wrong


# ------------------------------------------------------------------------------------------------------ the op's checks
def test_the_op_refuses_bad_counts_before_touching_a_device():
    from aura_snn_rag_amd import ops
    call = lambda counts: ops.attn_decode_extend(**_op_args(), counts=counts)
    for bad in ([1, 2], (1, 2), 2):
        with pytest.raises(TypeError, match="counts"):
            call(bad)
    with pytest.raises(TypeError, match="int32"):
        call(torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError, match="int32"):
        call(torch.zeros(2))
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                torch.zeros(4, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="counts"):
            call(bad)
    with pytest.raises(ValueError):                                     # the extend's own checks still come first
        ops.attn_decode_extend(**{**_op_args(), "q": torch.zeros(2, 33, 16)}, counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ops.AuraDeviceError):                            # everything else in order: CPU tensors
        call(torch.zeros(2, dtype=torch.int32))


def test_the_library_refuses_null_or_misaligned_counts_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 1 << 20                                                         # never dereferenced: every call below is refused

    def call(counts=P, m=3, B=2, q=P, lengths=P, wbytes=1 << 20):
        return lib.aura_attn_decode_extend_counts(q, P, P, P, P, P, P, P, P, lengths, counts, P, P, B, m, 2, 8, 20, 1, 1,
                                                  P, wbytes, P, None, None)
    assert call(counts=None) == -1                                      # AURA_E_INVAL
    assert call(counts=P + 2) == -3 and call(counts=P + 1) == -3        # AURA_E_ALIGN
    for kw in (dict(m=0), dict(m=33), dict(q=None), dict(wbytes=16)):    # the extend's validation
        assert call(**kw) == -1, kw
    assert call(q=P + 4) == -3 and call(lengths=P + 2) == -3
    assert call(B=0) == 0                                               # launches nothing


# ------------------------------------------------------------------------------------------------------ the pieces
def test_the_counts_are_cut_into_pieces_of_32():
    from aura_snn_rag_amd.core.language_zone.hippocampal_transformer import CachedDecodingMixin as M
    counts = torch.tensor([40, 3, 33, 0, 64, 70, 32], dtype=torch.int32)
    assert M.piece_counts(counts, 0).tolist() == [32, 3, 32, 0, 32, 32, 32]
    assert M.piece_counts(counts, 32).tolist() == [8, 0, 1, 0, 32, 32, 0]
    assert M.piece_counts(counts, 64).tolist() == [0, 0, 0, 0, 0, 6, 0]
    assert M.piece_counts(counts, 0).dtype == torch.int32
    assert sum(M.piece_counts(counts, t0) for t0 in (0, 32, 64)).tolist() == counts.tolist()


def test_the_masked_mean_is_the_mean_over_the_unpadded_row():
    from aura_snn_rag_amd.core.language_zone.memory_ops import masked_mean
    g = torch.Generator().manual_seed(0)
    hidden = torch.randn(4, 9, D, generator=g)
    lengths = torch.tensor([9, 1, 4, 8])
    padded = hidden.clone()
    for b, n in enumerate(lengths.tolist()):
        padded[b, n:] = float("nan")                                    # selected out, not multiplied by zero
    got = masked_mean(padded, lengths)
    assert got.dtype == hidden.dtype and bool(torch.isfinite(got).all())
    for b, n in enumerate(lengths.tolist()):
        want = hidden[b, :n].double().mean(dim=0)
        # n fp32 additions and one division of values of order 1: a few ulp; torch's own fp32 mean is no closer
        assert float((got[b].double() - want).abs().max()) <= 4e-7, b
        assert float((got[b] - hidden[b, :n].mean(dim=0)).abs().max()) <= 4e-7, b
    assert torch.equal(masked_mean(hidden, torch.full((4,), 9)), hidden.sum(dim=1) / 9.0)


# ------------------------------------------------------------------------------------------------------ the layers
def _install(monkeypatch):
    for stub in (DECODE, EXTEND, RAGGED):
        stub.install(monkeypatch)


def _pad(rows, width, tail):
    """Right-pads the [n_b, ..] rows to [B, width, ..] with ``tail`` values."""
    out = torch.full((len(rows), width) + tuple(rows[0].shape[1:]), tail, dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


@pytest.mark.parametrize("kind", ("plain",) + INJECTIONS)
def test_a_padded_prefill_a_ragged_extend_and_a_step_equal_forward_over_the_rows_own_tokens(monkeypatch, kind):
    _install(monkeypatch)
    layer = _layer(kind)
    B, lens, counts, m = 3, (7, 2, 5), (5, 0, 3), 5
    g = torch.Generator().manual_seed(11)
    rows = [torch.randn(lens[b] + counts[b] + 1, D, generator=g) for b in range(B)]
    pros = [1.5 * torch.randn(lens[b] + counts[b] + 1, 4, generator=g) for b in range(B)]
    cut = lambda t, b, lo, n: t[b][lo:lo + n]
    with torch.no_grad():
        cache = layer.new_cache(B, 16)
        first = layer.prefill(_pad([cut(rows, b, 0, lens[b]) for b in range(B)], max(lens), JUNK),
                              prosody=_pad([cut(pros, b, 0, lens[b]) for b in range(B)], max(lens), JUNK),
                              cache=cache, lengths=torch.tensor(lens))
        assert cache.lengths.tolist() == list(lens) and cache.max_length == max(lens)
        mid = layer.extend(_pad([cut(rows, b, lens[b], counts[b]) for b in range(B)], m, float("nan")),
                           prosody=_pad([cut(pros, b, lens[b], counts[b]) for b in range(B)], m, float("nan")),
                           cache=cache, counts=list(counts))
        assert mid.shape == (B, m, D)
        assert cache.lengths.tolist() == [lens[b] + counts[b] for b in range(B)]
        assert cache.max_length == max(lens) + max(counts), "a host sequence bounds by its largest count"
        last = layer.step(torch.stack([r[-1] for r in rows]), prosody=torch.stack([p[-1] for p in pros]), cache=cache)
        assert RAGGED.CALLS["ragged"] == 1 and RAGGED.COUNTS == [list(counts)] and EXTEND.CALLS["extend"] == 0
        for b in range(B):
            if kind == "plain":
                full = layer(rows[b][None], prosody=pros[b][None])[0]
            else:
                # the row alone pins the same memories: its own prefill, unpadded
                own = layer.new_cache(1, 16)
                layer.prefill(rows[b][None, :lens[b]], prosody=pros[b][None, :lens[b]], cache=own)
                assert torch.allclose(cache.memory.features[b], own.memory.features[0], atol=1e-5, rtol=0), b
                assert torch.allclose(cache.memory.scores[b], own.memory.scores[0], atol=1e-5, rtol=0), b
                full = layer(rows[b][None], prosody=pros[b][None], memory=own.memory)[0]
            tol = 2e-5 * max(1.0, float(full.abs().max()))              # the bound of test_host_memory_layer.py
            n, c = lens[b], counts[b]
            assert float((first[b, :n] - full[:n]).abs().max()) <= tol, (b, "prefill")
            assert c == 0 or float((mid[b, :c] - full[n:n + c]).abs().max()) <= tol, (b, "extend")
            assert float((last[b] - full[n + c]).abs().max()) <= tol, (b, "step")
        # counts as a tensor, and advance=False
        quiet = layer.new_cache(B, 16)
        layer.prefill(torch.randn(B, 4, D), cache=quiet)
        layer.extend(torch.randn(B, m, D), cache=quiet, counts=torch.tensor(counts, dtype=torch.int32), advance=False)
        assert quiet.max_length == 4 + m and quiet.lengths.tolist() == [4] * B


def test_extend_with_counts_refuses_what_the_host_can_see_before_any_op(monkeypatch):
    from aura_snn_rag_amd import HippocampalProsodyAttention
    _install(monkeypatch)
    torch.manual_seed(0)
    att = HippocampalProsodyAttention(_layer("plain").config, object()).eval()
    cache = att.new_cache(2, 10)
    att.prefill(torch.randn(2, 6, D), cache=cache)
    x = torch.randn(2, 5, D)
    for bad in ([6, 1], [-1, 1], [1], [1, 2, 3], [1.0, 2.0], torch.zeros(2), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="counts"):
            att.extend(x, cache=cache, counts=bad)
    with pytest.raises(RuntimeError, match="fit"):                      # 6 + 5 > 10, and the host knows the count
        att.extend(x, cache=cache, counts=[5, 0])
    with pytest.raises(ValueError, match="count_bound"):
        att.extend(x, cache=cache, count_bound=3)
    assert RAGGED.CALLS["ragged"] == 0 and EXTEND.CALLS["extend"] == 0 and cache.max_length == 6
    att.extend(x, cache=cache, counts=[4, 0])                           # m = 5 would not fit; the largest count does
    assert cache.max_length == 10 and cache.lengths.tolist() == [10, 6]


# ------------------------------------------------------------------------------------------------------ the models
def _ragged_model(monkeypatch, which):
    m = _model(monkeypatch, which)
    RAGGED.install(monkeypatch)
    return m


def _row_pinned(pinned, b):
    if pinned is None:
        return None
    return [None if c is None else type(c)(c.features[b:b + 1], c.scores[b:b + 1], None) for c in pinned]


@pytest.mark.parametrize("which", ["plain", "rag"])
def test_the_models_padded_prefill_and_ragged_extend_equal_forward_row_by_row(monkeypatch, which):
    m = _ragged_model(monkeypatch, which)
    g = torch.Generator().manual_seed(4)
    lens, counts = (9, 1, 4), (40, 3, 33)                               # 40 and 33 cross the piece edge at 32
    ids, ext = torch.randint(0, 61, (3, 9), generator=g), torch.randint(0, 61, (3, 40), generator=g)
    padded, padded_ext = ids.clone(), ext.clone()
    for b in range(3):
        padded[b, lens[b]:] = -7                                        # no token id at all: must not reach the embedding
        padded_ext[b, counts[b]:] = 10 ** 6
    state = m.new_state(3, 60)
    with torch.no_grad():
        first = m.prefill(padded, state=state, lengths=list(lens))
        assert state.ragged and state.lengths.tolist() == list(lens) and state.position == 9
        pinned = _pinned(m, state)
        logits = m.extend(padded_ext, state=state, counts=torch.tensor(counts))
        assert logits.shape == (3, 40, 61)
        assert RAGGED.CALLS["ragged"] == 2 * 2 and EXTEND.CALLS["extend"] == 0
        assert RAGGED.COUNTS == [[32, 3, 32]] * 2 + [[8, 0, 1]] * 2
        assert state.lengths.tolist() == [lens[b] + counts[b] for b in range(3)]
        assert state.position == 9 + 40 and all(c.max_length == 9 + 32 + 8 for c in state.caches)
        seen = torch.zeros(3, 61, dtype=torch.uint8)
        for b in range(3):
            hist = torch.cat([ids[b, :lens[b]], ext[b, :counts[b]]])
            seen[b, hist] = 1
            if pinned is not None:                                      # the row alone pins the same memories
                own = m.new_state(1, 16)
                m.prefill(ids[b:b + 1, :lens[b]], state=own)
                for c, o in zip(pinned, _pinned(m, own)):
                    assert torch.allclose(c.features[b], o.features[0], atol=1e-5, rtol=0)
                    assert torch.allclose(c.scores[b], o.scores[0], atol=1e-5, rtol=0)
            full = _forward(m, hist[None], _row_pinned(pinned, b))[0]
            tol = 2e-5 * max(1.0, float(full.abs().max())) * 4          # four sublayers deep, as in test_host_extend.py
            assert float((first[b, :lens[b]] - full[:lens[b]]).abs().max()) <= tol, (b, "prefill")
            assert float((logits[b, :counts[b]] - full[lens[b]:]).abs().max()) <= tol, (b, "extend")
        assert torch.equal(state.seen, seen), "only the tokens below the counts are marked"
    # 49 positions may be held of 60: the largest count decides what fits
    with pytest.raises(RuntimeError, match="fit"):
        m.extend(ext, state=state, counts=[40, 40, 40])
    before = RAGGED.CALLS["ragged"]
    with pytest.raises(ValueError, match="counts"):
        m.extend(ext[:, :4], state=state, counts=[5, 0, 0])
    with pytest.raises(ValueError, match="counts"):
        m.extend(ext[:, :4], state=state, counts=[0, -1, 0])
    with pytest.raises(ValueError, match="lengths"):
        m.prefill(ids, state=m.new_state(3, 20), lengths=[0, 1, 1])
    with pytest.raises(ValueError, match="lengths"):
        m.prefill(ids, state=m.new_state(3, 20), lengths=[10, 1, 1])
    assert RAGGED.CALLS["ragged"] == before


@pytest.mark.parametrize("which", ["plain", "rag"])
def test_a_ragged_batch_generates_what_every_row_generates_alone(monkeypatch, which):
    m = _ragged_model(monkeypatch, which)
    kw = dict(temperature=0.0, repetition_penalty=1.0, eos_token_id=None, pad_token_id=60)
    lens = (5, 1, 3)
    ids = torch.randint(0, 60, (3, 5), generator=torch.Generator().manual_seed(1))
    padded = ids.clone()
    for b in range(3):
        padded[b, lens[b]:] = 59
    got, state = m.generate(padded, max_new_tokens=6, prompt_lengths=list(lens), return_state=True, capacity=80, **kw)
    assert got.shape == (3, 11)
    rows = []
    for b in range(3):
        alone = m.generate(ids[b:b + 1, :lens[b]], max_new_tokens=6, stream_ids=[b], **kw)[0]
        assert torch.equal(got[b, :lens[b] + 6], alone), b
        assert bool((got[b, lens[b] + 6:] == 60).all()), "padding after a row's own tokens"
        rows.append(alone)
    assert state.ragged and state.lengths.tolist() == [len(r) - 1 for r in rows]
    assert state.pending.tolist() == [int(r[-1]) for r in rows]
    seen = torch.zeros(3, 61, dtype=torch.uint8)
    for b, r in enumerate(rows):
        seen[b, r] = 1
    assert torch.equal(state.seen, seen), "the padding is not in the repetition penalty's set"
    # lengths all equal to S: the tokens of the call without lengths
    assert torch.equal(m.generate(ids, max_new_tokens=6, prompt_lengths=torch.full((3,), 5), **kw),
                       m.generate(ids, max_new_tokens=6, **kw))
    # turn 2: every row equals a from-scratch greedy generation over its own history and its own new tokens
    news = (4, 0, 2)
    new_ids = torch.randint(0, 60, (3, 4), generator=torch.Generator().manual_seed(8))
    padded_new = new_ids.clone()
    for b in range(3):
        padded_new[b, news[b]:] = 59
    pinned = _pinned(m, state)
    want, gap = _recompute(m, [torch.cat([r, new_ids[b, :news[b]]]) for b, r in enumerate(rows)], 5, pinned)
    assert gap > 1e-4, "the fixed seed must leave no argmax open"
    turn2, state2 = m.generate(padded_new, max_new_tokens=5, new_lengths=torch.tensor(news), state=state,
                               return_state=True, **kw)
    assert state2 is state and turn2.shape == (3, 9)
    assert RAGGED.COUNTS[-1] == [n + 1 for n in news], "the pending token is always fed"
    for b in range(3):
        assert torch.equal(turn2[b, :news[b]], new_ids[b, :news[b]]), b
        assert torch.equal(turn2[b, news[b]:news[b] + 5], want[b]), b
        assert bool((turn2[b, news[b] + 5:] == 60).all()), b
    assert state.lengths.tolist() == [len(r) + news[b] + 5 - 1 for b, r in enumerate(rows)]
    assert state.pending.tolist() == [int(w[-1]) for w in want]


def test_generate_refuses_lengths_the_host_can_see_before_any_op(monkeypatch):
    m = _ragged_model(monkeypatch, "plain")
    ids = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(1))
    kw = dict(temperature=0.0, repetition_penalty=1.0, max_new_tokens=3)
    state = m.generate(ids, return_state=True, capacity=40, **kw)[1]
    calls = lambda: (RAGGED.CALLS["ragged"], EXTEND.CALLS["extend"], DECODE.CALLS["step"])
    before = calls()
    for bad in ([0, 1, 1], [6, 1, 1], [1, 1], [1.5, 1, 1], torch.tensor([1, 0, 1]), torch.ones(3)):
        with pytest.raises(ValueError, match="prompt_lengths"):
            m.generate(ids, prompt_lengths=bad, **kw)
    for bad in ([-1, 1, 1], [6, 1, 1], [1, 1, 1, 1], torch.tensor([1, 9, 1])):
        with pytest.raises(ValueError, match="new_lengths"):
            m.generate(ids, new_lengths=bad, state=state, **kw)
    with pytest.raises(ValueError, match="first turn"):
        m.generate(ids, new_lengths=[1, 1, 1], **kw)
    with pytest.raises(ValueError, match="first turn"):
        m.generate(ids, prompt_lengths=[1, 1, 1], state=state, **kw)
    assert calls() == before and state.pending is not None, "a refused turn leaves the state as it was"
