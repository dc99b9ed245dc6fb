"""Continuing a generation on the GPU: ``generate(.., return_state=True, capacity=)`` and ``generate(new_ids, state=)``
of ``HippocampalTransformer`` and ``SNNRAGTransformer`` (gate injection, MLP layers).

The model of tests/test_gpu_generate.py (D = 96, H = 4, two layers, V = 257, 200 place cells; B = 3).  Turn 1 is greedy
with an EOS id taken from an EOS-free run, so that the rows finish at different steps and one does not finish.  The
returned state must stand where the definition says (recomputed on the host from the returned tokens); turn 2 feeds five
new tokens per row, and every row's tokens must equal a generation from scratch over that row's own history and reply
(B = 1), for the memory model the loop that recomputes ``forward(.., memory=pinned)`` as tests/test_gpu_snn_rag_generate.py
does.  The seeds are committed ones for which no decision of the recompute side lies within ``1e-4 max|logit|`` of going
the other way (asserted; the smallest margin goes to the parity record)."""
import types

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

B, V, D, S1, N1, S2, N2 = 3, 257, 96, 5, 7, 5, 6
OPEN = 1e-4
KINDS = ["plain", "rag"]
_MADE = {}


def _config():
    return types.SimpleNamespace(vocab_size=V, embedding_dim=D, num_heads=4, num_layers=2, intermediate_size=192,
                                 n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                 gamma_frequency=40.0)


def _model(dev, kind):
    if kind not in _MADE:
        from aura_snn_rag_amd import HippocampalTransformer, SNNRAGTransformer
        from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
        torch.manual_seed(0)
        if kind == "plain":
            m = HippocampalTransformer(_config(), None)
        else:
            bank = HippocampalFormation(feature_dim=D, max_memories=128, n_place_cells=8, n_time_cells=4,
                                        n_grid_cells=4, device="cuda", use_centroid_index=False)
            bank.create_episodic_memories([f"m{i}" for i in range(64)],
                                          torch.randn(64, D, generator=torch.Generator().manual_seed(64)))
            m = SNNRAGTransformer(_config(), bank, snn_layers=[], memory_injection="gate")
        with torch.no_grad():
            m.semantic_encoder.token_embedding.weight.mul_(3.0)          # logits of order 1
        _MADE[kind] = m.to(dev).eval()
    return _MADE[kind]


def _ids(dev, S, seed):
    return torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(seed)).to(dev)


GREEDY = dict(temperature=0.0, repetition_penalty=1.0)


def _turn1(dev, kind):
    """The EOS id (from an EOS-free run: row 1's third token), and a fresh first turn with it: (ids, eos, tokens, state)."""
    m = _model(dev, kind)
    ids = _ids(dev, S1, 1)
    if (kind, "eos") not in _MADE:
        _MADE[kind, "eos"] = int(m.generate(ids, max_new_tokens=N1, **GREEDY)[1, S1 + 2])
    eos = _MADE[kind, "eos"]
    got, state = m.generate(ids, max_new_tokens=N1, eos_token_id=eos, return_state=True, capacity=64, **GREEDY)
    return ids, eos, got, state


def _histories(ids, got, eos):
    rows = []
    for b in range(B):
        new = got[b, ids.shape[1]:]
        hit = (new == eos).nonzero()
        rows.append(torch.cat([ids[b], new[:int(hit[0, 0]) + 1] if len(hit) else new]))
    return rows


def _row_memory(m, state, b):
    if not hasattr(m, "pinned_memory"):
        return {}
    return dict(memory=[None if c is None else type(c)(c.features[b:b + 1], c.scores[b:b + 1], None)
                        for c in m.pinned_memory(state)])


@pytest.mark.parametrize("kind", KINDS)
def test_the_returned_state_stands_at_the_end_of_every_rows_history(dev, kind):
    ids, eos, got, state = _turn1(dev, kind)
    rows = _histories(ids, got, eos)
    ends = [int(r[-1]) == eos for r in rows]
    assert len({len(r) for r in rows}) > 1 and not all(ends) and any(ends), "rows finish at different steps, one does not"
    assert state.ragged and state.capacity == 64 and state.step == N1
    assert state.finished.tolist() == [0] * B
    assert state.lengths.tolist() == [len(r) - 1 for r in rows]
    assert state.pending.tolist() == [int(r[-1]) for r in rows]
    assert all(c.lengths is state.lengths for c in state.caches)
    seen = torch.zeros(B, V, dtype=torch.uint8, device=dev)
    for b, r in enumerate(rows):
        seen[b, r] = 1
    assert torch.equal(state.seen, seen)


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_turn_equals_a_generation_from_scratch_over_each_rows_history(dev, kind):
    m = _model(dev, kind)
    ids, eos, got, state = _turn1(dev, kind)
    rows = _histories(ids, got, eos)
    new_ids = _ids(dev, S2, 8)
    turn2 = m.generate(new_ids, max_new_tokens=N2, state=state, eos_token_id=None, **GREEDY)
    assert turn2.shape == (B, S2 + N2) and torch.equal(turn2[:, :S2], new_ids)
    min_gap = float("inf")
    with torch.no_grad():
        for b in range(B):
            ctx = torch.cat([rows[b], new_ids[b]])[None]
            memory = _row_memory(m, state, b)
            for t in range(N2):
                lg = m(ctx, **memory)[0][:, -1]
                top2 = torch.topk(lg, 2, dim=-1).values
                min_gap = min(min_gap, float((top2[0, 0] - top2[0, 1]) / lg.abs().max()))
                assert int(turn2[b, S2 + t]) == int(lg.argmax(-1)), (b, t)
                ctx = torch.cat([ctx, lg.argmax(-1, keepdim=True)], dim=1)
            if kind == "plain":                                         # and the cached path from scratch, alone
                scratch = m.generate(torch.cat([rows[b], new_ids[b]])[None], max_new_tokens=N2, eos_token_id=None,
                                     **GREEDY)
                assert torch.equal(scratch[0, -N2:], turn2[b, S2:]), b
    print(f"continue generate {kind}: smallest relative top-2 gap {min_gap:.3e}")
    helpers.record_parity(f"continue generate greedy {kind}", B * N2, B * N2, min_relative_gap=min_gap)
    assert min_gap > OPEN, "the committed seeds must leave no argmax open"
    assert state.lengths.tolist() == [len(r) + S2 + N2 - 1 for r in rows]


SAMPLE_SEED = {"plain": 14, "rag": 16}                   # committed: no decision of the recompute side within OPEN


def _sampled_turn(dev, kind, SEED):
    """A sampled second turn against the recompute loop: (tokens that differ, the smallest decision gap)."""
    from aura_snn_rag_amd import ops
    m = _model(dev, kind)
    ids, eos, got, state = _turn1(dev, kind)
    rows = _histories(ids, got, eos)
    new_ids = _ids(dev, S2, 8)
    K, TOP_P, T = 20, 0.9, 0.8
    wrong = []
    turn2 = m.generate(new_ids, max_new_tokens=N2, state=state, eos_token_id=None, temperature=T, top_k=K, top_p=TOP_P,
                       seed=SEED)
    assert state.seed == SEED and state.step == N1 + N2
    mins = float("inf")
    with torch.no_grad():
        for b in range(B):
            ctx = torch.cat([rows[b], new_ids[b]])[None]
            memory = _row_memory(m, state, b)
            for t in range(N2):
                lg = m(ctx, **memory)[0][:, -1]
                seen = torch.zeros(1, V, dtype=torch.uint8, device=dev).scatter_(1, ctx, 1)
                skw = dict(penalty=1.2, temperature=T, top_p=TOP_P, seed=SEED, step=N1 + t, return_candidates=True,
                           stream_ids=torch.tensor([b], dtype=torch.int64, device=dev))
                tok, c = ops.sample_next(lg, seen=seen.clone(), top_k=K, **skw)
                _, c1 = ops.sample_next(lg, seen=seen.clone(), top_k=K + 1, **skw)
                scale = float(lg.abs().max())
                d2 = torch.topk(c["d"], 2, dim=-1).values
                S_ = c["cum"][:, -1:]
                gap = min(float((d2[0, 0] - d2[0, 1]) / scale), float((c1["z"][0, K - 1] - c1["z"][0, K]) / scale),
                          float(((c["cum"][:, :-1] - TOP_P * S_).abs() / S_).min()))
                mins = min(mins, gap)
                if int(turn2[b, S2 + t]) != int(tok[0]):
                    wrong.append((b, t))
                ctx = torch.cat([ctx, turn2[b, S2 + t].view(1, 1)], dim=1)   # follow generate: the row stays comparable
    return wrong, mins


@pytest.mark.parametrize("kind", KINDS)
def test_a_sampled_continuation_equals_the_recompute_loop_with_the_same_seed_step_and_stream(dev, kind):
    wrong, mins = _sampled_turn(dev, kind, SAMPLE_SEED[kind])
    print(f"continue generate sampled {kind}: smallest decision gap {mins:.3e}, tokens that differ {wrong}")
    helpers.record_parity(f"continue generate sampled {kind}", B * N2 - len(wrong), B * N2, min_decision_gap=mins)
    assert not wrong
    assert mins > OPEN, "the committed seeds must leave no decision open"


@pytest.mark.parametrize("kind", KINDS)
def test_the_same_seed_continues_two_equal_states_with_the_same_tokens(dev, kind):
    m = _model(dev, kind)
    new_ids = _ids(dev, S2, 8)
    kw = dict(max_new_tokens=N2, temperature=0.9, top_k=20, top_p=0.95, seed=5)
    a = m.generate(new_ids, state=_turn1(dev, kind)[3], **kw)
    b = m.generate(new_ids, state=_turn1(dev, kind)[3], **kw)
    c = m.generate(new_ids, state=_turn1(dev, kind)[3], **{**kw, "seed": 6})
    assert torch.equal(a, b) and not torch.equal(a, c)


@pytest.mark.parametrize("kind", KINDS)
def test_a_third_turn_works_and_an_overflowing_turn_raises_on_the_host(dev, kind):
    m = _model(dev, kind)
    ids, eos, got, state = _turn1(dev, kind)
    rows = _histories(ids, got, eos)
    new_ids = _ids(dev, S2, 8)
    turn2, again = m.generate(new_ids, max_new_tokens=N2, state=state, return_state=True, eos_token_id=None, **GREEDY)
    assert again is state and state.pending.tolist() == turn2[:, -1].tolist()
    third = _ids(dev, 3, 9)
    turn3 = m.generate(third, max_new_tokens=4, state=state, return_state=True, eos_token_id=None, **GREEDY)[0]
    assert turn3.shape == (B, 7)
    assert state.lengths.tolist() == [len(r) + S2 + N2 + 3 + 4 - 1 for r in rows]
    with torch.no_grad():                                               # the third turn, row 0 from scratch
        ctx = torch.cat([rows[0], new_ids[0], turn2[0, S2:], third[0]])[None]
        memory = _row_memory(m, state, 0)
        for t in range(4):
            lg = m(ctx, **memory)[0][:, -1]
            top2 = torch.topk(lg, 2, dim=-1).values
            assert float((top2[0, 0] - top2[0, 1]) / lg.abs().max()) > OPEN
            assert int(turn3[0, 3 + t]) == int(lg.argmax(-1)), t
            ctx = torch.cat([ctx, lg.argmax(-1, keepdim=True)], dim=1)
    held = max(c.max_length for c in state.caches)
    lengths = state.lengths.clone()
    with pytest.raises(RuntimeError, match="capacity"):
        m.generate(new_ids, max_new_tokens=64 - held - S2 + 1, state=state, **GREEDY)
    assert torch.equal(state.lengths, lengths) and state.pending is not None
    m.generate(new_ids, max_new_tokens=64 - held - S2, state=state, eos_token_id=None, **GREEDY)   # exactly fits


@pytest.mark.parametrize("kind", KINDS)
def test_generate_without_the_new_arguments_returns_what_it_returned(dev, kind):
    m = _model(dev, kind)
    ids = _ids(dev, S1, 1)
    for kw in (GREEDY, dict(temperature=0.8, top_k=20, top_p=0.9, seed=7), dict(fused_step=True, **GREEDY)):
        old = m.generate(ids, max_new_tokens=N1, **kw)
        new, state = m.generate(ids, max_new_tokens=N1, return_state=True, capacity=40, **kw)
        assert isinstance(old, torch.Tensor) and torch.equal(old, new), kw
        assert torch.equal(old, m.generate(ids, max_new_tokens=N1, **kw))
