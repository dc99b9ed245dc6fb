"""Ragged batches on the GPU: ``generate(.., prompt_lengths=)`` and ``generate(new_ids, state=, new_lengths=)`` of
``HippocampalTransformer`` and ``SNNRAGTransformer`` (gate injection, MLP layers, a bank of 64 rows), greedy and sampled,
with ``fused_step`` off and on.  The invariant: a row of a ragged batch generates what the row alone generates.

The model of tests/test_gpu_continue_generate.py (D = 96, H = 4, two layers, V = 257; B = 3).
  * First turn: prompt lengths (5, 1, 3) in a [3, 5] tensor whose padding holds a real token id; one run without the
    lengths shows that the padding, treated as real, changes the output.  Every row's tokens equal ``generate`` of that
    row alone (B = 1, its unpadded prompt, the same seed, ``stream_ids=[b]``); for the memory model the rows pin the
    memories they pin alone.
  * Second turn: ``new_lengths`` (4, 0, 2) in a [3, 4] tensor, and once (40, 3, 33), which crosses the 32-token piece
    edge.  Every row equals a generation from scratch over its own history, the loop that recomputes ``forward`` as
    tests/test_gpu_continue_generate.py does.
  * The returned state stands where the definition says: lengths, pending and seen recomputed on the host from the
    returned tokens.
The seeds are committed ones for which no decision of the reference side (the row alone, or from scratch) lies within
``1e-4 max|logit|`` of going the other way: asserted, a condition on the inputs and not a tolerance on the code under
test; the smallest margin goes to the parity record."""
import types

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

B, V, D = 3, 257, 96
S1, N1, LENS = 5, 6, (5, 1, 3)
S2, N2, NEWS = 4, 5, (4, 0, 2)
S3, N3, LONG = 40, 3, (40, 3, 33)
PADDING, PAD_OUT, CAPACITY = 123, 256, 128
OPEN = 1e-4
KINDS, MODES = ["plain", "rag"], ["greedy", "sampled"]
TOP_K, TOP_P, TEMPERATURE, PENALTY = 20, 0.9, 0.8, 1.2
IDS_SEED = {"plain": 1, "rag": 3}                        # committed: see the module docstring
SAMPLE_SEED = {"plain": 14, "rag": 16}
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


def _padded(dev, S, lens, seed):
    """(ids [B, S] with PADDING past every row's length, the rows' own tokens)."""
    ids = torch.randint(0, V - 1, (B, S), generator=torch.Generator().manual_seed(seed))
    for b in range(B):
        ids[b, lens[b]:] = PADDING
    ids = ids.to(dev)
    return ids, [ids[b, :lens[b]] for b in range(B)]


def _kw(mode, seed, fused=False):
    kw = dict(eos_token_id=None, pad_token_id=PAD_OUT, fused_step=fused)
    if mode == "greedy":
        return dict(temperature=0.0, repetition_penalty=1.0, **kw)
    return dict(temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, repetition_penalty=PENALTY, seed=seed, **kw)


def _memory(m, state, b):
    if not hasattr(m, "pinned_memory"):
        return {}
    return dict(memory=[None if c is None else type(c)(c.features[b:b + 1], c.scores[b:b + 1], None)
                        for c in m.pinned_memory(state)])


def _reference(m, dev, mode, seed, history, follow, memory, step0, stream):
    """The reference side's decisions over ``history`` (1-D), recomputed with ``forward`` token by token along
    ``follow``: (the places where its token is not ``follow``'s, its smallest decision margin / max|logit|)."""
    from aura_snn_rag_amd import ops
    wrong, mins = [], float("inf")
    ctx = history[None]
    with torch.no_grad():
        for t in range(follow.shape[0]):
            lg = m(ctx, **memory)[0][:, -1]
            scale = float(lg.abs().max())
            if mode == "greedy":
                top2 = torch.topk(lg, 2, dim=-1).values
                tok, gap = int(lg.argmax(-1)), float(top2[0, 0] - top2[0, 1]) / scale
            else:
                seen = torch.zeros(1, V, dtype=torch.uint8, device=dev).scatter_(1, ctx, 1)
                skw = dict(penalty=PENALTY, temperature=TEMPERATURE, top_p=TOP_P, seed=seed, step=step0 + t,
                           return_candidates=True, stream_ids=torch.tensor([stream], dtype=torch.int64, device=dev))
                tok, c = ops.sample_next(lg, seen=seen.clone(), top_k=TOP_K, **skw)
                _, c1 = ops.sample_next(lg, seen=seen.clone(), top_k=TOP_K + 1, **skw)
                d2 = torch.topk(c["d"], 2, dim=-1).values
                total = c["cum"][:, -1:]
                gap = min(float((d2[0, 0] - d2[0, 1]) / scale), float((c1["z"][0, TOP_K - 1] - c1["z"][0, TOP_K]) / scale),
                          float(((c["cum"][:, :-1] - TOP_P * total).abs() / total).min()))
                tok = int(tok[0])
            mins = min(mins, gap)
            if tok != int(follow[t]):
                wrong.append(t)
            ctx = torch.cat([ctx, follow[t].view(1, 1)], dim=1)          # follow generate: the row stays comparable
    return wrong, mins


def _host_state(histories):
    """lengths, pending and seen of a state that stands at the end of these histories."""
    seen = torch.zeros(B, V, dtype=torch.uint8)
    for b, h in enumerate(histories):
        seen[b, h.cpu()] = 1
    return [len(h) - 1 for h in histories], [int(h[-1]) for h in histories], seen


def _assert_state(state, histories):
    lengths, pending, seen = _host_state(histories)
    assert state.ragged and state.finished.tolist() == [0] * B
    assert state.lengths.tolist() == lengths and state.pending.tolist() == pending
    assert torch.equal(state.seen.cpu(), seen), "seen holds every row's own tokens and nothing of the padding"
    assert all(c.lengths is state.lengths for c in state.caches)


def first_turn(dev, kind, mode, fused, ids_seed, seed):
    """A ragged first turn against every row alone: (histories, state, tokens that differ, the smallest margin)."""
    m = _model(dev, kind)
    ids, own = _padded(dev, S1, LENS, ids_seed)
    kw = _kw(mode, seed, fused)
    got, state = m.generate(ids, max_new_tokens=N1, prompt_lengths=list(LENS), return_state=True, capacity=CAPACITY, **kw)
    assert got.shape == (B, S1 + N1)
    wrong, mins, histories = [], float("inf"), []
    for b in range(B):
        n = LENS[b]
        alone, st = m.generate(own[b][None], max_new_tokens=N1, stream_ids=[b], return_state=True, capacity=CAPACITY, **kw)
        assert torch.equal(got[b, :n], own[b]) and bool((got[b, n + N1:] == PAD_OUT).all()), "prompt, tokens, padding"
        wrong += [(b, t) for t in range(N1) if int(got[b, n + t]) != int(alone[0, n + t])]
        if kind == "rag":                                               # the row pins what it pins alone
            for c, o in zip(m.pinned_memory(state), m.pinned_memory(st)):
                assert torch.equal(c.features[b], o.features[0]), f"row {b} pins other memories than alone"
                # cosine scores of order 1 from two fp32 queries a few ulp apart (the masked and the plain mean)
                assert float((c.scores[b] - o.scores[0]).abs().max()) <= 1e-5
        ref_wrong, gap = _reference(m, dev, mode, seed, own[b], alone[0, n:], _memory(m, st, 0), 0, b)
        assert not ref_wrong, f"row {b} alone is not the recompute loop at {ref_wrong}"
        mins = min(mins, gap)
        histories.append(got[b, :n + N1])
    return histories, state, wrong, mins


def later_turn(dev, kind, mode, fused, ids_seed, seed, S, n_new, news, histories, state):
    """A ragged turn on ``state`` against a generation from scratch over every row's history."""
    m = _model(dev, kind)
    new_ids, own = _padded(dev, S, news, ids_seed + 7)
    step0 = state.step
    got, again = m.generate(new_ids, max_new_tokens=n_new, state=state, return_state=True,
                            new_lengths=torch.tensor(news, device=dev), **_kw(mode, seed, fused))
    assert again is state and got.shape == (B, S + n_new) and state.step == step0 + n_new
    wrong, mins, after = [], float("inf"), []
    for b in range(B):
        k = news[b]
        assert torch.equal(got[b, :k], own[b]) and bool((got[b, k + n_new:] == PAD_OUT).all()), "reply, tokens, padding"
        history = torch.cat([histories[b], own[b]])
        ref_wrong, gap = _reference(m, dev, mode, seed, history, got[b, k:k + n_new], _memory(m, state, b), step0, b)
        wrong += [(b, t) for t in ref_wrong]
        mins = min(mins, gap)
        after.append(torch.cat([history, got[b, k:k + n_new]]))
    return after, wrong, mins


def _record(name, n, wrong, mins):
    print(f"ragged generate {name}: smallest decision margin {mins:.3e}, tokens that differ {wrong}")
    helpers.record_parity(f"ragged generate {name}", n - len(wrong), n, min_decision_margin=mins)
    assert not wrong, f"{name}: tokens differ from the reference side at {wrong}"
    assert mins > OPEN, "the committed seeds must leave no decision of the reference side open"


@pytest.mark.parametrize("fused", [False, True], ids=["step", "fused"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_ragged_batch_generates_what_every_row_generates_alone_and_continues_so(dev, kind, mode, fused):
    seeds = IDS_SEED[kind], SAMPLE_SEED[kind]
    histories, state, wrong, mins = first_turn(dev, kind, mode, fused, *seeds)
    _assert_state(state, histories)
    assert state.capacity == CAPACITY and state.step == N1
    _record(f"first turn {kind} {mode} {'fused' if fused else 'step'}", B * N1, wrong, mins)
    after, wrong, mins = later_turn(dev, kind, mode, fused, *seeds, S2, N2, NEWS, histories, state)
    _assert_state(state, after)
    _record(f"second turn {kind} {mode} {'fused' if fused else 'step'}", B * N2, wrong, mins)


@pytest.mark.parametrize("kind", KINDS)
def test_a_ragged_turn_across_the_piece_edge_equals_a_generation_from_scratch(dev, kind):
    seeds = IDS_SEED[kind], SAMPLE_SEED[kind]
    histories, state, _, _ = first_turn(dev, kind, "greedy", False, *seeds)
    after, wrong, mins = later_turn(dev, kind, "greedy", False, *seeds, S3, N3, LONG, histories, state)
    _assert_state(state, after)
    _record(f"turn of (40, 3, 33) {kind} greedy", B * N3, wrong, mins)
    if kind == "plain":                                                 # and the cached path from scratch, alone
        m = _model(dev, kind)
        for b in range(B):
            scratch = m.generate(after[b][None, :-N3], max_new_tokens=N3, **_kw("greedy", 0))
            assert torch.equal(scratch[0], after[b]), b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_padding_would_change_the_output_if_it_were_read(dev, kind, mode):
    m = _model(dev, kind)
    ids, _ = _padded(dev, S1, LENS, IDS_SEED[kind])
    kw = _kw(mode, SAMPLE_SEED[kind])
    ragged = m.generate(ids, max_new_tokens=N1, prompt_lengths=list(LENS), **kw)
    real = m.generate(ids, max_new_tokens=N1, **kw)
    for b in range(1, B):
        assert not torch.equal(ragged[b, LENS[b]:LENS[b] + N1], real[b, S1:]), f"row {b}: the padding makes no difference"


@pytest.mark.parametrize("kind", KINDS)
def test_generate_without_the_lengths_returns_what_it_returned(dev, kind):
    m = _model(dev, kind)
    ids = torch.randint(0, V, (B, S1), generator=torch.Generator().manual_seed(1)).to(dev)
    new_ids = torch.randint(0, V, (B, S2), generator=torch.Generator().manual_seed(8)).to(dev)
    for kw in (_kw("greedy", 0), _kw("sampled", 7), _kw("greedy", 0, fused=True)):
        old, s_old = m.generate(ids, max_new_tokens=N1, return_state=True, capacity=40, **kw)
        new, s_new = m.generate(ids, max_new_tokens=N1, return_state=True, capacity=40, prompt_lengths=None,
                                new_lengths=None, **kw)
        assert torch.equal(old, new) and torch.equal(s_old.lengths, s_new.lengths), kw
        assert torch.equal(m.generate(new_ids, max_new_tokens=N2, state=s_old, **kw),
                           m.generate(new_ids, max_new_tokens=N2, state=s_new, prompt_lengths=None, new_lengths=None,
                                      **kw)), kw
        for a, b in zip(s_old.caches, s_new.caches):
            ka, kb = (c.attention.k if hasattr(c, "attention") else c.k for c in (a, b))
            assert torch.equal(ka.view(torch.int32), kb.view(torch.int32)), "the caches hold the same bits"
