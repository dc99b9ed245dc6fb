"""``SNNRAGTransformer(memory_injection="cross_attention")`` on the GPU: ``generate(fused_step=True)``, which folds the
pinned memories of every layer after the prefill (``fold_memory``) and then injects them with one launch per layer and
token (``ops.memory_attend``), against the loop that recomputes ``forward(context, memory=pinned)``.

The model of tests/test_gpu_snn_rag_generate.py (D = 96, H = 4, two layers, V = 257, 200 place cells, max_seq_len = 32;
B = 3; (S, n) = (5, 9) and (30, 6); the 64-row bank) with ``memory_injection="cross_attention"``.

MLP layers (``snn_layers=[]``): greedy and sampled, token for token the recompute loop under that file's open-step
protocol (a step is OPEN when a decision of the recompute side is closer than ``1e-4 max|logit|`` to going the other way;
at an open step a row may differ and comparing it ends there; at most one open step per test).  The seeds below are
committed ones for which the recompute side alone meets that cap.  A second turn with ``fused_step=True`` on the state
of an unfused first turn folds on demand and equals, row by row, the recompute loop over the row's own history.  The
counts go to the parity record (``profiles/cross_attention_generate_parity_counts.json``).

Default SNN layers: spikes are discontinuous, so the recompute loop is no yardstick; the same seed repeats its tokens
and a row generated alone gives the tokens it gave in the batch."""
import pytest
import torch

from tests import helpers
from tests import test_gpu_snn_rag_generate as BASE

pytestmark = pytest.mark.gpu

SHAPES = BASE.SHAPES
B, V, D, OPEN = BASE.B, BASE.V, BASE.D, BASE.OPEN
MODEL_SEED, SAMPLE_SEED, TURN2_SEED = 0, 7, 8             # committed: the recompute side leaves at most one step open
_MADE = {}


def _model(dev, kind):
    """``'mlp'``: ``snn_layers=[]``; ``'snn'``: the default (layer 0 is a HybridFFN layer).  Built once, left unchanged."""
    if kind not in _MADE:
        from aura_snn_rag_amd import SNNRAGTransformer
        torch.manual_seed(MODEL_SEED)
        m = SNNRAGTransformer(BASE._config(), BASE._bank(), memory_injection="cross_attention",
                              **(dict(snn_layers=[]) if kind == "mlp" else {}))
        with torch.no_grad():
            m.semantic_encoder.token_embedding.weight.mul_(3.0)          # logits of order 1
            for layer in m.layers:                                       # a memory_norm that is not the identity
                layer.memory_norm.weight.add_(0.3 * torch.randn(D))
                layer.memory_norm.bias.add_(0.3 * torch.randn(D))
        _MADE[kind] = m.to(dev).eval()
    return _MADE[kind]


def test_the_models_are_what_the_tests_say(dev):
    mlp, snn = _model(dev, "mlp"), _model(dev, "snn")
    assert [l.use_snn_ffn for l in mlp.layers] == [False, False] and [l.use_snn_ffn for l in snn.layers] == [True, False]
    assert all(l.memory_injection == "cross_attention" for l in list(mlp.layers) + list(snn.layers))
    assert BASE._bank().memory_count == 64


@pytest.mark.parametrize("S,n", SHAPES)
def test_greedy_fused_generate_equals_the_pinned_recompute_loop(dev, monkeypatch, S, n):
    m = _model(dev, "mlp")
    ids = BASE._prompts(dev, S)
    states = BASE._capture_states(m, monkeypatch)
    got = m.generate(ids, max_new_tokens=n, temperature=0.0, repetition_penalty=1.0, use_memory=True, fused_step=True)
    assert got.shape == (B, S + n) and got.dtype == torch.int64 and torch.equal(got[:, :S], ids)
    assert all(c.fold is not None and c.fold.G.shape == (B, 4, 5, D) for c in states[0].caches), "generate folds"
    pinned = m.pinned_memory(states[0])
    assert all(p is not None and p.features.shape == (B, 5, D) for p in pinned)
    ctx = ids.clone()
    alive = [True] * B
    opened, min_gap = 0, float("inf")
    with torch.no_grad():
        for t in range(n):
            lg = m(ctx, use_memory=True, memory=pinned)[0][:, -1]
            top2 = torch.topk(lg, 2, dim=-1).values
            gap = (top2[:, 0] - top2[:, 1]) / lg.abs().max()
            tok = lg.argmax(-1)
            for b in range(B):
                if not alive[b]:
                    continue
                min_gap = min(min_gap, float(gap[b]))
                if float(gap[b]) < OPEN:
                    opened += 1
                    alive[b] = False
                    continue
                assert int(got[b, S + t]) == int(tok[b]), (b, t)
            ctx = torch.cat([ctx, got[:, S + t:S + t + 1]], dim=1)           # follow generate: the rows stay comparable
        # the logits of the fused steps against forward's over the generated sequence
        full = m(got, use_memory=True, memory=pinned)[0]
        state = m.new_state(B, S + n)
        lgs = [m.prefill(got[:, :S], state=state, use_memory=True, memory=pinned)[:, -1]]
        m.fold_memory(state)
        for t in range(S, S + n):
            lgs.append(m.step(got[:, t], state=state, use_memory=True, fused=True))
        diff, mag = float((torch.stack(lgs, dim=1) - full[:, S - 1:]).abs().max()), float(full.abs().max())
        assert float((m(got, use_memory=False)[0] - full).abs().max()) > 1e-3 * mag, "the memories matter"
    name = f"cross-attention generate greedy fused S{S}-n{n}"
    print(f"{name}: smallest relative top-2 gap {min_gap:.3e}, open steps {opened}, max |step - forward| logits "
          f"{diff:.3e} at magnitude {mag:.2f}")
    helpers.record_parity(name, B * n - opened, B * n, min_relative_gap=min_gap, open_steps=opened,
                          max_step_forward_logit_diff=diff, logit_magnitude=mag)
    assert opened <= 1
    assert diff <= 1e-4 * mag


@pytest.mark.parametrize("S,n", SHAPES)
def test_sampled_fused_generate_equals_the_pinned_recompute_loop(dev, monkeypatch, S, n):
    from aura_snn_rag_amd import ops
    m = _model(dev, "mlp")
    ids = BASE._prompts(dev, S)
    K, TOP_P, T = 20, 0.9, 0.8
    kw = dict(max_new_tokens=n, temperature=T, top_k=K, top_p=TOP_P, seed=SAMPLE_SEED, use_memory=True, fused_step=True)
    states = BASE._capture_states(m, monkeypatch)
    got = m.generate(ids, **kw)
    assert got.shape == (B, S + n)
    assert torch.equal(got, m.generate(ids, **kw)), "the same seed repeats its tokens"
    pinned = m.pinned_memory(states[0])
    ctx = ids.clone()
    alive = [True] * B
    opened = 0
    mins = dict(draw=float("inf"), kth=float("inf"), nucleus=float("inf"))
    with torch.no_grad():
        for t in range(n):
            lg = m(ctx, use_memory=True, memory=pinned)[0][:, -1]
            seen = torch.zeros(B, V, dtype=torch.uint8, device=dev).scatter_(1, ctx, 1)
            skw = dict(penalty=1.2, temperature=T, top_p=TOP_P, seed=SAMPLE_SEED, step=t, return_candidates=True)
            tok, c = ops.sample_next(lg, seen=seen.clone(), top_k=K, **skw)
            _, c1 = ops.sample_next(lg, seen=seen.clone(), top_k=K + 1, **skw)
            scale = float(lg.abs().max())
            d2 = torch.topk(c["d"], 2, dim=-1).values
            g_draw = (d2[:, 0] - d2[:, 1]) / scale                           # inf with a single kept rank
            g_kth = (c1["z"][:, K - 1] - c1["z"][:, K]) / scale
            S_ = c["cum"][:, -1:]
            g_nuc = ((c["cum"][:, :-1] - TOP_P * S_).abs() / S_).min(dim=-1).values
            for b in range(B):
                if not alive[b]:
                    continue
                gaps = dict(draw=float(g_draw[b]), kth=float(g_kth[b]), nucleus=float(g_nuc[b]))
                for name, g in gaps.items():
                    mins[name] = min(mins[name], g)
                if min(gaps.values()) < OPEN:
                    opened += 1
                    alive[b] = False
                    continue
                assert int(got[b, S + t]) == int(tok[b]), (b, t)
            ctx = torch.cat([ctx, got[:, S + t:S + t + 1]], dim=1)
    name = f"cross-attention generate sampled fused S{S}-n{n}"
    print(f"{name}: smallest gaps {mins}, open steps {opened}")
    helpers.record_parity(name, B * n - opened, B * n, open_steps=opened,
                          **{f"min_{k}_gap": v for k, v in mins.items()})
    assert opened <= 1


def test_a_fused_second_turn_after_an_unfused_first_equals_a_generation_from_scratch(dev):
    m = _model(dev, "mlp")
    S1, N1, S2, N2 = 5, 7, 5, 6
    greedy = dict(temperature=0.0, repetition_penalty=1.0, eos_token_id=None)
    ids = BASE._prompts(dev, S1)
    got, state = m.generate(ids, max_new_tokens=N1, return_state=True, capacity=64, fused_step=False, **greedy)
    assert all(c.fold is None for c in state.caches), "an unfused turn folds nothing"
    new_ids = torch.randint(0, V, (B, S2), generator=torch.Generator().manual_seed(TURN2_SEED)).to(dev)
    turn2 = m.generate(new_ids, max_new_tokens=N2, state=state, fused_step=True, **greedy)
    assert turn2.shape == (B, S2 + N2) and torch.equal(turn2[:, :S2], new_ids)
    assert all(c.fold is not None for c in state.caches), "the turn folded on demand"
    pinned = m.pinned_memory(state)
    opened, min_gap = 0, float("inf")
    with torch.no_grad():
        for b in range(B):
            memory = [type(c)(c.features[b:b + 1], c.scores[b:b + 1], None) for c in pinned]
            ctx = torch.cat([got[b], new_ids[b]])[None]
            for t in range(N2):
                lg = m(ctx, memory=memory)[0][:, -1]
                top2 = torch.topk(lg, 2, dim=-1).values
                gap = float((top2[0, 0] - top2[0, 1]) / lg.abs().max())
                min_gap = min(min_gap, gap)
                if gap < OPEN:
                    opened += 1
                    break
                assert int(turn2[b, S2 + t]) == int(lg.argmax(-1)), (b, t)
                ctx = torch.cat([ctx, turn2[b:b + 1, S2 + t:S2 + t + 1]], dim=1)
    print(f"cross-attention second turn: smallest relative top-2 gap {min_gap:.3e}, open steps {opened}")
    helpers.record_parity("cross-attention generate second turn fused", B * N2 - opened, B * N2,
                          min_relative_gap=min_gap, open_steps=opened)
    assert opened <= 1
    assert state.lengths.tolist() == [S1 + N1 + S2 + N2 - 1] * B


def test_snn_layers_a_seed_repeats_and_a_row_alone_gives_its_tokens(dev):
    m = _model(dev, "snn")
    ids = BASE._prompts(dev, 5)
    kw = dict(max_new_tokens=9, temperature=0.8, top_k=20, top_p=0.9, use_memory=True, fused_step=True)
    a, b, c = m.generate(ids, seed=7, **kw), m.generate(ids, seed=7, **kw), m.generate(ids, seed=8, **kw)
    assert a.shape == (B, 14) and torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a, m.generate(ids, seed=7, **dict(kw, use_memory=False))), "the memories reach the tokens"
    for row in (0, B - 1):
        alone = m.generate(ids[row:row + 1], seed=7, stream_ids=[row], **kw)
        assert torch.equal(alone[0], a[row]), f"row {row} alone"
