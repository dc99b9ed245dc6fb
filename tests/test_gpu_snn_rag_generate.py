"""``SNNRAGTransformer`` on the GPU: cached ``generate`` with pinned retrieval against the loop that recomputes
``forward(context, memory=pinned)``, determinism, batch independence of the fused path, EOS handling and the switch-off.

The model of tests/test_gpu_generate.py (D = 96, H = 4, two layers, V = 257, 200 place cells, max_seq_len = 32; B = 3;
(S, n) = (5, 9) and (30, 6)) with a 64-row bank and ``use_memory=True``.

MLP layers (``snn_layers=[]``): greedy and sampled ``generate``, ``fused_step`` on and off, equal token for token the
loop that recomputes ``forward`` over the growing context with the contexts the generation pinned at its prompt, under
the open-step protocol of tests/test_gpu_generate.py (a step is OPEN when a decision of the recompute side is closer than
``1e-4 max|logit|`` to going the other way; at an open step a row may differ and comparing it ends there; at most one
open step per test).  The counts go to the parity record (``profiles/snn_rag_generate_parity_counts.json``).

Default SNN layers: spikes are discontinuous, so the recompute loop is no yardstick; the same seed repeats its tokens, a
row generated alone gives the tokens it gave in the batch on the fused path (batch-independent by construction: every
launch of the step is), and EOS pads and retires rows."""
import types

import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

SHAPES = [(5, 9), (30, 6)]
B, V, D = 3, 257, 96
OPEN = 1e-4
_MADE = {}


def _config(**kw):
    return types.SimpleNamespace(vocab_size=V, embedding_dim=D, num_heads=4, num_layers=2, intermediate_size=192,
                                 n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                 gamma_frequency=40.0, **kw)


def _bank():
    if "bank" not in _MADE:
        from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
        hf = HippocampalFormation(feature_dim=D, max_memories=128, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", use_centroid_index=False)
        hf.create_episodic_memories([f"m{i}" for i in range(64)],
                                    torch.randn(64, D, generator=torch.Generator().manual_seed(64)))
        _MADE["bank"] = hf
    return _MADE["bank"]


def _model(dev, kind):
    """``'mlp'``: ``snn_layers=[]``; ``'snn'``: the default (layer 0 is a HybridFFN layer).  Built once, left unchanged."""
    if kind not in _MADE:
        from aura_snn_rag_amd import SNNRAGTransformer
        torch.manual_seed(0)
        m = SNNRAGTransformer(_config(), _bank(), **(dict(snn_layers=[]) if kind == "mlp" else {}))
        with torch.no_grad():
            m.semantic_encoder.token_embedding.weight.mul_(3.0)          # logits of order 1
        _MADE[kind] = m.to(dev).eval()
    return _MADE[kind]


def _prompts(dev, S):
    return torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(S)).to(dev)


def _capture_states(model, monkeypatch):
    states = []
    new_state = model.new_state
    monkeypatch.setattr(model, "new_state", lambda *a, **k: states.append(new_state(*a, **k)) or states[-1])
    return states


def test_the_models_are_what_the_tests_say(dev):
    from aura_snn_rag_amd import MemoryAugmentedLayer
    mlp, snn = _model(dev, "mlp"), _model(dev, "snn")
    assert [l.use_snn_ffn for l in mlp.layers] == [False, False] and [l.use_snn_ffn for l in snn.layers] == [True, False]
    assert all(isinstance(l, MemoryAugmentedLayer) and l.memory_injection == "gate" for l in snn.layers)
    assert snn.output_head.weight is snn.semantic_encoder.token_embedding.weight
    assert _bank().memory_count == 64


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("S,n", SHAPES)
def test_greedy_generate_equals_the_pinned_recompute_loop(dev, monkeypatch, S, n, fused):
    m = _model(dev, "mlp")
    ids = _prompts(dev, S)
    states = _capture_states(m, monkeypatch)
    got = m.generate(ids, max_new_tokens=n, temperature=0.0, repetition_penalty=1.0, use_memory=True, fused_step=fused)
    assert got.shape == (B, S + n) and got.dtype == torch.int64 and torch.equal(got[:, :S], ids)
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
        # the logits of the steps against forward's over the generated sequence
        full = m(got, use_memory=True, memory=pinned)[0]
        state = m.new_state(B, S + n)
        lgs = [m.prefill(got[:, :S], state=state, use_memory=True, memory=pinned)[:, -1]]
        for t in range(S, S + n):
            lgs.append(m.step(got[:, t], state=state, use_memory=True, fused=fused))
        diff, mag = float((torch.stack(lgs, dim=1) - full[:, S - 1:]).abs().max()), float(full.abs().max())
        # the memories matter: without them the logits are others
        assert float((m(got, use_memory=False)[0] - full).abs().max()) > 1e-3 * mag
    name = f"snn-rag generate greedy {'fused' if fused else 'unfused'} S{S}-n{n}"
    print(f"{name}: smallest relative top-2 gap {min_gap:.3e}, open steps {opened}, max |step - forward| logits "
          f"{diff:.3e} at magnitude {mag:.2f}")
    helpers.record_parity(name, B * n - opened, B * n, min_relative_gap=min_gap, open_steps=opened,
                          max_step_forward_logit_diff=diff, logit_magnitude=mag)
    assert opened <= 1
    assert diff <= 1e-4 * mag


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("S,n", SHAPES)
def test_sampled_generate_equals_the_pinned_recompute_loop(dev, monkeypatch, S, n, fused):
    from aura_snn_rag_amd import ops
    m = _model(dev, "mlp")
    ids = _prompts(dev, S)
    K, TOP_P, T, SEED = 20, 0.9, 0.8, 7
    kw = dict(max_new_tokens=n, temperature=T, top_k=K, top_p=TOP_P, seed=SEED, use_memory=True, fused_step=fused)
    states = _capture_states(m, monkeypatch)
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
            skw = dict(penalty=1.2, temperature=T, top_p=TOP_P, seed=SEED, step=t, return_candidates=True)
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
    name = f"snn-rag generate sampled {'fused' if fused else 'unfused'} S{S}-n{n}"
    print(f"{name}: smallest gaps {mins}, open steps {opened}")
    helpers.record_parity(name, B * n - opened, B * n, open_steps=opened,
                          **{f"min_{k}_gap": v for k, v in mins.items()})
    assert opened <= 1


def test_without_memory_the_mlp_model_is_the_hippocampal_transformer(dev):
    from aura_snn_rag_amd import HippocampalTransformer
    m = _model(dev, "mlp")
    plain = HippocampalTransformer(_config(), None).to(dev).eval()
    theirs = plain.state_dict()                                         # all but the injections' and the bank's entries
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if k in theirs})
    ids = _prompts(dev, 5)
    with torch.no_grad():
        assert torch.equal(m(ids, use_memory=False)[0], plain(ids, use_memory=False)[0])
    for kw in (dict(temperature=0.0, repetition_penalty=1.0), dict(temperature=0.8, top_k=20, top_p=0.9, seed=7)):
        for fused in (False, True):
            a = m.generate(ids, max_new_tokens=9, use_memory=False, fused_step=fused, **kw)
            b = plain.generate(ids, max_new_tokens=9, use_memory=False, fused_step=fused, **kw)
            assert torch.equal(a, b), (kw, fused)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_snn_layers_a_seed_repeats_and_a_row_alone_gives_its_tokens(dev, fused):
    m = _model(dev, "snn")
    ids = _prompts(dev, 5)
    kw = dict(max_new_tokens=9, temperature=0.8, top_k=20, top_p=0.9, use_memory=True, fused_step=fused)
    a, b, c = m.generate(ids, seed=7, **kw), m.generate(ids, seed=7, **kw), m.generate(ids, seed=8, **kw)
    assert a.shape == (B, 14) and torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a, m.generate(ids, seed=7, **dict(kw, use_memory=False))), "the memories reach the tokens"
    if fused:
        for row in (0, B - 1):
            alone = m.generate(ids[row:row + 1], seed=7, stream_ids=[row], **kw)
            assert torch.equal(alone[0], a[row]), f"row {row} alone"


def test_snn_layers_eos_pads_and_retires_rows(dev, monkeypatch):
    m = _model(dev, "snn")
    S, n = 5, 9
    ids = _prompts(dev, S)
    kw = dict(max_new_tokens=n, temperature=0.0, repetition_penalty=1.3, use_memory=True, fused_step=True)
    free = m.generate(ids, **kw)
    eos = int(free[1, S + 2])
    first = [int((free[b, S:] == eos).nonzero()[0, 0]) if bool((free[b, S:] == eos).any()) else None for b in range(B)]
    assert first[1] is not None and first[1] <= 2
    states = _capture_states(m, monkeypatch)
    got = m.generate(ids, eos_token_id=eos, pad_token_id=256, sync_every=2, **kw)
    keep = n if None in first else max(first) + 1
    want = free[:, :S + keep].clone()
    for b, f in enumerate(first):
        if f is not None:
            want[b, S + f + 1:] = 256
    assert torch.equal(got, want), "the finished row is padded, the other rows are unchanged"
    st = states[0]
    assert all(c.lengths is st.lengths for c in st.caches)
    assert st.finished.tolist() == [int(f is not None) for f in first]
    assert all(int(c.lengths[1]) == -1 for c in st.caches)
    f1 = first[1]
    for c in st.caches:
        assert bool((c.attention.k[1, :, S + f1:] == 0).all()), "a retired row's cache is left alone"
