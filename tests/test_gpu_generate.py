"""``HippocampalTransformer`` on the GPU: ``forward`` against the composition of its parts, cached ``generate`` against
the loop that recomputes ``forward`` over the growing context (greedy and sampled), determinism, the row state and the
``state_dict`` surface.

The model: D = 96, H = 4, two layers, intermediate 192, V = 257, 200 place cells, max_seq_len = 32; B = 3.  Two shapes:
a prompt of 5 tokens and 9 new ones (the positions stay below max_seq_len) and a prompt of 30 and 6 new (they pass it).

Cached decoding and the recompute loop compute the same function in different orders of summation, so their logits
differ in the last bits (the project records 2.9e-7 for outputs of magnitude 1).  A step is OPEN when a decision of the
recompute side is closer than ``1e-4 max|logit|`` (about 300 times that difference) to going the other way: greedy, the
top-2 logit gap; sampled, the gap of the two best draw keys, the gap between the k-th and the (k + 1)-th logit, and the
nucleus boundary's ``|c_{j-1} - top_p S| / S`` (against 1e-4), all three from the recompute side's inspection outputs.
At an open step a row may differ, and comparing that row ends there.  At most one open step in a whole test; the
smallest gaps seen and the largest step-against-forward logit difference go to the parity record
(``profiles/generate_parity_counts.json``)."""
import json
import os
import types

import pytest
import torch
import torch.nn.functional as F

from tests import helpers

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hippocampal_transformer_keys.json")
SHAPES = [(5, 9), (30, 6)]
B, V = 3, 257
OPEN = 1e-4


def _config(**kw):
    return types.SimpleNamespace(vocab_size=V, embedding_dim=96, num_heads=4, num_layers=2, intermediate_size=192,
                                 n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                 gamma_frequency=40.0, **kw)


_MODEL = {}


def _model(dev):
    """The one model of this file, built once and left unchanged."""
    if "m" not in _MODEL:
        from aura_snn_rag_amd import HippocampalTransformer
        torch.manual_seed(0)
        m = HippocampalTransformer(_config(), None)
        with torch.no_grad():
            m.semantic_encoder.token_embedding.weight.mul_(3.0)          # logits of order 1
        _MODEL["m"] = m.to(dev).eval()
    return _MODEL["m"]


def _prompts(dev, S):
    return torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(S)).to(dev)


def _capture_states(model, monkeypatch):
    states = []
    new_state = model.new_state
    monkeypatch.setattr(model, "new_state", lambda *a, **k: states.append(new_state(*a, **k)) or states[-1])
    return states


def test_forward_is_the_composition_of_its_parts(dev):
    from aura_snn_rag_amd import embed_tokens
    m = _model(dev)
    ids = _prompts(dev, 30)
    prosody = torch.randn(B, 30, 4, generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        for pr in (None, prosody):
            logits, code = m(ids, prosody=pr, use_memory=False)
            h, code_w = embed_tokens(ids, m.semantic_encoder, m.pos_encoder, m.layer_norm)
            for layer in m.layers:
                h = layer(h, prosody=pr, use_memory=False)
            want = F.linear(h, m.semantic_encoder.token_embedding.weight)
            assert logits.shape == (B, 30, V) and torch.equal(logits, want) and torch.equal(code, code_w)
    assert m.output_head.weight is m.semantic_encoder.token_embedding.weight


def _step_vs_forward(m, seq, S):
    """The largest |step logits - forward logits| over the positions S - 1 .. of ``seq`` [B, T], both fed ``seq``."""
    with torch.no_grad():
        full = m(seq, use_memory=False)[0]
        state = m.new_state(seq.shape[0], seq.shape[1])
        got = [m.prefill(seq[:, :S], state=state, use_memory=False)[:, -1]]
        for t in range(S, seq.shape[1]):
            got.append(m.step(seq[:, t], state=state, use_memory=False))
        got = torch.stack(got, dim=1)
    return float((got - full[:, S - 1:]).abs().max()), float(full.abs().max())


@pytest.mark.parametrize("S,n", SHAPES)
def test_greedy_generate_equals_the_recompute_loop(dev, S, n):
    m = _model(dev)
    ids = _prompts(dev, S)
    got = m.generate(ids, max_new_tokens=n, temperature=0.0, repetition_penalty=1.0, use_memory=False)
    assert got.shape == (B, S + n) and got.dtype == torch.int64 and torch.equal(got[:, :S], ids)
    ctx = ids.clone()
    alive = [True] * B
    opened, min_gap = 0, float("inf")
    with torch.no_grad():
        for t in range(n):
            lg = m(ctx, use_memory=False)[0][:, -1]
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
    diff, mag = _step_vs_forward(m, got, S)
    print(f"greedy S={S}: smallest relative top-2 gap {min_gap:.3e}, open steps {opened}, "
          f"max |step - forward| logits {diff:.3e} at magnitude {mag:.2f}")
    helpers.record_parity(f"generate greedy S{S}-n{n}", B * n - opened, B * n, min_relative_gap=min_gap,
                          open_steps=opened, max_step_forward_logit_diff=diff, logit_magnitude=mag)
    assert opened <= 1
    assert diff <= 1e-4 * mag


@pytest.mark.parametrize("S,n", SHAPES)
def test_sampled_generate_equals_the_recompute_loop(dev, S, n):
    from aura_snn_rag_amd import ops
    m = _model(dev)
    ids = _prompts(dev, S)
    K, P, T, SEED = 20, 0.9, 0.8, 7
    got = m.generate(ids, max_new_tokens=n, temperature=T, top_k=K, top_p=P, seed=SEED, use_memory=False)
    assert got.shape == (B, S + n)
    ctx = ids.clone()
    alive = [True] * B
    opened = 0
    mins = dict(draw=float("inf"), kth=float("inf"), nucleus=float("inf"))
    with torch.no_grad():
        for t in range(n):
            lg = m(ctx, use_memory=False)[0][:, -1]
            seen = torch.zeros(B, V, dtype=torch.uint8, device=dev).scatter_(1, ctx, 1)
            kw = dict(penalty=1.2, temperature=T, top_p=P, seed=SEED, step=t, return_candidates=True)
            tok, c = ops.sample_next(lg, seen=seen.clone(), top_k=K, **kw)
            _, c1 = ops.sample_next(lg, seen=seen.clone(), top_k=K + 1, **kw)
            scale = float(lg.abs().max())
            d2 = torch.topk(c["d"], 2, dim=-1).values
            g_draw = (d2[:, 0] - d2[:, 1]) / scale                           # inf with a single kept rank
            g_kth = (c1["z"][:, K - 1] - c1["z"][:, K]) / scale
            S_ = c["cum"][:, -1:]
            g_nuc = ((c["cum"][:, :-1] - P * S_).abs() / S_).min(dim=-1).values
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
    print(f"sampled S={S}: smallest gaps {mins}, open steps {opened}")
    helpers.record_parity(f"generate sampled S{S}-n{n}", B * n - opened, B * n, open_steps=opened,
                          **{f"min_{k}_gap": v for k, v in mins.items()})
    assert opened <= 1


def test_determinism_streams_and_the_default_seed(dev):
    m = _model(dev)
    ids = _prompts(dev, 5)
    kw = dict(max_new_tokens=9, temperature=0.8, top_k=20, top_p=0.9, use_memory=False)
    a, b, c = m.generate(ids, seed=7, **kw), m.generate(ids, seed=7, **kw), m.generate(ids, seed=8, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(m.generate(ids[1:2], seed=7, stream_ids=[1], **kw)[0], a[1])
    assert torch.equal(m.generate(ids, seed=7, stream_ids=torch.arange(B, device=dev), **kw), a)
    torch.manual_seed(99)
    d = m.generate(ids, **kw)
    torch.manual_seed(99)
    e = m.generate(ids, **kw)
    f = m.generate(ids, **kw)
    assert torch.equal(d, e) and not torch.equal(d, f)


def test_eos_pads_trims_and_retires_the_rows_of_the_caches(dev, monkeypatch):
    m = _model(dev)
    S, n = 5, 9
    ids = _prompts(dev, S)
    kw = dict(max_new_tokens=n, temperature=0.0, repetition_penalty=1.3, use_memory=False)
    states = _capture_states(m, monkeypatch)
    free = m.generate(ids, **kw)
    eos = int(free[1, S + 2])
    first = [int((free[b, S:] == eos).nonzero()[0, 0]) if bool((free[b, S:] == eos).any()) else None for b in range(B)]
    assert first[1] is not None and first[1] <= 2
    got = m.generate(ids, eos_token_id=eos, pad_token_id=256, sync_every=2, **kw)
    keep = n if None in first else max(first) + 1
    want = free[:, :S + keep].clone()
    for b, f in enumerate(first):
        if f is not None:
            want[b, S + f + 1:] = 256
    assert torch.equal(got, want), "the finished row is padded, the other rows are unchanged"
    st_free, st_eos = states
    assert all(c.lengths is st_eos.lengths for c in st_eos.caches)
    assert st_eos.finished.tolist() == [int(f is not None) for f in first]
    f1 = first[1]
    for c_free, c_eos in zip(st_free.caches, st_eos.caches):
        assert int(c_eos.lengths[1]) == -1
        for kv_free, kv_eos in ((c_free.k, c_eos.k), (c_free.v, c_eos.v)):
            assert torch.equal(kv_eos[1, :, :S + f1], kv_free[1, :, :S + f1])      # what the row wrote before it finished
            assert bool((kv_eos[1, :, S + f1:] == 0).all()), "a retired row's cache is left alone"
    # every row finished: trimmed to the step at which the last one did; the config's EOS id is the default
    cfg_eos = types.SimpleNamespace(**dict(vars(m.config), eos_token_id=eos))
    monkeypatch.setattr(m, "config", cfg_eos)
    alone = m.generate(ids[1:2], stream_ids=[1], sync_every=1, **kw)
    assert alone.shape == (1, S + f1 + 1) and torch.equal(alone[0], free[1, :S + f1 + 1])
    assert torch.equal(m.generate(ids[1:2], eos_token_id=None, **kw)[0], free[1])


def test_advance_false_leaves_the_lengths_alone(dev):
    m = _model(dev)
    layer = m.layers[0]
    g = torch.Generator().manual_seed(5)
    hidden = torch.randn(B, 5, 96, generator=g).to(dev)
    row = torch.randn(B, 96, generator=g).to(dev)
    with torch.no_grad():
        for mod, x in ((layer, hidden), (layer.attention, hidden)):
            cache = mod.new_cache(B, 8)
            mod.prefill(x, use_memory=False, cache=cache)
            assert cache.lengths.tolist() == [5] * B
            a = mod.step(row, use_memory=False, cache=cache, advance=False)
            assert cache.lengths.tolist() == [5] * B
            b = mod.step(row, use_memory=False, cache=cache)                 # the same position again, now advancing
            assert cache.lengths.tolist() == [6] * B and torch.equal(a, b)


def test_state_dict_matches_the_reference(dev):
    from aura_snn_rag_amd import HippocampalTransformer
    golden = json.load(open(GOLDEN))
    ref = HippocampalTransformer(types.SimpleNamespace(**golden["config"]), None)
    assert [[k, list(v.shape)] for k, v in ref.state_dict().items()] == golden["keys"]
    mine = _model(dev).state_dict()
    assert list(mine) == [k for k, _ in golden["keys"]]
