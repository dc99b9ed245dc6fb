"""The fused decoding step on the GPU: ``HippocampalTransformerLayer.step(fused=True)`` against the layer's formula in
fp64, and ``HippocampalTransformer.generate(fused_step=True)`` against the loop that recomputes ``forward``.

Layer level (D = 96, H = 4 and D = 768, H = 12; B = 3; a prompt of 7 and 6 steps; with prosody and memory gate, and
without both).  The fp64 result is the module's own causal forward in double precision over the whole sequence: the
forward at position t is the stepped function of the rows 0 .. t (tests/test_host_decode_attention.py holds the two
within 1e-12 of each other), so it is the fp64 formula of the layer stepped over the same inputs.  Yardstick: the
unfused ``step()``'s largest error against that fp64 result at the same shape.  Margin: a factor of 4 over it; both
sides are fp32 evaluations that differ only in summation order, and a wrong sub-stage is orders of magnitude beyond it.
Both errors go to the parity record (``profiles/fused_step_parity_counts.json``).  The appended K and V are held against
the row-linear rule's bound (tests/row_linear_rule.py) of the LayerNorm + projection of the same hidden row.

Model level: the model, prompts, shapes and seeds of tests/test_gpu_generate.py (D 96, two layers, V 257, (S, n) =
(5, 9) and (30, 6), B = 3) and its open-step protocol: a step is OPEN when a decision of the recompute side is closer
than ``1e-4 max|logit|`` to going the other way; at an open step a row may differ and comparing it ends there; at most
one open step per test.  At these seeds the recompute side has none (profiles/generate_parity_counts.json)."""
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import row_linear_rule as RULE

pytestmark = pytest.mark.gpu

B, P, N_NEW = 3, 7, 6
S_ALL = P + N_NEW
LAYER_CASES = [(96, 4, True), (96, 4, False), (768, 12, True), (768, 12, False)]
LAYER_IDS = [f"D{d}-H{h}-{'gated' if g else 'plain'}" for d, h, g in LAYER_CASES]
_RUNS = {}


def _layer_config(D, H):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D)


def _prefilled(layer, r, rows=slice(None)):
    """A cache holding the rows ``rows`` of the batch prefill (copied, so that every run starts from the same bits)."""
    src = r["prefilled"]
    n = src.k[rows].shape[0]
    c = layer.new_cache(n, 16)
    c.k.copy_(src.k[rows])
    c.v.copy_(src.v[rows])
    c.lengths.copy_(src.lengths[rows])
    c.max_length = src.max_length
    return c


def _steps(layer, r, cache, fused, rows=slice(None)):
    out = []
    for t in range(P, S_ALL):
        pr = None if r["prosody"] is None else r["prosody"][rows, t]
        out.append(layer.step(r["hidden"][rows, t], prosody=pr, use_memory=r["gated"], cache=cache, fused=fused))
    return torch.stack(out, dim=1)


def _run(dev, case):
    """Everything the layer tests share, computed once per case and left unchanged."""
    if case in _RUNS:
        return _RUNS[case]
    from aura_snn_rag_amd import HippocampalTransformerLayer
    D, H, gated = case
    torch.manual_seed(D + H + int(gated))
    layer = HippocampalTransformerLayer(_layer_config(D, H), hippocampus=object()).to(dev).eval()
    with torch.no_grad():
        for n in (layer.attention_norm, layer.ffn_norm):                # norms that are not the identity
            n.weight.add_(0.3 * torch.randn(D, device=dev))
            n.bias.add_(0.3 * torch.randn(D, device=dev))
    r = dict(layer=layer, gated=gated, hidden=torch.randn(B, S_ALL, D, device=dev),
             prosody=1.5 * torch.randn(B, S_ALL, 4, device=dev) if gated else None)
    with torch.no_grad():
        pr64 = None if r["prosody"] is None else r["prosody"].double()
        r["ref64"] = layer.double()(r["hidden"].double(), prosody=pr64, use_memory=gated)[:, P:]
        layer.float()
        r["prefilled"] = layer.new_cache(B, 16)
        layer.prefill(r["hidden"][:, :P], prosody=None if not gated else r["prosody"][:, :P], use_memory=gated,
                      cache=r["prefilled"])
        r["plain_cache"], r["fused_cache"] = _prefilled(layer, r), _prefilled(layer, r)
        r["plain"] = _steps(layer, r, r["plain_cache"], fused=False)
        r["fused"] = _steps(layer, r, r["fused_cache"], fused=True)
    _RUNS[case] = r
    return r


@pytest.mark.parametrize("case", LAYER_CASES, ids=LAYER_IDS)
def test_the_fused_step_is_as_close_to_fp64_as_the_unfused_step(dev, case):
    r = _run(dev, case)
    err_plain = float((r["plain"].double() - r["ref64"]).abs().max())
    err_fused = float((r["fused"].double() - r["ref64"]).abs().max())
    mag = float(r["ref64"].abs().max())
    print(f"fused step {LAYER_IDS[LAYER_CASES.index(case)]}: fused {err_fused:.3e}, unfused {err_plain:.3e}, "
          f"ratio {err_fused / err_plain:.3f}, magnitude {mag:.2f}")
    helpers.record_parity(f"fused step {LAYER_IDS[LAYER_CASES.index(case)]}", int(err_fused <= 4.0 * err_plain), 1,
                          fused_error=err_fused, unfused_error=err_plain, magnitude=mag,
                          ratio=round(err_fused / err_plain, 4))
    assert r["fused"].shape == (B, N_NEW, case[0]) and bool(torch.isfinite(r["fused"]).all())
    assert err_fused <= 4.0 * err_plain


@pytest.mark.parametrize("case", LAYER_CASES, ids=LAYER_IDS)
def test_the_fused_step_appends_the_keys_and_values_the_rule_predicts(dev, case):
    r = _run(dev, case)
    D, H, gated = case
    layer, cache = r["layer"], r["fused_cache"]
    assert cache.lengths.tolist() == [S_ALL] * B and cache.max_length == S_ALL
    assert torch.equal(cache.k[:, :, :P], r["prefilled"].k[:, :, :P]), "the prompt's keys are left alone"
    assert bool((cache.k[:, :, S_ALL:] == 0).all()) and bool((cache.v[:, :, S_ALL:] == 0).all())
    att = layer.attention
    n = lambda t: t.detach().cpu().numpy()
    norm = (n(layer.attention_norm.weight), n(layer.attention_norm.bias))
    for t in (P, S_ALL - 1):
        want = RULE.linear64(n(r["hidden"][:, t]), [n(att.k_proj.weight), n(att.v_proj.weight)],
                             [n(att.k_proj.bias), n(att.v_proj.bias)], norm=norm, eps=layer.attention_norm.eps)
        for j, kv in enumerate((cache.k, cache.v)):
            got = n(kv[:, :, t]).reshape(B, D).astype(np.float64)       # [B, H, dh] is the row's head-concatenated layout
            assert np.all(np.abs(got - want["y"][j]) <= 0.5 * want["bound"][j]), (t, j)


@pytest.mark.parametrize("case", LAYER_CASES, ids=LAYER_IDS)
def test_a_row_steps_to_the_same_bits_alone_and_a_retired_row_keeps_its_cache(dev, case):
    r = _run(dev, case)
    layer = r["layer"]
    bits = lambda t: t.contiguous().view(torch.int32)
    with torch.no_grad():
        for b in (0, B - 1):
            alone = _steps(layer, r, _prefilled(layer, r, slice(b, b + 1)), fused=True, rows=slice(b, b + 1))
            assert torch.equal(bits(alone[0]), bits(r["fused"][b])), f"row {b} alone"
        cache = _prefilled(layer, r)
        cache.retire([1])
        k0, v0 = cache.k.clone(), cache.v.clone()
        out = _steps(layer, r, cache, fused=True)
    assert torch.equal(cache.k[1], k0[1]) and torch.equal(cache.v[1], v0[1]), "a retired row's cache stays untouched"
    assert cache.lengths.tolist() == [S_ALL, -1, S_ALL]
    assert torch.equal(bits(out[0]), bits(r["fused"][0])) and torch.equal(bits(out[2]), bits(r["fused"][2]))
    assert torch.equal(cache.k[0], r["fused_cache"].k[0]) and torch.equal(cache.v[2], r["fused_cache"].v[2])


# ------------------------------------------------------------------------------------------------------- the model
SHAPES = [(5, 9), (30, 6)]
V = 257
OPEN = 1e-4
_MODEL = {}


def _config(**kw):
    return types.SimpleNamespace(vocab_size=V, embedding_dim=96, num_heads=4, num_layers=2, intermediate_size=192,
                                 n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                 gamma_frequency=40.0, **kw)


def _model(dev):
    """The model of tests/test_gpu_generate.py, built once and left unchanged."""
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


def _step_vs_forward(m, seq, S):
    """The largest |fused step logits - forward logits| over the positions S - 1 .. of ``seq`` [B, T]."""
    with torch.no_grad():
        full = m(seq, use_memory=False)[0]
        state = m.new_state(seq.shape[0], seq.shape[1])
        got = [m.prefill(seq[:, :S], state=state, use_memory=False)[:, -1]]
        for t in range(S, seq.shape[1]):
            got.append(m.step(seq[:, t], state=state, use_memory=False, fused=True))
        got = torch.stack(got, dim=1)
    return float((got - full[:, S - 1:]).abs().max()), float(full.abs().max())


@pytest.mark.parametrize("S,n", SHAPES)
def test_greedy_fused_generate_equals_the_recompute_loop(dev, S, n):
    m = _model(dev)
    ids = _prompts(dev, S)
    got = m.generate(ids, max_new_tokens=n, temperature=0.0, repetition_penalty=1.0, use_memory=False, fused_step=True)
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
    print(f"fused greedy S={S}: smallest relative top-2 gap {min_gap:.3e}, open steps {opened}, "
          f"max |step - forward| logits {diff:.3e} at magnitude {mag:.2f}")
    helpers.record_parity(f"fused generate greedy S{S}-n{n}", B * n - opened, B * n, min_relative_gap=min_gap,
                          open_steps=opened, max_step_forward_logit_diff=diff, logit_magnitude=mag)
    assert opened <= 1
    assert diff <= 1e-4 * mag


@pytest.mark.parametrize("S,n", SHAPES)
def test_sampled_fused_generate_equals_the_recompute_loop(dev, S, n):
    from aura_snn_rag_amd import ops
    m = _model(dev)
    ids = _prompts(dev, S)
    K, TOP_P, T, SEED = 20, 0.9, 0.8, 7
    kw = dict(max_new_tokens=n, temperature=T, top_k=K, top_p=TOP_P, seed=SEED, use_memory=False)
    got = m.generate(ids, fused_step=True, **kw)
    assert got.shape == (B, S + n)
    assert torch.equal(got, m.generate(ids, fused_step=True, **kw)), "the same seed repeats its tokens"
    ctx = ids.clone()
    alive = [True] * B
    opened = 0
    mins = dict(draw=float("inf"), kth=float("inf"), nucleus=float("inf"))
    with torch.no_grad():
        for t in range(n):
            lg = m(ctx, use_memory=False)[0][:, -1]
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
    print(f"fused sampled S={S}: smallest gaps {mins}, open steps {opened}")
    helpers.record_parity(f"fused generate sampled S{S}-n{n}", B * n - opened, B * n, open_steps=opened,
                          **{f"min_{k}_gap": v for k, v in mins.items()})
    assert opened <= 1


def test_the_switch_off_is_the_generate_of_before(dev):
    m = _model(dev)
    ids = _prompts(dev, 5)
    kw = dict(max_new_tokens=9, temperature=0.8, top_k=20, top_p=0.9, seed=7, use_memory=False)
    assert torch.equal(m.generate(ids, fused_step=False, **kw), m.generate(ids, **kw))
    greedy = dict(max_new_tokens=9, temperature=0.0, repetition_penalty=1.0, use_memory=False)
    assert torch.equal(m.generate(ids, fused_step=False, **greedy), m.generate(ids, **greedy))
    # and a step with the switch off is the step of before, bit for bit
    with torch.no_grad():
        a, b = m.new_state(B, 8), m.new_state(B, 8)
        m.prefill(ids, state=a, use_memory=False)
        m.prefill(ids, state=b, use_memory=False)
        tok = ids[:, -1]
        assert torch.equal(m.step(tok, state=a, use_memory=False), m.step(tok, state=b, use_memory=False, fused=False))
