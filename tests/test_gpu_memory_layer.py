"""``MemoryAugmentedLayer`` on the GPU: ``prefill`` + ``step`` against the layer's formula in fp64 over the whole sequence
with the pinned memory context, and the fused step of a HybridFFN layer against the chain of library calls it is.

Setup: D = 96 / H = 4 and D = 768 / H = 12, B = 3, a prompt of 7 and 6 steps, k = 5 memories from a
``HippocampalFormation`` holding 64 rows; with prosody.  ``prefill`` retrieves from the prompt and pins the context; every
other run of a case is handed that context, so all of them inject the same memories.

MLP layers.  The fp64 result is the module's own ``forward(.., memory=pinned)`` in double precision over all 13
positions: with the memories fixed the layer is causal, so that is the stepped formula.  The unfused step (all three
injections) is held to 1e-4 of the result's magnitude, the yardstick of the project's cached steps; the fused step
(``gate`` and ``concat``) to 4 times the unfused step's error at the same shape, the margin of
tests/test_gpu_fused_step.py for the same reason: two fp32 evaluations that differ in summation order.  Both errors go
to the parity record (``profiles/memory_layer_parity_counts.json``).

HybridFFN layers.  Spikes are discontinuous, so a comparison with fp64 would flip on last-bit differences.  The fused
step must instead be bit-equal to the chain of ``ops.row_linear``, ``ops.row_linear_gate`` and ``ops.gif_run`` calls
written out here, call for call the module's formula, with the mix ``hidden + ((1 - g) mlp + g snn)`` from torch ops and
``g = 1 / (1 + exp(-gate))``, the sigmoid as the rule of the GIF epilogue writes it.  The chain's currents are held to the
row-linear rule's bound against fp64 (tests/row_linear_rule.py), and grouping the ``B * T`` rows of layer 2 does not
change a bit."""
import types

import numpy as np
import pytest
import torch

from tests import helpers
from tests import row_linear_rule as RULE

pytestmark = pytest.mark.gpu

B, P, N_NEW, K_MEM, BANK_ROWS = 3, 7, 6, 5, 64
S_ALL = P + N_NEW
SHAPES = [(96, 4), (768, 12)]
INJECTIONS = ("cross_attention", "concat", "gate")
MLP_CASES = [(d, h, inj) for d, h in SHAPES for inj in INJECTIONS]
MLP_IDS = [f"D{d}-H{h}-{inj}" for d, h, inj in MLP_CASES]
SNN_CASES = [(d, h, inj) for d, h in SHAPES for inj in ("gate", "concat")]
SNN_IDS = [f"D{d}-H{h}-{inj}-snn" for d, h, inj in SNN_CASES]
_BANKS, _RUNS = {}, {}


def _config(D, H):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D)


def _bank(D):
    """One bank of 64 memories per feature width, written once and only read afterwards."""
    if D not in _BANKS:
        from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
        hf = HippocampalFormation(feature_dim=D, max_memories=128, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", use_centroid_index=False)
        feats = torch.randn(BANK_ROWS, D, generator=torch.Generator().manual_seed(D))
        hf.create_episodic_memories([f"m{i}" for i in range(BANK_ROWS)], feats)
        _BANKS[D] = hf
    return _BANKS[D]


def _prefilled(layer, r, rows=slice(None)):
    """A cache holding the rows ``rows`` of the batch prefill (copied: every run starts from the same bits)."""
    from aura_snn_rag_amd import MemoryContext
    src = r["prefilled"]
    n = src.attention.k[rows].shape[0]
    c = layer.new_cache(n, 16)
    c.attention.k.copy_(src.attention.k[rows])
    c.attention.v.copy_(src.attention.v[rows])
    c.attention.lengths.copy_(src.attention.lengths[rows])
    c.attention.max_length = src.attention.max_length
    m = src.memory
    layer._pin(c, MemoryContext(m.features[rows], m.scores[rows], None))
    return c


def _steps(layer, r, cache, fused, rows=slice(None)):
    out = []
    for t in range(P, S_ALL):
        out.append(layer.step(r["hidden"][rows, t].contiguous(), prosody=r["prosody"][rows, t], use_memory=True,
                              cache=cache, fused=fused))
    return torch.stack(out, dim=1)


def _run(dev, case, snn):
    """Everything a case's tests share, computed once and left unchanged."""
    key = case + (snn,)
    if key in _RUNS:
        return _RUNS[key]
    from aura_snn_rag_amd import MemoryAugmentedLayer
    D, H, inj = case
    torch.manual_seed(D + H + len(inj) + int(snn))
    layer = MemoryAugmentedLayer(_config(D, H), _bank(D), use_snn_ffn=snn, memory_injection=inj,
                                 num_retrieved=K_MEM).to(dev).eval()
    with torch.no_grad():
        for n in (layer.attention_norm, layer.ffn_norm):                # norms that are not the identity
            n.weight.add_(0.3 * torch.randn(D, device=dev))
            n.bias.add_(0.3 * torch.randn(D, device=dev))
    r = dict(layer=layer, hidden=torch.randn(B, S_ALL, D, device=dev),
             prosody=1.5 * torch.randn(B, S_ALL, 4, device=dev))
    with torch.no_grad():
        r["prefilled"] = layer.new_cache(B, 16)
        r["prefill_out"] = layer.prefill(r["hidden"][:, :P], prosody=r["prosody"][:, :P], use_memory=True,
                                         cache=r["prefilled"])
        r["memory"] = r["prefilled"].memory
        r["plain_cache"] = _prefilled(layer, r)
        r["plain"] = _steps(layer, r, r["plain_cache"], fused=False)
        if inj != "cross_attention":
            r["fused_cache"] = _prefilled(layer, r)
            r["fused"] = _steps(layer, r, r["fused_cache"], fused=True)
        if not snn:
            # the fp64 formula on a twin with the same weights and no bank of its own (the shared bank stays fp32)
            from aura_snn_rag_amd import MemoryContext
            twin = MemoryAugmentedLayer(_config(D, H), object(), use_snn_ffn=False, memory_injection=inj,
                                        num_retrieved=K_MEM).to(dev).eval()
            twin.load_state_dict({k: v for k, v in layer.state_dict().items() if "hippocampus." not in k})
            m64 = MemoryContext(r["memory"].features.double(), r["memory"].scores.double(), None)
            r["ref64"] = twin.double()(r["hidden"].double(), prosody=r["prosody"].double(), use_memory=True,
                                       memory=m64)
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("case", MLP_CASES, ids=MLP_IDS)
def test_prefill_and_steps_are_the_forward_with_the_pinned_context(dev, case):
    D, H, inj = case
    r = _run(dev, case, snn=False)
    name = MLP_IDS[MLP_CASES.index(case)]
    m = r["memory"]
    assert m is not None and m.features.shape == (B, K_MEM, D) and m.scores.shape == (B, K_MEM)
    assert bool((m.features.abs().sum(-1) > 0).all()), "a bank of 64 rows fills all k slots"
    mag = float(r["ref64"].abs().max())
    err_prefill = float((r["prefill_out"].double() - r["ref64"][:, :P]).abs().max())
    err_plain = float((r["plain"].double() - r["ref64"][:, P:]).abs().max())
    print(f"memory layer {name}: prefill {err_prefill:.3e}, unfused steps {err_plain:.3e}, magnitude {mag:.2f}")
    extra = {}
    assert r["plain"].shape == (B, N_NEW, D) and bool(torch.isfinite(r["plain"]).all())
    assert r["plain_cache"].lengths.tolist() == [S_ALL] * B and r["plain_cache"].max_length == S_ALL
    ok = err_prefill <= 1e-4 * mag and err_plain <= 1e-4 * mag
    if inj != "cross_attention":
        err_fused = float((r["fused"].double() - r["ref64"][:, P:]).abs().max())
        print(f"memory layer {name}: fused steps {err_fused:.3e}, ratio {err_fused / err_plain:.3f}")
        extra = dict(fused_error=err_fused, ratio=round(err_fused / err_plain, 4))
        ok = ok and err_fused <= 4.0 * err_plain
    helpers.record_parity(f"memory layer {name}", int(ok), 1, unfused_error=err_plain, prefill_error=err_prefill,
                          magnitude=mag, **extra)
    assert err_prefill <= 1e-4 * mag and err_plain <= 1e-4 * mag
    if inj != "cross_attention":
        assert r["fused_cache"].lengths.tolist() == [S_ALL] * B
        assert extra["fused_error"] <= 4.0 * err_plain


@pytest.mark.parametrize("case", MLP_CASES, ids=MLP_IDS)
def test_the_injection_is_not_a_no_op_and_use_memory_false_skips_it(dev, case):
    from aura_snn_rag_amd import HippocampalTransformerLayer
    r = _run(dev, case, snn=False)
    layer = r["layer"]
    with torch.no_grad():
        cache = _prefilled(layer, r)
        off = layer.step(r["hidden"][:, P].contiguous(), prosody=r["prosody"][:, P], use_memory=False, cache=cache)
        assert float((off - r["plain"][:, 0]).abs().max()) > 1e-3, "the memories change the output"
        # without memory the layer is the plain attention + MLP layer with the same weights
        plain = HippocampalTransformerLayer(_config(case[0], case[1]), hippocampus=None).to(dev).eval()
        theirs = plain.state_dict()
        plain.load_state_dict({k: v for k, v in layer.state_dict().items() if k in theirs})
        kv = plain.new_cache(B, 16)
        plain.prefill(r["hidden"][:, :P], prosody=r["prosody"][:, :P], use_memory=False, cache=kv)
        want = plain.step(r["hidden"][:, P].contiguous(), prosody=r["prosody"][:, P], use_memory=False, cache=kv)
        mine = layer.new_cache(B, 16)
        layer.prefill(r["hidden"][:, :P], prosody=r["prosody"][:, :P], use_memory=False, cache=mine)
        assert mine.memory is None and mine.c is None
        got = layer.step(r["hidden"][:, P].contiguous(), prosody=r["prosody"][:, P], use_memory=False, cache=mine)
        assert float((got - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("case", [c for c in MLP_CASES if c[2] != "cross_attention"],
                         ids=[n for c, n in zip(MLP_CASES, MLP_IDS) if c[2] != "cross_attention"])
def test_a_row_steps_to_the_same_bits_alone(dev, case):
    r = _run(dev, case, snn=False)
    layer = r["layer"]
    bits = lambda t: t.contiguous().view(torch.int32)
    with torch.no_grad():
        for b in (0, B - 1):
            alone = _steps(layer, r, _prefilled(layer, r, slice(b, b + 1)), fused=True, rows=slice(b, b + 1))
            assert torch.equal(bits(alone[0]), bits(r["fused"][b])), f"row {b} alone"


# ------------------------------------------------------------------------------------------------ HybridFFN layers
def _chain(layer, r, cache, t, group_rows=None):
    """One fused step written out call for call; returns the output and the intermediate currents."""
    from aura_snn_rag_amd import ops
    D = layer.config.embedding_dim
    x = r["hidden"][:, t].contiguous()
    hidden = layer.attention.step(x, prosody=r["prosody"][:, t], use_memory=True, cache=cache.attention, fused=True,
                                  residual=x, norm=layer.attention_norm)
    if layer.memory_injection == "gate":
        hidden = ops.row_linear_gate(hidden, layer.memory_gate[0].weight[:, :D], None, cache.u, cache.c, hidden)
    else:
        hidden = hidden + 0.1 * cache.c
    ffn, snn = layer.ffn, layer.ffn.snn
    mid, xh = ops.row_linear(hidden, ffn.mlp[0].weight, ffn.mlp[0].bias,
                             norm=(layer.ffn_norm.weight, layer.ffn_norm.bias), eps=layer.ffn_norm.eps,
                             activation="gelu", return_normed=True)
    mlp_out = ops.row_linear(mid, ffn.mlp[2].weight, ffn.mlp[2].bias)
    n1, n2, T = snn.neuron1, snn.neuron2, snn.num_timesteps
    h1 = ops.row_linear(xh, snn.syn1.weight, snn.syn1.bias)
    c1 = ops.row_linear(h1, n1.linear.weight, n1.linear.bias)
    I = snn.hidden_dim
    spikes1 = torch.empty(B, T, I, device=x.device)
    ops.gif_run(c1, spikes1, torch.zeros(B, I, device=x.device), torch.full((B, I), float(n1.threshold), device=x.device),
                n1.decay, n1.L, n1.alpha, n1.threshold, T, time_invariant=True)
    rows = spikes1.view(B * T, I)
    step = B * T if group_rows is None else group_rows
    h2 = torch.cat([ops.row_linear(rows[a:a + step], snn.syn2.weight, snn.syn2.bias) for a in range(0, B * T, step)])
    c2 = torch.cat([ops.row_linear(h2[a:a + step], n2.linear.weight, n2.linear.bias) for a in range(0, B * T, step)])
    out = torch.empty(B, D, device=x.device)
    ops.gif_run(c2.view(B, T, D), out, torch.zeros(B, D, device=x.device),
                torch.full((B, D), float(n2.threshold), device=x.device), n2.decay, n2.L, n2.alpha, n2.threshold, T,
                mean_out=True)
    g = 1.0 / (1.0 + torch.exp(-ffn.gate))                             # the sigmoid as the rule writes it
    y = hidden + ((1 - g) * mlp_out + g * out)
    return dict(y=y, xh=xh, h1=h1, c1=c1, spikes1=spikes1, h2=h2, c2=c2, snn_out=out, hidden=hidden, mlp_out=mlp_out)


@pytest.mark.parametrize("case", SNN_CASES, ids=SNN_IDS)
def test_the_fused_snn_step_is_the_chain_of_library_calls_bit_for_bit(dev, case):
    r = _run(dev, case, snn=True)
    layer = r["layer"]
    bits = lambda t: t.contiguous().view(torch.int32)
    n = lambda t: t.detach().cpu().numpy()
    snn = layer.ffn.snn
    with torch.no_grad():
        cache = _prefilled(layer, r)
        for j, t in enumerate(range(P, S_ALL)):
            c = _chain(layer, r, cache, t)
            assert torch.equal(bits(layer._snn_branch(c["xh"])), bits(c["snn_out"])), f"step {j}: the spiking branch"
            assert torch.equal(bits(c["y"]), bits(r["fused"][:, j])), f"step {j}"
            if j in (0, N_NEW - 1):
                # the currents against fp64, each from the fp32 input the kernel was given
                for got, x_in, lin in ((c["h1"], c["xh"], snn.syn1), (c["c1"], c["h1"], snn.neuron1.linear),
                                       (c["h2"], c["spikes1"].view(-1, snn.hidden_dim), snn.syn2),
                                       (c["c2"], c["h2"], snn.neuron2.linear)):
                    want = RULE.linear64(n(x_in), [n(lin.weight)], [n(lin.bias)])
                    assert np.all(np.abs(n(got).astype(np.float64) - want["y"][0]) <= 0.5 * want["bound"][0])
                rate1, rate2 = float((c["spikes1"] > 0).float().mean()), float((c["snn_out"] > 0).float().mean())
                print(f"memory layer {SNN_IDS[SNN_CASES.index(case)]} step {j}: layer-1 neurons spiking {rate1:.3f}, "
                      f"layer-2 outputs above zero {rate2:.3f}")
                assert 0.0 < rate1 < 1.0, "the spiking branch is neither silent nor saturated"
        assert cache.lengths.tolist() == [S_ALL] * B
    assert r["fused"].shape == (B, N_NEW, case[0]) and bool(torch.isfinite(r["fused"]).all())
    assert r["plain"].shape == r["fused"].shape and bool(torch.isfinite(r["plain"]).all())


@pytest.mark.parametrize("case", SNN_CASES, ids=SNN_IDS)
def test_grouping_the_rows_of_layer_two_changes_no_bit(dev, case):
    r = _run(dev, case, snn=True)
    layer = r["layer"]
    T = layer.ffn.snn.num_timesteps
    bits = lambda t: t.contiguous().view(torch.int32)
    x = r["fused"][:, 0].contiguous()
    res, m = r["fused"][:, 1].contiguous(), r["fused"][:, 2].contiguous()
    with torch.no_grad():
        for mix in (None, (res, m)):
            single = layer._snn_branch(x, mix=mix)
            assert torch.equal(bits(layer._snn_branch(x, mix=mix, group_rows=T)), bits(single)), "a token per launch"
            assert torch.equal(bits(layer._snn_branch(x, mix=mix, group_rows=2 * T + 1)), bits(single)), "two, then one"
            for b in (0, B - 1):
                part = None if mix is None else (res[b:b + 1], m[b:b + 1])
                alone = layer._snn_branch(x[b:b + 1], mix=part)
                assert torch.equal(bits(alone[0]), bits(single[b])), f"row {b} alone"
        cache = _prefilled(layer, r)
        grouped = _chain(layer, r, cache, P, group_rows=T)
        assert torch.equal(bits(grouped["snn_out"]), bits(layer._snn_branch(grouped["xh"])))
