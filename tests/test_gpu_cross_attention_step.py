"""The fused step of a ``cross_attention`` ``MemoryAugmentedLayer`` on the GPU, with the setup of
tests/test_gpu_memory_layer.py: D = 96 / H = 4 and D = 768 / H = 12, B = 3, a prompt of 7 and 6 steps, k = 5 memories from
a ``HippocampalFormation`` holding 64 rows; with prosody.  ``prefill`` retrieves from the prompt and pins the context; every
other run of a case is handed that context and folds it (``fold_memory``).

MLP layers.  The fp64 result is the module's own ``forward(.., memory=pinned)`` in double precision over all 13 positions.
The fused steps are held to 1e-4 of the result's magnitude, the yardstick of the project's cached steps, and to 4 times the
unfused step's error at the same shape, the margin of tests/test_gpu_memory_layer.py and tests/test_gpu_fused_step.py for
the same reason: two fp32 evaluations that differ in summation order.  Both errors go to the parity record
(``profiles/cross_attention_step_parity_counts.json``).  A row steps to the same bits alone.

HybridFFN layers.  Spikes are discontinuous, so the fused step must be bit-equal to the chain of library calls written
out here: the chain of tests/test_gpu_memory_layer.py with ``ops.memory_attend`` where the gate stood."""
import pytest
import torch

from tests import helpers
from tests import test_gpu_memory_layer as BASE

pytestmark = pytest.mark.gpu

B, P, N_NEW, S_ALL, K_MEM = BASE.B, BASE.P, BASE.N_NEW, BASE.S_ALL, BASE.K_MEM
SHAPES = BASE.SHAPES
IDS = [f"D{d}-H{h}" for d, h in SHAPES]
_RUNS = {}


def _prefilled(layer, r, rows=slice(None)):
    cache = BASE._prefilled(layer, r, rows)
    assert cache.fold is None
    assert layer.fold_memory(cache) is cache.fold and cache.fold.G.shape[0] == cache.batch
    return cache


def _run(dev, shape, snn):
    """Everything a case's tests share, computed once and left unchanged."""
    key = shape + (snn,)
    if key in _RUNS:
        return _RUNS[key]
    from aura_snn_rag_amd import MemoryAugmentedLayer, MemoryContext
    D, H = shape
    torch.manual_seed(7 * D + H + int(snn))
    layer = MemoryAugmentedLayer(BASE._config(D, H), BASE._bank(D), use_snn_ffn=snn, memory_injection="cross_attention",
                                 num_retrieved=K_MEM).to(dev).eval()
    with torch.no_grad():
        for n in (layer.attention_norm, layer.memory_norm, layer.ffn_norm):      # norms that are not the identity
            n.weight.add_(0.3 * torch.randn(D, device=dev))
            n.bias.add_(0.3 * torch.randn(D, device=dev))
        layer.memory_attention.in_proj_bias.add_(0.3 * torch.randn(3 * D, device=dev))
        layer.memory_attention.out_proj.bias.add_(0.3 * torch.randn(D, device=dev))
    r = dict(layer=layer, hidden=torch.randn(B, S_ALL, D, device=dev),
             prosody=1.5 * torch.randn(B, S_ALL, 4, device=dev))
    with torch.no_grad():
        r["prefilled"] = layer.new_cache(B, 16)
        layer.prefill(r["hidden"][:, :P], prosody=r["prosody"][:, :P], use_memory=True, cache=r["prefilled"])
        r["memory"] = r["prefilled"].memory
        assert r["prefilled"].fold is None, "prefill folds nothing"
        r["plain"] = BASE._steps(layer, r, BASE._prefilled(layer, r), fused=False)
        r["fused_cache"] = _prefilled(layer, r)
        r["fused"] = BASE._steps(layer, r, r["fused_cache"], fused=True)
        if not snn:
            twin = MemoryAugmentedLayer(BASE._config(D, H), object(), use_snn_ffn=False,
                                        memory_injection="cross_attention", num_retrieved=K_MEM).to(dev).eval()
            twin.load_state_dict({k: v for k, v in layer.state_dict().items() if "hippocampus." not in k})
            m64 = MemoryContext(r["memory"].features.double(), r["memory"].scores.double(), None)
            r["ref64"] = twin.double()(r["hidden"].double(), prosody=r["prosody"].double(), use_memory=True, memory=m64)
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_steps_are_the_forward_with_the_pinned_context(dev, shape):
    D, H = shape
    r = _run(dev, shape, snn=False)
    name = IDS[SHAPES.index(shape)]
    m = r["memory"]
    assert m is not None and m.features.shape == (B, K_MEM, D)
    assert bool((m.features.abs().sum(-1) > 0).all()), "a bank of 64 rows fills all k slots"
    mag = float(r["ref64"].abs().max())
    err_plain = float((r["plain"].double() - r["ref64"][:, P:]).abs().max())
    err_fused = float((r["fused"].double() - r["ref64"][:, P:]).abs().max())
    print(f"cross_attention layer {name}: unfused steps {err_plain:.3e}, fused steps {err_fused:.3e}, ratio "
          f"{err_fused / err_plain:.3f}, magnitude {mag:.2f}")
    ok = err_fused <= 1e-4 * mag and err_fused <= 4.0 * err_plain
    helpers.record_parity(f"cross_attention layer {name}", int(ok), 1, unfused_error=err_plain, fused_error=err_fused,
                          ratio=round(err_fused / err_plain, 4), magnitude=mag)
    assert r["fused"].shape == (B, N_NEW, D) and bool(torch.isfinite(r["fused"]).all())
    assert r["fused_cache"].lengths.tolist() == [S_ALL] * B and r["fused_cache"].max_length == S_ALL
    assert err_plain <= 1e-4 * mag and err_fused <= 1e-4 * mag
    assert err_fused <= 4.0 * err_plain


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_injection_is_not_a_no_op_and_the_step_never_folds(dev, shape):
    r = _run(dev, shape, snn=False)
    layer = r["layer"]
    x, pros = r["hidden"][:, P].contiguous(), r["prosody"][:, P]
    with torch.no_grad():
        cache = BASE._prefilled(layer, r)
        with pytest.raises(ValueError, match="cross_attention.*fold_memory"):
            layer.step(x, prosody=pros, cache=cache, fused=True)
        assert cache.fold is None and cache.lengths.tolist() == [P] * B, "refused before anything moved"
        off = layer.step(x, prosody=pros, use_memory=False, cache=cache, fused=True, advance=False)
        assert float((off - r["fused"][:, 0]).abs().max()) > 1e-3, "the memories change the output"
        want = layer.step(x, prosody=pros, use_memory=False, cache=cache, advance=False)
        assert float((off - want).abs().max()) <= 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_row_steps_to_the_same_bits_alone(dev, shape):
    r = _run(dev, shape, snn=False)
    layer = r["layer"]
    bits = lambda t: t.contiguous().view(torch.int32)
    with torch.no_grad():
        for b in (0, B - 1):
            alone = BASE._steps(layer, r, _prefilled(layer, r, slice(b, b + 1)), fused=True, rows=slice(b, b + 1))
            assert torch.equal(bits(alone[0]), bits(r["fused"][b])), f"row {b} alone"


# ------------------------------------------------------------------------------------------------ HybridFFN layers
def _chain(layer, r, cache, t):
    """One fused step written out call for call."""
    from aura_snn_rag_amd import ops
    D = layer.config.embedding_dim
    x = r["hidden"][:, t].contiguous()
    hidden = layer.attention.step(x, prosody=r["prosody"][:, t], use_memory=True, cache=cache.attention, fused=True,
                                  residual=x, norm=layer.attention_norm)
    fold, mn = cache.fold, layer.memory_norm
    hidden = ops.memory_attend(hidden, (mn.weight, mn.bias), fold.G, fold.s0, fold.U,
                               layer.memory_attention.out_proj.bias, eps=mn.eps)
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
    h2 = ops.row_linear(spikes1.view(B * T, I), snn.syn2.weight, snn.syn2.bias)
    c2 = ops.row_linear(h2, n2.linear.weight, n2.linear.bias)
    out = torch.empty(B, D, device=x.device)
    ops.gif_run(c2.view(B, T, D), out, torch.zeros(B, D, device=x.device),
                torch.full((B, D), float(n2.threshold), device=x.device), n2.decay, n2.L, n2.alpha, n2.threshold, T,
                mean_out=True)
    g = 1.0 / (1.0 + torch.exp(-ffn.gate))                             # the sigmoid as the rule writes it
    return dict(y=hidden + ((1 - g) * mlp_out + g * out), spikes1=spikes1, injected=hidden, attended=hidden)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}-snn" for n in IDS])
def test_the_fused_snn_step_is_the_chain_of_library_calls_bit_for_bit(dev, shape):
    r = _run(dev, shape, snn=True)
    layer = r["layer"]
    bits = lambda t: t.contiguous().view(torch.int32)
    with torch.no_grad():
        cache = _prefilled(layer, r)
        for j, t in enumerate(range(P, S_ALL)):
            c = _chain(layer, r, cache, t)
            assert torch.equal(bits(c["y"]), bits(r["fused"][:, j])), f"step {j}"
            if j == 0:
                rate1 = float((c["spikes1"] > 0).float().mean())
                assert 0.0 < rate1 < 1.0, "the spiking branch is neither silent nor saturated"
        assert cache.lengths.tolist() == [S_ALL] * B
    assert r["fused"].shape == (B, N_NEW, shape[0]) and bool(torch.isfinite(r["fused"]).all())
    assert r["plain"].shape == r["fused"].shape and bool(torch.isfinite(r["plain"]).all())
