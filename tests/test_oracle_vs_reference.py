"""Pins the oracle to the upstream reference: the reference modules' seeded inputs, initial state,
outputs and gradients, recorded by oracle/gen_golden_pins.py into tests/golden/reference_pins.pt.
As with the other fixtures under tests/golden/, the bits are those of torch's CPU kernels on the
x86 host (AVX-512) that recorded them; a CPU that takes other vector paths may differ in the last bit."""
import os

import pytest
import torch
import torch.nn.functional as Fn

from oracle import aura_oracle as O

PINS = os.path.join(os.path.dirname(__file__), "golden", "reference_pins.pt")


def pins(name):
    return torch.load(PINS, weights_only=False)[name]


def test_neuron_loops_bit_exact():
    d = pins("neuron_loops")
    r = d["izh"]
    v, u = O.izh_initial_state(300, 0.2)
    s, v, u = O.izh_run(r["I"], v, u, 0.02, 0.2, -65, 8, 0.2)
    assert torch.equal(r["spikes"], s) and torch.equal(r["v"], v) and torch.equal(r["u"], u)
    r = d["adex"]
    p = O.adex_params(a=2.0, b=60.0)
    sa, V, w = O.adex_run(r["I"], torch.full((32,), float(p[1])), torch.zeros(32), p)
    assert torch.equal(r["spikes"], sa) and torch.equal(r["V"], V) and torch.equal(r["w"], w)
    r = d["lif"]
    mem = torch.zeros(3, 16)
    for x, rs, rm in zip(r["x"], r["spikes"], r["mem"]):
        os_, mem = O.lif_step(x, mem, r["beta"], r["threshold"])
        assert torch.equal(rs, os_) and torch.equal(rm, mem)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gif_and_ffn_bit_exact(dtype):
    d = pins("gif_and_ffn")["f32" if dtype == torch.float32 else "bf16"]
    x = d["x"]
    assert x.dtype == dtype
    with torch.no_grad():
        os_, (ov, ot) = O.gif_forward(x, d["weight"], d["bias"], L=8, decay=d["decay"])
    assert torch.equal(d["spikes"], os_) and torch.equal(d["v"], ov) and torch.equal(d["theta"], ot)
    b = d["balanced"]
    with torch.no_grad():
        os_, _ = O.balanced_gif_forward(x, b["w_exc"], b["b_exc"], b["w_inh"], b["b_inh"], L=8, decay=b["decay"])
    assert torch.equal(b["spikes"], os_)
    if dtype == torch.float32:
        f = d["ffn"]
        with torch.no_grad():
            assert torch.equal(f["out"], O.snnffn_forward(f["x"], dict(f["state"]), T=4, L=8))


def test_bank_bit_exact_and_defects_pinned():
    d = pins("bank")
    NOW, feats, q, loc = d["now"], d["feats"], d["q"], d["loc"]
    D, M = 16, 500
    ob = O.OracleBank(M, D)
    ob.centroids_k = 8
    ob.centroids_update_interval = 32
    torch.manual_seed(9)
    for i in range(200):
        ob.write(f"m{i}", feats[i], NOW)
    assert torch.equal(d["features"], ob.features) and torch.equal(d["metadata"], ob.metadata)
    assert torch.equal(d["centroids"], ob.centroids) and torch.equal(d["centroid_counts"], ob.centroid_counts)
    ob.use_centroid_index = False
    assert d["recall_exact"] == ob.recall_ids(q, 7, NOW)
    assert d["recall_exact_loc"] == ob.recall_ids(q, 7, NOW, location=loc)
    ob.use_centroid_index = True
    r = d["recall_index"]
    rows, sc = ob.recall(q, 5, NOW)
    assert [x[1] for x in r] == [float(s) for s in sc]           # scores agree ...
    cand = ob.candidates(q)
    if cand is not None and not torch.equal(cand[:5], torch.arange(5)):
        assert [x[0] for x in r] != [f"m{int(i)}" for i in rows]  # ... ids are wrong upstream (pinned defect)
    # full bank always overwrites slot 0 (pinned defect, reproduced)
    ob2 = O.OracleBank(3, D, use_centroid_index=False)
    for i in range(6):
        ob2.write(f"m{i}", feats[i], NOW)
    assert torch.equal(d["full_features"], ob2.features) and d["full_id_to_idx"] == ob2.id_to_idx


def test_zone_and_addition_linear_bit_exact():
    d = pins("addition_linear")
    with torch.no_grad():
        assert torch.equal(d["out"], O.addition_linear(d["x"], d["weight_patterns"], d["bias"]))


def test_product_modules_construct_like_the_reference():
    """Same constructor arguments -> same state_dict keys, shapes and (seeded) initial values: an
    upstream checkpoint loads into the product modules unchanged."""
    from aura_snn_rag_amd.base.neuron import AdExNeuron, IzhikevichNeuron, VectorizedLIFNeuron
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    from aura_snn_rag_amd.core.language_zone.gif_neuron import BalancedGIFNeuron, GIFNeuron
    from aura_snn_rag_amd.core.language_zone.snn_ffn import HybridFFN, SNNFFN
    from aura_snn_rag_amd.core.language_zone.synapsis import Synapsis
    from aura_snn_rag_amd.maths.addition_linear import AdditionLinear
    d = pins("construction")
    cases = {
        "HippocampalFormation": lambda: HippocampalFormation(2, 30, 10, 20, 50, 16, "cpu"),
        "IzhikevichNeuron": lambda: IzhikevichNeuron(0.1, 0.26, -60, 0, 0.5),
        "AdExNeuron": lambda: AdExNeuron(a=2.0, b=60.0),
        "VectorizedLIFNeuron": lambda: VectorizedLIFNeuron(12, 0.9, 0.4),
        "GIFNeuron": lambda: GIFNeuron(6, 10, L=8),
        "BalancedGIFNeuron": lambda: BalancedGIFNeuron(6, 10, L=8),
        "Synapsis": lambda: Synapsis(9, 4),
        "SNNFFN": lambda: SNNFFN(16, 32),
        "HybridFFN": lambda: HybridFFN(16, 32),
        "AdditionLinear": lambda: AdditionLinear(7, 5, bias=True),
    }
    assert list(cases) == list(d["states"])
    for name, make_ours in cases.items():
        ref = dict(d["states"][name])
        torch.manual_seed(11); ours = make_ours().state_dict()
        assert list(ref) == list(ours), (name, list(ref), list(ours))
        for k in ref:
            assert ref[k].shape == ours[k].shape and ref[k].dtype == ours[k].dtype, k
            assert torch.equal(ref[k], ours[k]), k
    g = GIFNeuron(6, 10, L=8)
    assert (g.decay, g.threshold, g.alpha, g.L) == d["gif_scalars"]


def test_surrogate_gradients_and_prosody_bit_exact():
    """Differentiable restatements (section 8f-4) == the reference's autograd graph."""
    d = pins("surrogate_and_prosody")
    for r in d["gif"]:
        weight = r["weight"].clone().requires_grad_(True)
        x, v0, t0 = (r[k].clone().requires_grad_(True) for k in ("x", "v0", "t0"))
        os_, ov, ot = O.gif_run_grad(Fn.linear(x, weight, r["bias"]), v0, t0, r["decay"], 4, r["alpha"], r["threshold"])
        mine = torch.autograd.grad((os_ * r["ws"]).sum() + ov.sum() - ot.sum(), [x, v0, t0, weight])
        assert torch.equal(r["spikes"], os_) and all(torch.equal(a, b) for a, b in zip(r["grads"], mine))
    r = d["lif"]
    x = r["x"].clone().requires_grad_(True)
    slope = r["slope"].clone().requires_grad_(True)
    a1, b1 = O.lif_step_grad(x, torch.zeros_like(x), r["beta"], r["threshold"], slope)
    a2, b2 = O.lif_step_grad(x * 0.5, b1, r["beta"], r["threshold"], slope)
    mine = torch.autograd.grad(((a1 + a2) * r["w"]).sum() + b2.sum(), [x, slope])
    assert all(torch.equal(a, b) for a, b in zip(r["grads"], mine))
    p = d["prosody"]
    thr = p["threshold"]
    with torch.no_grad():
        for gn, (rs, rv, rt) in zip((p["gains"], None), p["forward"]):
            os_, ov, ot = O.prosody_gif_run(Fn.linear(p["x"], p["weight"], p["bias"]), torch.zeros(3, 20),
                                            torch.full((3, 20), thr), gn, p["decay"], 8, 0.02, thr, 0.4)
            assert torch.equal(rs, os_) and torch.equal(rv, ov) and torch.equal(rt, ot)
    # ... and its autograd graph: gradients w.r.t. input, gains, carried state and the linear layer
    for r in p["backward"]:
        use_gains = r["gains"] is not None
        weight = p["weight"].clone().requires_grad_(True)
        xg, v0, t0 = (r[k].clone().requires_grad_(True) for k in ("x", "v0", "t0"))
        gg = r["gains"].clone().requires_grad_(True) if use_gains else None
        wrt = [xg, v0, t0, weight] + ([gg] if use_gains else [])
        os_, ov, ot = O.prosody_gif_run_grad(Fn.linear(xg, weight, p["bias"]), v0, t0, gg, p["decay"], 8, 0.02, thr, 0.4)
        mine = torch.autograd.grad((os_ * r["ws"]).sum() + ov.sum() - ot.sum(), wrt)
        assert torch.equal(r["spikes"], os_) and all(torch.equal(a, b) for a, b in zip(r["grads"], mine))


@pytest.mark.parametrize("mode", ["cross_attention", "concat", "gate"])
def test_memory_injection_modes_match_reference_layer(mode):
    """inject_memories of the reference layer (memory_augmented_layer.py:155-203), all three modes, against
    aura_snn_rag_amd's MemoryInjection with the layer's own weights loaded: bit-equal on CPU."""
    from aura_snn_rag_amd.core.language_zone.memory_ops import MemoryInjection
    d = pins("memory_injection")[mode]
    mine = MemoryInjection(None, 32, num_heads=4, dropout=0.0, memory_injection=mode).eval()
    missing, unexpected = mine.load_state_dict(d["state"], strict=False)
    assert not missing, f"keys the reference layer does not provide: {missing}"
    with torch.no_grad():
        assert torch.equal(d["out"], mine.inject_memories(d["h"], d["mf"], d["ms"]))
