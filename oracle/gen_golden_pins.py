#!/usr/bin/env python3
"""Record what tests/test_oracle_vs_reference.py pins, FROM THE REFERENCE ITSELF, into
tests/golden/reference_pins.pt.

Run where the reference checkout is available (AURA_REFERENCE_ROOT, see oracle/_ref_loader.py):
    python oracle/gen_golden_pins.py
The fixture holds the seeded inputs, the reference modules' initial state and their outputs and
gradients -- data only, no reference source.  The tests then hold the oracle and the product
modules to it without the reference.
"""
from __future__ import annotations

import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from oracle import _ref_loader as L

OUT = os.path.join(ROOT, "tests", "golden", "reference_pins.pt")
NOW = 1.7e9 + 777.0


def _t(x):
    return x.detach().clone()


def neuron_loops():
    N = L.load("base.neuron")
    torch.manual_seed(0)
    I = 20 * torch.rand(300, 77)
    izh = N.IzhikevichNeuron(0.02, 0.2, -65, 8, 0.2)
    s = izh(I)
    d = dict(izh=dict(I=I, spikes=_t(s), v=_t(izh.v), u=_t(izh.u)))
    ad = N.AdExNeuron(a=2.0, b=60.0)
    Ia = 600 * torch.rand(32, 150)
    sa = ad(Ia)
    d["adex"] = dict(I=Ia, spikes=_t(sa), V=_t(ad.V), w=_t(ad.w))
    lif = N.VectorizedLIFNeuron(16, 0.9, 0.6)
    xs, spk, mem = [], [], []
    for _ in range(4):
        x = torch.randn(3, 16)
        rs, rm = lif(x)
        xs.append(x); spk.append(_t(rs)); mem.append(_t(rm))
    d["lif"] = dict(beta=_t(lif.beta), threshold=_t(lif.threshold), x=xs, spikes=spk, mem=mem)
    return d


def gif_and_ffn(dtype):
    G = L.load("src.core.language_zone.gif_neuron")
    F = L.load("src.core.language_zone.snn_ffn")
    torch.manual_seed(1)
    g = G.GIFNeuron(24, 40, L=8).to(dtype)
    x = (torch.randn(4, 9, 24) * 3).to(dtype)
    with torch.no_grad():
        rs, (rv, rt) = g(x)
    d = dict(x=x, weight=_t(g.linear.weight), bias=_t(g.linear.bias), decay=g.decay, spikes=rs, v=rv, theta=rt)
    bg = G.BalancedGIFNeuron(24, 40, L=8).to(dtype)
    with torch.no_grad():
        rs, _ = bg(x)
    d["balanced"] = dict(w_exc=_t(bg.linear_exc.weight), b_exc=_t(bg.linear_exc.bias), w_inh=_t(bg.linear_inh.weight),
                         b_inh=_t(bg.linear_inh.bias), decay=bg.decay, spikes=rs)
    if dtype == torch.float32:
        ffn = F.SNNFFN(32, 96, num_timesteps=4, L=8).eval()
        xx = torch.randn(2, 8, 32)
        with torch.no_grad():
            d["ffn"] = dict(state={k: _t(v) for k, v in ffn.state_dict().items()}, x=xx, out=ffn(xx))
    return d


def bank():
    H = L.load("core.hippocampal")
    H.time.time = lambda: NOW
    D, M = 16, 500
    ref = H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D, device="cpu")
    ref.centroids_k = 8
    ref.centroids_update_interval = 32
    feats = torch.randn(200, D) * torch.rand(200, 1) * 2
    torch.manual_seed(9)
    for i in range(200):
        ref.create_episodic_memory(f"m{i}", "e", feats[i])
    d = dict(now=NOW, feats=feats, features=_t(ref.memory_features), metadata=_t(ref.memory_metadata),
             centroids=_t(ref.centroids), centroid_counts=_t(ref.centroid_counts))
    q = feats[3] + 0.05 * torch.randn(D)
    loc = torch.tensor([1.0, -1.0])
    ref.use_centroid_index = False
    d.update(q=q, loc=loc, recall_exact=ref.retrieve_similar_memories(q, k=7),
             recall_exact_loc=ref.retrieve_similar_memories(q, location=loc, k=7))
    ref.use_centroid_index = True
    d["recall_index"] = ref.retrieve_similar_memories(q, k=5)
    ref2 = H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=3, feature_dim=D,
                                  device="cpu", use_centroid_index=False)
    for i in range(6):
        ref2.create_episodic_memory(f"m{i}", "e", feats[i])
    d.update(full_features=_t(ref2.memory_features), full_id_to_idx=dict(ref2.id_to_idx))
    return d


def addition_linear():
    A = L.load("src.maths.addition_linear")
    torch.manual_seed(2)
    al = A.AdditionLinear(20, 30, bias=True)
    x = torch.randn(5, 20)
    with torch.no_grad():
        return dict(weight_patterns=_t(al.weight_patterns), bias=_t(al.bias), x=x, out=al(x))


def construction():
    R = {"hip": L.load("core.hippocampal"), "neu": L.load("base.neuron"),
         "gif": L.load("src.core.language_zone.gif_neuron"), "ffn": L.load("src.core.language_zone.snn_ffn"),
         "syn": L.load("src.core.language_zone.synapsis"), "al": L.load("src.maths.addition_linear")}
    cases = {
        "HippocampalFormation": lambda: R["hip"].HippocampalFormation(2, 30, 10, 20, 50, 16, "cpu"),
        "IzhikevichNeuron": lambda: R["neu"].IzhikevichNeuron(0.1, 0.26, -60, 0, 0.5),
        "AdExNeuron": lambda: R["neu"].AdExNeuron(a=2.0, b=60.0),
        "VectorizedLIFNeuron": lambda: R["neu"].VectorizedLIFNeuron(12, 0.9, 0.4),
        "GIFNeuron": lambda: R["gif"].GIFNeuron(6, 10, L=8),
        "BalancedGIFNeuron": lambda: R["gif"].BalancedGIFNeuron(6, 10, L=8),
        "Synapsis": lambda: R["syn"].Synapsis(9, 4),
        "SNNFFN": lambda: R["ffn"].SNNFFN(16, 32),
        "HybridFFN": lambda: R["ffn"].HybridFFN(16, 32),
        "AdditionLinear": lambda: R["al"].AdditionLinear(7, 5, bias=True),
    }
    states = {}
    for name, make in cases.items():
        torch.manual_seed(11)
        states[name] = [(k, _t(v)) for k, v in make().state_dict().items()]
    r = R["gif"].GIFNeuron(6, 10, L=8)
    return dict(states=states, gif_scalars=(r.decay, r.threshold, r.alpha, r.L))


def surrogate_and_prosody():
    G = L.load("src.core.language_zone.gif_neuron")
    N = L.load("base.neuron")
    PG = L.load("src.core.language_zone.prosody_gif")
    torch.manual_seed(11)
    gif = []
    for alpha in (0.0, 0.05):
        g = G.GIFNeuron(12, 28, L=4, alpha=alpha)
        x = (torch.randn(3, 9, 12) * 4).requires_grad_(True)
        v0 = (0.5 * torch.randn(3, 28)).requires_grad_(True)
        t0 = (1 + 0.3 * torch.rand(3, 28)).requires_grad_(True)
        ws = torch.randn(3, 9, 28)
        rs, (rv, rt) = g(x, state=(v0, t0))
        grads = torch.autograd.grad((rs * ws).sum() + rv.sum() - rt.sum(), [x, v0, t0, g.linear.weight])
        gif.append(dict(alpha=alpha, weight=_t(g.linear.weight), bias=_t(g.linear.bias), decay=g.decay,
                        threshold=g.threshold, x=_t(x), v0=_t(v0), t0=_t(t0), ws=ws, spikes=_t(rs),
                        grads=[_t(a) for a in grads]))
    lif = N.VectorizedLIFNeuron(10, 0.9, 0.6, init_slope=3.0)
    x = torch.randn(2, 4, 10).requires_grad_(True)
    w = torch.randn(2, 4, 10)
    s1, m1 = lif(x)
    s2, m2 = lif(x * 0.5)
    grads = torch.autograd.grad(((s1 + s2) * w).sum() + m2.sum(), [x, lif.slope])
    lifd = dict(beta=_t(lif.beta), threshold=_t(lif.threshold), slope=_t(lif.slope), x=_t(x), w=w,
                grads=[_t(a) for a in grads])
    pg = PG.ProsodyModulatedGIF(8, 20, L=8, alpha=0.02, attention_modulation_strength=0.4)
    pro = dict(weight=_t(pg.linear.weight), bias=_t(pg.linear.bias), decay=pg.decay, threshold=pg.threshold)
    x = torch.randn(3, 7, 8) * 3
    gains = 0.5 + 2.5 * torch.rand(3, 7)
    pro.update(x=x, gains=gains, forward=[])
    with torch.no_grad():
        for gn in (gains, None):
            rs, (rv, rt) = pg(x, attention_gains=gn)
            pro["forward"].append((rs, rv, rt))
    pro["backward"] = []
    for use_gains in (True, False):
        xg = (torch.randn(3, 7, 8) * 3).requires_grad_(True)
        gg = (0.5 + 2.5 * torch.rand(3, 7)).requires_grad_(True) if use_gains else None
        v0 = (0.5 * torch.randn(3, 20)).requires_grad_(True)
        t0 = (1 + 0.3 * torch.rand(3, 20)).requires_grad_(True)
        ws = torch.randn(3, 7, 20)
        wrt = [xg, v0, t0, pg.linear.weight] + ([gg] if use_gains else [])
        rs, (rv, rt) = pg(xg, state=(v0, t0), attention_gains=gg)
        grads = torch.autograd.grad((rs * ws).sum() + rv.sum() - rt.sum(), wrt)
        pro["backward"].append(dict(x=_t(xg), gains=_t(gg) if use_gains else None, v0=_t(v0), t0=_t(t0), ws=ws,
                                    spikes=_t(rs), grads=[_t(a) for a in grads]))
    return dict(gif=gif, lif=lifd, prosody=pro)


def memory_injection(mode):
    M = L.load("src.core.language_zone.memory_augmented_layer")
    cfg = types.SimpleNamespace(embedding_dim=32, num_heads=4, dropout=0.0, intermediate_size=64)
    torch.manual_seed(0)
    layer = M.MemoryAugmentedLayer(cfg, hippocampus=None, use_snn_ffn=False, memory_injection=mode, num_retrieved=5).eval()
    h, mf, ms = torch.randn(3, 7, 32), torch.randn(3, 5, 32), torch.randn(3, 5)
    with torch.no_grad():
        out = layer.inject_memories(h, mf, ms)
    return dict(state={k: _t(v) for k, v in layer.state_dict().items()}, h=h, mf=mf, ms=ms, out=out)


def main():
    pins = dict(neuron_loops=neuron_loops(),
                gif_and_ffn={"f32": gif_and_ffn(torch.float32), "bf16": gif_and_ffn(torch.bfloat16)},
                bank=bank(), addition_linear=addition_linear(), construction=construction(),
                surrogate_and_prosody=surrogate_and_prosody(),
                memory_injection={m: memory_injection(m) for m in ("cross_attention", "concat", "gate")})
    torch.save(pins, OUT)
    print(f"{os.path.relpath(OUT, ROOT)}: {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
