"""Measurements of the memory-augmented layer's decoding step and of ``SNNRAGTransformer.generate``
-> profiles/snn_rag_bench.json.

    python tools/snn_rag_bench.py [--batch 1 8 32] [--prompt 16 512] [--only layer|generate] [--out ...]

Needs a GPU (no fallback).  One process.
  layer     one ``MemoryAugmentedLayer.step`` with the ``gate`` injection at D = 768, H = 12, intermediate 3072, a cache
            holding a prompt of 64 positions and k = 5 pinned memories, B = 1, 8, 32: an MLP layer and a HybridFFN layer
            (T = 4), ``fused=True`` against ``fused=False``.  Both sides are first checked against each other (the MLP
            layer within a relative 1e-4; the HybridFFN layer's share of equal outputs is recorded: spikes may flip
            between two summation orders).  Device events, windows alternated in one process (tools/diverse_bench.py's
            scheme): the figure is the time per step of a stream of back-to-back steps at one position (the step does
            not advance the cache), host launch cost included where the host is the slower side.
  generate  ``SNNRAGTransformer.generate`` with the default SNN layers and a 64-row bank, the recorded configuration of
            tools/generate_bench.py (D 256, H 4, 4 layers, V 32 000, 48 sampled tokens, prompts of 16 and 512, B = 1, 8,
            32): ``fused_step=True``, ``False`` and the loop that recomputes ``forward(context, memory=pinned)`` for every
            token (greedy, one run).  Host clock around a device synchronisation, median of three runs after a warm-up,
            fused and unfused alternated.
The launch counts are counted from the code, not measured.  Bars: the fused median below the unfused minimum at every
point.  Exit status 1 when a bar is missed; the figures are written either way."""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

D, H, FF, K_MEM, PROMPT = 768, 12, 3072, 5, 64
# launches of one layer step, read off the code.  Unfused: attention_norm, q, k, v, decode x 2, o_proj, add; the gate
# injection (softmax, multiply, sum, memory_proj, cat, linear, sigmoid, multiply, add); ffn_norm and the FFN.
ATTENTION_UNFUSED, GATE_UNFUSED = 8, 9
MLP_UNFUSED = 5                     # ffn_norm, ffn.0, GELU, ffn.2, add
# ffn_norm; mlp.0, GELU, mlp.2; syn1, neuron1.linear, state x 2, GIF, syn2, neuron2.linear, state x 2, GIF; sigmoid,
# 1 - g, two products, their sum; the residual add
HYBRID_UNFUSED = 1 + 3 + 10 + 5 + 1
LAYER_FUSED = {"mlp": 7, "snn": 11}
LAYER_UNFUSED = {"mlp": ATTENTION_UNFUSED + GATE_UNFUSED + MLP_UNFUSED,
                 "snn": ATTENTION_UNFUSED + GATE_UNFUSED + HYBRID_UNFUSED}


def _bank(dim, dev):
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    hf = HippocampalFormation(feature_dim=dim, max_memories=128, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                              device="cuda", use_centroid_index=False)
    hf.create_episodic_memories([f"m{i}" for i in range(64)],
                                torch.randn(64, dim, generator=torch.Generator().manual_seed(dim)))
    return hf


def layer_part(batches, dev, out, missed):
    from aura_snn_rag_amd import MemoryAugmentedLayer
    cfg = types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=FF)
    bank = _bank(D, dev)
    for kind in ("mlp", "snn"):
        torch.manual_seed(1)
        layer = MemoryAugmentedLayer(cfg, bank, use_snn_ffn=kind == "snn", memory_injection="gate",
                                     num_retrieved=K_MEM).to(dev).eval()
        for B in batches:
            gen = torch.Generator(device=dev).manual_seed(B)
            hidden = torch.randn(B, PROMPT + 1, D, generator=gen, device=dev)
            row = hidden[:, PROMPT].contiguous()
            with torch.no_grad():
                cache = layer.new_cache(B, PROMPT + 8)
                layer.prefill(hidden[:, :PROMPT], cache=cache)

            def step(fused):
                cache.attention.max_length = PROMPT                     # the same position again: nothing advances
                return layer.step(row, cache=cache, advance=False, fused=fused)

            a, b = step(True), step(False)
            diff = float((a - b).abs().max() / b.abs().max())
            equal = float(((a - b).abs() <= 1e-4 * b.abs().max()).float().mean())
            if kind == "mlp":
                assert diff <= 1e-4, (kind, B, diff)
            ms, iters = alternated({"fused": lambda: step(True), "unfused": lambda: step(False)}, events_window)
            f, u = summary(ms["fused"]), summary(ms["unfused"])
            met = f["median_ms"] < u["min_ms"]
            key = f"layer_{kind}_B{B}"
            out[key] = dict(B=B, D=D, H=H, intermediate=FF, prompt=PROMPT, k=K_MEM, fused=f, unfused=u, iters=iters,
                            launches_fused=LAYER_FUSED[kind], launches_unfused=LAYER_UNFUSED[kind],
                            ratio_fused_over_unfused=f["median_ms"] / u["median_ms"], max_rel_diff=diff,
                            share_of_outputs_within_1e_4=equal, bar_met=bool(met))
            print(f"{key}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}] "
                  f"({LAYER_FUSED[kind]} launches), unfused {u['median_ms']:.4f} ms [{u['min_ms']:.4f}, "
                  f"{u['max_ms']:.4f}] ({LAYER_UNFUSED[kind]} launches); max relative difference {diff:.2e}", flush=True)
            if not met:
                missed.append(key)


def generate_point(B, S, dev, bank, out, missed):
    from aura_snn_rag_amd import SNNRAGTransformer
    V, N, LAYERS = 32000, 48, 4
    cfg = types.SimpleNamespace(vocab_size=V, embedding_dim=256, num_heads=4, num_layers=LAYERS, intermediate_size=1024,
                                n_place_cells=2000, max_seq_len=1024, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    torch.manual_seed(0)
    m = SNNRAGTransformer(cfg, bank).to(dev).eval()
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(1)).to(dev)
    run = lambda fused: m.generate(ids, max_new_tokens=N, use_memory=True, temperature=0.8, top_k=50, top_p=0.9,
                                   seed=5, fused_step=fused)
    agree = float((run(True) == run(False)).float().mean())             # the warm-up of both
    times = {True: [], False: []}
    for rnd in range(3):
        for fused in ((True, False) if rnd % 2 == 0 else (False, True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fused)
            torch.cuda.synchronize()
            times[fused].append(1e3 * (time.perf_counter() - t0) / N)
    # the loop a user would write without the caches: forward over the growing context with the pinned memories
    with torch.no_grad():
        state = m.new_state(B, S + 1)
        m.prefill(ids, state=state)
        pinned = m.pinned_memory(state)
        ctx = ids
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            ctx = torch.cat([ctx, m(ctx, memory=pinned)[0][:, -1].argmax(-1, keepdim=True)], dim=1)
        torch.cuda.synchronize()
        recompute = 1e3 * (time.perf_counter() - t0) / N
    snn = sum(int(l.use_snn_ffn) for l in m.layers)
    res = {}
    for fused, name in ((True, "fused"), (False, "unfused")):
        ts = sorted(times[fused])
        per_layer = LAYER_FUSED if fused else LAYER_UNFUSED
        res[name] = dict(median_ms_per_token=ts[1], min_ms_per_token=ts[0], max_ms_per_token=ts[-1],
                         layer_launches_per_token=snn * per_layer["snn"] + (LAYERS - snn) * per_layer["mlp"])
    met = res["fused"]["median_ms_per_token"] < res["unfused"]["min_ms_per_token"]
    key = f"generate_B{B}_S{S}"
    out[key] = dict(B=B, V=V, prompt=S, new_tokens=N, layers=LAYERS, snn_layers=snn, D=256,
                    share_of_equal_tokens=agree, recompute_ms_per_token=recompute,
                    ratio_fused_over_unfused=res["fused"]["median_ms_per_token"] / res["unfused"]["median_ms_per_token"],
                    bar_met=bool(met), **res)
    print(f"{key}: fused {res['fused']['median_ms_per_token']:.3f} ms/token, unfused "
          f"{res['unfused']['median_ms_per_token']:.3f} ms/token [min {res['unfused']['min_ms_per_token']:.3f}], pinned "
          f"recompute loop {recompute:.3f} ms/token; {agree:.3f} of the tokens equal", flush=True)
    if not met:
        missed.append(key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prompt", type=int, nargs="+", default=[16, 512])
    ap.add_argument("--only", choices=["layer", "generate"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snn_rag_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("snn_rag_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    if a.only != "generate":
        layer_part(a.batch, dev, out, missed)
    if a.only != "layer":
        bank = _bank(256, dev)
        for B in a.batch:
            for S in a.prompt:
                generate_point(B, S, dev, bank, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
