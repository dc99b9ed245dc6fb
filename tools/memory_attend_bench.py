"""Measurements of the fused ``cross_attention`` injection (``ops.memory_attend`` over the tables of
``MemoryAugmentedLayer.fold_memory``) -> profiles/memory_attend_bench.json.

    python tools/memory_attend_bench.py [--batch 1 8 32] [--prompt 16 512] [--only op|layer|generate] [--out ...]

Needs a GPU (no fallback).  One process.  D = 768, H = 12, B = 1, 8, 32.
  op        the injection alone, k = 5 pinned memories: ``ops.memory_attend`` against (1) the unfused step's own
            composition (``memory_norm``, ``nn.MultiheadAttention`` over the memories, add) and (2) the unfolded fused
            alternative from existing pieces (``ops.row_linear`` with the LayerNorm prologue for Q, SDPA over K and V
            projected once, ``ops.row_linear`` with the residual for ``out_proj``).  All three are first checked against
            each other (relative 1e-4).  Bar: the fused maximum below each comparator's minimum at every point.  The
            same at k = 32 without a bar: where the fold stops paying.  The bytes a call must read (the two tables, the
            row, gamma, beta, bias) over the median give the achieved bandwidth of the launch stream.
  layer     one ``MemoryAugmentedLayer.step`` of a ``cross_attention`` MLP layer (intermediate 3072, a cache holding a
            prompt of 64 positions, k = 5), ``fused=True`` against ``fused=False``; next to it ``fold_memory``'s one-off
            cost for that layer and batch and the number of tokens after which it is repaid.
  generate  ``SNNRAGTransformer(memory_injection="cross_attention", snn_layers=[])`` in the recorded configuration of
            tools/generate_bench.py (D 256, H 4, 4 layers, V 32 000, 48 sampled tokens, prompts of 16 and 512):
            ``fused_step=True`` (the fold included) against ``False``.  Host clock around a device synchronisation, median
            of three runs after a warm-up, alternated.
Device events and alternated windows for op and layer (tools/diverse_bench.py's scheme): the figure is the time per call
of a stream of back-to-back calls, host launch cost included where the host is the slower side.  Bars for layer and
generate: the fused median below the unfused minimum.  Exit status 1 when a bar is missed; the figures are written
either way."""
import argparse
import json
import os
import sys
import time
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402
from tools.snn_rag_bench import _bank  # noqa: E402

D, H, FF, PROMPT = 768, 12, 3072, 64
# launches of one MLP layer step, read off the code.  Unfused: the attention's eight; memory_norm, the attention's packed
# projections of q and of the memories, the scaled product, softmax, the weighted sum, out_proj and the add (about ten,
# torch's own choice of kernels: not measured); ffn_norm and the FFN's five.
LAUNCHES_FUSED = 7


def _layer(dev, k, bank=None):
    from aura_snn_rag_amd import MemoryAugmentedLayer
    cfg = types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=FF)
    torch.manual_seed(1)
    return MemoryAugmentedLayer(cfg, bank if bank is not None else object(), use_snn_ffn=False,
                                memory_injection="cross_attention", num_retrieved=k).to(dev).eval()


def op_part(batches, dev, out, missed):
    from aura_snn_rag_amd import MemoryContext, ops
    from aura_snn_rag_amd.core.language_zone.memory_ops import inject_cross_attention
    for k, barred in ((5, True), (32, False)):
        layer = _layer(dev, k)
        mn, att = layer.memory_norm, layer.memory_attention
        Wq, Wk, Wv = att.in_proj_weight[:D], att.in_proj_weight[D:2 * D], att.in_proj_weight[2 * D:]
        bq, bk, bv = att.in_proj_bias[:D], att.in_proj_bias[D:2 * D], att.in_proj_bias[2 * D:]
        for B in batches:
            gen = torch.Generator(device=dev).manual_seed(100 * k + B)
            feats = torch.randn(B, k, D, generator=gen, device=dev)
            h = torch.randn(B, D, generator=gen, device=dev)
            with torch.no_grad():
                cache = layer.new_cache(B, 4)
                layer._pin(cache, MemoryContext(feats, torch.zeros(B, k, device=dev), None))
                fold = layer.fold_memory(cache)
                keys = F.linear(feats, Wk, bk).view(B, k, H, D // H).transpose(1, 2).contiguous()
                values = F.linear(feats, Wv, bv).view(B, k, H, D // H).transpose(1, 2).contiguous()
                y = torch.empty(B, D, device=dev)

                def fused():
                    return ops.memory_attend(h, (mn.weight, mn.bias), fold.G, fold.s0, fold.U, att.out_proj.bias,
                                             eps=mn.eps, out=y)

                def unfused():
                    return inject_cross_attention(h[:, None], feats, mn, att, layer.dropout)[:, 0]

                def unfolded():
                    q = ops.row_linear(h, Wq, bq, norm=(mn.weight, mn.bias), eps=mn.eps)
                    o = F.scaled_dot_product_attention(q.view(B, H, 1, D // H), keys, values)
                    return ops.row_linear(o.reshape(B, D), att.out_proj.weight, att.out_proj.bias, residual=h)

                a, b, c = fused().clone(), unfused(), unfolded()
                scale = float(b.abs().max())
                diffs = (float((a - b).abs().max()) / scale, float((c - b).abs().max()) / scale)
                assert max(diffs) <= 1e-4, (k, B, diffs)
                ms, iters = alternated({"fused": fused, "unfused": unfused, "unfolded": unfolded}, events_window)
            s = {n: summary(v) for n, v in ms.items()}
            met = s["fused"]["max_ms"] < min(s["unfused"]["min_ms"], s["unfolded"]["min_ms"])
            nbytes = 4 * (2 * B * H * k * D + B * H * k + 2 * B * D + 3 * D)
            key = f"op_k{k}_B{B}"
            out[key] = dict(B=B, D=D, H=H, k=k, iters=iters, table_bytes=4 * 2 * B * H * k * D, bytes_per_call=nbytes,
                            fused_GBps_at_median=nbytes / (s["fused"]["median_ms"] * 1e6),
                            ratio_fused_over_unfused=s["fused"]["median_ms"] / s["unfused"]["median_ms"],
                            ratio_fused_over_unfolded=s["fused"]["median_ms"] / s["unfolded"]["median_ms"],
                            max_rel_diff_fused=diffs[0], max_rel_diff_unfolded=diffs[1],
                            bar=bool(barred), bar_met=bool(met), **s)
            print(f"{key}: " + ", ".join(f"{n} {v['median_ms']:.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]"
                                         for n, v in s.items()) +
                  f"; tables {4 * 2 * B * H * k * D / 1e6:.2f} MB; fused against unfused {diffs[0]:.2e}", flush=True)
            if barred and not met:
                missed.append(key)


def layer_part(batches, dev, out, missed):
    bank = _bank(D, dev)
    layer = _layer(dev, 5, bank)
    for B in batches:
        gen = torch.Generator(device=dev).manual_seed(B)
        hidden = torch.randn(B, PROMPT + 1, D, generator=gen, device=dev)
        row = hidden[:, PROMPT].contiguous()
        with torch.no_grad():
            cache = layer.new_cache(B, PROMPT + 8)
            layer.prefill(hidden[:, :PROMPT], cache=cache)
            layer.fold_memory(cache)

            def step(fused):
                cache.attention.max_length = PROMPT                     # the same position again: nothing advances
                return layer.step(row, cache=cache, advance=False, fused=fused)

            def fold():
                cache.fold = None
                return layer.fold_memory(cache)

            a, b = step(True), step(False)
            diff = float((a - b).abs().max() / b.abs().max())
            assert diff <= 1e-4, (B, diff)
            ms, iters = alternated({"fused": lambda: step(True), "unfused": lambda: step(False), "fold": fold},
                                   events_window)
        f, u, fo = summary(ms["fused"]), summary(ms["unfused"]), summary(ms["fold"])
        met = f["median_ms"] < u["min_ms"]
        saving = u["median_ms"] - f["median_ms"]
        key = f"layer_mlp_B{B}"
        out[key] = dict(B=B, D=D, H=H, intermediate=FF, prompt=PROMPT, k=5, fused=f, unfused=u, fold=fo, iters=iters,
                        launches_fused=LAUNCHES_FUSED, ratio_fused_over_unfused=f["median_ms"] / u["median_ms"],
                        saving_ms_per_token=saving,
                        tokens_to_repay_the_fold=(fo["median_ms"] / saving if saving > 0 else None),
                        max_rel_diff=diff, bar_met=bool(met))
        print(f"{key}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}], unfused "
              f"{u['median_ms']:.4f} ms [{u['min_ms']:.4f}, {u['max_ms']:.4f}], fold_memory {fo['median_ms']:.4f} ms once; "
              f"max relative difference {diff:.2e}", flush=True)
        if not met:
            missed.append(key)


def generate_point(B, S, dev, bank, out, missed):
    from aura_snn_rag_amd import SNNRAGTransformer
    V, N, LAYERS = 32000, 48, 4
    cfg = types.SimpleNamespace(vocab_size=V, embedding_dim=256, num_heads=4, num_layers=LAYERS, intermediate_size=1024,
                                n_place_cells=2000, max_seq_len=1024, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    torch.manual_seed(0)
    m = SNNRAGTransformer(cfg, bank, snn_layers=[], memory_injection="cross_attention").to(dev).eval()
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
    res = {}
    for fused, name in ((True, "fused"), (False, "unfused")):
        ts = sorted(times[fused])
        res[name] = dict(median_ms_per_token=ts[1], min_ms_per_token=ts[0], max_ms_per_token=ts[-1])
    met = res["fused"]["median_ms_per_token"] < res["unfused"]["min_ms_per_token"]
    key = f"generate_B{B}_S{S}"
    out[key] = dict(B=B, V=V, prompt=S, new_tokens=N, layers=LAYERS, D=256, share_of_equal_tokens=agree,
                    ratio_fused_over_unfused=res["fused"]["median_ms_per_token"] / res["unfused"]["median_ms_per_token"],
                    bar_met=bool(met), **res)
    print(f"{key}: fused {res['fused']['median_ms_per_token']:.3f} ms/token, unfused "
          f"{res['unfused']['median_ms_per_token']:.3f} ms/token [min {res['unfused']['min_ms_per_token']:.3f}]; "
          f"{agree:.3f} of the tokens equal", flush=True)
    if not met:
        missed.append(key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prompt", type=int, nargs="+", default=[16, 512])
    ap.add_argument("--only", choices=["op", "layer", "generate"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memory_attend_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("memory_attend_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    if a.only in (None, "op"):
        op_part(a.batch, dev, out, missed)
    if a.only in (None, "layer"):
        layer_part(a.batch, dev, out, missed)
    if a.only in (None, "generate"):
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
