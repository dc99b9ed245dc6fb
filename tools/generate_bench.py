"""Measurements of the fused sampler and of cached generation -> profiles/generate_bench.json.

    python tools/generate_bench.py [--batch 1 8 32] [--vocab 32000 50257] [--prompt 16 512] [--out ...]

Needs a GPU (no fallback).  One process.
  sampler   ``ops.sample_next`` (one launch; penalty 1.2 over a 5 % mask, temperature 0.8, top_k 50, top_p 0.9, the row
            state on the device) next to the composition to beat: the same decision from torch ops on the same GPU --
            the penalty by a masked division, ``topk``, ``sort``, ``softmax``, ``cumsum``, ``scatter``, ``softmax``,
            ``multinomial``, the write of the token column and of the mask.  The composition keeps no finished flags
            and makes no host sync, which favours it.  The two sides draw from different random streams, so they are
            not compared token by token; the kept sets are (equal on every row, outside near-ties at the boundary).
  generate  ``HippocampalTransformer.generate`` (D 256, H 4, 4 layers, V 32000, prompts of 16 and 512 tokens, 48 new
            tokens) next to the loop that recomputes ``forward`` over the growing context and samples with the same
            op: what generation costs per token with and without the caches.  At the short prompt both sides are
            bound by the host's launches, not by the device.
Every sampler figure is the median over the windows of tools/diverse_bench.py's scheme (device events, warm-up, the
candidates alternated inside each round); the generate figures are the median of five whole runs by the host clock
around a device synchronisation, after one warm-up run each.
Bar: the fused sampler's median below the composition's, outside both spreads, at every point.  Exit status 1 when a
bar is missed; the figures are written either way."""
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

PENALTY, T, K, P = 1.2, 0.8, 50, 0.9


def torch_sampler(logits, seen, column):
    """The reference loop's tail from torch ops, without its Python double loop: one token per row into ``column``."""
    z = torch.where(seen.bool(), logits / PENALTY, logits) / T
    kth = torch.topk(z, K, dim=-1).values[..., -1:]
    z = z.masked_fill(z < kth, float("-inf"))
    sorted_z, order = torch.sort(z, dim=-1, descending=True)
    drop = torch.cumsum(torch.softmax(sorted_z, dim=-1), dim=-1) > P
    drop = torch.cat([torch.zeros_like(drop[..., :1]), drop[..., :-1]], dim=-1)
    z = z.masked_fill(torch.zeros_like(drop).scatter(-1, order, drop), float("-inf"))
    tok = torch.multinomial(torch.softmax(z, dim=-1), 1)
    column.copy_(tok[:, 0])
    seen.scatter_(1, tok, 1)
    return z


def sampler_point(B, V, dev, out, missed):
    from aura_snn_rag_amd import ops
    gen = torch.Generator(device=dev).manual_seed(11)
    logits = 4 * torch.randn(B, V, generator=gen, device=dev)
    seen0 = (torch.rand(B, V, generator=gen, device=dev) < 0.05).to(torch.uint8)
    buf = torch.zeros(B, 8, dtype=torch.int64, device=dev)
    state = dict(step=0)
    seen_f, seen_t, fin = seen0.clone(), seen0.clone(), torch.zeros(B, dtype=torch.uint8, device=dev)

    def fused():
        state["step"] += 1
        return ops.sample_next(logits, seen=seen_f, finished=fin, penalty=PENALTY, temperature=T, top_k=K, top_p=P,
                               seed=3, step=state["step"], out=buf[:, 3])

    comp = lambda: torch_sampler(logits, seen_t, buf[:, 4])
    _, c = ops.sample_next(logits, seen=seen0.clone(), penalty=PENALTY, temperature=T, top_k=K, top_p=P,
                           return_candidates=True)
    kept = torch.zeros(B, V, dtype=torch.bool, device=dev).scatter_(1, c["ids"].long(), c["d"] > float("-inf"))
    rows_equal = int((kept == torch.isfinite(torch_sampler(logits, seen0.clone(), buf[:, 4]))).all(dim=1).sum())
    ms, iters = alternated({"fused": fused, "torch": comp}, events_window)
    f, t = summary(ms["fused"]), summary(ms["torch"])
    met = f["max_ms"] < t["min_ms"]
    name = f"sampler_B{B}_V{V}"
    out[name] = dict(B=B, V=V, fused=f, torch=t, iters=iters, ratio_fused_over_torch=f["median_ms"] / t["median_ms"],
                     row_bytes=4 * V, kept_sets_equal_rows=rows_equal, bar_met=bool(met))
    print(f"{name}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}], torch {t['median_ms']:.4f} ms "
          f"[{t['min_ms']:.4f}, {t['max_ms']:.4f}]; kept sets equal on {rows_equal} of {B} rows", flush=True)
    if not met:
        missed.append(name)


def generate_point(B, S, dev, out):
    from aura_snn_rag_amd import HippocampalTransformer, ops
    V, N = 32000, 48
    cfg = types.SimpleNamespace(vocab_size=V, embedding_dim=256, num_heads=4, num_layers=4, intermediate_size=1024,
                                n_place_cells=2000, max_seq_len=1024, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    torch.manual_seed(0)
    m = HippocampalTransformer(cfg, None).to(dev).eval()
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(temperature=T, top_k=K, top_p=P, seed=5)

    def cached():
        return m.generate(ids, max_new_tokens=N, use_memory=False, **kw)

    def recompute():
        ctx = ids
        seen = torch.zeros(B, V, dtype=torch.uint8, device=dev).scatter_(1, ids, 1)
        with torch.no_grad():
            for t in range(N):
                lg = m(ctx, use_memory=False)[0][:, -1]
                tok = ops.sample_next(lg, seen=seen, penalty=PENALTY, temperature=T, top_k=K, top_p=P, seed=5, step=t)
                ctx = torch.cat([ctx, tok[:, None]], dim=1)
        return ctx

    agree = float((cached() == recompute()).float().mean())
    res = {}
    for name, fn in (("cached", cached), ("recompute", recompute)):
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0) / N)
        times.sort()
        res[name] = dict(median_ms_per_token=times[2], min_ms_per_token=times[0], max_ms_per_token=times[-1])
    out[f"generate_B{B}_S{S}"] = dict(B=B, V=V, prompt=S, new_tokens=N, layers=4, D=256, share_of_equal_tokens=agree,
                                 recompute_over_cached=res["recompute"]["median_ms_per_token"]
                                 / res["cached"]["median_ms_per_token"], **res)
    print(f"generate B={B} prompt {S}: cached {res['cached']['median_ms_per_token']:.3f} ms/token, recompute "
          f"{res['recompute']['median_ms_per_token']:.3f} ms/token; {agree:.3f} of the tokens equal", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--vocab", type=int, nargs="+", default=[32000, 50257])
    ap.add_argument("--prompt", type=int, nargs="+", default=[16, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for B in a.batch:
        for V in a.vocab:
            sampler_point(B, V, dev, out, missed)
    for B in a.batch:
        for S in a.prompt:
            generate_point(B, S, dev, out)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
