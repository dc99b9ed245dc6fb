"""Measurements of the fused MoE zone (``MoELanguageZone.route_experts``: ``ops.moe_route`` + ``ops.moe_experts``)
-> profiles/moe_bench.json.

    python tools/moe_bench.py [--tokens 4096 16384] [--hidden 128 256] [--out ...]

Needs a GPU (no fallback).  One process.  Dm = 64, E = 8, k = 2, two layers, the router's hidden size 64.
  route_experts  fused, against the reference's op sequence composed from torch ops and this package's modules on the
                 same GPU: the router with its time-constant path (``LiquidMoERouter.compose``), then every expert that
                 any token selected run over ALL tokens (``SNNExpert.predict``), masked by the routing weight and added.
                 Both are first compared (tokens of equal routing, relative 1e-3 of the largest output).  Bar: the fused
                 maximum window below the composition's minimum at every point.  Without a bar: the share of the fp32
                 matrix floor ``2 P (2 Dm Hh + (2 layers - 1) Hh^2) / 157 TF`` at the median, and the launch count (five,
                 read off the code).
  forward        the whole ``MoELanguageZone.forward`` at B S = 4096 (vocabulary 8192, embed 128), fused, no bar.
Device events and alternated windows (tools/diverse_bench.py's scheme): the figure is the time per call of a stream of
back-to-back calls.  Exit status 1 when a bar is missed; the figures are written either way."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

DM, E, K, LAYERS = 64, 8, 2, 2
PEAK_FP32_MATRIX = 157.3e12
LAUNCHES_FUSED = 5


def _zone(dev, Hh, vocab=512, embed=32):
    from aura_snn_rag_amd.core.language_zone.moe_language_zone import MoELanguageZone
    torch.manual_seed(0)
    zone = MoELanguageZone(vocab_size=vocab, embed_dim=embed, hidden_dim=2 * Hh, num_experts=E, top_k=K,
                           moe_hidden_dim=DM)
    with torch.no_grad():
        zone.moe_router.gate_proj.weight.mul_(150.0)          # routing that varies between tokens
    return zone.to(dev).eval()


def dense_reference(zone, x):
    route = zone.moe_router.compose(x)
    idx, w = route['indices'], route['weights']
    out = torch.zeros(x.shape[0], DM, device=x.device)
    for i in range(E):
        chosen = idx == i
        if not chosen.any():
            continue
        y = zone.experts[f'expert_{i}'].predict(x)
        out += y * (w * chosen.float()).sum(dim=1).unsqueeze(1)
    return out, idx


def point(N, Hh, dev, out, missed):
    zone = _zone(dev, Hh)
    x = torch.randn(N, DM, generator=torch.Generator(device=dev).manual_seed(N + Hh), device=dev)
    with torch.no_grad():
        fused = lambda: zone.route_experts(x).expert_outputs
        dense = lambda: dense_reference(zone, x)[0]
        a = zone.route_experts(x)
        b, idx = dense_reference(zone, x)
        same = (a.indices.sort(dim=1).values == idx.sort(dim=1).values).all(dim=1)
        diff = (a.expert_outputs - b)[same].abs()
        # a spike that falls the other way moves a few outputs of a token: compare the median token, report the worst
        rel = float(diff.max(dim=1).values.median() / b.abs().max())
        assert rel <= 1e-3, (N, Hh, rel)
        ms, iters = alternated({"fused": fused, "dense": dense}, events_window)
    f, d = summary(ms["fused"]), summary(ms["dense"])
    P = N * K
    flops = 2.0 * P * (2 * DM * Hh + (2 * LAYERS - 1) * Hh * Hh)
    floor_ms = 1e3 * flops / PEAK_FP32_MATRIX
    met = f["max_ms"] < d["min_ms"]
    key = f"route_experts_N{N}_Hh{Hh}"
    out[key] = dict(N=N, Dm=DM, Hh=Hh, E=E, k=K, layers=LAYERS, iters=iters, fused=f, dense=d,
                    ratio_fused_over_dense=f["median_ms"] / d["median_ms"], matrix_floor_ms=floor_ms,
                    share_of_matrix_floor=floor_ms / f["median_ms"], launches_fused=LAUNCHES_FUSED,
                    share_of_tokens_with_equal_routing=float(same.float().mean()), median_token_rel_diff=rel,
                    worst_rel_diff=float(diff.max() / b.abs().max()), bar_met=bool(met))
    print(f"{key}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}], dense {d['median_ms']:.4f} ms "
          f"[{d['min_ms']:.4f}, {d['max_ms']:.4f}]; floor {floor_ms:.4f} ms ({100 * floor_ms / f['median_ms']:.1f} %)",
          flush=True)
    if not met:
        missed.append(key)


def forward_point(dev, out):
    zone = _zone(dev, 128, vocab=8192, embed=128)
    ids = torch.randint(0, 8192, (8, 512), generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        ms, iters = alternated({"forward": lambda: zone(ids, keep_on_device=True)[0]}, events_window)
    out["forward_BS4096"] = dict(B=8, S=512, vocab=8192, embed=128, hidden=256, Hh=128, iters=iters,
                                 **summary(ms["forward"]))
    print(f"forward_BS4096: {out['forward_BS4096']['median_ms']:.4f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for N in a.tokens:
        for Hh in a.hidden:
            point(N, Hh, dev, out, missed)
    forward_point(dev, out)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
