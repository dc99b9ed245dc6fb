"""Measurements of the seeded Poisson bridge (``ops.poisson_rate``) and of ``MoELanguageZone``'s stepped decoding
-> profiles/zone_decode_bench.json.

    python tools/zone_decode_bench.py [--only bridge generate] [--out ...]

Needs a GPU (no fallback).  One process.
  poisson_rate  K = 64, H = 512, T = 10 at N = 4096 and 16 384, against the bridge's own torch op sequence on the same
                GPU (``F.linear``, ``sigmoid``, ``torch.rand``, compare, cast, ``mean``).  Bar: the fused call's slowest
                window below the composition's fastest.  Without a bar: the share of the byte floor ``(N K + N H) 4 B``
                at 8 TB/s and of the generator's instruction floor (96 vector instructions per output
                element and word group, ``ceil(T / 4)`` groups, every one at full rate on 256 CUs x 64 lanes, 2.4 GHz)
                at the median.
  generate      embed 256, hidden 512, V = 32 000, 8 experts, 48 sampled tokens after prompts of 16 and 512, B = 1, 8,
                32: ms per token through ``step`` (``ops.sample_next`` + ``step`` from a prefilled state) next to the loop
                that recomputes the seeded ``forward`` over the growing context.  Bar: at the 512-token prompt the
                stepped median below the recompute minimum at every B.  At a prompt of 16 both are launch-bound: no bar.
Device events and alternated windows (tools/diverse_bench.py's scheme).  Exit status 1 when a bar is missed; the
figures are written either way."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import WINDOWS, alternated, events_window, summary  # noqa: E402

K, H, T = 64, 512, 10
PEAK_HBM = 8.0e12
LANES_PER_CLOCK, CLOCK = 256 * 4 * 16, 2.4e9
GENERATOR_VALU = 96                     # per output element and group of four timesteps, counted from the compiled ISA
NEW, SAMPLING = 48, dict(temperature=0.8, top_k=50, top_p=0.9, penalty=1.2)


def bridge_point(N, dev, out, missed):
    g = torch.Generator(device=dev).manual_seed(N)
    x = torch.randn(N, K, generator=g, device=dev)
    lin = torch.nn.Linear(K, H).to(dev)
    W, b = lin.weight.detach(), lin.bias.detach()
    from aura_snn_rag_amd import ops

    def composed():
        feat = F.linear(x, W, b)
        draw = torch.rand(N, T, H, device=dev, dtype=x.dtype)
        return (draw < torch.sigmoid(feat).unsqueeze(1)).to(x.dtype).mean(dim=1)

    fused = lambda: ops.poisson_rate(x, W, b, T=T, seed=1)
    with torch.no_grad():
        a, c = fused(), composed()
        assert abs(float(a.mean()) - float(c.mean())) < 5e-3, "the two draws do not have the same mean rate"
        ms, iters = alternated({"fused": fused, "composed": composed}, events_window)
    f, d = summary(ms["fused"]), summary(ms["composed"])
    byte_floor = 1e3 * (N * K + N * H) * 4 / PEAK_HBM
    inst_floor = 1e3 * GENERATOR_VALU * ((T + 3) // 4) * N * H / LANES_PER_CLOCK / CLOCK
    met = f["max_ms"] < d["min_ms"]
    key = f"poisson_rate_N{N}"
    out[key] = dict(N=N, K=K, H=H, T=T, iters=iters, fused=f, composed=d,
                    ratio_fused_over_composed=f["median_ms"] / d["median_ms"], byte_floor_ms=byte_floor,
                    share_of_byte_floor=byte_floor / f["median_ms"], generator_floor_ms=inst_floor,
                    share_of_generator_floor=inst_floor / f["median_ms"], bar_met=bool(met))
    print(f"{key}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}], composed {d['median_ms']:.4f} ms "
          f"[{d['min_ms']:.4f}, {d['max_ms']:.4f}]; byte floor {byte_floor:.4f} ms, generator floor {inst_floor:.4f} ms",
          flush=True)
    if not met:
        missed.append(key)


def generate_point(zone, B, S, dev, out, missed):
    from aura_snn_rag_amd import ops
    V = zone.vocab_size
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(S + B)).to(dev)
    seed = 5
    state = zone.new_state(B, seed=seed)
    logits0 = zone.prefill(ids, state)[:, -1].contiguous()
    tok = torch.empty(B, dtype=torch.int64, device=dev)

    def stepped():
        """NEW tokens from the held state: the positions simply continue from window to window."""
        logits = logits0
        for t in range(NEW):
            ops.sample_next(logits, seen=state.seen, seed=seed, step=t, out=tok, **SAMPLING)
            logits = zone.step(tok, state)

    def recompute():
        ctx = ids
        seen = torch.zeros(B, V, dtype=torch.uint8, device=dev).scatter_(1, ids, 1)
        for t in range(NEW):
            logits, _ = zone(ctx, seed=seed, keep_on_device=True)
            ops.sample_next(logits[:, -1], seen=seen, seed=seed, step=t, out=tok, **SAMPLING)
            ctx = torch.cat([ctx, tok[:, None]], dim=1)

    with torch.no_grad():
        ms = {"stepped": [], "recompute": []}
        fns = {"stepped": stepped, "recompute": recompute}
        for fn in fns.values():
            fn()
        names = list(fns)
        for rnd in range(WINDOWS):
            for name in (names if rnd % 2 == 0 else names[::-1]):
                ms[name].append(events_window(fns[name], 1) / NEW)
    s, r = summary(ms["stepped"]), summary(ms["recompute"])
    barred = S >= 512
    met = s["median_ms"] < r["min_ms"]
    key = f"generate_B{B}_S{S}"
    out[key] = dict(B=B, prompt=S, new_tokens=NEW, ms_per_token_stepped=s, ms_per_token_recompute=r,
                    ratio_stepped_over_recompute=s["median_ms"] / r["median_ms"], has_bar=barred,
                    bar_met=bool(met) if barred else None)
    print(f"{key}: stepped {s['median_ms']:.4f} ms/token [{s['min_ms']:.4f}, {s['max_ms']:.4f}], recompute "
          f"{r['median_ms']:.4f} ms/token [{r['min_ms']:.4f}, {r['max_ms']:.4f}]", flush=True)
    if barred and not met:
        missed.append(key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", choices=("bridge", "generate"), default=["bridge", "generate"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zone_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zone_decode_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    if "bridge" in a.only:
        for N in (4096, 16384):
            bridge_point(N, dev, out, missed)
    if "generate" in a.only:
        from aura_snn_rag_amd import MoELanguageZone
        torch.manual_seed(0)
        zone = MoELanguageZone(vocab_size=32000, embed_dim=256, hidden_dim=512, num_experts=8, top_k=2)
        with torch.no_grad():
            zone.moe_router.gate_proj.weight.mul_(150.0)
        zone = zone.to(dev).eval()
        for S in (16, 512):
            for B in (1, 8, 32):
                generate_point(zone, B, S, dev, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["launches_per_step"] = 14
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
