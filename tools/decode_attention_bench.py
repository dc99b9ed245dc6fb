"""Measurements of the cached decoding step -> profiles/decode_attention_bench.json.

    python tools/decode_attention_bench.py [--batch 1 8 32] [--length 128 512 2048] [--out ...]

Needs a GPU (no fallback).  One process.  D = 768, H = 12 (dh = 64); every row of a batch has the same length L, the
cache holds L + 1 positions after the step.
  step      ``ops.attn_decode_step`` (two launches) next to the composition to beat: the same step from torch ops on the
            same GPU -- the query modulation, an ``index_copy_`` of the new key and value into a preallocated cache and
            the library attention over the ``[.., :L + 1]`` slice.  The fused call runs with ``advance=False`` so that
            every call of a window does the same work; both sides rewrite position L with the same bits.
  recompute one row of the module-level ``step`` (three projections, the op, ``o_proj``) next to the module's ``forward``
            over the whole context of L + 1 positions: what a ``generate()`` that keeps no cache pays per token.
Both sides are first checked against each other (ctx within a relative 1e-4 of the largest entry).
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), device
events, after a warm-up of every candidate, the candidates taken in alternating order inside each round
(tools/diverse_bench.py's scheme).
Floor: the step must read K and V once, ``2 B H (L + 1) dh 4`` bytes, at 6.3 TB/s.  The caches are not rotated: a point
whose K/V fit the 256 MiB Infinity Cache (marked ``cache_resident``) is served from it on both sides and its share of the
HBM floor can exceed what HBM would allow; a point whose floor time is below ``LAUNCH_BOUND_US`` per launch is marked
``launch_bound``: its time is its two launches, not its bytes.
Bar: the fused median below the composition's median, outside both spreads (fused max < composition min), at every
point.  Exit status 1 when a bar is missed; the figures are written either way."""
import argparse
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
INFINITY_CACHE_BYTES = 256 << 20
LAUNCH_BOUND_US = 5.0                                   # a launch's own cost; two of them per step
D, H = 768, 12


def torch_step(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, Kc, Vc, at, L):
    """The step from torch ops: modulation, index_copy_ into the cache, the library attention over the slice."""
    B = q.shape[0]
    dh = D // H
    qh = q.view(B, H, 1, dh)
    gain = torch.sigmoid(prosody @ Wp.T + bp)
    qh = qh * (1.0 + gain)[:, :, None, None] * (1.0 + 0.2 * torch.tanh(prosody[:, 0]))[:, None, None, None] \
        * (1.0 + 0.05 * torch.tanh(prosody[:, 1]))[:, None, None, None]
    qh = qh * (1.0 + 0.5 * torch.sigmoid(x @ wm.T + bm))[:, :, None, None]
    Kc.index_copy_(2, at, k_new.view(B, H, 1, dh))
    Vc.index_copy_(2, at, v_new.view(B, H, 1, dh))
    ctx = F.scaled_dot_product_attention(qh, Kc[:, :, :L + 1], Vc[:, :, :L + 1])
    return ctx.transpose(1, 2).reshape(B, D)


def one(B, L, dev, out, missed):
    from aura_snn_rag_amd import ops
    dh, cap = D // H, L + 1
    gen = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)
    q, k_new, v_new, x, prosody = rnd(B, D), rnd(B, D), rnd(B, D), rnd(B, D), rnd(B, 4)
    Wp, bp, wm, bm = rnd(H, 4), rnd(H), rnd(1, D) / D ** 0.5, rnd(1)
    Kc, Vc = rnd(B, H, cap, dh), rnd(B, H, cap, dh)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    at = torch.tensor([L], device=dev)
    nc = ops.attn_decode_chunks(cap)
    ws = torch.empty(ops.attn_decode_workspace_floats(B, H, dh, nc), device=dev)

    fused = lambda: ops.attn_decode_step(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, Kc, Vc, ws, n_chunks=nc,
                                         advance=False)
    comp = lambda: torch_step(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, Kc, Vc, at, L)
    a, b = fused(), comp()
    diff = float((a - b).abs().max() / b.abs().max())
    assert diff <= 1e-4, diff
    assert int(lengths[0]) == L

    ms, iters = alternated({"fused": fused, "torch": comp}, events_window)
    f, t = summary(ms["fused"]), summary(ms["torch"])
    floor = 2 * B * H * (L + 1) * dh * 4
    floor_ms = 1e3 * floor / HBM_BYTES_PER_S
    met = f["max_ms"] < t["min_ms"]
    name = f"B{B}_L{L}"
    out[name] = dict(B=B, L=L, D=D, H=H, fused=f, torch=t, iters=iters, ratio_fused_over_torch=f["median_ms"] / t["median_ms"],
                     floor_bytes=floor, floor_ms=floor_ms, share_of_hbm_floor=floor_ms / f["median_ms"],
                     torch_share_of_hbm_floor=floor_ms / t["median_ms"],
                     cache_resident=bool(floor <= INFINITY_CACHE_BYTES),
                     launch_bound=bool(floor_ms * 1e3 < 2 * LAUNCH_BOUND_US), max_rel_diff_vs_torch=diff, bar_met=bool(met))
    print(f"{name}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}], torch {t['median_ms']:.4f} ms "
          f"[{t['min_ms']:.4f}, {t['max_ms']:.4f}]; floor {floor_ms:.4f} ms (share {floor_ms / f['median_ms']:.2f})",
          flush=True)
    if not met:
        missed.append(name)


def recompute(L, dev, out):
    """One row: the module's cached step against its forward over the whole context of L + 1 positions."""
    from aura_snn_rag_amd import HippocampalProsodyAttention
    torch.manual_seed(3)
    att = HippocampalProsodyAttention(types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0),
                                      hippocampus=object()).to(dev).eval()
    hidden, prosody = torch.randn(1, L + 1, D, device=dev), torch.randn(1, L + 1, 4, device=dev)
    with torch.no_grad():
        cache = att.new_cache(1, L + 1)
        att.prefill(hidden[:, :L], prosody=prosody[:, :L], cache=cache)
        tok, pr = hidden[:, L].contiguous(), prosody[:, L].contiguous()

        def step():
            cache.lengths.fill_(L)                      # the same step again: part of the timed work, one tiny launch
            cache.max_length = L
            return att.step(tok, prosody=pr, cache=cache)

        full = lambda: att(hidden, prosody=prosody)[0]
        diff = float((step()[0] - full()[0, L]).abs().max())
        assert diff <= 1e-4, diff
        ms, iters = alternated({"step": step, "forward": full}, events_window)
    s, f = summary(ms["step"]), summary(ms["forward"])
    out[f"recompute_L{L}"] = dict(L=L, step=s, forward=f, iters=iters, forward_over_step=f["median_ms"] / s["median_ms"],
                                  max_abs_diff=diff)
    print(f"recompute L={L}: step {s['median_ms']:.4f} ms, forward over the context {f['median_ms']:.4f} ms "
          f"({f['median_ms'] / s['median_ms']:.1f}x)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--length", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_attention_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_attention_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for B in a.batch:
        for L in a.length:
            one(B, L, dev, out, missed)
    for L in a.length:
        recompute(L, dev, out)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
