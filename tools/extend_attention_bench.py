"""Measurements of the multi-token cached step -> profiles/extend_attention_bench.json.

    python tools/extend_attention_bench.py [--batch 1 8] [--length 512 2048] [--tokens 8 32] [--out ...]

Needs a GPU (no fallback).  One process.  D = 768, H = 12 (dh = 64); every row of a batch holds L positions and takes m
new tokens, the cache holds L + m positions afterwards.  Per point three candidates that leave the same caches:
  extend    ``ops.attn_decode_extend`` (two launches, ``advance=False``);
  steps     ``m`` calls of ``ops.attn_decode_step`` (2 m launches);
            both start from one tiny launch that sets the lengths to L, so that every call of a window does the same work;
  torch     the same result from torch ops: the query modulation, an ``index_copy_`` of the m keys and values into the
            cache and the library attention of the m queries over the ``[.., :L + m]`` slice with an explicit mask.
The three are first checked against each other (extend and steps bit for bit; torch within a relative 1e-4).
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), device
events, after a warm-up of every candidate, the candidates taken in alternating order inside each round
(tools/diverse_bench.py's scheme).
Floor: K and V read once, ``2 B H L dh 4`` bytes, at 6.3 TB/s.  The caches are not rotated: a point whose K/V fit the
256 MiB Infinity Cache is marked ``cache_resident`` and its share of the HBM floor is not a share of anything HBM did.
Bar: the extend's slowest window below the ``m`` steps' fastest window at every point.  The torch composition has no
bar: its ratio is reported with its spread.  Exit status 1 when a bar is missed; the figures are written either way.
Model level (no bar): on tools/generate_bench.py's model (D 256, 4 layers, V 32 000, B = 1) a 32-token turn through
``extend`` against 32 calls of ``step(fused=True)``, both from the same prefilled state of 64 positions."""
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
D, H = 768, 12


def torch_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, Kc, Vc, at, mask, L):
    """The extend from torch ops: modulation, index_copy_ into the cache, the library attention with a mask."""
    B, m, _ = q.shape
    dh = D // H
    qh = q.view(B, m, H, dh).transpose(1, 2)                                            # [B, H, m, dh]
    gain = torch.sigmoid(prosody @ Wp.T + bp).transpose(1, 2)[..., None]                # [B, H, m, 1]
    qh = qh * (1.0 + gain) * (1.0 + 0.2 * torch.tanh(prosody[..., 0]))[:, None, :, None] \
        * (1.0 + 0.05 * torch.tanh(prosody[..., 1]))[:, None, :, None]
    qh = qh * (1.0 + 0.5 * torch.sigmoid(x @ wm.T + bm)).transpose(1, 2)[..., None]
    Kc.index_copy_(2, at, k_new.view(B, m, H, dh).transpose(1, 2))
    Vc.index_copy_(2, at, v_new.view(B, m, H, dh).transpose(1, 2))
    ctx = F.scaled_dot_product_attention(qh, Kc[:, :, :L + m], Vc[:, :, :L + m], attn_mask=mask)
    return ctx.transpose(1, 2).reshape(B, m, D)


def one(B, L, m, dev, out, missed):
    from aura_snn_rag_amd import ops
    dh, cap = D // H, L + m
    gen = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)
    q, k_new, v_new, x, prosody = rnd(B, m, D), rnd(B, m, D), rnd(B, m, D), rnd(B, m, D), rnd(B, m, 4)
    Wp, bp, wm, bm = rnd(H, 4), rnd(H), rnd(1, D) / D ** 0.5, rnd(1)
    Kc, Vc = rnd(B, H, cap, dh), rnd(B, H, cap, dh)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    at = torch.arange(L, L + m, device=dev)
    mask = torch.arange(cap, device=dev)[None, :] <= at[:, None]                        # [m, L + m]: query j sees <= L + j
    nc = ops.attn_decode_chunks(cap)
    ws = torch.empty(ops.attn_decode_extend_workspace_floats(B, m, H, dh, nc), device=dev)
    ws1 = torch.empty(ops.attn_decode_workspace_floats(B, H, dh, nc), device=dev)
    rows = [tuple(t[:, j].contiguous() for t in (q, k_new, v_new, x, prosody)) for j in range(m)]

    def extend():
        lengths.fill_(L)
        return ops.attn_decode_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, Kc, Vc, ws, n_chunks=nc,
                                      advance=False)

    def steps():
        lengths.fill_(L)
        return [ops.attn_decode_step(*r[:4], r[4], Wp, bp, wm, bm, lengths, Kc, Vc, ws1, n_chunks=nc) for r in rows]

    comp = lambda: torch_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, Kc, Vc, at, mask, L)
    a, s, t = extend(), torch.stack(steps(), dim=1), comp()
    assert int(lengths[0]) == L + m
    assert torch.equal(a.view(torch.int32), s.view(torch.int32)), "extend and the m steps differ in bits"
    diff = float((a - t).abs().max() / t.abs().max())
    assert diff <= 1e-4, diff

    ms, iters = alternated({"extend": extend, "steps": steps, "torch": comp}, events_window)
    assert bool((extend() != 0).any()), "the timed extend was an inactive one"
    e, s, t = summary(ms["extend"]), summary(ms["steps"]), summary(ms["torch"])
    floor = 2 * B * H * L * dh * 4
    floor_ms = 1e3 * floor / HBM_BYTES_PER_S
    met = e["max_ms"] < s["min_ms"]
    name = f"B{B}_L{L}_m{m}"
    out[name] = dict(B=B, L=L, m=m, D=D, H=H, extend=e, steps=s, torch=t, iters=iters,
                     ratio_extend_over_steps=e["median_ms"] / s["median_ms"],
                     ratio_extend_over_torch=e["median_ms"] / t["median_ms"],
                     extend_beats_torch_outside_spreads=bool(e["max_ms"] < t["min_ms"]),
                     torch_beats_extend_outside_spreads=bool(t["max_ms"] < e["min_ms"]),
                     floor_bytes=floor, floor_ms=floor_ms, share_of_hbm_floor=floor_ms / e["median_ms"],
                     cache_resident=bool(floor <= INFINITY_CACHE_BYTES), max_rel_diff_vs_torch=diff, bar_met=bool(met))
    print(f"{name}: extend {e['median_ms']:.4f} ms [{e['min_ms']:.4f}, {e['max_ms']:.4f}], {m} steps "
          f"{s['median_ms']:.4f} ms [{s['min_ms']:.4f}, {s['max_ms']:.4f}], torch {t['median_ms']:.4f} ms "
          f"[{t['min_ms']:.4f}, {t['max_ms']:.4f}]; floor {floor_ms:.5f} ms", flush=True)
    if not met:
        missed.append(name)


def model_level(dev, out, P=64, m=32):
    """A 32-token turn fed into a prefilled state: one ``extend`` against 32 fused steps."""
    from aura_snn_rag_amd import HippocampalTransformer
    cfg = types.SimpleNamespace(vocab_size=32000, embedding_dim=256, num_heads=4, num_layers=4, intermediate_size=1024,
                                n_place_cells=2000, max_seq_len=1024, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    torch.manual_seed(0)
    model = HippocampalTransformer(cfg, None).to(dev).eval()
    ids = torch.randint(0, 32000, (1, P + m), generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        state = model.new_state(1, P + m)
        model.prefill(ids[:, :P], state=state)

        def rewind():
            state.lengths.fill_(P)
            state.position = P
            for c in state.caches:
                c.max_length = P

        def extend():
            rewind()
            return model.extend(ids[:, P:], state=state)

        def steps():
            rewind()
            return [model.step(ids[:, P + j], state=state, fused=True) for j in range(m)]

        a, b = extend(), torch.stack(steps(), dim=1)
        diff = float((a - b).abs().max() / b.abs().max())
        assert diff <= 1e-4, diff
        ms, iters = alternated({"extend": extend, "fused_steps": steps}, events_window)
    e, s = summary(ms["extend"]), summary(ms["fused_steps"])
    out["model_turn"] = dict(prefilled=P, m=m, D=256, layers=4, V=32000, B=1, extend=e, fused_steps=s, iters=iters,
                             ratio_extend_over_fused_steps=e["median_ms"] / s["median_ms"], max_rel_logit_diff=diff)
    print(f"model turn of {m}: extend {e['median_ms']:.3f} ms, {m} fused steps {s['median_ms']:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--length", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--tokens", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_attention_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extend_attention_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for B in a.batch:
        for L in a.length:
            for m in a.tokens:
                one(B, L, m, dev, out, missed)
    model_level(dev, out)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
