"""Measurements of the extend with per-row counts -> profiles/ragged_extend_bench.json.

    python tools/ragged_extend_bench.py [--length 512 2048] [--out ...]

Needs a GPU (no fallback).  One process.  D = 768, H = 12 (dh = 64), B = 8, m = 32; every row holds L positions.
  (a) full     ``ops.attn_decode_extend(.., counts=)`` with every count equal to m next to the call without counts (the
               same work; first checked bit for bit).  The bar: it costs the same, where "the same" is the call
               without counts' own window spread in this run: the medians differ by no more than (max - min) of its
               windows.  Both are written down; no number is fixed beforehand.
  (b) mixed    counts (32, 1, 8, 17, 0, 32, 4, 9) in one call next to the only thing possible without counts: one
               unragged extend per distinct count on the rows that share it (six calls; their caches are split
               beforehand, which costs that side nothing here).  Checked bit for bit.  The ratio, no bar.
  (c) turn     on tools/generate_bench.py's model (D 256, 4 layers, V 32 000) a second turn of ``generate`` with
               ``new_lengths`` = the mixed counts and 16 new tokens, B = 8, next to the eight rows run one by one
               (B = 1, each from its own state; the row without new tokens, which no unragged call can take, as a
               ragged call of its own).  The ratio, no bar.
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), device
events, after a warm-up of every candidate, the candidates taken in alternating order inside each round
(tools/diverse_bench.py's scheme).  Both calls of (a) and (b) start from one tiny launch that sets the lengths to L.
Exit status 1 when the bar of (a) is missed; the figures are written either way."""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

D, H, B, M = 768, 12, 8, 32
MIXED = (32, 1, 8, 17, 0, 32, 4, 9)


def kernel_level(L, dev, out, missed):
    from aura_snn_rag_amd import ops
    dh, cap = D // H, L + M
    gen = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)
    q, k_new, v_new, x, prosody = rnd(B, M, D), rnd(B, M, D), rnd(B, M, D), rnd(B, M, D), rnd(B, M, 4)
    Wp, bp, wm, bm = rnd(H, 4), rnd(H), rnd(1, D) / D ** 0.5, rnd(1)
    Kc, Vc = rnd(B, H, cap, dh), rnd(B, H, cap, dh)
    lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
    nc = ops.attn_decode_chunks(cap)
    ws = torch.empty(ops.attn_decode_extend_workspace_floats(B, M, H, dh, nc), device=dev)
    full = torch.full((B,), M, dtype=torch.int32, device=dev)
    mixed = torch.tensor(MIXED, dtype=torch.int32, device=dev)

    def call(counts):
        lengths.fill_(L)
        return ops.attn_decode_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, Kc, Vc, ws, n_chunks=nc,
                                      advance=False, counts=counts)

    # (b)'s other side: the rows that share a count, each group with its own contiguous tensors and caches
    groups = []
    for c in sorted(set(MIXED) - {0}):
        rows = [b for b in range(B) if MIXED[b] == c]
        part = lambda t: t[rows][:, :c].contiguous()
        g = dict(rows=rows, c=c, q=part(q), k=part(k_new), v=part(v_new), x=part(x), p=part(prosody),
                 K=Kc[rows].contiguous(), V=Vc[rows].contiguous(),
                 lengths=torch.full((len(rows),), L, dtype=torch.int32, device=dev))
        g["ws"] = torch.empty(ops.attn_decode_extend_workspace_floats(len(rows), c, H, dh, nc), device=dev)
        groups.append(g)

    def grouped():
        outs = []
        for g in groups:
            g["lengths"].fill_(L)
            outs.append(ops.attn_decode_extend(g["q"], g["k"], g["v"], g["x"], g["p"], Wp, bp, wm, bm, g["lengths"],
                                               g["K"], g["V"], g["ws"], n_chunks=nc, advance=False))
        return outs

    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(call(None)), bits(call(full))), "counts == m and the call without counts differ in bits"
    ragged = call(mixed)
    for g, o in zip(groups, grouped()):
        assert torch.equal(bits(ragged[g["rows"]][:, :g["c"]]), bits(o)), "mixed counts and the grouped calls differ"
    assert bool((ragged[4] == 0).all()) and bool((ragged[1, 1:] == 0).all())

    ms, iters = alternated({"plain": lambda: call(None), "full": lambda: call(full)}, events_window)
    p, f = summary(ms["plain"]), summary(ms["full"])
    spread = p["max_ms"] - p["min_ms"]
    met = abs(f["median_ms"] - p["median_ms"]) <= spread
    ms2, iters2 = alternated({"mixed": lambda: call(mixed), "grouped": grouped}, events_window)
    r, g = summary(ms2["mixed"]), summary(ms2["grouped"])
    name = f"B{B}_L{L}_m{M}"
    out[name] = dict(B=B, L=L, m=M, D=D, H=H, without_counts=p, counts_all_m=f, iters=iters,
                     ratio_counts_all_m_over_without=f["median_ms"] / p["median_ms"], without_counts_spread_ms=spread,
                     bar_same_cost_met=bool(met), mixed_counts=list(MIXED), mixed=r, grouped_unragged_calls=g,
                     grouped_calls=len(groups), iters_mixed=iters2,
                     ratio_mixed_over_grouped=r["median_ms"] / g["median_ms"],
                     ratio_mixed_over_counts_all_m=r["median_ms"] / f["median_ms"],
                     tokens_share=sum(MIXED) / (B * M))
    print(f"{name}: without counts {p['median_ms']:.4f} ms [{p['min_ms']:.4f}, {p['max_ms']:.4f}], counts all m "
          f"{f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}]; mixed {r['median_ms']:.4f} ms "
          f"[{r['min_ms']:.4f}, {r['max_ms']:.4f}], {len(groups)} grouped calls {g['median_ms']:.4f} ms "
          f"[{g['min_ms']:.4f}, {g['max_ms']:.4f}]", flush=True)
    if not met:
        missed.append(name)


def _snapshot(state):
    return dict(lengths=state.lengths.clone(), pending=state.pending.clone(), seen=state.seen.clone(), step=state.step,
                position=state.position, held=[c.max_length for c in state.caches])


def _restore(state, snap):
    state.lengths.copy_(snap["lengths"])
    state.pending = snap["pending"].clone()
    state.seen.copy_(snap["seen"])
    state.finished.zero_()
    state.step, state.position = snap["step"], snap["position"]
    for c, held in zip(state.caches, snap["held"]):
        (c.attention if hasattr(c, "attention") else c).max_length = held


def model_level(dev, out, P=64, n_new=16):
    """A ragged second turn of ``generate`` against the rows one by one, each from the state of its own first turn."""
    from aura_snn_rag_amd import HippocampalTransformer
    cfg = types.SimpleNamespace(vocab_size=32000, embedding_dim=256, num_heads=4, num_layers=4, intermediate_size=1024,
                                n_place_cells=2000, max_seq_len=1024, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    torch.manual_seed(0)
    model = HippocampalTransformer(cfg, None).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 32000, (B, P), generator=g).to(dev)
    new_ids = torch.randint(0, 32000, (B, M), generator=g).to(dev)
    kw = dict(temperature=0.0, repetition_penalty=1.0, eos_token_id=None, pad_token_id=0)
    capacity = P + 8 + M + 1 + n_new
    _, batch = model.generate(ids, max_new_tokens=8, return_state=True, capacity=capacity, **kw)
    alone = [model.generate(ids[b:b + 1], max_new_tokens=8, return_state=True, capacity=capacity, stream_ids=[b], **kw)[1]
             for b in range(B)]
    snap, snaps = _snapshot(batch), [_snapshot(s) for s in alone]
    counts = torch.tensor(MIXED, device=dev)

    def ragged():
        _restore(batch, snap)
        return model.generate(new_ids, max_new_tokens=n_new, state=batch, new_lengths=counts, **kw)

    def one_by_one():
        outs = []
        for b in range(B):
            _restore(alone[b], snaps[b])
            if MIXED[b] == 0:                                           # a turn without new tokens has no unragged form
                outs.append(model.generate(new_ids[b:b + 1, :1], max_new_tokens=n_new, state=alone[b], new_lengths=[0],
                                           **kw))
            else:
                outs.append(model.generate(new_ids[b:b + 1, :MIXED[b]], max_new_tokens=n_new, state=alone[b], **kw))
        return outs

    a, singles = ragged(), one_by_one()
    same = sum(int((a[b, MIXED[b]:MIXED[b] + n_new] == singles[b][0, MIXED[b]:MIXED[b] + n_new]).sum()) for b in range(B))
    ms, iters = alternated({"ragged": ragged, "one_by_one": one_by_one}, events_window)
    r, s = summary(ms["ragged"]), summary(ms["one_by_one"])
    out["model_turn"] = dict(prefilled=P + 8, new_lengths=list(MIXED), max_new_tokens=n_new, D=256, layers=4, V=32000,
                             B=B, ragged=r, one_by_one=s, iters=iters,
                             ratio_ragged_over_one_by_one=r["median_ms"] / s["median_ms"],
                             greedy_tokens_equal=same, greedy_tokens=B * n_new)
    print(f"model turn: ragged batch {r['median_ms']:.3f} ms, rows one by one {s['median_ms']:.3f} ms; "
          f"{same} of {B * n_new} greedy tokens equal", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_extend_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_extend_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for L in a.length:
        kernel_level(L, dev, out, missed)
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
