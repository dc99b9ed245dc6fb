"""Measurements of replay -> profiles/replay_bench.json.

    python tools/replay_bench.py [--rows 1000000] [--dim 128] [--out profiles/replay_bench.json]

Needs a GPU (no fallback).  One process.  Every figure is the median over WINDOWS windows of at least WINDOW_S of work
each (min and max beside it), after a warm-up, the things compared taken in alternating order inside each round
(tools/diverse_bench.py's scheme), host clock with a synchronise at both ends of a window.

A bank of ``rows`` rows without a centroid index whose retention keys are distinct (random strengths, 64 timestamp
buckets: a bank of equal keys lets ``bank_select_weakest`` leave after pass 0).  For n = 256 and 4096, alternated:
  replay            ``hf.replay(n, return_features=False)``, the counter numbering the draws
  select_weakest    ``ops.bank_select_weakest(meta, rows, now, 0, n)`` on the same metadata
  replay_features   ``hf.replay(n)``: the same with the gather of the n rows
The first two move the same bytes (16 B per row once, then 4 B per row per pass) through the same digit passes and
compaction; replay's pass 0 adds the generator and three logarithms per row.
  The bar: replay's median may exceed select_weakest's by at most 10 % plus select_weakest's own spread (max - min over
  its windows) in the same run.  Exit status 1 when the bar is missed; the figures are written either way."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, wall_window, summary, WINDOWS, WINDOW_S  # noqa: E402

NOW = 1.7e9
SIZES = (256, 4096)
ALLOWED = 1.10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(31)
    hf = HippocampalFormation(feature_dim=a.dim, max_memories=a.rows, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                              device="cuda", use_centroid_index=False, replay_seed=2024)
    chunk = 1 << 17
    for r0 in range(0, a.rows, chunk):
        n = min(chunk, a.rows - r0)
        hf.bulk_write(torch.randn(n, a.dim, generator=g, device=dev), rebuild=False, tags=1 + (np.arange(r0, r0 + n) % 8))
    meta = hf.memory_metadata
    meta[:, 0] = 0.25 + 0.75 * torch.rand(a.rows, generator=g, device=dev)
    meta[:, 1] = float(np.float32(NOW)) - 128.0 * torch.randint(0, 64, (a.rows,), generator=g, device=dev).float()
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "windows": WINDOWS,
           "window_s_at_least": WINDOW_S, "allowed_ratio": ALLOWED, "sizes": {}}
    missed = []
    for n in SIZES:
        # the draw is what the rule says, before it is timed
        d = hf.replay_keys(draw=0, now=NOW)
        s = hf.replay(n, draw=0, now=NOW, return_features=False)
        order = torch.sort(d, descending=True, stable=True).indices[:n]
        assert torch.equal(s.rows.long(), order) and torch.equal(s.keys, d[order]) and int(s.eligible) == a.rows
        ms, iters = alternated({
            "replay": lambda: hf.replay(n, now=NOW, return_features=False),
            "select_weakest": lambda: ops.bank_select_weakest(meta, a.rows, NOW, 0, n),
            "replay_features": lambda: hf.replay(n, now=NOW)}, wall_window)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        res = {**{k: summary(v) for k, v in ms.items()}, "calls_per_window": iters, "spread_ms": spread,
               "replay_over_select": med["replay"] / med["select_weakest"],
               "bar_ms": ALLOWED * med["select_weakest"] + spread["select_weakest"]}
        print("replay", n, res, flush=True)
        out["sizes"][str(n)] = res
        if med["replay"] > res["bar_ms"]:
            missed.append(f"n={n}: replay {med['replay']:.4f} ms, select_weakest {med['select_weakest']:.4f} ms x {ALLOWED} "
                          f"+ spread {spread['select_weakest']:.4f} ms")
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)
    if missed:
        raise SystemExit("bars missed:\n  " + "\n  ".join(missed))


if __name__ == "__main__":
    main()
