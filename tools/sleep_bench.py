"""Measurements of the bank compaction and of ``consolidate`` -> profiles/sleep_bench.json.

    python tools/sleep_bench.py [--rows 1000000] [--dim 768] [--out profiles/sleep_bench.json] [--only mover|consolidate]

Needs a GPU (no fallback).  One process; the things compared are taken in alternating order (tools/diverse_bench.py's
scheme); every figure is the median over the windows (min and max beside it).

  the mover, on a bank of ``rows`` x ``dim`` with the bf16 shadow present (six arrays, 4640 B per row at D = 768, S = 2):
    row0 / random10 / last   what is removed: row 0 (every row shifts by one: all rounds staged), a random 10 % (staged
                             rounds until the removed rows add up to a round, direct ones from there), the last row
                             (nothing moves)
    mover                    ops.bank_compact: the numpy checks, ONE upload of the int32 sources, the launches
    torch                    the same move composed from torch ops: one upload of the int64 sources, then per array
                             index_select into a temporary + copy back
    The bar: mover <= 1.10 x torch.  The floor: one read and one write per moved row at the copy rate of DESIGN.md
    4.3b; the fraction of it the mover reaches is reported (staged rounds pay it twice).
  consolidate, on a bank of ``rows`` rows one sixth of which stand in groups of 6 near-copies, index off, tau 0.9:
    consolidate              bulk_write (not timed), then HippocampalFormation.consolidate
    replay                   the same rows written to an empty bank by create_episodic_memories(merge_similarity=tau)
                             (chunks of 1024), what the parent could already do
    The bar: consolidate <= 1.10 x replay.  The floor beside it: N^2 D FLOP on the bf16 matrix pipe (half a pass over
    the image per slab on average)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.diverse_bench import wall_window, summary  # noqa: E402

COPY_BYTES_PER_S = 1.54e9 / 271e-6
PEAK_BF16_MATRIX_FLOPS = 2.5e15
WINDOWS = 5
TAU = 0.9
BAR = 1.10


def new_bank(rows, D, **kw):
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    hf = HippocampalFormation(feature_dim=D, max_memories=rows, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                              device="cuda", use_centroid_index=False, **kw)
    hf.centroids_update_interval = 10 ** 9
    return hf


def mover_cases(rows, D, dev):
    from aura_snn_rag_amd import ops
    hf = new_bank(rows, D)
    bench.fill_bank(hf, rows, D, 1234, dev)
    assert hf._ensure_shadow() is not None, "the bench wants the bf16 shadow present"
    arrays = [hf.memory_features, hf.memory_locations, hf.memory_metadata, hf._inv_norm, hf._shadow, hf._rho]
    row_bytes = sum(a[0].numel() * a.element_size() for a in arrays)
    every = np.arange(rows, dtype=np.int64)
    rng = np.random.default_rng(5)
    cases = {"row0": every[1:], "random10": np.nonzero(rng.random(rows) >= 0.1)[0], "last": every[:-1]}
    out = {"row_bytes": row_bytes, "round_rows": ops.bank_compact_round_rows(), "cases": {}}
    for name, src in cases.items():
        moved = int((src != np.arange(src.size)).sum())

        def mover():
            ops.bank_compact(arrays[0], arrays[1], arrays[2], arrays[3], src, 0, shadow=arrays[4], rho=arrays[5])

        def composed():
            idx = torch.from_numpy(src).to(dev)
            for a in arrays:
                a[:src.size].copy_(a.index_select(0, idx))
        # the same move on a copy of a slice, once, before anything is timed: the two must agree bit for bit
        if name != "last":
            small = [a[:20_000].clone() for a in arrays]
            want = [a.clone() for a in small]
            s = src[src < 20_000]
            idx = torch.from_numpy(s).to(dev)
            for a in want:
                a[:s.size].copy_(a.index_select(0, idx))
            ops.bank_compact(small[0], small[1], small[2], small[3], s, 0, shadow=small[4], rho=small[5])
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(small, want))
        fns = {"mover": mover, "torch": composed}
        for fn in fns.values():
            fn()
        ms = {k: [] for k in fns}
        names = list(fns)
        for rnd in range(WINDOWS):
            for k in (names if rnd % 2 == 0 else names[::-1]):
                ms[k].append(wall_window(fns[k], 3))
        mv, tc = statistics.median(ms["mover"]), statistics.median(ms["torch"])
        floor_ms = 1e3 * 2.0 * moved * row_bytes / COPY_BYTES_PER_S
        res = {"rows_kept": int(src.size), "rows_moved": moved, "mover": summary(ms["mover"]), "torch": summary(ms["torch"]),
               "mover_over_torch": mv / tc, "bar_met": mv <= BAR * tc, "floor_ms": floor_ms,
               "fraction_of_floor": (floor_ms / mv) if moved else None}
        print(name, res, flush=True)
        out["cases"][name] = res
    return out


def grouped_rows(rows, D, dev):
    """``rows`` x D: one sixth of the rows stand in groups of 6 near-copies (group + 0.05 randn), shuffled."""
    g = torch.Generator(device=dev).manual_seed(77)
    groups = rows // 36
    base = torch.randn(groups, D, generator=g, device=dev)
    copies = base.repeat_interleave(6, 0) + 0.05 * torch.randn(groups * 6, D, generator=g, device=dev)
    feats = torch.empty(rows, D, device=dev)
    feats[:groups * 6] = copies
    for lo in range(groups * 6, rows, 1 << 17):
        hi = min(rows, lo + (1 << 17))
        feats[lo:hi] = torch.randn(hi - lo, D, generator=g, device=dev)
    return feats[torch.randperm(rows, generator=g, device=dev)].contiguous(), groups


def consolidate_case(rows, D, dev):
    import time
    feats, groups = grouped_rows(rows, D, dev)
    ids = [f"bulk-{i}" for i in range(rows)]
    ms = {"consolidate": [], "replay": []}
    kept = {}

    def run(which):
        hf = new_bank(rows, D)
        if which == "consolidate":
            for lo in range(0, rows, 1 << 17):
                hf.bulk_write(feats[lo:lo + (1 << 17)], rebuild=False)
            hf._ensure_shadow()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "consolidate":
            hf.consolidate(TAU, rebuild=False)
        else:
            hf.create_episodic_memories(ids, feats, merge_similarity=TAU)
        torch.cuda.synchronize()
        ms[which].append(1e3 * (time.perf_counter() - t0))
        kept[which] = hf.memory_count
        return hf
    banks = {k: run(k) for k in ("consolidate", "replay")}            # warm-up round, and the two results compared
    n = kept["consolidate"]
    same = kept["replay"] == n and bool(torch.equal(banks["consolidate"].memory_features[:n],
                                                    banks["replay"].memory_features[:n]))
    del banks
    ms = {"consolidate": [], "replay": []}
    for rnd in range(2):
        for k in (("consolidate", "replay") if rnd % 2 == 0 else ("replay", "consolidate")):
            run(k)
    c, r = statistics.median(ms["consolidate"]), statistics.median(ms["replay"])
    floor_ms = 1e3 * float(n) * float(n) * D / PEAK_BF16_MATRIX_FLOPS
    res = {"rows": rows, "groups_of_6": groups, "rows_kept": n, "equals_the_replay": same, "tau": TAU,
           "consolidate": summary(ms["consolidate"]), "replay": summary(ms["replay"]), "consolidate_over_replay": c / r,
           "bar_met": c <= BAR * r, "floor_matrix_pipe_ms": floor_ms, "fraction_of_matrix_pipe_floor": floor_ms / c}
    print("consolidate", res, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sleep_bench.json"))
    ap.add_argument("--only", choices=("mover", "consolidate"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sleep_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "windows": WINDOWS, "bar": BAR,
           "copy_bytes_per_s_assumed": COPY_BYTES_PER_S, "peak_bf16_matrix_flops_assumed": PEAK_BF16_MATRIX_FLOPS}
    if a.only in (None, "mover"):
        out["mover"] = mover_cases(a.rows, a.dim, dev)
        torch.cuda.empty_cache()
    if a.only in (None, "consolidate"):
        out["consolidate"] = consolidate_case(a.rows, a.dim, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)
    missed = [k for k, v in out.get("mover", {}).get("cases", {}).items() if not v["bar_met"]]
    if "consolidate" in out and not out["consolidate"]["bar_met"]:
        missed.append("consolidate")
    if "consolidate" in out and not out["consolidate"]["equals_the_replay"]:
        raise SystemExit("consolidate and the replay left different banks")
    if missed:
        raise SystemExit(f"slower than {BAR} x the comparison: {missed}")


if __name__ == "__main__":
    main()
