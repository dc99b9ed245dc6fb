"""Measurements of scoped recall -> profiles/scoped_recall_bench.json.

    python tools/scoped_bench.py [--rows 1000000] [--dim 768] [--queries 2048] [--out profiles/scoped_recall_bench.json]

Needs a GPU (no fallback).  One process, one bank of ``rows`` random rows without a centroid index, tags 1 .. 64 dealt
round-robin (row r carries tag 1 + r % 64, so tags 1 .. 4 together hold 1/16 of the rows -- they are re-tagged to ONE
tag, 100, for the first case), timestamps ascending with the row so that "the last N rows" is a time window.  Every figure
is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), after a warm-up, the things
compared taken in alternating order inside each round (tools/diverse_bench.py's scheme), host clock with a synchronise at
both ends of a window; k = 8.

  cases, ``queries`` queries each:
    one_scope_16th     all queries in the one scope of tag 100, 1/16 of the rows
    64_scopes_64th     the queries dealt over 60 scopes (tags 5 .. 64) of 1/64 of the rows each
    last_n_window      all queries with ``newer_than`` = the timestamp of the row ``rows / 16`` from the end, any tag
  per case:
    scoped             recall_batch(tags= / newer_than=, check_overflow=False)
    full_bank   (a)    recall_batch(use_candidates=False, check_overflow=False) over the whole bank, the same queries
    torch_ops   (b)    the same selection composed from torch ops on the same GPU: mask, nonzero, gather of the scope's
                       rows, normalise, mm, the combined score, topk -- per scope of the call
  Before anything is timed the scoped results are compared with (b)'s (same rows up to near-ties of 2e-6, scores
  within 1e-5).
  The bars, checked at the end (exit status 1 when missed): case one_scope_16th takes less time than (a); every case
  takes less time than (b).
  floors: the scope build reads 16 B per held row at the copy rate of DESIGN.md 4.3b; the scan does
  2 D sum_i |scope(i)| FLOP at the fp32 matrix peak and gathers 4 D bytes per row of a scope per tile of 64 queries.

``--only trace``: the three scoped calls alone, for ``rocprofv3 --kernel-trace --stats -- python tools/scoped_bench.py
--only trace`` in a run of its own."""
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
from tools.diverse_bench import alternated, wall_window, summary, WINDOWS, WINDOW_S  # noqa: E402

COPY_BYTES_PER_S = 1.54e9 / 271e-6
PEAK_FP32_MATRIX_FLOPS = 157.3e12             # MI355X, fp32 matrix
K = 8
N_TAGS = 64
ONE_TAG = 100


def torch_scoped(hf, q, qtags, k, now, newer_than=None):
    """The scoped selection from torch ops (the rule restated): per distinct tag one mask, gather, mm and topk."""
    n = hf.memory_count
    meta = hf.memory_metadata[:n]
    out_s = torch.full((q.shape[0], k), float("-inf"), device=q.device)
    out_r = torch.full((q.shape[0], k), -1, dtype=torch.int32, device=q.device)
    qn = torch.nn.functional.normalize(q, dim=1)
    base = torch.ones(n, dtype=torch.bool, device=q.device)
    if newer_than is not None:
        base &= meta[:, 1] >= torch.tensor(float(np.float32(newer_than)), device=q.device)
    qt = torch.as_tensor(qtags, device=q.device)
    for tag in np.unique(qtags).tolist():
        mask = base if tag < 0 else base & (meta[:, 3].to(torch.int32) == tag)
        rows = torch.nonzero(mask).flatten()
        if rows.numel() == 0:
            continue
        sel = torch.nonzero(qt == tag).flatten()
        feats = torch.nn.functional.normalize(hf.memory_features.index_select(0, rows), dim=1)
        m = meta.index_select(0, rows)
        comb = (0.5 * (qn.index_select(0, sel) @ feats.t()) + 0.2 * torch.exp(-(now - m[:, 1]) / 3600.0)) * m[:, 0]
        kk = min(k, rows.numel())
        s, p = torch.topk(comb, kk, dim=1)
        out_s[sel, :kk], out_r[sel, :kk] = s, rows[p].to(torch.int32)
    return out_s, out_r


def agree(s, r, ts, tr):
    """Scores within 1e-5 everywhere; a row may differ only where the two scores at that place are within 2e-6."""
    if not torch.allclose(s, ts, atol=1e-5, rtol=0):
        return False
    diff = r != tr
    return bool(((s - ts).abs()[diff] <= 2e-6).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoped_recall_bench.json"))
    ap.add_argument("--only", choices=("trace",), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scoped_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    dev = torch.device("cuda", 0)
    D, rows, nq = a.dim, a.rows, a.queries
    hf = HippocampalFormation(feature_dim=D, max_memories=rows, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                              device="cuda", use_centroid_index=False)
    g = torch.Generator(device=dev).manual_seed(1234)
    chunk = 1 << 17
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        tags = 1 + (np.arange(r0, r0 + n) % N_TAGS)
        tags[tags <= 4] = ONE_TAG
        hf.bulk_write(torch.randn(n, D, generator=g, device=dev), rebuild=False, tags=tags)
    now = 1.7e9
    # fp32 timestamps 128 s apart per block of rows, ascending with the row: the last rows are the newest
    stamps = (now - 128.0 * ((rows - 1 - torch.arange(rows, dtype=torch.float64)) // 4096)).float()
    hf.memory_metadata[:rows, 1] = stamps.to(dev)
    hf.memory_metadata[:rows, 0] = (0.25 + 0.75 * torch.rand(rows, generator=g, device=dev))
    pick = torch.randint(0, rows, (nq // 2,), generator=g, device=dev)
    q = torch.cat([hf.memory_features[pick] + 0.05 * torch.randn(nq // 2, D, generator=g, device=dev),
                   torch.randn(nq - nq // 2, D, generator=g, device=dev)]).contiguous()
    newest = float(stamps[rows - max(1, rows // 16)])
    cases = {
        "one_scope_16th": dict(tags=np.full(nq, ONE_TAG)),
        "64_scopes_64th": dict(tags=5 + (np.arange(nq) % (N_TAGS - 4))),
        "last_n_window": dict(tags=np.full(nq, -1), newer_than=newest),
    }

    def scoped(c):
        return hf.recall_batch(q, k=K, now=now, check_overflow=False, **c)

    if a.only == "trace":
        for c in cases.values():
            for _ in range(10):
                scoped(c)
        torch.cuda.synchronize()
        return
    hf.recall_batch(q, k=K, now=now, use_candidates=False)          # (builds the bf16 shadow before anything is timed)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "dim": D, "queries": nq, "k": K, "windows": WINDOWS,
           "window_s_at_least": WINDOW_S, "copy_bytes_per_s_assumed": COPY_BYTES_PER_S,
           "peak_fp32_matrix_flops_assumed": PEAK_FP32_MATRIX_FLOPS, "cases": {}}
    missed = []
    for name, c in cases.items():
        s, r = scoped(c)
        ts, tr = torch_scoped(hf, q, c["tags"], K, now, c.get("newer_than"))
        same = agree(s, r, ts, tr)
        meta = hf.memory_metadata[:rows]
        in_window = meta[:, 1] >= c["newer_than"] if "newer_than" in c else torch.ones(rows, dtype=torch.bool, device=dev)
        sizes = {t: int((in_window & ((meta[:, 3].to(torch.int32) == t) if t >= 0 else in_window)).sum())
                 for t in np.unique(c["tags"]).tolist()}
        pairs = float(sum(sizes[t] for t in c["tags"].tolist()))
        tiles = sum(-(-int((c["tags"] == t).sum()) // 64) * sizes[t] for t in sizes)
        ms, iters = alternated({
            "scoped": lambda: scoped(c),
            "full_bank": lambda: hf.recall_batch(q, k=K, now=now, use_candidates=False, check_overflow=False),
            "torch_ops": lambda: torch_scoped(hf, q, c["tags"], K, now, c.get("newer_than"))}, wall_window)
        med = {k: statistics.median(v) for k, v in ms.items()}
        floor_build = 1e3 * 16.0 * rows / COPY_BYTES_PER_S
        floor_flop = 1e3 * 2.0 * D * pairs / PEAK_FP32_MATRIX_FLOPS
        floor_gather = 1e3 * 4.0 * D * tiles / COPY_BYTES_PER_S
        res = {"scopes": len(sizes), "rows_in_scopes": sizes if len(sizes) <= 4 else {"min": min(sizes.values()),
                                                                                      "max": max(sizes.values())},
               "query_row_pairs": pairs, "agrees_with_torch_ops": same,
               **{k: summary(v) for k, v in ms.items()}, "calls_per_window": iters,
               "scoped_over_full_bank": med["scoped"] / med["full_bank"],
               "scoped_over_torch_ops": med["scoped"] / med["torch_ops"],
               "floor_scope_build_ms": floor_build, "floor_matrix_pipe_ms": floor_flop, "floor_gather_ms": floor_gather,
               "fraction_of_floors": (floor_build + max(floor_flop, floor_gather)) / med["scoped"]}
        print(name, res, flush=True)
        out["cases"][name] = res
        if not same:
            missed.append(f"{name}: the scoped results differ from the torch composition")
        if med["scoped"] >= med["torch_ops"]:
            missed.append(f"{name}: scoped recall takes {med['scoped']:.3f} ms, the torch composition {med['torch_ops']:.3f} ms")
        if name == "one_scope_16th" and med["scoped"] >= med["full_bank"]:
            missed.append(f"{name}: scoped recall takes {med['scoped']:.3f} ms, the full-bank recall {med['full_bank']:.3f} ms")
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)
    if missed:
        raise SystemExit("bars missed:\n  " + "\n  ".join(missed))


if __name__ == "__main__":
    main()
