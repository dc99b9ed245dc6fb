"""Measurements of the retention feature -> profiles/retention_bench.json.

    python tools/retention_bench.py [--rows 1000000] [--dim 768] [--out profiles/retention_bench.json]

Needs a GPU (no fallback).  Three groups, every shape warmed up, times from device events or a host clock
around work that ends in a synchronise, the two policies alternated inside this one process:

  select_weakest   ops.bank_select_weakest alone on metadata of 1 M and 10 M rows, n = 512 and 4096, for a bank of
                   distinct keys and a bank of equal keys: time per call (library launches + the torch.sort of the
                   n composites) and the bytes the call moves, computed from the shapes and from which passes read
                   the rows (the selection's own state, read back after the timing), as a share of 8 TB/s.
  full_bank_write  create_episodic_memories into a FULL bank, rows/s, index off and on, batches of 512 and 4096,
                   'weakest' next to 'fifo' (the policy of ONE bank object is switched between rounds so both see
                   the same bank), for equal keys and for varied strengths.
  recall           recall_batch at the headline shape with reinforce=None (repeated: the spread) and with
                   reinforce (an amount that changes strengths on every call: the added time per call).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
NOW = 1.7e9 + 777.0


def align256(b):
    return (b + 255) // 256 * 256


def selection_passes(count):
    """Digits of the radix select (aura_bank.hip: sel_passes): three of the key, then the rotated row's."""
    s = 0
    while s < 31 and (1 << s) < count:
        s += 1
    return 3 + (s + 11) // 12


def passes_that_read(ops, device, count, n):
    """How many launches of the last call read the rows: pass 0 (16 B per row, writes 4 B per row), every later
    pass that was not cut short (4 B per row), the compaction (4 B per row).  From the call's state records."""
    P = selection_passes(count)
    ws = ops._workspace_view(device, align256(8 * n) + 32 * (P + 1))[align256(8 * n):].cpu()
    done = [int(ws[32 * i + 12:32 * i + 16].view(torch.int32).item()) for i in range(P + 1)]
    later = sum(1 for i in range(1, P) if not done[i])
    return 1 + later + 1, later


def bench_select(ops, dev, out):
    res = []
    for count in (1_000_000, 10_000_000):
        g = torch.Generator(device=dev).manual_seed(count)
        meta = torch.zeros(count, 4, device=dev)
        meta[:, 1] = NOW - 100.0
        for keys in ("distinct", "equal"):
            meta[:, 0] = 0.25 + 0.75 * torch.rand(count, generator=g, device=dev) if keys == "distinct" else 1.0
            for n in (512, 4096):
                cursor = count // 3

                def call():
                    return ops.bank_select_weakest(meta, count, NOW, cursor, n)
                iters = 200 if count <= 1_000_000 else 60
                ms = bench.timed_events(call, iters=iters, warm=10)
                call()
                torch.cuda.synchronize()
                reads, later = passes_that_read(ops, dev, count, n)
                nbytes = count * (16 + 4) + (reads - 1) * 4 * count
                res.append({"count": count, "n": n, "keys": keys, "median_us_per_call": 1e3 * ms,
                            "launches_per_call": 1 + selection_passes(count) + 1,        # memset + passes + compaction (+ torch.sort)
                            "passes_after_the_first_that_read_rows": later,
                            "bytes_per_call_from_shapes": nbytes,
                            "share_of_8TBps_peak": nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S})
                print(res[-1], flush=True)
        del meta
        torch.cuda.empty_cache()
    out["select_weakest"] = res


def bench_writes(dev, rows, D, out):
    res = []
    g = torch.Generator(device=dev).manual_seed(5)
    for index in (False, True):
        hf = bench.new_bank(rows, D, dev, use_index=index)
        hf._overflow = "fifo"
        bench.fill_bank(hf, rows, D, 1234, dev)
        if index:
            hf.rebuild_centroids(perm=torch.randperm(rows, generator=torch.Generator().manual_seed(7)))
            hf.recall_batch(torch.randn(2048, D, generator=g, device=dev), k=32)      # builds the inverted lists
        for keys in ("equal", "varied"):
            if keys == "varied":
                hf.memory_metadata[:, 0] = 0.25 + 0.75 * torch.rand(rows, generator=g, device=dev)
            for batch in (512, 4096):
                n_batches = 24 if batch == 512 else 8
                feats = torch.randn(batch, D, generator=g, device=dev)
                ids = [f"w{i}" for i in range(batch)]

                def burst():
                    for _ in range(n_batches):
                        hf.create_episodic_memories(ids, feats)
                rates = {"fifo": [], "weakest": []}
                for policy in ("fifo", "weakest"):                                     # warm-up of both paths
                    hf._overflow = policy
                    burst()
                torch.cuda.synchronize()
                for rnd in range(7):
                    for policy in (("fifo", "weakest") if rnd % 2 == 0 else ("weakest", "fifo")):
                        hf._overflow = policy
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        burst()
                        torch.cuda.synchronize()
                        rates[policy].append(n_batches * batch / (time.perf_counter() - t0))
                med = {p: statistics.median(v) for p, v in rates.items()}
                res.append({"rows": rows, "dim": D, "index": index, "keys": keys, "batch": batch,
                            "fifo_rows_per_s": med["fifo"], "fifo_min_max": [min(rates["fifo"]), max(rates["fifo"])],
                            "weakest_rows_per_s": med["weakest"],
                            "weakest_min_max": [min(rates["weakest"]), max(rates["weakest"])],
                            "weakest_over_fifo": med["weakest"] / med["fifo"]})
                print(res[-1], flush=True)
        del hf
        torch.cuda.empty_cache()
    out["full_bank_write"] = res


def bench_recall(dev, rows, D, out):
    nq, k = 2048, 32
    hf = bench.new_bank(rows, D, dev)
    bench.fill_bank(hf, rows, D, 1234, dev)
    hf.rebuild_centroids(perm=torch.randperm(rows, generator=torch.Generator().manual_seed(7)))
    now = float(hf.memory_metadata[0, 1].item())
    g = torch.Generator(device=dev).manual_seed(99)
    pick = torch.randint(0, rows, (nq // 2,), generator=g, device=dev)
    q = torch.cat([hf.memory_features[pick] + 0.05 * torch.randn(nq // 2, D, generator=g, device=dev),
                   torch.randn(nq - nq // 2, D, generator=g, device=dev)]).contiguous()
    hf.decay_memories(0.2)                                             # below the cap: a reinforcement does change strengths

    def plain():
        return hf.recall_batch(q, k=k, now=now)

    def reinforced():
        # cap far away: every call adds, so every following recall rebuilds the lists' cached score constants
        return hf.recall_batch(q, k=k, now=now, reinforce=1e-4, reinforce_cap=1e9)
    for _ in range(10):
        plain()
    reinforced()
    a, b = [], []
    for rnd in range(9):
        for which in ((plain, reinforced) if rnd % 2 == 0 else (reinforced, plain)):
            (a if which is plain else b).append(bench.timed_events(which, iters=30, warm=3))
    ma, mb = statistics.median(a), statistics.median(b)
    out["recall"] = {"rows": rows, "dim": D, "queries": nq, "k": k, "index": True,
                     "reinforce_none_ms_per_call": ma, "reinforce_none_min_max_ms": [min(a), max(a)],
                     "reinforce_ms_per_call": mb, "reinforce_min_max_ms": [min(b), max(b)],
                     "added_ms_per_call_with_reinforce": mb - ma,
                     "note": "each figure: median over 9 alternated rounds of the median of 30 event-timed calls; with "
                             "reinforce the added time is the reinforce launch plus the rebuild of the inverted lists' "
                             "cached score constants that the changed strengths force on the next recall"}
    print(out["recall"], flush=True)
    del hf
    torch.cuda.empty_cache()


def write_workload(dev, rows, D):
    """The workload of profiles/retention_write_kernel_stats.csv: 45 full-bank 'weakest' writes of 4096 rows, index
    off, varied strengths -- to be run under ``rocprofv3 --kernel-trace --stats -- python tools/retention_bench.py
    --only write-trace`` (a run of its own: tracing slows the host)."""
    g = torch.Generator(device=dev).manual_seed(5)
    hf = bench.new_bank(rows, D, dev, use_index=False)
    hf._overflow = "weakest"
    bench.fill_bank(hf, rows, D, 1234, dev)
    hf.memory_metadata[:, 0] = 0.25 + 0.75 * torch.rand(rows, generator=g, device=dev)
    feats = torch.randn(4096, D, generator=g, device=dev)
    ids = [f"w{i}" for i in range(4096)]
    for _ in range(45):
        hf.create_episodic_memories(ids, feats)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retention_bench.json"))
    ap.add_argument("--only", choices=("select", "write", "recall", "write-trace"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retention_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    from aura_snn_rag_amd import ops
    dev = torch.device("cuda", 0)
    if a.only == "write-trace":
        write_workload(dev, a.rows, a.dim)
        return
    out = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s_assumed": PEAK_BYTES_PER_S}
    if a.only in (None, "select"):
        bench_select(ops, dev, out)
    if a.only in (None, "write"):
        bench_writes(dev, a.rows, a.dim, out)
    if a.only in (None, "recall"):
        bench_recall(dev, a.rows, a.dim, out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
