"""Measurements of diverse recall -> profiles/diverse_recall_bench.json.

    python tools/diverse_bench.py [--rows 1000000] [--dim 768] [--queries 2048] [--out profiles/diverse_recall_bench.json]

Needs a GPU (no fallback).  One process, one bank (index on, rebuilt), two shapes -- (k = 32, F = 128) and
(k = 5, F = 32) -- with diversity = 0.5 and max_similarity = 0.9.  Every shape is warmed up first; every figure is the
median over WINDOWS windows of at least 0.5 s of work each (the spread over the windows beside it), the things
compared taken in alternating order inside each round:

  recall_k        recall_batch(k)                     the plain call                          (host clock + synchronise)
  recall_F        recall_batch(k=F)                   the fetch the diverse call starts with  (host clock + synchronise)
  diverse         recall_batch(k, diversity, max_similarity, fetch_k=F)                       (host clock + synchronise)
  select_kernel   ops.diverse_select alone on the F candidates                                (device events)
  torch_baseline  the same selection composed from torch ops on the same GPU: bank_gather -> [nq, F, D], scaled by
                  inv_norm, bmm -> [nq, F, F], a loop of k steps                              (device events)

The picks of the kernel AND of the torch composition are replayed against the rule in fp64 on the CPU for the first
CHECKED queries (tests/cpu_stub_diverse.replay_check: check 1 of the GPU tests) before anything is timed.  The kernel
must be faster than the composition at both shapes or the tool exits non-zero.  Bytes and FLOP come from the shapes:
the F rows of every query read once (4 nq F D bytes) and the full F x F Gram (2 nq F^2 D FLOP), against 8 TB/s and the
157.3 TFLOP/s fp32 matrix peak.

``--only trace``: the workload of profiles/diverse_select_kernel_stats.csv (the selection alone, both shapes), to be
run under ``rocprofv3 --kernel-trace --stats -- python tools/diverse_bench.py --only trace`` in a run of its own."""
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
PEAK_F32_MATRIX_FLOPS = 157.3e12
WINDOWS = 7
WINDOW_S = 0.5
CHECKED = 256
SHAPES = ((32, 128), (5, 32))
DIVERSITY, MAX_SIMILARITY = 0.5, 0.9


def torch_select(ops, bank, inv_norm, cand_rows, cand_scores, k, d, tau):
    """The rule from torch ops: what a caller without the kernel would write."""
    nq, F = cand_rows.shape
    valid = cand_rows >= 0
    idx = cand_rows.clamp(min=0).long()
    x = ops.bank_gather(bank, cand_rows) * (inv_norm[idx] * valid).unsqueeze(-1)           # [nq, F, D]
    gram = torch.bmm(x, x.transpose(1, 2))                                                 # [nq, F, F]
    ar = torch.arange(nq, device=bank.device)
    neg = torch.full_like(cand_scores, float("-inf"))
    picked = torch.zeros_like(valid)
    m = neg.clone()
    out_r = torch.full((nq, k), -1, dtype=torch.int32, device=bank.device)
    out_s = torch.full((nq, k), float("-inf"), device=bank.device)
    alive = torch.ones(nq, dtype=torch.bool, device=bank.device)
    for s in range(k):
        elig = valid & ~picked & ((m < tau) if s else valid)
        val = torch.where(elig, (1.0 - d) * cand_scores - (d * m if s else 0.0), neg)
        best = val.argmax(1)
        alive = alive & elig.any(1)
        out_r[:, s] = torch.where(alive, cand_rows[ar, best], out_r[:, s])
        out_s[:, s] = torch.where(alive, cand_scores[ar, best], out_s[:, s])
        picked[ar, best] |= alive
        m = torch.where(alive.unsqueeze(1), torch.maximum(m, gram[ar, best]), m)
    return out_s, out_r


def events_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wall_window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def alternated(fns, window):
    """{name: [ms per call, one per window]} -- WINDOWS rounds, the order of the candidates reversed every round."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        ms = window(fn, 3)
        iters[name] = max(3, int(WINDOW_S * 1e3 / max(ms, 1e-3)) + 1)
    out = {name: [] for name in fns}
    names = list(fns)
    for rnd in range(WINDOWS):
        for name in (names if rnd % 2 == 0 else names[::-1]):
            out[name].append(window(fns[name], iters[name]))
    return out, iters


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "windows": len(ms)}


def setup(dev, rows, D, nq):
    hf = bench.new_bank(rows, D, dev)
    bench.fill_bank(hf, rows, D, 1234, dev)
    hf.rebuild_centroids(perm=torch.randperm(rows, generator=torch.Generator().manual_seed(7)))
    now = float(hf.memory_metadata[0, 1].item())
    g = torch.Generator(device=dev).manual_seed(99)
    pick = torch.randint(0, rows, (nq // 2,), generator=g, device=dev)
    q = torch.cat([hf.memory_features[pick] + 0.05 * torch.randn(nq // 2, D, generator=g, device=dev),
                   torch.randn(nq - nq // 2, D, generator=g, device=dev)]).contiguous()
    return hf, q, now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_recall_bench.json"))
    ap.add_argument("--only", choices=("trace",), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diverse_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    from aura_snn_rag_amd import ops
    from tests import cpu_stub_diverse as R
    dev = torch.device("cuda", 0)
    hf, q, now = setup(dev, a.rows, a.dim, a.queries)
    nq, D = q.shape
    if a.only == "trace":
        for k, F in SHAPES:
            cs, cr = hf.recall_batch(q, k=F, now=now)
            for _ in range(50):
                ops.diverse_select(hf.memory_features, hf._inv_norm, hf.memory_count, cr, cs, k, DIVERSITY, MAX_SIMILARITY)
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": D, "queries": nq, "index": True,
           "diversity": DIVERSITY, "max_similarity": MAX_SIMILARITY, "windows": WINDOWS, "window_s_at_least": WINDOW_S,
           "peak_bytes_per_s_assumed": PEAK_BYTES_PER_S, "peak_f32_matrix_flops_assumed": PEAK_F32_MATRIX_FLOPS,
           "shapes": []}
    ok = True
    for k, F in SHAPES:
        cs, cr = hf.recall_batch(q, k=F, now=now)

        def kernel():
            return ops.diverse_select(hf.memory_features, hf._inv_norm, hf.memory_count, cr, cs, k, DIVERSITY, MAX_SIMILARITY)

        def baseline():
            return torch_select(ops, hf.memory_features, hf._inv_norm, cr, cs, k, DIVERSITY, MAX_SIMILARITY)
        # both candidates' picks against the rule in fp64 (check 1), on the first CHECKED queries
        n = min(CHECKED, nq)
        cos = R.cosines(hf.memory_features, hf._inv_norm, cr[:n], hf.memory_count)
        tol = R.tolerance(D)
        ks, kr = kernel()
        bs, br = baseline()
        R.replay_check(cr[:n], cs[:n], cos, hf.memory_count, k, DIVERSITY, MAX_SIMILARITY, ks[:n], kr[:n], tol)
        R.replay_check(cr[:n], cs[:n], cos, hf.memory_count, k, DIVERSITY, MAX_SIMILARITY, bs[:n], br[:n], tol)
        same = int((kr == br).all(1).sum())
        sel, sel_iters = alternated({"select_kernel": kernel, "torch_baseline": baseline}, events_window)
        e2e, e2e_iters = alternated({
            "recall_k": lambda: hf.recall_batch(q, k=k, now=now),
            "recall_F": lambda: hf.recall_batch(q, k=F, now=now),
            "diverse": lambda: hf.recall_batch(q, k=k, now=now, diversity=DIVERSITY, max_similarity=MAX_SIMILARITY,
                                               fetch_k=F)}, wall_window)
        nbytes = 4 * nq * F * D
        flop = 2 * nq * F * F * D
        floor_ms = 1e3 * max(nbytes / PEAK_BYTES_PER_S, flop / PEAK_F32_MATRIX_FLOPS)
        km, bm = statistics.median(sel["select_kernel"]), statistics.median(sel["torch_baseline"])
        res = {"k": k, "F": F, "checked_queries": n, "queries_with_the_same_picks_as_the_torch_composition": same,
               "select_kernel": summary(sel["select_kernel"]), "torch_baseline": summary(sel["torch_baseline"]),
               "torch_baseline_over_kernel": bm / km,
               "recall_k": summary(e2e["recall_k"]), "recall_F": summary(e2e["recall_F"]), "diverse": summary(e2e["diverse"]),
               "diverse_minus_recall_k_ms": statistics.median(e2e["diverse"]) - statistics.median(e2e["recall_k"]),
               "calls_per_window": {**sel_iters, **e2e_iters},
               "bytes_from_shapes": nbytes, "flop_from_shapes": flop,
               "bound": "matrix pipe" if flop / PEAK_F32_MATRIX_FLOPS > nbytes / PEAK_BYTES_PER_S else "HBM",
               "floor_ms": floor_ms, "floor_over_kernel": floor_ms / km}
        print(res, flush=True)
        out["shapes"].append(res)
        ok = ok and km < bm
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    if not ok:
        raise SystemExit("the selection kernel was not faster than the torch composition")


if __name__ == "__main__":
    main()
