"""Measurements of consolidating writes -> profiles/consolidate_bench.json.

    python tools/consolidate_bench.py [--rows 1000000] [--dim 768] [--out profiles/consolidate_bench.json]

Needs a GPU (no fallback).  One process, one bank (index on, rebuilt, room for the rows the write streams append).
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), after a
warm-up, the things compared taken in alternating order inside each round (tools/diverse_bench.py's scheme).

  per batch size n in (256, 1024), the batch half noisy copies of held rows, half fresh rows:
    find_repeats_kernels   ops.find_repeats on the list-sorted image, launches only            (device events)
    find_repeats           HippocampalFormation.find_repeats: image choice + launches + THE host read     (host clock)
    recall_k1_kernels      recall_batch(k=1, use_candidates=False, check_overflow=False), n queries  (device events)
    recall_k1              recall_batch(k=1, use_candidates=False): the exact two-stage scan of the same bank with the
                           same number of queries, its flag read included -- the bar: find_repeats may take at most
                           1.10 x this                                                                  (host clock)
  Before anything is timed the image scan's result is compared with the dense fp32 scan's on the same batch.
  floors: one pass over the image at the copy rate of DESIGN.md 4.3b (1.54 GB in 271 us) and 2 N n D FLOP at the
  bf16 matrix peak; the fraction of each that find_repeats_kernels reaches is reported.

  write rate, batches of 256 rows appended to the same bank (no centroid rebuild inside the windows), rows / s:
    plain_0 / merge_0      a stream without repeats, without / with merge_similarity = 0.9
    plain_50 / merge_50    a stream whose rows are half noisy copies of held rows
    merge_tagged_0 / merge_tagged_50   the same streams as tagged merging writes (tags=..., merge_within_tags=True): a
                           copy carries the tag of the row it copies, a fresh row one of the 64 tags

  consolidation within tags ("within tags"): the bank's rows carry tags spread evenly over 64 values
  (row r: r % 64); a batch row that repeats a held row carries that row's tag, so both searches find the same repeats.
  Per batch size, alternated in one process on the same bank and batch, the unscoped call taken TWICE (a, b) so that the
  spread of the unscoped measurement itself is known before the two are compared:
    unscoped_a / scoped / unscoped_b                  ops.find_repeats / ops.find_repeats_scoped, launches  (device events)
    call_unscoped_a / call_scoped / call_unscoped_b   HippocampalFormation.find_repeats(tags=None / tags)   (host clock)
  The bar: the scoped search costs what the unscoped one costs -- its median may not exceed the largest window of the
  unscoped call in the same run (the margin is the unscoped call's own spread, nothing else).

  blending merges ("blending"): merging writes with ``merge_blend = 0.5`` next to the same writes without,
  a stream whose rows are half noisy copies of held rows, batches of 256 and of 1024 rows, alternated in one process on
  the same bank, the unblended call taken TWICE (a, b) as above; then ``consolidate(blend=0.5)`` next to
  ``consolidate()`` on fresh banks of ``--consolidate-rows`` bulk-written rows, a fifth of them noisy copies (a pass
  consumes its bank, so every measurement builds one; only the pass is timed).  The bar, both times: the blended median
  may not exceed the largest unblended window of the same run.  ``--only blend`` measures this section alone and
  replaces it in an existing ``--out`` file, leaving the other sections as they were recorded.

``--only trace``: find_repeats alone, both batch sizes, for ``rocprofv3 --kernel-trace --stats -- python
tools/consolidate_bench.py --only trace`` in a run of its own."""
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
from tools.diverse_bench import events_window, wall_window, summary  # noqa: E402

COPY_BYTES_PER_S = 1.54e9 / 271e-6
PEAK_BF16_MATRIX_FLOPS = 2.5e15
WINDOWS = 5
WINDOW_S = 0.3
TAU = 0.9
BATCHES = (256, 1024)
WRITE_BATCH = 256
HEADROOM = 1 << 17
BETA = 0.5
BAR = 1.10
N_TAGS = 64


def alternated(fns, window):
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


def make_batch(hf, n, repeats, g, sources=False):
    """n rows: the first ``repeats`` are held rows + 0.05 randn (cosine about 0.9988), the rest fresh.  ``sources``:
    also the held row every row copies, -1 for a fresh one."""
    D = hf.memory_features.shape[1]
    pick = torch.randint(0, hf.memory_count, (repeats,), generator=g, device=hf.device)
    rows = torch.cat([hf.memory_features[pick] + 0.05 * torch.randn(repeats, D, generator=g, device=hf.device),
                      torch.randn(n - repeats, D, generator=g, device=hf.device)])
    perm = torch.randperm(n, generator=g, device=hf.device)
    rows = rows[perm].contiguous()
    if not sources:
        return rows
    src = torch.cat([pick, torch.full((n - repeats,), -1, dtype=pick.dtype, device=hf.device)])[perm]
    return rows, src


def tags_for(hf, src, g):
    """int32 tags of a batch: a copy carries the tag of the row it copies, a fresh row one of the N_TAGS tags."""
    held = hf.memory_metadata[src.clamp(min=0), 3].to(torch.int32)
    fresh = torch.randint(0, N_TAGS, src.shape, generator=g, device=hf.device, dtype=torch.int32)
    return torch.where(src >= 0, held, fresh).contiguous()


def blend_section(hf, g, consolidate_rows, D, dev):
    """Blended next to unblended merging writes on ``hf``, then consolidate(blend=) next to consolidate()."""
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    res = {"beta": BETA, "repeat_share": 0.5, "writes": [], "batches_per_window": 5}
    serial = [0]
    per_writer = 3 + 5 * WINDOWS

    def writer(n, beta):
        todo = []
        for _ in range(per_writer):
            todo.append(([f"b{serial[0]}-{i}" for i in range(n)], make_batch(hf, n, n // 2, g)))
            serial[0] += 1

        def fn():
            ids, f = todo.pop()
            if beta is None:
                hf.create_episodic_memories(ids, f, merge_similarity=TAU)
            else:
                hf.create_episodic_memories(ids, f, merge_similarity=TAU, merge_blend=beta)
        return fn

    def compare(ms, n=None):
        un = ms["unblended_a"] + ms["unblended_b"]
        med_un, med_bl = statistics.median(un), statistics.median(ms["blended"])
        r = {**{k: summary(v) for k, v in ms.items()}, "unblended_median_ms": med_un, "unblended_min_ms": min(un),
             "unblended_max_ms": max(un), "unblended_spread": (max(un) - min(un)) / med_un, "blended_median_ms": med_bl,
             "blended_over_unblended": med_bl / med_un, "bar_met": med_bl <= max(un)}
        if n is not None:
            r["n"] = n
            r["blended_rows_per_s"] = n / (med_bl * 1e-3 / 5)
            r["unblended_rows_per_s"] = n / (med_un * 1e-3 / 5)
        return r
    for n in BATCHES:
        fns = {"unblended_a": writer(n, None), "blended": writer(n, BETA), "unblended_b": writer(n, None)}
        ms = {name: [] for name in fns}
        for fn in fns.values():
            for _ in range(3):
                fn()
        names = list(fns)
        for rnd in range(WINDOWS):
            for name in (names if rnd % 2 == 0 else names[::-1]):
                ms[name].append(wall_window(fns[name], 5) * 5)          # ms per window of 5 batches
        r = compare(ms, n)
        print(r, flush=True)
        res["writes"].append(r)
    res["bank_rows_at_the_end"] = hf.memory_count
    # ---- consolidate(blend=) next to consolidate(): fresh banks of the same rows
    gc = torch.Generator(device=dev).manual_seed(5)
    base = torch.randn(consolidate_rows - consolidate_rows // 5, D, generator=gc, device=dev)
    pick = torch.randint(0, base.shape[0], (consolidate_rows // 5,), generator=gc, device=dev)
    rows = torch.cat([base, base[pick] + 0.05 * torch.randn(pick.numel(), D, generator=gc, device=dev)])
    rows = rows[torch.randperm(rows.shape[0], generator=gc, device=dev)].contiguous()
    kept = {}

    def one_pass(beta):
        bank = HippocampalFormation(feature_dim=D, max_memories=rows.shape[0], n_place_cells=8, n_time_cells=4,
                                    n_grid_cells=4, device="cuda", use_centroid_index=False)
        bank.bulk_write(rows, rebuild=False)
        bank._ensure_shadow()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = bank.consolidate(TAU) if beta is None else bank.consolidate(TAU, blend=beta)
        torch.cuda.synchronize()
        kept[beta] = (rep.n_kept, rep.n_merged, rep.n_blended)
        return 1e3 * (time.perf_counter() - t0)
    one_pass(None), one_pass(BETA)                                       # warm-up
    ms = {"unblended_a": [], "blended": [], "unblended_b": []}
    order = [("unblended_a", None), ("blended", BETA), ("unblended_b", None)]
    for rnd in range(WINDOWS):
        for name, beta in (order if rnd % 2 == 0 else order[::-1]):
            ms[name].append(one_pass(beta))
    r = compare(ms)
    r.update(rows=int(rows.shape[0]), kept_merged_blended_unblended=kept[None], kept_merged_blended_blended=kept[BETA])
    print(r, flush=True)
    res["consolidate"] = r
    return res


def report_blend(res):
    for r in res["writes"] + [res["consolidate"]]:
        if not r["bar_met"]:
            what = f"merging writes, n = {r['n']}" if "n" in r else "consolidate"
            print(f"blending, {what}: the blended median {r['blended_median_ms']:.4f} ms lies above every unblended "
                  f"window (max {r['unblended_max_ms']:.4f} ms): the bar is MISSED")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consolidate_bench.json"))
    ap.add_argument("--only", choices=("trace", "blend"), default=None)
    ap.add_argument("--consolidate-rows", type=int, default=100_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consolidate_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    dev = torch.device("cuda", 0)
    D = a.dim
    hf = HippocampalFormation(feature_dim=D, max_memories=a.rows + HEADROOM, n_place_cells=8, n_time_cells=4,
                              n_grid_cells=4, device="cuda", use_centroid_index=True)
    hf.centroids_update_interval = 10 ** 9
    bench.fill_bank(hf, a.rows, D, 1234, dev)
    hf.rebuild_centroids(perm=torch.randperm(a.rows, generator=torch.Generator().manual_seed(7)))
    now = float(hf.memory_metadata[0, 1].item())
    # tags spread evenly over N_TAGS values (the unscoped calls do not read them)
    hf.retag(rows=torch.arange(a.rows), tag=torch.arange(a.rows) % N_TAGS)
    g = torch.Generator(device=dev).manual_seed(99)
    batches, batch_tags = {}, {}
    for n in BATCHES:
        batches[n], src = make_batch(hf, n, n // 2, g, sources=True)
        batch_tags[n] = tags_for(hf, src, g)
    if a.only == "trace":
        for n in BATCHES:
            for _ in range(30):
                hf.find_repeats(batches[n], TAU)
        torch.cuda.synchronize()
        return
    if a.only == "blend":
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                out = json.load(fh)
        out["blend"] = dict(blend_section(hf, g, a.consolidate_rows, D, dev), device=torch.cuda.get_device_name(0),
                            rows=a.rows, dim=D, tau=TAU, windows=WINDOWS)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", a.out)
        report_blend(out["blend"])
        return
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": D, "index": True, "tau": TAU,
           "windows": WINDOWS, "window_s_at_least": WINDOW_S, "copy_bytes_per_s_assumed": COPY_BYTES_PER_S,
           "peak_bf16_matrix_flops_assumed": PEAK_BF16_MATRIX_FLOPS, "bar": BAR, "find_repeats": [], "write_rate": {},
           "n_tags": N_TAGS, "find_repeats_within_tags": []}
    ok = True
    for n in BATCHES:
        f = batches[n]
        st, bl, _ = hf.find_repeats(f, TAU)
        ivf = hf._ivf
        assert ivf is not None and ivf.valid, "the bank was expected to scan the list-sorted image"
        dense = ops.find_repeats(hf.memory_features, hf._inv_norm, hf.memory_count, f, TAU)[3].cpu()
        same = bool(torch.equal(dense[:n], st)) and bool(torch.equal(dense[n:2 * n], bl))
        image_bytes = ivf.n_sorted * D * 2

        def kernels():
            return ops.find_repeats(hf.memory_features, hf._inv_norm, hf.memory_count, f, TAU, image=ivf.sorted_bf16,
                                    image_rows=ivf.sorted_rows, n_image=ivf.n_sorted, rho=hf._rho, rho16=hf._rho16,
                                    lists_flag=ivf.flag)
        ev, ev_iters = alternated({
            "find_repeats_kernels": kernels,
            "recall_k1_kernels": lambda: hf.recall_batch(f, k=1, now=now, use_candidates=False, check_overflow=False)},
            events_window)
        wl, wl_iters = alternated({
            "find_repeats": lambda: hf.find_repeats(f, TAU),
            "recall_k1": lambda: hf.recall_batch(f, k=1, now=now, use_candidates=False)}, wall_window)
        km = statistics.median(ev["find_repeats_kernels"])
        fr, rc = statistics.median(wl["find_repeats"]), statistics.median(wl["recall_k1"])
        floor_bytes_ms = 1e3 * image_bytes / COPY_BYTES_PER_S
        floor_flop_ms = 1e3 * 2.0 * ivf.n_sorted * n * D / PEAK_BF16_MATRIX_FLOPS
        res = {"n": n, "repeats_in_batch": int((st >= 0).sum()), "image_rows": ivf.n_sorted, "image_bytes": image_bytes,
               "image_scan_equals_dense_scan": same,
               **{k: summary(v) for k, v in {**ev, **wl}.items()}, "calls_per_window": {**ev_iters, **wl_iters},
               "find_repeats_over_recall_k1": fr / rc, "bar_met": fr <= BAR * rc,
               "kernels_over_recall_k1_kernels": km / statistics.median(ev["recall_k1_kernels"]),
               "floor_image_pass_ms": floor_bytes_ms, "floor_matrix_pipe_ms": floor_flop_ms,
               "fraction_of_image_pass_floor": floor_bytes_ms / km, "fraction_of_matrix_pipe_floor": floor_flop_ms / km}
        print(res, flush=True)
        out["find_repeats"].append(res)
        ok = ok and same
        # ---- the same batch within tags, next to the unscoped call (taken twice: its own spread is the margin)
        bt = batch_tags[n]
        st_s, bl_s, _ = hf.find_repeats(f, TAU, tags=bt)
        same_s = bool(torch.equal(st_s, st)) and bool(torch.equal(bl_s, bl))      # (every repeat carries its target's tag)

        def kernels_scoped():
            return ops.find_repeats_scoped(hf.memory_features, hf._inv_norm, hf.memory_metadata, hf.memory_count, f, bt,
                                           TAU, image=ivf.sorted_bf16, image_rows=ivf.sorted_rows, n_image=ivf.n_sorted,
                                           rho=hf._rho, rho16=hf._rho16, lists_flag=ivf.flag)
        ev, ev_iters = alternated({"unscoped_a": kernels, "scoped": kernels_scoped, "unscoped_b": kernels}, events_window)
        wl, wl_iters = alternated({"call_unscoped_a": lambda: hf.find_repeats(f, TAU),
                                   "call_scoped": lambda: hf.find_repeats(f, TAU, tags=bt),
                                   "call_unscoped_b": lambda: hf.find_repeats(f, TAU)}, wall_window)
        res = {"n": n, "scoped_equals_unscoped_on_this_batch": same_s,
               **{k: summary(v) for k, v in {**ev, **wl}.items()}, "calls_per_window": {**ev_iters, **wl_iters}}
        for key, (a_, s_, b_) in {"kernels": ("unscoped_a", "scoped", "unscoped_b"),
                                  "call": ("call_unscoped_a", "call_scoped", "call_unscoped_b")}.items():
            both = {**ev, **wl}
            un = both[a_] + both[b_]
            med_un, med_sc = statistics.median(un), statistics.median(both[s_])
            res[key] = {"unscoped_median_ms": med_un, "unscoped_min_ms": min(un), "unscoped_max_ms": max(un),
                        "unscoped_a_over_b": statistics.median(both[a_]) / statistics.median(both[b_]),
                        "unscoped_spread": (max(un) - min(un)) / med_un, "scoped_median_ms": med_sc,
                        "scoped_over_unscoped": med_sc / med_un, "bar_met": med_sc <= max(un)}
        print(res, flush=True)
        out["find_repeats_within_tags"].append(res)
        ok = ok and same_s
    # ---- write rate
    serial = [0]

    per_writer = 3 + 5 * WINDOWS                   # warm-up calls + timed calls of one writer

    def writer(repeats, tau, tagged=False):
        # batches and ids are made BEFORE the windows: only the write is timed.  (Copies are taken of rows held now;
        # the rows the streams append in between are fresh ones.)
        todo = []
        for _ in range(per_writer):
            f, src = make_batch(hf, WRITE_BATCH, repeats, g, sources=True)
            tags = tags_for(hf, src, g).cpu().numpy() if tagged else None
            todo.append(([f"w{serial[0]}-{i}" for i in range(WRITE_BATCH)], f, tags))
            serial[0] += 1

        def fn():
            ids, f, tags = todo.pop()
            if tagged:
                hf.create_episodic_memories(ids, f, merge_similarity=tau, tags=tags, merge_within_tags=True)
            else:
                hf.create_episodic_memories(ids, f, merge_similarity=tau)
        return fn
    wr, wr_iters = {}, {}
    for share, rep in (("0", 0), ("50", WRITE_BATCH // 2)):
        fns = {f"plain_{share}": writer(rep, None), f"merge_{share}": writer(rep, TAU),
               f"merge_tagged_{share}": writer(rep, TAU, tagged=True)}
        for name, fn in fns.items():
            for _ in range(3):
                fn()
            wr_iters[name] = 5
            wr[name] = []
        names = list(fns)
        for rnd in range(WINDOWS):
            for name in (names if rnd % 2 == 0 else names[::-1]):
                wr[name].append(wall_window(fns[name], wr_iters[name]))
    for name, ms in wr.items():
        s = summary(ms)
        s["rows_per_s"] = WRITE_BATCH / (s["median_ms"] * 1e-3)
        out["write_rate"][name] = s
    out["write_rate"]["batch"] = WRITE_BATCH
    out["write_rate"]["batches_per_window"] = 5
    out["write_rate"]["bank_rows_at_the_end"] = hf.memory_count
    for share in ("0", "50"):
        out["write_rate"][f"merge_over_plain_{share}"] = (out["write_rate"][f"merge_{share}"]["median_ms"] /
                                                          out["write_rate"][f"plain_{share}"]["median_ms"])
        out["write_rate"][f"merge_tagged_over_merge_{share}"] = (out["write_rate"][f"merge_tagged_{share}"]["median_ms"] /
                                                                 out["write_rate"][f"merge_{share}"]["median_ms"])
    print(out["write_rate"], flush=True)
    out["blend"] = blend_section(hf, g, a.consolidate_rows, D, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)
    if not ok:
        raise SystemExit("the image scan and the dense scan disagree")
    for r in out["find_repeats_within_tags"]:
        for key in ("kernels", "call"):
            if not r[key]["bar_met"]:
                print(f"within tags, n = {r['n']}, {key}: the scoped median {r[key]['scoped_median_ms']:.4f} ms lies above "
                      f"every unscoped window (max {r[key]['unscoped_max_ms']:.4f} ms): the bar is MISSED")
    report_blend(out["blend"])
    missed = [r["n"] for r in out["find_repeats"] if not r["bar_met"]]
    if missed:
        raise SystemExit(f"find_repeats takes more than {BAR} x recall_batch(k=1, use_candidates=False) at n = {missed}")


if __name__ == "__main__":
    main()
