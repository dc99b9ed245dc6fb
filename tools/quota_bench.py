"""Measurements of per-tag quotas -> profiles/tag_quota_bench.json.

    python tools/quota_bench.py [--rows 1000000] [--dim 768] [--out profiles/tag_quota_bench.json] [--only selection|writes]

Needs a GPU (no fallback).  One process.  Every figure is the median over WINDOWS windows of at least WINDOW_S of work
each (min and max beside it), after a warm-up, the things compared taken in alternating order inside each round
(tools/diverse_bench.py's scheme), host clock with a synchronise at both ends of a window.

  selection   a metadata table of ``rows`` rows, tags 1 .. 64 dealt round-robin, under two key profiles: "distinct"
              (random strengths: a selection is decided by the key digits) and "tied" (4 strengths x 3 timestamps: every
              threshold falls inside a tie and the row digits decide).  ``ops.bank_select_weakest_scoped`` of 4096 victims
              over 64 scopes (64 each, origins spread over the bank) against ``ops.bank_select_weakest(n=4096)`` on the
              same table.  No host read on either side.
              The bar: the unscoped call's median plus the time to stream the extra bytes the scoped passes read and
              write (40 B per row, at 6.3 TB/s); the margin: the unscoped call's own spread (max - min).
  writes      a full bank ``rows`` x ``dim`` under overflow='weakest' without a centroid index, every tag holding
              rows / 64 memories; ``create_episodic_memories`` of 512 and of 4096 rows with random tags 1 .. 64, on a bank
              whose tags are all AT their quota (every row replaces a row of its own tag) and on the same bank without
              quotas (every row replaces the bank's weakest).
              The bar: the quotas-off time per batch of the same session; the margin: its spread (max - min) plus one
              device-to-host read (35 us) per run.
  Exit status 1 when a bar is missed; the figures are written either way."""
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

COPY_BYTES_PER_S = 6.3e12
EXTRA_BYTES_PER_ROW = 40.0                    # 80 B per row against the unscoped selection's 40
HOST_READ_MS = 0.035
N_TAGS = 64
VICTIMS = 4096
NOW = 1.7e9


def selection(rows, dev, out, missed):
    from aura_snn_rag_amd import ops
    g = torch.Generator(device=dev).manual_seed(11)
    meta = torch.zeros(rows, 4, device=dev)
    meta[:, 2] = -1
    meta[:, 3] = (1 + torch.arange(rows, device=dev) % N_TAGS).float()
    scope_tags = list(range(1, N_TAGS + 1))
    per = VICTIMS // N_TAGS
    held = [int(((torch.arange(rows) % N_TAGS) == s).sum()) for s in range(N_TAGS)]
    origins = [(s * rows) // N_TAGS for s in range(N_TAGS)]
    incoming = [per] * N_TAGS
    for profile in ("distinct", "tied"):
        if profile == "distinct":
            meta[:, 0] = 0.25 + 0.75 * torch.rand(rows, generator=g, device=dev)
            meta[:, 1] = float(np.float32(NOW)) - 128.0 * torch.randint(0, 64, (rows,), generator=g, device=dev).float()
        else:
            meta[:, 0] = (1 + torch.randint(0, 4, (rows,), generator=g, device=dev)).float() / 4
            meta[:, 1] = float(np.float32(NOW)) - 1280.0 * torch.randint(0, 3, (rows,), generator=g, device=dev).float()
        packed, _ = ops.bank_select_weakest_scoped(meta, rows, NOW, scope_tags, origins, incoming, held)
        _, x, victims = ops.scoped_selection_decode(packed.cpu(), incoming)
        assert x.tolist() == incoming and all(v.size == per for v in victims)
        ms, iters = alternated({
            "scoped": lambda: ops.bank_select_weakest_scoped(meta, rows, NOW, scope_tags, origins, incoming, held),
            "unscoped": lambda: ops.bank_select_weakest(meta, rows, NOW, 0, VICTIMS)}, wall_window)
        med = {k: statistics.median(v) for k, v in ms.items()}
        extra_ms = 1e3 * EXTRA_BYTES_PER_ROW * rows / COPY_BYTES_PER_S
        margin = max(ms["unscoped"]) - min(ms["unscoped"])
        res = {**{k: summary(v) for k, v in ms.items()}, "calls_per_window": iters, "extra_bytes": EXTRA_BYTES_PER_ROW * rows,
               "extra_stream_ms": extra_ms, "bar_ms": med["unscoped"] + extra_ms, "margin_ms": margin,
               "scoped_over_unscoped": med["scoped"] / med["unscoped"]}
        print("selection", profile, res, flush=True)
        out["selection"][profile] = res
        if med["scoped"] > med["unscoped"] + extra_ms + margin:
            missed.append(f"selection/{profile}: scoped {med['scoped']:.4f} ms, bar {med['unscoped'] + extra_ms:.4f} ms "
                          f"+ margin {margin:.4f} ms")


def writes(rows, D, dev, out, missed):
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    g = torch.Generator(device=dev).manual_seed(12)

    def bank(quota):
        hf = HippocampalFormation(feature_dim=D, max_memories=rows, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", use_centroid_index=False, overflow="weakest", tag_quota=quota)
        chunk = 1 << 17
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            hf.bulk_write(torch.randn(n, D, generator=g, device=dev), rebuild=False,
                          tags=1 + (np.arange(r0, r0 + n) % N_TAGS))
        return hf
    counts = np.bincount(1 + (np.arange(rows) % N_TAGS), minlength=N_TAGS + 1)
    banks = {"quotas_on": bank({t: int(counts[t]) for t in range(1, N_TAGS + 1)}), "quotas_off": bank(None)}
    serial = [0]
    for batch in (512, 4096):
        feats = torch.randn(batch, D, generator=g, device=dev)
        tags = torch.randint(1, N_TAGS + 1, (batch,), generator=torch.Generator().manual_seed(batch)).numpy()

        def write(hf):
            serial[0] += 1
            hf.create_episodic_memories([f"w{serial[0]}-{i}" for i in range(batch)], feats, tags=tags)
        ms, iters = alternated({name: (lambda hf=hf: write(hf)) for name, hf in banks.items()}, wall_window)
        med = {k: statistics.median(v) for k, v in ms.items()}
        margin = max(ms["quotas_off"]) - min(ms["quotas_off"]) + HOST_READ_MS
        res = {**{k: summary(v) for k, v in ms.items()}, "calls_per_window": iters,
               "rows_per_s": {k: 1e3 * batch / v for k, v in med.items()}, "margin_ms": margin,
               "on_over_off": med["quotas_on"] / med["quotas_off"]}
        print("writes", batch, res, flush=True)
        out["writes"][str(batch)] = res
        if med["quotas_on"] > med["quotas_off"] + margin:
            missed.append(f"writes/{batch}: quotas on {med['quotas_on']:.4f} ms per batch, off {med['quotas_off']:.4f} ms "
                          f"+ margin {margin:.4f} ms")
    on = banks["quotas_on"]
    assert all(c <= on.tag_quotas[t] for t, c in on.tag_counts().items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tag_quota_bench.json"))
    ap.add_argument("--only", choices=("selection", "writes"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quota_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "tags": N_TAGS, "victims": VICTIMS,
           "windows": WINDOWS, "window_s_at_least": WINDOW_S, "copy_bytes_per_s_assumed": COPY_BYTES_PER_S,
           "host_read_ms_assumed": HOST_READ_MS, "selection": {}, "writes": {}}
    missed = []
    if a.only in (None, "selection"):
        selection(a.rows, dev, out, missed)
    if a.only in (None, "writes"):
        writes(a.rows, a.dim, dev, out, missed)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)
    if missed:
        raise SystemExit("bars missed:\n  " + "\n  ".join(missed))


if __name__ == "__main__":
    main()
