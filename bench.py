#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X.

Metric (BASELINE.json): retrievals/s of the episodic cosine-kNN at a 1M x 768 bank.  One "step" =
one batch of queries per rank recalled through the PRODUCT API (``HippocampalFormation.recall_batch``
with its defaults: centroid-index recall -- the 8 nearest of 256 centroids, hippocampal.py:259-270 --
and the per-call overflow check), inputs resident in HBM.

  N = 1  : 1 000 000 x 768 fp32 bank on one GPU, 2048-query batches, top-32.
  N > 1  : BASELINE config 4 -- the same bank row-sharded over N ranks (1M / N rows each, the centroid
           table replicated); every rank brings its own 2048-query batch; a step = all-gather the
           queries (RCCL), recall on the local shard for all N*2048 of them, all-gather the per-shard
           top-k, merge (``sharded.ShardedHippocampus``).  value = N*2048*steps / time.

A plain run sets up, warms up, times ``--steps`` steps and prints one JSON line (``ms_per_step`` = wall
milliseconds of one timed step).  ``--dump-outputs DIR`` writes what the last timed step returned
(``scores.npy`` float32, ``rows.npy`` as float64) for output-for-output comparisons between builds; the bank,
its timestamps and the queries are seeded, so the inputs are the same from run to run.

``--full`` adds, on the same JSON line: `roofline` of the dominant kernel (the bf16 prefilter over the
list-sorted shadow, timed with HIP events on its launch stream via aura_profile_* in a pass of its own after
the timed steps), `cpu_baseline` (the oracle's reference-cost recall on the same bank, a handful of queries,
with the parity of the GPU result on those queries) and `secondary` (exact recall at 1M, recall@k of the
index, config 2, rebuild / interleaved-write timings, config 5 seeding, neuron-timestep throughput).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
MFMA_F32_PEAK_TF = 157.3    # fp32 matrix peak (v_mfma_f32_32x32x2_f32), dense
# every bank row gets this write time (fp32-exact; the write path stamps wall-clock time, whose fp32 value
# moves in 128 s steps and could land two chunks of one fill in different steps)
BENCH_WRITE_TIME = 1.7e9
PMC_FILE = os.path.join(ROOT, "profiles", "r03_pmc_per_dispatch.json")
KERNEL_OF_KIND = {0: "knn_scan_filter_v2<true, true>",
                  1: "coarse_scan_kernel<24, 1, false, false, false, 4>",
                  2: "coarse_scan_kernel<24, 1, true, false, false, 8>",
                  3: "coarse_scan_kernel<24, 1, true, false, true, 8>"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bank-rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=2048, help="queries per rank and step")
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--exact", action="store_true", help="headline = exact recall instead of the centroid index")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true")
    ap.add_argument("--cpu-queries", type=int, default=64)
    ap.add_argument("--c5-rows", type=int, default=10_000_000, help="rows of the config-5 seeding secondary (0: skip)")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline pass, the CPU baseline and the secondaries (--no-cpu-baseline / "
                         "--no-secondary deselect the last two)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's scores and rows as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def new_bank(rows, dim, dev, use_index=True):
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    return HippocampalFormation(feature_dim=dim, max_memories=rows, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                device="cuda", use_centroid_index=use_index)


def fill_bank(hf, rows, dim, seed, dev, dtype=torch.float32, chunk=1 << 17):
    """Synthetic random embeddings, generated on the device in chunks and written through bulk_write."""
    g = torch.Generator(device=dev).manual_seed(seed)
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        hf.bulk_write(torch.randn(n, dim, generator=g, device=dev, dtype=torch.float32).to(dtype), rebuild=False)


def timed_events(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    st = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    en = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
    for i in range(iters):
        st[i].record(); fn(); en[i].record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in zip(st, en))
    return ms[len(ms) // 2]


def timed_wall(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def profiled(lib, fn, iters, warm=3):
    """(seconds per call, mean HIP-event ms of the dominant scan launch, launches per call, kind, rows, nq)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    lib.aura_profile_begin(max(1, iters * 16))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    buf = (ctypes.c_float * (iters * 16))()
    n = lib.aura_profile_end(buf, iters * 16)
    kms = sum(buf[i] for i in range(n)) / max(n, 1)
    rows_c, nq_c = ctypes.c_int64(0), ctypes.c_int64(0)
    lib.aura_profile_last_scan(ctypes.byref(rows_c), ctypes.byref(nq_c))
    return dt, kms, n / iters, lib.aura_profile_last_scan_kind(), rows_c.value, nq_c.value


def pmc_traffic(kernel, config_key):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (profiles/r03_*; PMC and
    timing runs are never mixed).  FETCH_SIZE counts half of a wide streaming read on gfx950
    (MI355X_MICROARCH.md): 2 * FETCH_SIZE + WRITE_SIZE, both in KiB."""
    try:
        d = json.load(open(PMC_FILE)).get(config_key, {}).get(kernel, {})
        if "FETCH_SIZE" in d and "WRITE_SIZE" in d:
            return (2.0 * d["FETCH_SIZE"] + d["WRITE_SIZE"]) * 1024.0
    except Exception:
        pass
    return None


def ivf_issued_flop(hf, q, D):
    """bf16 MFMA FLOP one inverted-list filter launch ISSUES for the batch `q`: per (list, block of <= 256 probing
    queries) every 16-row tile of the list is multiplied against the 16-query column blocks that hold a query
    (a wave owns 32 query slots and runs ceil(its queries / 16) column blocks; coarse_scan_kernel), k padded to a
    multiple of 32.  Also returns the USEFUL FLOP (list rows x probing queries x 2 D)."""
    ids = hf.probe(q)
    ivf = hf._ivf
    if ids is None or ivf is None or not ivf.valid:
        return None, None
    cnt = torch.bincount(ids.flatten().long().clamp_(0, 255), minlength=256).cpu().tolist()
    lens = ivf.list_len.cpu().tolist()
    kpad = (D + 31) // 32 * 32
    issued = useful = 0
    for c in range(256):
        tiles = (lens[c] + 15) // 16
        left = cnt[c]
        useful += 2 * D * lens[c] * cnt[c]
        while left > 0:
            nb = min(left, 256)
            cols = sum(16 * ((min(max(nb - 32 * w, 0), 32) + 15) // 16) for w in range(8))
            issued += 2 * kpad * 16 * tiles * cols
            left -= nb
    return float(issued), float(useful)


def hbm_roofline(kind, kms, launches_per_step, rows, D, nq_launch, config_key, issued_flop=None, useful_flop=None):
    """Roofline of the dominant (prefilter) launch.  Algorithmic bytes: every row once -- 2 D (bf16 shadow)
    or 4 D (fp32 rows) + 16 B of row constants."""
    if kms <= 0:
        return None
    if kind == 0:
        flop = 2.0 * nq_launch * rows * D
        tf = flop / (kms * 1e-3) / 1e12
        return {"bound": "mfma", "kernel": KERNEL_OF_KIND[0] + " (v_mfma_f32_32x32x2_f32, fp32 in / fp32 acc)",
                "achieved": tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_F32_PEAK_TF,
                "avg_kernel_ms": kms, "launches_per_step": launches_per_step, "algorithmic_flop_per_launch": flop,
                "traffic": pmc_traffic(KERNEL_OF_KIND[0], config_key)}
    esz = 4 if kind == 1 else 2
    nbytes = rows * (D * esz + 16)
    gbs = nbytes / (kms * 1e-3) / 1e9
    if issued_flop is None and kind in (1, 2):
        # full scan: every 256-query block multiplies every row (padded query columns and k included)
        issued_flop = 2.0 * ((nq_launch + 255) // 256 * 256) * rows * ((D + 31) // 32 * 32)
        useful_flop = 2.0 * nq_launch * rows * D
    out = {"bound": "hbm", "kernel": KERNEL_OF_KIND[kind] + " (rows streamed once by global_load_lds, "
           "v_mfma_f32_16x16x32_bf16 against register-resident query fragments)",
           "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
           "avg_kernel_ms": kms, "launches_per_step": launches_per_step, "rows_per_launch": rows,
           "queries_per_launch": nq_launch, "algorithmic_bytes_per_launch": nbytes,
           "traffic": pmc_traffic(KERNEL_OF_KIND[kind], config_key),
           "traffic_source": "profiles/r03_pmc_per_dispatch.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes), key "
                             + config_key}
    if issued_flop:
        out["bf16_mfma_flop_issued_per_launch"] = issued_flop
        out["bf16_tflops_issued"] = issued_flop / (kms * 1e-3) / 1e12
        out["bf16_tflops_issued_frac_of_2500"] = out["bf16_tflops_issued"] / 2500.0
        out["bf16_flop_useful_per_launch"] = useful_flop
    return out


def recall_at(r_pruned, r_exact, ks=(1, 5, 32)):
    out = {}
    for kk in ks:
        kk = min(kk, r_exact.shape[1])
        hit = (r_pruned[:, :kk].unsqueeze(2) == r_exact[:, :kk].unsqueeze(1)).any(dim=2).float().mean().item()
        out[f"recall@{kk}"] = hit
    return out


# ------------------------------------------------------------------------------------------------
# secondaries
# ------------------------------------------------------------------------------------------------
def secondary_neurons(dev):
    """Fused neuron-loop throughput: Izhikevich 2^22 x 100 (both layouts), the GIF loop of one SNNFFN
    layer at config 3 (bf16), the whole spiking FFN of config 3."""
    from aura_snn_rag_amd import ops
    res = {}
    N, T = 1 << 22, 100
    I = 20 * torch.rand(N, T, device=dev)
    S = torch.empty_like(I)
    v = torch.full((N,), -65.0, device=dev); u = 0.2 * v
    ms = timed_events(lambda: ops.izh_run_nt(I, S, v, u, 0.02, 0.2, -65.0, 8.0, 0.2))
    bytes_alg = N * T * 8 + N * 16
    res["izhikevich_nt"] = {"neurons": N, "timesteps": T, "dtype": "f32", "neuron_timesteps_per_s": N * T / (ms * 1e-3),
                            "ms": ms, "algorithmic_bytes": bytes_alg, "hbm_gbs": bytes_alg / (ms * 1e-3) / 1e9,
                            "hbm_frac_of_8TBs": bytes_alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    del I, S, v, u
    B, T2, D = 4096, 100, 1024
    I = 20 * torch.rand(B, T2, D, device=dev); S = torch.empty_like(I)
    v = torch.full((B * D,), -65.0, device=dev); u = 0.2 * v
    ms = timed_events(lambda: ops.izh_run_btd(I, S, v, u, 0.02, 0.2, -65.0, 8.0, 0.2))
    bytes_alg = B * D * T2 * 8 + B * D * 16
    res["izhikevich_btd"] = {"neurons": B * D, "timesteps": T2, "dtype": "f32",
                             "neuron_timesteps_per_s": B * D * T2 / (ms * 1e-3), "ms": ms, "algorithmic_bytes": bytes_alg,
                             "hbm_gbs": bytes_alg / (ms * 1e-3) / 1e9,
                             "hbm_frac_of_8TBs": bytes_alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    del I, S, v, u
    rows, T3, H = 8192, 16, 3072
    h = (torch.randn(rows, T3, H, device=dev) * 2).to(torch.bfloat16)
    out = torch.empty_like(h)
    vv = torch.zeros(rows, H, device=dev, dtype=torch.bfloat16); th = torch.ones_like(vv)
    ms = timed_events(lambda: ops.gif_run(h, out, vv, th, math.exp(-0.1), 8, 0.01, 1.0, T3))
    bytes_alg = rows * T3 * H * 4 + rows * H * 8
    # the bf16 loop is bound by vector instructions (the reference's bf16 tensors round after every op: 13
    # roundings per step; ~40 VALU instructions per neuron-step at 16 lanes/clk/SIMD for unpacked fp32 ops)
    ms_core = timed_events(lambda: ops.gif_run(h[:, 0].contiguous(), out[:, 0].contiguous(), vv, th, math.exp(-0.1), 8,
                                               0.01, 1.0, T3, time_invariant=True, mean_out=True))
    valu_peak = 256 * 4 * 16 * 2.4e9                       # lane-ops/s: 256 CUs x 4 SIMDs x 16 lanes/clk (non-packed fp32)
    res["gif_bf16"] = {"rows": rows, "timesteps": T3, "hidden": H, "dtype": "bf16",
                       "neuron_timesteps_per_s": rows * T3 * H / (ms * 1e-3), "ms": ms, "algorithmic_bytes": bytes_alg,
                       "hbm_gbs": bytes_alg / (ms * 1e-3) / 1e9,
                       "hbm_frac_of_8TBs": bytes_alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                       "bound": "valu", "valu_instructions_per_neuron_step": 40,
                       "valu_frac_of_peak": rows * T3 * H * 40 / (ms * 1e-3) / valu_peak,
                       "ms_without_streams": ms_core,
                       "valu_frac_of_peak_without_streams": rows * T3 * H * 40 / (ms_core * 1e-3) / valu_peak}
    del h, out, vv, th
    from aura_snn_rag_amd.core.language_zone.snn_ffn import SNNFFN
    torch.manual_seed(0)
    ffn = SNNFFN(768, 3072, num_timesteps=16, L=8).to(dev).to(torch.bfloat16).eval()
    x = torch.randn(1, 512, 768, device=dev, dtype=torch.bfloat16)

    def ffn_forward():
        with torch.no_grad():
            return ffn(x)
    ms = timed_events(ffn_forward)
    res["snnffn_config3_bf16"] = {"ms": ms, "neuron_timesteps_per_s": 512 * 16 * (3072 + 768) / (ms * 1e-3),
                                  "note": "module forward incl. 4 GEMMs; reference CPU path measured 315 ms (BASELINE.md)"}
    return res


def secondary_config2(lib, dev, k):
    """BASELINE config 2 (100k x 768, 256-query batches, top-32) through the product API and, for
    continuity with round 1, through the tensor-level op without the per-call overflow read."""
    from aura_snn_rag_amd import ops
    N, D, nq = 100_000, 768, 256
    hf = new_bank(N, D, dev)
    fill_bank(hf, N, D, 1234, dev)
    torch.manual_seed(7)
    hf.rebuild_centroids()
    now = float(hf.memory_metadata[0, 1].item())
    g = torch.Generator(device=dev).manual_seed(99)
    pick = torch.randint(0, N, (nq // 2,), generator=g, device=dev)
    q = torch.cat([hf.memory_features[pick] + 0.05 * torch.randn(nq // 2, D, generator=g, device=dev),
                   torch.randn(nq - nq // 2, D, generator=g, device=dev)]).contiguous()
    out = {"bank_rows": N, "dim": D, "queries_per_batch": nq, "k": k}
    s_e, r_e = hf.recall_batch(q, k=k, now=now, use_candidates=False)
    out["planted_neighbours_found"] = bool((r_e[: nq // 2, 0] == pick.to(torch.int32)).float().mean() > 0.99)
    dt, kms, lps, kind, rows, nql = profiled(lib, lambda: hf.recall_batch(q, k=k, now=now, use_candidates=False), 200)
    out["exact_recall_product_api"] = {"retrievals_per_s": nq / dt, "ms_per_step": dt * 1e3,
                                       "roofline": hbm_roofline(kind, kms, lps, rows, D, nql, "config2")}
    shadow, rho = hf._ensure_shadow(), hf._rho

    def raw():
        return ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, count=N,
                              shadow=shadow, rho=rho, check_overflow=False)
    dt, kms, lps, kind, rows, nql = profiled(lib, raw, 400, warm=50)
    out["exact_recall_no_overflow_read"] = {"retrievals_per_s": nq / dt, "ms_per_step": dt * 1e3,
                                            "roofline": hbm_roofline(kind, kms, lps, rows, D, nql, "config2")}
    dt = timed_wall(lambda: hf.recall_batch(q, k=k, now=now), 200)
    s_c, r_c = hf.recall_batch(q, k=k, now=now)
    out["centroid_index_recall_product_api"] = {"retrievals_per_s": nq / dt, "ms_per_step": dt * 1e3,
                                                "vs_exact": recall_at(r_c, r_e)}
    # the all-fp32 scan of the same workload: same results bit for bit, bound by the fp32 matrix pipe
    def f32():
        return ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, count=N,
                              fp32_scan=True, check_overflow=False)
    dt, kms, lps, kind, rows, nql = profiled(lib, f32, 50)
    s_f, r_f = f32()
    out["fp32_scan_only"] = {"retrievals_per_s": nq / dt, "ms_per_step": dt * 1e3,
                             "identical_to_two_stage": bool(torch.equal(r_f, r_e) and torch.equal(s_f, s_e)),
                             "roofline": hbm_roofline(kind, kms, lps, rows, D, nql, "config2")}
    return out


def secondary_c5(dev, rows, D, k):
    """BASELINE config 5 on one GPU: `rows` one-shot writes (bf16 producers, chunked bulk_write), one
    centroid rebuild, then recall@k of the centroid-index recall against the exact recall on 10k held-in
    queries (query = stored row + noise)."""
    hf = new_bank(rows, D, dev)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fill_bank(hf, rows, D, 4321, dev, dtype=torch.bfloat16, chunk=1 << 18)
    torch.cuda.synchronize(); t_write = time.perf_counter() - t0
    torch.manual_seed(11)
    t0 = time.perf_counter(); hf.rebuild_centroids(); torch.cuda.synchronize(); t_rebuild = time.perf_counter() - t0
    now = float(hf.memory_metadata[0, 1].item())
    g = torch.Generator(device=dev).manual_seed(5)
    nq = 10_000
    pick = torch.randint(0, rows, (nq,), generator=g, device=dev)
    q = (hf.memory_features[pick] + 0.3 * torch.randn(nq, D, generator=g, device=dev)).contiguous()
    t0 = time.perf_counter(); s_c, r_c = hf.recall_batch(q, k=k, now=now); torch.cuda.synchronize()
    t_first = time.perf_counter() - t0                      # includes the one-off build of the inverted lists
    t_c = timed_wall(lambda: hf.recall_batch(q, k=k, now=now), 3, warm=1)
    t_e = timed_wall(lambda: hf.recall_batch(q, k=k, now=now, use_candidates=False), 2, warm=1)
    s_e, r_e = hf.recall_batch(q, k=k, now=now, use_candidates=False)
    out = {"rows": rows, "dim": D, "producer_dtype": "bf16 (stored fp32)",
           "write_path": "bulk_write: NO online centroid update, ONE rebuild at the end (not the reference's "
                         "rebuild-every-512-inserts schedule; see secondary.reference_semantics_write for that path)",
           "write_s": t_write,
           "writes_per_s": rows / t_write, "write_hbm_gbs": rows * D * (2 + 4) / t_write / 1e9,
           "rebuild_centroids_s": t_rebuild, "first_recall_incl_list_build_s": t_first, "queries": nq, "k": k,
           "centroid_index": dict(retrievals_per_s=nq / t_c, held_in_row_is_top1=float((r_c[:, 0] == pick.to(torch.int32)).float().mean()),
                                  **{f"{n}_vs_exact": v for n, v in recall_at(r_c, r_e).items()}),
           "exact": dict(retrievals_per_s=nq / t_e, held_in_row_is_top1=float((r_e[:, 0] == pick.to(torch.int32)).float().mean()))}
    del hf
    torch.cuda.empty_cache()
    return out


def cpu_baseline(hf, q, k, now, n_sample, gpu_rows, gpu_scores, candidates):
    """The oracle's recall at the REFERENCE's cost model (hippocampal.py:259-307: 8 full-bank compares for
    the candidate mask, per-query normalisation of the candidate rows, mm, topk) over a host copy of the
    SAME bank, centroid table and metadata; also the parity of the GPU result on those queries."""
    from oracle import aura_oracle as O
    from tests.helpers import topk_equivalent
    # the GPU box gives a 1-GPU job a 16-core CPU share (all 256 host cores are visible, but
    # oversubscribing them is several times slower than using the share: 4.4 s vs 0.1 s per query)
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(16, ncpu)))
    N, D = hf.memory_count, hf.memory_features.shape[1]
    ob = O.OracleBank(1, D, use_centroid_index=candidates)
    ob.M = N
    ob.features = hf.memory_features[:N].cpu()
    ob.metadata = hf.memory_metadata[:N].cpu()
    ob.locations = torch.zeros(N, 2)
    ob.centroids = hf.centroids.cpu()
    ob.index_ready = candidates
    ob.count = N
    qs = q[:n_sample].cpu()
    ob.recall(qs[0], k, now)  # warm-up
    rows, scores = [], []
    t0 = time.perf_counter()
    for i in range(n_sample):
        r, s = ob.recall(qs[i], k, now)
        rows.append(r); scores.append(s)
    dt = time.perf_counter() - t0
    full = all(r.numel() == k for r in rows)
    parity = None
    if full:
        ref_r, ref_s = torch.stack(rows), torch.stack(scores)
        exact_q = (gpu_rows[:n_sample].cpu().long() == ref_r).all(dim=1)
        # A query whose 8th and 9th nearest centroids are a near-tie in fp32 (all 256 distances of a
        # Gaussian query lie within a few percent of each other) may probe a different 8th list on the two
        # machines: both results are the reference's algorithm; such queries are counted apart
        tie = torch.zeros(n_sample, dtype=torch.bool)
        if candidates:
            for i in range(n_sample):
                d = torch.sort(torch.norm(ob.centroids - qs[i], dim=1)).values
                tie[i] = bool((d[8] - d[7]) <= 2e-6 * d[7])
        sel = ~tie
        ex, n, ok = topk_equivalent(gpu_rows[:n_sample][sel], gpu_scores[:n_sample][sel], ref_r[sel], ref_s[sel])
        if os.environ.get("AURA_BENCH_PARITY_DEBUG"):        # where and by how much the rows differ (stderr)
            gr, gs = gpu_rows[:n_sample].cpu().long(), gpu_scores[:n_sample].cpu()
            for i in torch.nonzero(~exact_q).flatten().tolist():
                for p_ in torch.nonzero(gr[i] != ref_r[i]).flatten().tolist()[:4]:
                    print(f"[parity] query {i} pos {p_}: gpu row {int(gr[i, p_])} score {float(gs[i, p_]):.9g} | "
                          f"oracle row {int(ref_r[i, p_])} score {float(ref_s[i, p_]):.9g} | oracle next "
                          f"{float(ref_s[i, min(p_ + 1, k - 1)]):.9g}", file=sys.stderr)
        parity = {"queries": int(n_sample), "index_exact": int(exact_q.sum()), "probe_near_ties": int(tie.sum()),
                  "within_tolerance_excluding_probe_near_ties": bool(ok),
                  "tolerance": "rows equal except where the oracle's own scores of the two rows differ by <= 2e-6; scores within 1e-5"}
    return {"value": n_sample / dt, "unit": "retrievals/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{n_sample} single-query recalls of the reference algorithm ("
                      f"{'8 candidate-mask compares + ' if candidates else ''}per-query normalise + mm + topk) over a "
                      f"host copy of the same {N}x{D} fp32 bank, k={k}; {torch.get_num_threads()} threads = the "
                      f"16-core CPU share of a 1-GPU job ({ncpu} cores visible)",
            "gpu_parity_on_sample": parity}


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    # AURA_BENCH_BACKEND=gloo: functional rehearsal of the N > 1 path on a box with fewer GPUs than ranks
    # (ranks share devices, collectives go through gloo); the measured configuration is always nccl = RCCL
    backend = os.environ.get("AURA_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    use_dist = world > 1 or os.environ.get("AURA_BENCH_FORCE_DIST") == "1"   # 1-rank RCCL smoke test
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # RCCL prints a version banner ("RCCL version : ...", five lines) on STDOUT when its first communicator comes
        # up; the contract is ONE JSON line there.  File descriptor 1 points at stderr until the communicator exists.
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
            t0_ = torch.zeros(1, device=dev)
            dist.all_reduce(t0_)
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    from aura_snn_rag_amd import _lib
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    lib = _lib.load()

    D, k, nq = args.dim, args.k, args.nq
    rows = (args.bank_rows + world - 1) // world          # per rank
    total = rows * world
    hf = new_bank(rows, D, dev)
    sh = ShardedHippocampus(hf, total, force_collectives=use_dist and world == 1)
    fill_bank(hf, rows, D, 1234 + rank, dev)
    hf.memory_metadata[:hf.memory_count, 1] = BENCH_WRITE_TIME
    sh.memory_count = total
    sh.rebuild_centroids(perm=torch.randperm(total, generator=torch.Generator().manual_seed(7)))
    now = float(hf.memory_metadata[0, 1].item())
    if use_dist:
        t = torch.tensor([now], device=dev, dtype=torch.float64)
        dist.broadcast(t, src=0)
        now = float(t.item())
    g = torch.Generator(device=dev).manual_seed(99 + rank)
    pick = torch.randint(0, rows, (nq // 2,), generator=g, device=dev)
    q = torch.cat([hf.memory_features[pick] + 0.05 * torch.randn(nq // 2, D, generator=g, device=dev),
                   torch.randn(nq - nq // 2, D, generator=g, device=dev)]).contiguous()
    cand = not args.exact

    def step():
        return sh.recall_batch(q, k=k, now=now, all_gather_queries=use_dist, use_candidates=cand)

    # the first call builds the inverted lists (setup); guard on its output: planted neighbours found
    # (query = stored row + 5 % noise)
    s, i = step()
    torch.cuda.synchronize()
    planted_ok = bool((i[: nq // 2, 0] == (pick + sh.row_base).to(torch.int32)).float().mean() > 0.98)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "scores.npy"), last[0].cpu().numpy().astype(np.float32))
        np.save(os.path.join(args.dump_outputs, "rows.npy"), last[1].cpu().numpy().astype(np.float64))
    del last

    value = nq * world * args.steps / elapsed
    roof = None
    if args.full:
        # the dominant launch timed with HIP events, in a pass of its own over as many steps
        lib.aura_profile_begin(max(1, args.steps * 16))
        torch.cuda.synchronize()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        buf = (ctypes.c_float * (args.steps * 16))()
        nprof = lib.aura_profile_end(buf, args.steps * 16)
        kms = sum(buf[j] for j in range(nprof)) / max(nprof, 1)
        rows_c, nq_c = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.aura_profile_last_scan(ctypes.byref(rows_c), ctypes.byref(nq_c))
        kind = lib.aura_profile_last_scan_kind()
        cfg_key = f"headline_{args.bank_rows}x{D}_n{world}_{'index' if cand else 'exact'}"
        # kind 3 reports the allocated sorted rows (slack and padding included); the algorithmic unit is one
        # read of every bank row
        issued = useful = None
        if kind == 3 and world == 1:
            issued, useful = ivf_issued_flop(hf, q, D)
        roof = hbm_roofline(kind, kms, nprof / max(args.steps, 1), hf.memory_count if kind == 3 else rows_c.value,
                            D, nq_c.value, cfg_key, issued, useful) if nprof else None

    mode = ("centroid-index recall (8 nearest of 256 centroids, hippocampal.py:259-270) through inverted lists on "
            "the two-stage scan" if cand else "exact recall (two-stage scan)")
    out = {
        "metric": "retrievals/sec", "value": value, "unit": "retrievals/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "collective_backend": (backend if use_dist else None),
        "config": {"workload": f"episodic cosine-kNN, {mode}: {total}x{D} fp32 bank "
                               f"({'row-sharded over %d ranks, %d rows each' % (world, rows) if world > 1 else 'one GPU'}), "
                               f"{nq}-query batch per rank and step, top-{k}, through HippocampalFormation.recall_batch "
                               f"with its default per-call overflow check; exact fp32 scores of the candidates "
                               f"(bf16 matrix-core prefilter over a list-sorted bf16 shadow with a rigorous error bound "
                               f"+ fp32 re-scoring of the survivors: rows and score bits of the fp32 lists)",
                   "bank_rows": total, "dim": D, "queries_per_rank": nq, "k": k, "nprobe": 8, "lists": 256,
                   "parallelism": f"bank-sharded x{world}" if world > 1 else "single"},
        "planted_neighbours_found": planted_ok,
    }
    if args.full:
        out["roofline"] = roof
    if args.full and rank == 0 and world == 1:
        s_c, r_c = s, i
        # CPU baseline and the GPU's parity on its sample FIRST, on the bank the headline ran on: the write
        # benchmarks of the secondary section store the same random batch several times over (exact duplicate
        # rows, i.e. exactly tied scores, whose order torch.topk and the GPU break differently: r03's first records
        # read 51 of 64 index-exact queries for that reason alone; 64 of 64 on the untouched bank)
        if not args.no_cpu_baseline:
            s_h, r_h = hf.recall_batch(q[:args.cpu_queries].contiguous(), k=k, now=now, use_candidates=cand)
            out["cpu_baseline"] = cpu_baseline(hf, q, k, now, args.cpu_queries, r_h, s_h, cand)
        if not args.no_secondary:
            sec = {}
            # exact recall on the same bank and queries, beside the headline
            s_e, r_e = hf.recall_batch(q, k=k, now=now, use_candidates=False)
            for name, nqq in (("exact_recall_2048q", nq), ("exact_recall_256q", 256)):
                qq = q[:nqq].contiguous()
                dt, kms2, lps, kind2, rws, nql = profiled(lib, lambda: hf.recall_batch(qq, k=k, now=now, use_candidates=False), 20)
                sec[name] = {"retrievals_per_s": nqq / dt, "ms_per_step": dt * 1e3,
                             "roofline": hbm_roofline(kind2, kms2, lps, rws, D, nql,
                                                      f"exact_{args.bank_rows}x{D}" + ("_2048q" if nqq > 256 else ""))}
            qq = q[:256].contiguous()
            dt = timed_wall(lambda: hf.recall_batch(qq, k=k, now=now), 50)
            sec["centroid_index_recall_256q"] = {"retrievals_per_s": 256 / dt, "ms_per_step": dt * 1e3}
            dt = timed_wall(lambda: hf.recall_batch(q, k=k, now=now, check_overflow=False), 50)
            sec["centroid_index_recall_no_overflow_read"] = {"retrievals_per_s": nq / dt, "ms_per_step": dt * 1e3}
            # the query block one rank of an 8-GPU run sees after the all-gather (8 x 2048): passes of 8192
            g16 = torch.Generator(device=dev).manual_seed(4242)
            q16 = torch.randn(8 * nq, D, generator=g16, device=dev)
            dt = timed_wall(lambda: hf.recall_batch(q16, k=k, now=now), 10)
            sec[f"centroid_index_recall_{8 * nq}q"] = {"retrievals_per_s": 8 * nq / dt, "ms_per_step": dt * 1e3}
            del q16
            sec["centroid_index_vs_exact"] = dict(planted_half=recall_at(r_c[: nq // 2], r_e[: nq // 2]),
                                                  random_half=recall_at(r_c[nq // 2:], r_e[nq // 2:]),
                                                  note="synthetic Gaussian rows have no cluster structure: the "
                                                       "index's recall on them is a property of the reference's "
                                                       "algorithm (8 of 256 lists), not of this implementation")
            # rebuild + the write -> recall interleave of MemoryAugmentedLayer (store B rows, retrieve B queries
            # per forward, memory_augmented_layer.py:231-245) on the full 1M bank
            torch.manual_seed(3)
            t0 = time.perf_counter(); hf.rebuild_centroids(); torch.cuda.synchronize()
            sec["rebuild_centroids_ms"] = (time.perf_counter() - t0) * 1e3
            hf.recall_batch(q, k=k, now=now)                       # re-pack of the lists after the rebuild
            hf._overflow = 'fifo'
            for B in (8, 256):
                qb = q[:B].contiguous()
                newrows = torch.randn(B, D, device=dev)
                ids = [f"x{j}" for j in range(B)]

                def fwd():
                    hf.create_episodic_memories(ids, newrows)
                    return hf.recall_batch(qb, k=5, now=now)
                dt = timed_wall(fwd, 20)
                sec[f"interleaved_store_retrieve_B{B}"] = {"ms_per_forward": dt * 1e3, "bank_rows": hf.memory_count}
            # reference-semantics ingest: create_episodic_memories with the index on -- every row
            # is assigned to its nearest centroid and moves that centroid's running mean before the next row is
            # looked at (hippocampal.py:218-230).  The bank is full, so rows overwrite the FIFO ring and the
            # reference's "rebuild every 512 inserts" never fires (memory_count stays put): this is the write path
            # alone.  With the rebuild cadence of a GROWING bank the rate is bounded by the rebuild itself.
            rs = {}
            for B in (512, 4096):
                newrows = torch.randn(B, D, device=dev)
                ids = [f"w{j}" for j in range(B)]
                dt = timed_wall(lambda: hf.create_episodic_memories(ids, newrows), 10, warm=2)
                rs[f"rows_per_s_batches_of_{B}"] = B / dt
            t_rb = sec["rebuild_centroids_ms"] * 1e-3
            rs["rows_per_s_with_a_rebuild_every_512_inserts_derived"] = 512.0 / (512.0 / rs["rows_per_s_batches_of_512"] + t_rb)
            rs["note"] = ("online nearest-centroid / running-mean update through create_episodic_memories at "
                          f"{hf.memory_count} x {D}, index on; r02: one workgroup, 15 us per row = 6.6e4 rows/s")
            sec["reference_semantics_write"] = rs
            out["secondary"] = sec
        if not args.no_secondary:
            del hf, sh
            torch.cuda.empty_cache()
            out["secondary"]["config2_100k"] = secondary_config2(lib, dev, k)
            torch.cuda.empty_cache()
            out["secondary"]["neurons"] = secondary_neurons(dev)
            torch.cuda.empty_cache()
            if args.c5_rows > 0:
                out["secondary"]["config5_seeding"] = secondary_c5(dev, args.c5_rows, D, k)
    if rank == 0:
        print(json.dumps(out))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
