"""Round-3 regressions of the recall kernels."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nq", [40, 900])
def test_rows_stamped_in_the_future_score_inf_and_do_not_fault(dev, nq):
    """Rows whose timestamp lies far in the future of `now` score exp(+huge) = +inf in the reference
    (hippocampal.py:288-289) and here.  The prefilter used +inf as the "nothing passes" threshold of padding
    query columns; U = +inf passed it, and the candidate of query -1 corrupted the candidate counters (a device
    fault in round 3's first sharded test, whose seeding and recall clocks disagreed).  Padding thresholds are NaN
    now; every path returns the same rows as the all-fp32 kernels: the inf rows first, ties to the lower row."""
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    D, N, k = 64, 30000, 9
    g = torch.Generator().manual_seed(3)
    centres = torch.randn(150, D, generator=g) * 3
    feats = centres[torch.randint(0, 150, (N,), generator=g)] + torch.randn(N, D, generator=g)
    q = (centres[torch.randint(0, 150, (nq,), generator=g)] + torch.randn(nq, D, generator=g)).to(dev).contiguous()
    hf = HippocampalFormation(feature_dim=D, max_memories=N + 100, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                              device="cuda", use_centroid_index=True)
    hf.bulk_write(feats.to(dev), rebuild=False)
    hf.rebuild_centroids(perm=torch.randperm(N, generator=g))
    now = 1.7e9
    hf.memory_metadata[:, 1] = now
    hf.memory_metadata[: 2 * N // 3, 1] = now + 9.0e7            # two thirds of the rows: exp(25000) = +inf
    hf.memory_metadata[5:N:7, 0] = 0.25                           # (inf * strength stays inf)
    s_m, r_m = ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, count=N,
                              centroids=hf.centroids, nprobe=8, fp32_scan=True)
    s_p, r_p = hf.recall_batch(q, k=k, now=now)                   # product path (probe masks / inverted lists)
    assert torch.equal(r_p, r_m) and torch.equal(s_p, s_m)
    assert bool(torch.isinf(s_p[:, 0]).all())
    s_e, r_e = hf.recall_batch(q, k=k, now=now, use_candidates=False)
    s_f, r_f = ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, count=N, fp32_scan=True)
    assert torch.equal(r_e, r_f) and torch.equal(s_e, s_f)
    # the two-stage kernels themselves (no fallback): they must flag the overflow, never fault
    ivf = hf._ensure_ivf()
    s2, r2, ovf = ops.knn_search_ivf2(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, hf.centroids, 8,
                                      ivf.sorted_bf16, hf._rho, ivf.sorted_rows, ivf.pad_off, ivf.list_len,
                                      n_sorted=ivf.n_sorted, lists_flag=ivf.flag)
    f = int(ovf.item())
    assert (f & 16) == 0, "a candidate with an invalid row id reached the refine stage"
    if (f & ~ops.KNN_FLAG_NO_CANDIDATES) == 0:
        assert torch.equal(r2, r_m) and torch.equal(s2, s_m)


@pytest.mark.parametrize("D,nq,kc", [(32, 1, 16), (32, 37, 16), (8, 5, 256), (64, 900, 200), (96, 16, 256), (100, 33, 256),
                                     (50, 7, 40), (768, 300, 256), (1024, 20, 256), (1280, 9, 256)])
def test_centroid_probe_ids_against_float64(dev, D, nq, kc):
    """aura_centroid_probe (fp32 matrix cores: key = ||c||^2 - 2 q.c; centroid rows through the LDS transposer for
    D <= 1024, register path above, scalar loads for D % 4 != 0) against the fp64 distances over ALL 256 table
    rows -- the zero rows beyond centroids_k included, as hippocampal.py:261-262 ranks them too.  A position may
    differ only where the fp64 distances of the two rows agree to 1e-6 relative (an fp32 near-tie)."""
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(D * 1000 + nq)
    cent = torch.zeros(256, D)
    cent[:kc] = torch.randn(kc, D, generator=g) * 0.7
    q = torch.randn(nq, D, generator=g) * (0.2 + 2 * torch.rand(nq, 1, generator=g))
    ids = ops.centroid_probe(q.to(dev).contiguous(), cent.to(dev).contiguous(), 8).cpu().long()
    d = torch.cdist(q.double(), cent.double())
    ref = torch.topk(d, 8, dim=1, largest=False, sorted=True).indices
    # ties between the identical zero rows go to the lower row in both (topk is not stable: compare distances)
    bad = 0
    for i in range(nq):
        for p in range(8):
            if ids[i, p] != ref[i, p]:
                a, b = float(d[i, ids[i, p]]), float(d[i, ref[i, p]])
                if abs(a - b) > 1e-6 * max(abs(b), 1e-30):
                    bad += 1
    assert bad == 0, f"{bad} probe positions differ beyond an fp32 near-tie"
    assert bool((ids >= 0).all()) and bool((ids < 256).all())
    assert all(len(set(r.tolist())) == 8 for r in ids)


def test_inverted_list_scan_returns_the_fp32_masked_scan(dev):
    """The inverted-list scan (eight waves per workgroup over 256-slot blocks, the only form there is) returns the
    rows and score bits of the fp32 masked scan and raises no flag besides NO_CANDIDATES.  The 2100-query shape is a
    pass of more than 8 queries per CU over a bank of at most 300 000 rows: its refine runs one wave per query
    (coarse_refine_wave6_kernel) with the workgroup-per-query kernel walking the heavy list behind it."""
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    for D, N, nq, k in ((64, 40000, 900, 9), (768, 30000, 2100, 32), (200, 20000, 70, 5)):
        g = torch.Generator().manual_seed(D + nq)
        centres = torch.randn(120, D, generator=g) * 2
        feats = centres[torch.randint(0, 120, (N,), generator=g)] + torch.randn(N, D, generator=g)
        q = (centres[torch.randint(0, 120, (nq,), generator=g)] + torch.randn(nq, D, generator=g)).to(dev).contiguous()
        hf = HippocampalFormation(feature_dim=D, max_memories=N, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", use_centroid_index=True)
        hf.bulk_write(feats.to(dev), rebuild=False)
        hf.rebuild_centroids(perm=torch.randperm(N, generator=g))
        now = float(hf.memory_metadata[0, 1].item())
        ivf = hf._ensure_ivf()
        s2, r2, ovf = ops.knn_search_ivf2(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, hf.centroids, 8,
                                          ivf.sorted_bf16, hf._rho, ivf.sorted_rows, ivf.pad_off, ivf.list_len,
                                          n_sorted=ivf.n_sorted, lists_flag=ivf.flag)
        assert (int(ovf.item()) & ~ops.KNN_FLAG_NO_CANDIDATES) == 0, (D, N, nq, k)
        s_m, r_m = ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, k, now, count=N,
                                  centroids=hf.centroids, nprobe=8, fp32_scan=True)
        assert torch.equal(r2, r_m) and torch.equal(s2, s_m), (D, N, nq, k)


def test_tuning_hooks_keep_results_intact(dev):
    """``aura_debug_cs_flags`` (in-process A/B of the scan kernels' switches) and ``aura_debug_clock_mhz``: the
    result-preserving switches -- early LDS-DMA issue on waves 4-7 (4096), no row-split form (256), no two-tile
    form (1024), an even split of the sample tiles (32768) -- give the default's rows and score bits; the flag word
    is restored; the shader clock reads as a plausible number."""
    import ctypes
    from aura_snn_rag_amd import _lib
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    lib = _lib.load()
    torch.manual_seed(3)
    N, D, nq, k = 60_000, 256, 700, 16
    hf = HippocampalFormation(feature_dim=D, max_memories=N, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                              device="cuda", use_centroid_index=True)
    hf.bulk_write(torch.randn(N, D, device=dev), rebuild=True)
    now = float(hf.memory_metadata[0, 1].item()) + 5.0
    q = torch.randn(nq, D, device=dev)
    assert lib.aura_debug_cs_flags(-1) == 0
    s0, r0 = hf.recall_batch(q, k=k, now=now)
    try:
        for flags in (4096, 256, 1024, 32768, 4096 | 256 | 1024 | 32768):
            assert lib.aura_debug_cs_flags(flags) in (0, 4096, 256, 1024, 32768)
            s1, r1 = hf.recall_batch(q, k=k, now=now)
            assert torch.equal(r1, r0) and torch.equal(s1, s0), flags
    finally:
        lib.aura_debug_cs_flags(0)
    assert lib.aura_debug_cs_flags(-1) == 0
    clk = torch.zeros(1, device=dev)
    assert lib.aura_debug_clock_mhz(ctypes.c_void_p(clk.data_ptr()), 500,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert 300.0 < float(clk.item()) < 4000.0, float(clk.item())
    assert lib.aura_debug_clock_mhz(None, 500, None) != 0
