"""GPU tests of the retention feature: the retention key, the weakest-first selection (checked EXACTLY
against the order rebuilt on the CPU from the kernel's own keys), ``overflow='weakest'`` against the ring and
against the rule, reinforcement, the inverted lists under eviction, and the C ABI's argument checks.

The rule (restated in tests/cpu_stub_retention.py with torch on the CPU):
  key(r) = strength(r) * expf(-(now32 - timestamp(r)) / 3600); rows leave in ascending
  (key, (r - cursor) mod count), a NaN key first; reinforce: s < cap -> min(s + amount, cap) once per row."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_retention as R

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
NOW32 = float(np.float32(NOW))


@pytest.fixture()
def H(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    return H


def _hf(H, M, D, **kw):
    return H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", **kw)


def _tied_meta(count, seed=21):
    """Strengths k / 64 and ages that are multiples of 128 s (exact in fp32 at 1.7e9): few distinct keys, so the
    threshold key of a selection is shared by rows that only the rotated row can separate."""
    g = torch.Generator().manual_seed(seed)
    meta = torch.zeros(count, 4)
    meta[:, 0] = torch.randint(13, 65, (count,), generator=g).float() / 64
    meta[:, 1] = torch.tensor(NOW32) - 128.0 * torch.randint(0, 64, (count,), generator=g).float()
    meta[:, 2] = -1
    return meta


def _check_selection(ops, meta_dev, count, cursor, n):
    """The selection equals the first n rows of the order rebuilt from the kernel's own keys: no tolerance."""
    keys = ops.bank_retention_keys(meta_dev, count, NOW).cpu()
    slots, got = ops.bank_select_weakest(meta_dev, count, NOW, cursor, n)
    want = R.eviction_order(keys, cursor)[:n]
    assert slots.dtype == torch.int64 and got.dtype == torch.float32 and slots.shape == (n,) and got.shape == (n,)
    assert torch.equal(slots.cpu(), want), f"count={count} cursor={cursor} n={n}: rows differ"
    assert torch.equal(got.cpu().view(torch.int32), keys[want].view(torch.int32)), "keys differ"
    return keys, want


# ---------------------------------------------------------------------------------------------- 1. keys
def test_retention_keys_match_the_formula(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(3)
    count = 70001
    meta = torch.zeros(count + 9, 4)
    meta[:, 0] = 1.2 * torch.rand(count + 9, generator=g)
    meta[:, 1] = torch.tensor(NOW32) - 20000.0 * torch.rand(count + 9, generator=g)
    meta[17, 0] = float("nan")
    meta[23, 0] = 0.0
    want = meta[:count, 0] * torch.exp(-(torch.tensor(NOW32) - meta[:count, 1]) / 3600.0)
    got = ops.bank_retention_keys(meta.to(dev), count, NOW).cpu()
    assert got.shape == (count,)
    ok = ~torch.isnan(want)
    assert int((~ok).sum()) == 1 and bool(torch.isnan(got[17]))
    print(f"retention keys: max |device - host| = {(got[ok] - want[ok]).abs().max():.3e}")
    assert torch.allclose(got[ok], want[ok], atol=1e-5, rtol=0)
    # a NaN key is the weakest: ranked first by the selection
    slots, keys = ops.bank_select_weakest(meta.to(dev), count, NOW, 5, 3)
    assert int(slots[0]) == 17 and bool(torch.isnan(keys[0])) and not bool(torch.isnan(keys[1:]).any())


# ---------------------------------------------------------------------------------------------- 2. selection
@pytest.mark.parametrize("cursor", [0, 12345])
def test_selection_is_exact_with_threshold_ties(dev, cursor):
    from aura_snn_rag_amd import ops
    count = 50_000
    meta = _tied_meta(count).to(dev)
    for n in (1, 64, 512, 4096, count):
        keys, want = _check_selection(ops, meta, count, cursor, n)
        if n in (512, 4096):
            # the fixture does what it is for: the threshold key is shared by more rows than are taken
            thr = keys[want[-1]]
            shared, taken = int((keys == thr).sum()), int((keys[want] == thr).sum())
            assert shared > taken >= 1, (n, shared, taken)
    assert torch.unique(ops.bank_retention_keys(meta, count, NOW)).numel() < count // 10


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_selection_small_banks(dev, count):
    from aura_snn_rag_amd import ops
    meta = _tied_meta(count, seed=count).to(dev)
    for cursor in (0, count // 3, count - 1):
        for n in sorted({1, max(1, count // 2), count}):
            _check_selection(ops, meta, count, cursor, n)
    g = torch.Generator().manual_seed(count)
    meta[:, 0] = torch.rand(count, generator=g).to(dev)             # distinct keys
    for n in sorted({1, max(1, count - 1), count}):
        _check_selection(ops, meta, count, 1 % count, n)


def test_selection_equal_keys_is_the_rotated_row_and_wraps(dev):
    from aura_snn_rag_amd import ops
    count, n, cursor = 100_000, 700, 99_600
    meta = torch.zeros(count, 4, device=dev)
    meta[:, 0] = 1.0
    meta[:, 1] = NOW32 - 256.0
    slots, keys = ops.bank_select_weakest(meta, count, NOW, cursor, n)
    assert torch.equal(slots.cpu(), (cursor + torch.arange(n)) % count)
    assert torch.equal(keys, ops.bank_retention_keys(meta, count, NOW)[slots])
    _check_selection(ops, meta, count, cursor, n)


def test_selection_ranks_nan_then_negative_first(dev):
    from aura_snn_rag_amd import ops
    count = 1000
    meta = _tied_meta(count, seed=5)
    meta[5, 0] = float("nan")
    meta[9, 0] = -0.5
    meta[11, 0] = 0.0
    meta = meta.to(dev)
    for n in (1, 2, 3, 40):
        _, want = _check_selection(ops, meta, count, 7, n)
        assert want.tolist()[:3] == [5, 9, 11][:n]


def test_selection_ten_million_rows(dev):
    from aura_snn_rag_amd import ops
    count, n, cursor = 10_000_000, 4096, 7_654_321
    meta = _tied_meta(count, seed=8).to(dev)
    keys, want = _check_selection(ops, meta, count, cursor, n)
    thr = keys[want[-1]]
    assert int((keys == thr).sum()) > int((keys[want] == thr).sum())        # ties at the threshold
    g = torch.Generator().manual_seed(9)
    meta[:, 0] = (0.25 + 0.75 * torch.rand(count, generator=g)).to(dev)     # (nearly) distinct keys
    _check_selection(ops, meta, count, cursor, n)


# ---------------------------------------------------------------------------------------------- 3. the ring
@pytest.mark.parametrize("index", [False, True])
def test_equal_keys_evict_exactly_like_fifo(dev, H, index):
    D, M = 64, 3000
    g = torch.Generator().manual_seed(31)
    feats = torch.randn(7700, D, generator=g)
    q = feats[torch.randint(0, 7700, (90,), generator=g)] + 0.05 * torch.randn(90, D, generator=g)
    banks = []
    for policy in ("fifo", "weakest"):
        hf = _hf(H, M, D, use_centroid_index=index, overflow=policy)
        torch.manual_seed(4)                                        # (the rebuilds draw their sample from torch's RNG)
        for lo in range(0, 7700, 700):
            hf.create_episodic_memories([f"m{i}" for i in range(lo, lo + 700)], feats[lo:lo + 700])
        banks.append(hf)
    f, w = banks
    assert f.memory_count == w.memory_count == M and f._write_cursor == w._write_cursor == 4700
    assert torch.equal(f.memory_features, w.memory_features) and torch.equal(f.memory_metadata, w.memory_metadata)
    assert torch.equal(f._inv_norm, w._inv_norm)
    assert f.id_to_idx == w.id_to_idx and f._idx_to_id == w._idx_to_id
    sf, rf = f.recall_batch(q, k=6, now=NOW)
    sw, rw = w.recall_batch(q, k=6, now=NOW)
    assert torch.equal(rf, rw) and torch.equal(sf, sw)


# ---------------------------------------------------------------------------------------------- 4. retention
def test_used_memories_survive_and_the_rule_names_the_evicted(dev, H, monkeypatch):
    D, M = 64, 4096
    g = torch.Generator().manual_seed(41)
    feats = torch.randn(M + M // 2, D, generator=g)
    subset = torch.randperm(M, generator=g)[:300]
    q = feats[subset] + 0.01 * torch.randn(300, D, generator=g)
    used = torch.zeros(M, dtype=torch.bool)
    used[subset] = True
    decayed = torch.tensor(1.0) * (torch.tensor(1.0) - torch.tensor(0.3))          # fp32, as the decay kernel
    lost = {}
    for policy in ("weakest", "fifo"):
        monkeypatch.setattr(H.time, "time", lambda: NOW)
        hf = _hf(H, M, D, use_centroid_index=False, overflow=policy)
        hf.create_episodic_memories([f"m{i}" for i in range(M)], feats[:M])
        _, rows = hf.recall_batch(q, k=1, now=NOW, reinforce=0.2)           # at the cap: nothing to add yet
        assert torch.equal(rows[:, 0].cpu().long(), subset)
        assert torch.equal(hf.memory_metadata[:, 0], torch.ones(M, device=dev))
        hf.decay_memories(0.3)
        hf.recall_batch(q, k=1, now=NOW, reinforce=0.2)
        s = hf.memory_metadata[:, 0].cpu()
        assert torch.equal(s, torch.where(used, decayed + torch.tensor(0.2), decayed))
        now2 = NOW + 256.0
        monkeypatch.setattr(H.time, "time", lambda: now2)
        keys = hf.retention_keys(now=now2).cpu()
        victims = R.eviction_order(keys, hf._write_cursor)[:M // 2]        # the rule, from the kernel's own keys
        if policy == "weakest":
            rows_w, keys_w = hf.weakest(M // 2, now=now2)
            assert torch.equal(rows_w.cpu(), victims) and torch.equal(keys_w.cpu(), keys[victims])
        new_ids = [f"n{i}" for i in range(M // 2)]
        hf.create_episodic_memories(new_ids, feats[M:])
        assert hf.memory_count == M and hf._write_cursor == M // 2
        for r in range(M):                                                  # the two id maps agree for every slot
            assert hf.id_to_idx[hf.id_of_row(r)] == r
        evicted = {f"m{i}" for i in range(M) if hf.id_of_row(hf.id_to_idx[f"m{i}"]) != f"m{i}"}
        assert len(evicted) == M // 2
        lost[policy] = sorted(int(i) for i in subset if f"m{int(i)}" in evicted)
        if policy == "weakest":
            assert evicted == {f"m{int(r)}" for r in victims}
            assert [hf.id_to_idx[m] for m in new_ids] == victims.tolist()  # input row i goes to the i-th victim
            assert torch.equal(hf.memory_features[victims.to(dev)].cpu(), feats[M:])
            assert not used[victims].any()
    assert lost["weakest"] == [], "a reinforced memory was evicted"
    assert len(lost["fifo"]) > 0, "the ring was expected to drop part of the used subset"


# ---------------------------------------------------------------------------------------------- 5. reinforce
def test_reinforce_matches_the_rule_bit_for_bit(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(51)
    rows_alloc, count = 5000, 4000
    meta = torch.rand(rows_alloc, 4, generator=g)
    meta[:, 0] = 1.3 * torch.rand(rows_alloc, generator=g)
    amount, cap = 0.1, 1.0
    meta[100, 0] = cap                                             # at the cap
    meta[101, 0] = 1.25                                            # above it
    meta[102, 0] = 0.95                                            # clipped by the min
    meta[103, 0] = float("nan")
    rows = torch.randint(0, count, (60, 9), generator=g).to(torch.int32)
    rows[:, 0] = rows[:, 1]                                         # duplicates inside a row
    rows[::3, 2] = -1
    rows[::4, 3] = torch.tensor([count, count + 7, rows_alloc - 1, 2 ** 30, -5] * 3, dtype=torch.int32)
    rows[0, 4:9] = torch.tensor([100, 101, 102, 103, 102], dtype=torch.int32)
    want = R.reinforce_reference(meta, count, rows, amount, cap)
    m = meta.to(dev)
    ops.bank_reinforce(m, count, rows.to(dev), amount, cap)
    got = m.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[:, 1:].view(torch.int32), meta[:, 1:].view(torch.int32))       # the other three columns
    assert torch.equal(got[count:].view(torch.int32), meta[count:].view(torch.int32))     # rows beyond count
    assert got[102, 0].item() == 1.0 and got[100, 0].item() == 1.0 and got[101, 0].item() == 1.25
    touched = int((got[:, 0].view(torch.int32) != meta[:, 0].view(torch.int32)).sum())
    assert 250 < touched <= 540
    # a second call adds again (once per CALL, not once ever); amount 0 changes nothing
    ops.bank_reinforce(m, count, rows.to(dev), amount, cap)
    want2 = R.reinforce_reference(want, count, rows, amount, cap)
    assert torch.equal(m.cpu().view(torch.int32), want2.view(torch.int32))
    ops.bank_reinforce(m, count, rows.to(dev), 0.0, cap)
    assert torch.equal(m.cpu().view(torch.int32), want2.view(torch.int32))
    with pytest.raises(ValueError):
        ops.bank_reinforce(m, count, rows.to(dev), -0.1, cap)
    with pytest.raises(TypeError):
        ops.bank_reinforce(m, count, rows.to(dev).long(), 0.1, cap)


def test_indexed_recall_after_reinforce_sees_the_new_strengths(dev, H):
    """The stale-constants trap: the inverted lists cache each row's score constants; a reinforcement must drop
    that cache, or the next indexed recall ranks with the old strengths."""
    D, N = 64, 10000
    g = torch.Generator().manual_seed(52)
    centres = torch.randn(300, D, generator=g) * 3

    def draw(n):
        return centres[torch.randint(0, 300, (n,), generator=g)] + torch.randn(n, D, generator=g)
    feats = draw(N)
    q = draw(700).to(dev)                                           # > MASKED_SCAN_MAX_QUERIES: the lists
    kw = dict(use_centroid_index=True, overflow="weakest")
    a, b = _hf(H, 12000, D, **kw), _hf(H, 12000, D, **kw)
    for hf in (a, b):
        hf.centroids_update_interval = 100000
        torch.manual_seed(1)
        hf.bulk_write(feats, rebuild=True)
    assert torch.equal(a.memory_metadata, b.memory_metadata) and torch.equal(a.centroids, b.centroids)
    a.decay_memories(0.5)
    s0, r0 = a.recall_batch(q, k=9, now=NOW)                        # builds the lists and their constants
    assert a._ivf is not None and a._ivf.valid and a._ivf.rowc_live
    lucky = torch.randperm(N, generator=g)[:3000].to(torch.int32)
    a.reinforce(lucky.to(dev).reshape(60, 50), amount=0.5)
    s1, r1 = a.recall_batch(q, k=9, now=NOW)
    # the same bank with the metadata edited by torch and lists built from scratch
    b.decay_memories(0.5)
    b.memory_metadata[lucky.long().to(dev), 0] += 0.5
    b._invalidate_lists()
    s2, r2 = b.recall_batch(q, k=9, now=NOW)
    assert torch.equal(a.memory_metadata, b.memory_metadata)
    assert torch.equal(r1, r2) and torch.equal(s1, s2)
    assert not torch.equal(r0, r1), "the reinforcement was expected to change the ranking"
    # recall_batch(reinforce=...) drops the cache too
    a.recall_batch(q, k=9, now=NOW, reinforce=0.05, reinforce_cap=2.0)
    assert not a._ivf.rowc_live
    s3, r3 = a.recall_batch(q, k=9, now=NOW)
    b.memory_metadata.copy_(a.memory_metadata)
    b._invalidate_lists()
    s4, r4 = b.recall_batch(q, k=9, now=NOW)
    assert torch.equal(r3, r4) and torch.equal(s3, s4)


# ---------------------------------------------------------------------------------------------- 6. lists + eviction
def test_inverted_lists_follow_weakest_first_writes(dev, H):
    """Overflowing ``'weakest'`` writes (victims scattered over the bank: holes in many lists) with the index on:
    recall through the list-sorted bf16 shadow == recall on a second bank given the same writes without shadows
    (the fp32 lists), before and after a centroid rebuild."""
    D, M = 64, 10000
    g = torch.Generator().manual_seed(61)
    centres = torch.randn(300, D, generator=g) * 3

    def draw(n):
        return centres[torch.randint(0, 300, (n,), generator=g)] + torch.randn(n, D, generator=g)
    feats = draw(9000)
    kw = dict(use_centroid_index=True, overflow="weakest")
    a, b = _hf(H, M, D, **kw), _hf(H, M, D, bf16_shadow=False, **kw)
    strengths = (0.3 + 0.7 * torch.rand(M, generator=g)).to(dev)
    for hf in (a, b):
        hf.centroids_update_interval = 100000                        # rebuilds are explicit in this test
        torch.manual_seed(1)
        hf.bulk_write(feats, rebuild=True)
        hf.memory_metadata[:, 0] = strengths
    q = draw(700).to(dev)

    def same():
        assert torch.equal(a.memory_metadata, b.memory_metadata) and torch.equal(a.centroids, b.centroids)
        assert a.id_to_idx == b.id_to_idx and a._write_cursor == b._write_cursor
        sa, ra = a.recall_batch(q, k=9, now=NOW)
        sb, rb = b.recall_batch(q, k=9, now=NOW)
        assert torch.equal(ra, rb) and torch.equal(sa, sb)
    same()
    assert a._ivf is not None and a._ivf.valid and b._ivf is None
    written = 0
    for step in range(6):                                            # 1000 rows append, the other 800 evict
        new = draw(300)
        keys = a.retention_keys(now=NOW).cpu()
        n_app = min(300, M - a.memory_count)
        victims = R.eviction_order(keys, a._write_cursor)[:300 - n_app]
        for hf in (a, b):
            hf.create_episodic_memories([f"s{step}_{i}" for i in range(300)], new)
        assert [a.id_to_idx[f"s{step}_{i}"] for i in range(n_app, 300)] == victims.tolist()
        written += 300
        same()
    assert a.memory_count == M and a._write_cursor == written - 1000
    # the rows just written are found through the lists
    _, r = a.recall_batch(new[:5].to(dev).repeat(140, 1), k=1, now=NOW)
    assert [a.id_of_row(int(x)) for x in r[:5, 0]] == [f"s5_{i}" for i in range(5)]
    for hf in (a, b):
        hf.rebuild_centroids(perm=torch.randperm(M, generator=torch.Generator().manual_seed(3)))
    same()
    for step in range(3):
        new = draw(250)
        for hf in (a, b):
            hf.create_episodic_memories([f"t{step}_{i}" for i in range(250)], new)
        same()
    listed = a._ivf.sorted_rows[a._ivf.sorted_rows >= 0]
    assert a._ivf.valid and torch.equal(torch.sort(listed).values, torch.arange(M, device=dev, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- 7. ABI
def test_abi_rejects_bad_arguments_without_launching(dev):
    from aura_snn_rag_amd import _lib
    L = _lib.load()
    count, n = 1000, 10
    meta = _tied_meta(count).to(dev)
    before = meta.clone()
    slots = torch.full((n,), -7, dtype=torch.int64, device=dev)
    keys = torch.full((n,), -7.0, device=dev)
    nbytes = L.aura_bank_select_weakest_workspace_bytes(count, n)
    assert nbytes > 4 * count + 8 * n
    assert L.aura_bank_select_weakest_workspace_bytes(count, 0) < 0
    assert L.aura_bank_select_weakest_workspace_bytes(count, count + 1) < 0
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    m, s, k = meta.data_ptr(), slots.data_ptr(), keys.data_ptr()

    def select(meta_p=m, count_=count, cursor=0, n_=n, s_p=s, k_p=k, ws_p=base, ws_bytes=nbytes):
        return L.aura_bank_select_weakest(meta_p, count_, NOW, cursor, n_, s_p, k_p, ws_p, ws_bytes, None)
    assert select(n_=0) == -1 and select(n_=count + 1) == -1 and select(count_=0) == -1 and select(cursor=-1) == -1
    assert select(ws_bytes=nbytes - 1) == -1
    assert select(meta_p=None) == -1 and select(s_p=None) == -1 and select(k_p=None) == -1 and select(ws_p=None) == -1
    assert select(ws_p=base + 4) == -3
    out = torch.zeros(count, device=dev)
    assert L.aura_bank_retention_keys(None, count, NOW, out.data_ptr(), None) == -1
    assert L.aura_bank_retention_keys(m, count, NOW, None, None) == -1
    assert L.aura_bank_retention_keys(m, -1, NOW, out.data_ptr(), None) == -1
    rows = torch.arange(20, dtype=torch.int32, device=dev)
    rb = L.aura_bank_reinforce_workspace_bytes(count)
    assert rb >= (count + 7) // 8 and L.aura_bank_reinforce_workspace_bytes(-1) < 0

    def reinforce(meta_p=m, rows_p=rows.data_ptr(), n_rows=20, amount=0.1, ws_p=base, ws_bytes=rb):
        return L.aura_bank_reinforce(meta_p, count, rows_p, n_rows, amount, 1.0, ws_p, ws_bytes, None)
    assert reinforce(meta_p=None) == -1 and reinforce(rows_p=None) == -1 and reinforce(ws_p=None) == -1
    assert reinforce(ws_bytes=rb - 1) == -1 and reinforce(amount=-1.0) == -1 and reinforce(n_rows=-1) == -1
    assert reinforce(amount=float("nan")) == -1
    torch.cuda.synchronize()
    assert torch.equal(meta, before) and bool((slots == -7).all()) and bool((keys == -7.0).all())
    assert not bool(out.any()) and not bool(ws.any())
    # and the same calls with good arguments work
    assert L.aura_bank_retention_keys(m, count, NOW, out.data_ptr(), None) == 0
    assert select() == 0
    torch.cuda.synchronize()
    assert sorted(slots.tolist()) == sorted(R.eviction_order(out.cpu(), 0)[:n].tolist())
    assert reinforce() == 0
    torch.cuda.synchronize()
    assert torch.equal(meta.cpu(), R.reinforce_reference(before.cpu(), count, rows.cpu(), 0.1, 1.0))
