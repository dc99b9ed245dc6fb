"""Host-side logic of ``forget`` / ``prune`` / ``consolidate`` on the CPU (``ops`` replaced by tests/cpu_stub_forget.py,
whose ``bank_compact`` is the move in torch): the kill set, the id maps over split implicit ranges, the state round trip,
the cleared tail, the centroid counts, a wrapped ring, and ``consolidate`` against a fresh bank fed the same rows through
consolidating writes."""
import pickle

import numpy as np
import pytest
import torch

from tests import cpu_stub_forget as stub

NOW = 1.7e9 + 9.0


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    stub.FIND_SIZES.clear()
    stub.MOVES.clear()
    return H


def _hf(H, D=16, M=64, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _ids(a, b, p="m"):
    return [f"{p}{i}" for i in range(a, b)]


def _filled(H, n=12, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(n, 16, generator=g)
    hf = _hf(H, **kw)
    hf.create_episodic_memories(_ids(0, n), feats)
    hf.memory_locations[:n] = torch.arange(n, dtype=torch.float32)[:, None]
    hf.memory_metadata[:n, 0] = torch.linspace(0.2, 0.9, n)
    hf._slot_time[:n] = NOW + np.arange(n)
    return hf, feats


class _NoOps:
    def __getattr__(self, name):
        raise AssertionError(f"ops.{name} was used")


def test_forget_by_rows(hmod):
    hf, feats = _filled(hmod)
    meta = hf.memory_metadata.clone()
    inv = hf._inv_norm.clone()
    rep = hf.forget(rows=torch.tensor([[3, -1], [7, 3], [99, 12]]))            # -1, outside and duplicates: ignored
    keep = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]
    assert isinstance(rep, hmod.CompactionReport) and rep.n_removed == 2 and hf.memory_count == 10
    want = np.full(12, -1)
    want[keep] = np.arange(10)
    assert rep.old_to_new.dtype == np.int64 and rep.old_to_new.tolist() == want.tolist()
    assert torch.equal(hf.memory_features[:10], feats[keep]) and torch.equal(hf.memory_metadata[:10], meta[keep])
    assert torch.equal(hf._inv_norm[:10], inv[keep])
    assert hf.memory_locations[:10, 0].tolist() == [float(i) for i in keep]
    # the freed tail is cleared: what was forgotten is not in the state_dict
    for name in ("memory_features", "memory_locations", "memory_metadata"):
        assert not bool(hf.state_dict()[name][10:].any()), name
    # host maps
    assert [hf.id_of_row(r) for r in range(10)] == [f"m{i}" for i in keep]
    assert hf.id_to_idx == {f"m{i}": r for r, i in enumerate(keep)} and list(hf.id_to_idx) == [f"m{i}" for i in keep]
    assert "m3" not in hf.episodic_memories and len(hf.episodic_memories) == 10
    assert hf.episodic_memories["m8"].feature_idx == 6 and hf.episodic_memories["m8"].timestamp == NOW + 8
    assert hf._slot_time[:10].tolist() == [NOW + i for i in keep] and not hf._slot_time[10:].any()
    assert hf._idx_to_id[10:12] == [None, None] and hf._write_cursor == 0 and hf._norms_valid_upto == 10
    assert stub.CALLS["compact"] == 1 and stub.MOVES == [(10, 0, 7)]
    # later writes append behind the survivors
    hf.create_episodic_memories(["x"], torch.ones(1, 16))
    assert hf.memory_count == 11 and hf.id_of_row(10) == "x"
    # recall sees the survivors only
    hf.memory_metadata[:11, 0] = 1.0                                 # (equal strengths: the cosine decides)
    _, rows = hf.recall_batch(feats[[3, 4]], k=1, now=NOW)
    assert rows[1].item() == 3 and hf.id_of_row(int(rows[0])) != "m3"


def test_forget_by_ids_and_unknown_ids(hmod):
    hf, feats = _filled(hmod)
    with pytest.raises(KeyError):
        hf.forget(ids=["m2", "nobody"])
    assert hf.memory_count == 12 and "m2" in hf.id_to_idx and stub.CALLS["compact"] == 0
    rep = hf.forget(rows=[11], ids=["m0", "m5"])
    assert rep.n_removed == 3 and hf.memory_count == 9
    assert [hf.id_of_row(r) for r in range(9)] == [f"m{i}" for i in (1, 2, 3, 4, 6, 7, 8, 9, 10)]
    assert rep.old_to_new.tolist() == [-1, 0, 1, 2, 3, -1, 4, 5, 6, 7, 8, -1]
    assert torch.equal(hf.memory_features[:9], feats[[1, 2, 3, 4, 6, 7, 8, 9, 10]])


def test_an_empty_kill_set_uses_no_op(hmod, monkeypatch):
    hf, feats = _filled(hmod)
    before = (hf.memory_features.clone(), hf.memory_metadata.clone(), dict(hf.id_to_idx), hf._slot_time.copy())
    monkeypatch.setattr(hmod, "ops", _NoOps())
    for kw in (dict(), dict(rows=[]), dict(rows=torch.tensor([-1, 12, 500])), dict(ids=[]), dict(rows=np.zeros((0, 3)))):
        rep = hf.forget(**kw)
        assert rep.n_removed == 0 and rep.old_to_new.tolist() == list(range(12))
    assert hf.memory_count == 12 and torch.equal(hf.memory_features, before[0]) and torch.equal(hf.memory_metadata, before[1])
    assert hf.id_to_idx == before[2] and np.array_equal(hf._slot_time, before[3])
    empty = _hf(hmod)
    assert empty.forget(rows=[0, 1]).n_removed == 0 and empty.forget(rows=[0]).old_to_new.size == 0


def test_forget_everything(hmod):
    hf, feats = _filled(hmod)
    rep = hf.forget(rows=np.arange(12))
    assert rep.n_removed == 12 and hf.memory_count == 0 and (rep.old_to_new == -1).all()
    assert hf.id_to_idx == {} and len(hf.episodic_memories) == 0 and hf._idx_to_id[:12] == [None] * 12
    assert not bool(hf.memory_features.any()) and not bool(hf.memory_metadata.any()) and not hf._slot_time.any()
    assert hf.recall_batch(feats[:2], k=3)[1].shape == (2, 0)
    hf.create_episodic_memories(["again"], feats[:1])
    assert hf.memory_count == 1 and hf.id_of_row(0) == "again" and torch.equal(hf.memory_features[0], feats[0])
    # the last row alone: nothing changes place
    stub.MOVES.clear()
    hf2, _ = _filled(hmod)
    assert hf2.forget(rows=[11]).n_removed == 1 and stub.MOVES == [(11, 0, 0)] and hf2.memory_count == 11


def test_implicit_ids_over_split_ranges_and_the_state_round_trip(hmod):
    g = torch.Generator().manual_seed(1)
    hf = _hf(hmod)
    hf.bulk_write(torch.randn(10, 16, generator=g), id_prefix="bulk-", first_index=100, rebuild=False)   # rows 0..9
    hf.create_episodic_memories(_ids(0, 3, "e"), torch.randn(3, 16, generator=g))                        # rows 10..12
    hf.bulk_write(torch.randn(5, 16, generator=g), id_prefix="b2-", rebuild=False)                       # rows 13..17
    feats = hf.memory_features[:18].clone()
    before = [hf.id_of_row(r) for r in range(18)]
    assert before[:2] == ["bulk-100", "bulk-101"] and before[10] == "e0" and before[13] == "b2-0"
    gone = [0, 4, 5, 11, 17]
    keep = [r for r in range(18) if r not in gone]
    rep = hf.forget(rows=gone)
    assert rep.n_removed == 5 and hf.memory_count == 13
    assert [hf.id_of_row(r) for r in range(13)] == [before[r] for r in keep]
    assert torch.equal(hf.memory_features[:13], feats[keep])
    # implicit ids stay implicit: no string per bulk row, one entry per range, the thinned range as an index array
    assert hf._idx_to_id[:13].count(None) == 11 and hf.id_to_idx == {"e0": 7, "e2": 8}
    assert len(hf._implicit_ids) == 2
    (a0, a1, ap, an), (b0, b1, bp, bn) = sorted(hf._implicit_ids, key=lambda e: e[0])
    assert (a0, a1, ap) == (0, 7, "bulk-") and isinstance(an, np.ndarray) and an.tolist() == [101, 102, 103, 106, 107, 108, 109]
    assert (b0, b1, bp, bn) == (9, 13, "b2-", 0)                      # only its end was cut: still first index + offset
    # a second compaction thins the thinned range again; a range cut at its start keeps the arithmetic form
    hf.forget(rows=[1, 9])
    assert [hf.id_of_row(r) for r in range(11)] == [before[r] for r in keep if r not in (2, 13)]
    assert sorted(hf._implicit_ids, key=lambda e: e[0])[1] == (8, 11, "b2-", 1)
    # round trip through state_dict + bank_state (pickled, as a checkpoint would be)
    other = _hf(hmod)
    other.load_state_dict(hf.state_dict())
    other.load_bank_state(pickle.loads(pickle.dumps(hf.bank_state())))
    assert other.memory_count == 11 and other.id_to_idx == hf.id_to_idx
    assert [other.id_of_row(r) for r in range(11)] == [hf.id_of_row(r) for r in range(11)]
    assert np.array_equal(other._slot_time, hf._slot_time) and torch.equal(other.memory_features, hf.memory_features)
    other.forget(rows=[0])                                            # and the loaded form compacts again
    assert [other.id_of_row(r) for r in range(10)] == [hf.id_of_row(r) for r in range(1, 11)]


def test_a_state_saved_before_compaction_existed_still_loads(hmod):
    g = torch.Generator().manual_seed(2)
    src = _hf(hmod)
    src.bulk_write(torch.randn(6, 16, generator=g), id_prefix="old-", first_index=7, rebuild=False)
    src.create_episodic_memories(["a", "b"], torch.randn(2, 16, generator=g))
    state = {"memory_count": 8, "index_ready": False, "write_cursor": 0, "centroids_k": 256,
             "centroids_update_interval": 512, "ids_by_slot": [None] * 6 + ["a", "b"], "id_to_idx": {"a": 6, "b": 7},
             "slot_time": np.full(8, NOW).tobytes(), "implicit_ids": [(0, 6, "old-", 7)]}
    assert set(state) == set(src.bank_state())                        # the keys a bank writes today
    hf = _hf(hmod)
    hf.load_state_dict(src.state_dict())
    hf.load_bank_state(state)
    assert [hf.id_of_row(r) for r in range(8)] == [f"old-{i}" for i in range(7, 13)] + ["a", "b"]
    hf.forget(rows=[2], ids=["a"])
    assert [hf.id_of_row(r) for r in range(6)] == ["old-7", "old-8", "old-10", "old-11", "old-12", "b"]


def test_centroid_counts_lose_the_removed_rows(hmod):
    hf, _ = _filled(hmod)
    cids = torch.tensor([0, 1, 1, 2, 2, 2, 3, -1, 5, 5, 255, 0], dtype=torch.float32)
    hf.memory_metadata[:12, 2] = cids
    hf.centroid_counts[:] = torch.bincount(cids[cids >= 0].long(), minlength=256).float()
    means = torch.randn_like(hf.centroids)
    hf.centroids.copy_(means)
    hf.forget(rows=[1, 3, 7, 10, 11])
    left = cids[[0, 2, 4, 5, 6, 8, 9]]
    assert torch.equal(hf.centroid_counts, torch.bincount(left.long(), minlength=256).float())
    assert torch.equal(hf.memory_metadata[:7, 2], left) and torch.equal(hf.centroids, means)      # the means stay


def test_a_wrapped_fifo_ring_comes_out_oldest_first(hmod):
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(13, 16, generator=g)
    hf = _hf(hmod, M=8, overflow="fifo")
    for i in range(13):
        hf.create_episodic_memories([f"m{i}"], feats[i:i + 1])
    assert hf.memory_count == 8 and hf._write_cursor % 8 == 5
    assert [hf.id_of_row(r) for r in range(8)] == ["m8", "m9", "m10", "m11", "m12", "m5", "m6", "m7"]
    hf._slot_time[:8] = NOW + np.array([8, 9, 10, 11, 12, 5, 6, 7])
    rep = hf.forget(ids=["m6", "m9"])
    alive = [5, 7, 8, 10, 11, 12]                                     # oldest first
    assert rep.n_removed == 2 and hf.memory_count == 6 and hf._write_cursor == 0
    assert [hf.id_of_row(r) for r in range(6)] == [f"m{i}" for i in alive]
    assert torch.equal(hf.memory_features[:6], feats[alive]) and not bool(hf.memory_features[6:].any())
    assert rep.old_to_new.tolist() == [2, -1, 3, 4, 5, 0, -1, 1]
    assert hf._slot_time[:6].tolist() == [NOW + i for i in alive]
    assert torch.equal(hf._inv_norm[:6], 1.0 / feats[alive].norm(dim=1).clamp_min(1e-12))
    # the next writes append, then overwrite the oldest
    new = torch.randn(4, 16, generator=g)
    hf.create_episodic_memories(_ids(0, 4, "n"), new)
    assert hf.memory_count == 8
    assert [hf.id_of_row(r) for r in range(8)] == ["n2", "n3", "m8", "m10", "m11", "m12", "n0", "n1"]
    assert torch.equal(hf.memory_features[[6, 7, 0, 1]], new)


def test_prune(hmod):
    hf, feats = _filled(hmod)
    strength = hf.memory_metadata[:12, 0].clone()
    with pytest.raises(ValueError):
        hf.prune()
    rep = hf.prune(min_strength=0.5)
    keep = torch.nonzero(strength >= 0.5).flatten().tolist()
    assert rep.n_removed == 12 - len(keep) and hf.memory_count == len(keep)
    assert [hf.id_of_row(r) for r in range(len(keep))] == [f"m{i}" for i in keep]
    assert hf.prune(min_strength=0.5).n_removed == 0 and stub.CALLS["compact"] == 1
    # by retention key: strength * exp(-age / 3600)
    hf2, _ = _filled(hmod)
    hf2.memory_metadata[:12, 0] = 1.0
    hf2.memory_metadata[:12, 1] = torch.tensor([NOW - 3600.0 * i for i in range(12)])
    keys = hf2.retention_keys(NOW)
    rep = hf2.prune(min_key=0.01, now=NOW)
    assert rep.n_removed == int((keys < 0.01).sum()) and 0 < rep.n_removed < 12
    assert [hf2.id_of_row(r) for r in range(hf2.memory_count)] == [f"m{i}" for i in range(12) if keys[i] >= 0.01]
    both = _filled(hmod)[0]
    assert both.prune(min_strength=0.25, min_key=0.85, now=NOW).n_removed == int(((strength < 0.25) | (strength < 0.85)).sum())
    assert _hf(hmod).prune(min_strength=1.0).n_removed == 0


def _hand_made(seed=4):
    """14 rows: four groups of near-copies spread over the slabs of 4, degenerate rows, and rows of their own."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(8, 16, generator=g)
    rows = torch.stack([b[0], b[1], b[0] * 2.0, b[2],                # 2 repeats 0 inside the first slab
                        b[1] + 1e-4 * b[3], b[3], torch.zeros(16), b[3] * 0.5,     # 4 -> stored 1; 7 -> leader 5
                        b[4], b[0] + 1e-4 * b[5], b[4] * 3.0, b[5],  # 9 -> stored 0; 10 -> leader 8
                        b[5] * 1.5, torch.zeros(16)])                # 12 -> stored; a second zero row is kept
    rows[3, 2] = float("nan")                                         # a NaN row is kept
    return rows


def _same_bank(a, b):
    assert a.memory_count == b.memory_count
    n = a.memory_count
    assert [a.id_of_row(r) for r in range(n)] == [b.id_of_row(r) for r in range(n)]
    for name in ("memory_features", "memory_locations", "memory_metadata"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0)), name
    assert torch.equal(torch.nan_to_num(a._inv_norm[:n], nan=-1.0), torch.nan_to_num(b._inv_norm[:n], nan=-1.0))
    assert a.id_to_idx == b.id_to_idx


@pytest.mark.parametrize("slab", [4, 1024])
def test_consolidate_equals_the_replay_through_consolidating_writes(hmod, monkeypatch, slab):
    monkeypatch.setattr(stub, "CONSOLIDATE_MAX_BATCH", slab)
    if slab == 4:
        rows = _hand_made()
    else:
        g = torch.Generator().manual_seed(5)
        base = torch.randn(1100, 16, generator=g)
        rows = torch.cat([base, base[:300] * 1.5])[torch.randperm(1400, generator=g)]
    n = rows.shape[0]
    hf = _hf(hmod, M=2048)
    hf.create_episodic_memories(_ids(0, n), rows)                                    # every row is stored
    assert hf.memory_count == n
    with pytest.raises(ValueError):
        hf.consolidate()                                                             # no threshold anywhere
    with pytest.raises(ValueError):
        hf.consolidate(1.5)
    rep = hf.consolidate(0.999)
    fresh = _hf(hmod, M=2048)
    wrep = fresh.create_episodic_memories(_ids(0, n), rows, merge_similarity=0.999)
    _same_bank(hf, fresh)
    assert isinstance(rep, hmod.BankConsolidationReport)
    assert (rep.n_before, rep.n_kept, rep.n_merged) == (n, wrep.n_stored, wrep.n_merged) and rep.n_merged > 0
    assert rep.old_to_new.tolist() == wrep.rows.tolist()              # where the memory every row became is held
    assert stub.FIND_SIZES[:-(-n // slab)] == [min(slab, n - lo) for lo in range(0, n, slab)]
    assert not bool(hf.memory_features[rep.n_kept:].any()) and hf._write_cursor == 0
    if slab == 4:
        assert rep.n_kept == 8 and rep.old_to_new.tolist() == [0, 1, 0, 2, 1, 3, 4, 3, 5, 0, 5, 6, 6, 7]
    # the default threshold is the bank's own
    own = _hf(hmod, M=2048, merge_similarity=0.999)
    own.create_episodic_memories(_ids(0, n), rows, merge_similarity=None)
    assert own.consolidate().n_kept == rep.n_kept
    assert hf.consolidate(0.999).n_merged == 0                        # nothing left to merge


def test_a_kept_memory_takes_the_largest_strength_and_the_latest_timestamp(hmod, monkeypatch):
    monkeypatch.setattr(stub, "CONSOLIDATE_MAX_BATCH", 3)
    g = torch.Generator().manual_seed(6)
    b = torch.randn(3, 16, generator=g)
    rows = torch.stack([b[0], b[1], b[0] * 2.0,                       # slab 1: 2 repeats its leader 0
                        b[0] * 3.0, b[2], b[1] * 0.5,                 # slab 2: 3 -> stored 0, 5 -> stored 1
                        b[0] * 4.0])                                  # slab 3: 6 -> stored 0
    hf = _hf(hmod, merge_reinforce=0.05, merge_cap=0.97)
    hf.create_episodic_memories(_ids(0, 7), rows)
    hf.memory_metadata[:7, 0] = torch.tensor([0.30, 0.50, 0.60, 0.20, 0.40, 0.45, 0.95])
    hf.memory_metadata[:7, 1] = torch.tensor([100.0, 200.0, 50.0, 700.0, 300.0, 150.0, 20.0])
    hf._slot_time[:7] = [100.0, 200.0, 50.0, 700.0, 300.0, 150.0, 20.0]
    rep = hf.consolidate(0.999)
    assert rep.n_kept == 3 and rep.old_to_new.tolist() == [0, 1, 0, 0, 2, 1, 0]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)             # noqa: E731
    # m0: the leader takes 0.60 in slab 1 (no reinforcement: an in-slab leader); a stored target in slab 2: max(0.60,
    # 0.20) + 0.05; in slab 3: max(0.65, 0.95) = 0.95, below the cap 0.97 -> reinforced to the cap
    want0 = torch.minimum(torch.maximum(f32(0.60) + f32(0.05), f32(0.95)) + f32(0.05), f32(0.97))
    assert hf.memory_metadata[0, 0] == want0 and hf.memory_metadata[0, 1].item() == 700.0
    # m1: a stored target once: max(0.50, 0.45) + 0.05, the later of the two timestamps
    assert hf.memory_metadata[1, 0] == f32(0.50) + f32(0.05) and hf.memory_metadata[1, 1].item() == 200.0
    assert hf.memory_metadata[2, 0] == f32(0.40) and hf.memory_metadata[2, 1].item() == 300.0
    assert hf._slot_time[:3].tolist() == [700.0, 200.0, 300.0]
    assert [hf.id_of_row(r) for r in range(3)] == ["m0", "m1", "m4"] and stub.CALLS["reinforce"] == 2
    assert torch.equal(hf.memory_features[:3], rows[[0, 1, 4]])      # the first observation stands


def test_a_failing_slab_leaves_a_consistent_bank(hmod, monkeypatch):
    monkeypatch.setattr(stub, "CONSOLIDATE_MAX_BATCH", 4)
    rows = _hand_made()
    hf = _hf(hmod)
    hf.create_episodic_memories(_ids(0, 14), rows)
    real, calls = stub.find_repeats, []

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("the second slab fails")
        return real(*a, **kw)
    monkeypatch.setattr(stub, "find_repeats", failing)
    with pytest.raises(RuntimeError, match="second slab"):
        hf.consolidate(0.999)
    keep = [0, 1, 3] + list(range(4, 14))                             # slab 1 decided, the rest moved down unchanged
    assert hf.memory_count == 13 and [hf.id_of_row(r) for r in range(13)] == [f"m{i}" for i in keep]
    assert torch.equal(torch.nan_to_num(hf.memory_features[:13]), torch.nan_to_num(rows[keep]))
    assert not bool(hf.memory_features[13:].any()) and hf.id_to_idx == {f"m{i}": r for r, i in enumerate(keep)}
    assert hf._norms_valid_upto == 13 and hf._write_cursor == 0
    monkeypatch.setattr(stub, "find_repeats", real)
    rep = hf.consolidate(0.999)                                       # and the pass can simply be run again
    assert rep.n_kept == 8 and [hf.id_of_row(r) for r in range(8)] == [f"m{i}" for i in (0, 1, 3, 5, 6, 8, 11, 13)]


def test_consolidate_on_a_wrapped_ring_and_with_the_index(hmod, monkeypatch):
    g = torch.Generator().manual_seed(7)
    b = torch.randn(8, 16, generator=g)
    hf = _hf(hmod, M=8, overflow="fifo")
    seq = [b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[5] * 2.0, b[7], b[6] * 2.0, b[4] * 2.0]
    for i, f in enumerate(seq):
        hf.create_episodic_memories([f"m{i}"], f[None])
    # held, oldest first: m3 .. m10; m7 repeats m5, m9 repeats m6, m10 repeats m4
    rep = hf.consolidate(0.999)
    assert rep.n_before == 8 and rep.n_kept == 5 and [hf.id_of_row(r) for r in range(5)] == ["m3", "m4", "m5", "m6", "m8"]
    # rows as they were: m8 m9 m10 m3 m4 m5 m6 m7
    assert rep.old_to_new.tolist() == [4, 3, 1, 0, 1, 2, 3, 2]
    # with the index in use the pass ends in a rebuild
    big = _hf(hmod, M=400, use_centroid_index=True)
    big.centroids_k, big.centroids_update_interval = 8, 10 ** 9
    base = torch.randn(60, 16, generator=g)
    big.bulk_write(torch.cat([base, base[:20] * 2.0]), rebuild=True)
    assert big._index_ready and big.memory_count == 80
    rebuilt = []
    real = big.rebuild_centroids
    monkeypatch.setattr(big, "rebuild_centroids", lambda *a, **k: (rebuilt.append(1), real(*a, **k))[1])
    torch.manual_seed(1)
    rep = big.consolidate(0.999)
    assert rep.n_kept == 60 and rebuilt == [1] and float(big.centroid_counts.sum()) == 60.0
    assert [big.id_of_row(r) for r in (0, 59)] == ["bulk-0", "bulk-59"] and big._implicit_ids == [(0, 60, "bulk-", 0)]
    big.bulk_write(base[:10] * 3.0, id_prefix="again-", rebuild=True)
    rep = big.consolidate(0.999, rebuild=False)
    assert rep.n_kept == 60 and rebuilt == [1, 1] and float(big.centroid_counts.sum()) == 60.0   # (bulk_write's rebuild)
    _, rows = big.recall_batch(base[:5], k=1, now=NOW)
    assert rows.flatten().tolist() == [0, 1, 2, 3, 4]


def test_layer_helper(hmod):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    g = torch.Generator().manual_seed(8)
    base = torch.randn(5, 16, generator=g)
    hf = _hf(hmod)
    hf.create_episodic_memories(_ids(0, 8), torch.cat([base, base[:3] * 2.0]))

    class Layer(MO.BatchedMemoryMixin):
        hippocampus = hf
    rep = Layer().consolidate_memory(similarity=0.999)
    assert rep.n_kept == 5 and rep.n_merged == 3 and hf.memory_count == 5
    assert MO.MemoryInjection(hf, 16, num_heads=2).consolidate_memory(0.999).n_merged == 0
