"""Host-side logic of the retention feature on CPU (the three new ops replaced by
tests/cpu_stub_retention.py, which restates the rule with torch): slot planning of
``overflow='weakest'``, the split of runs that would evict more rows than the bank holds, the
transactional write, the sharded refusal, and that recall without ``reinforce`` launches nothing."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_retention as stub

NOW = 1.7e9 + 5.0


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    return H


def _hf(H, D=16, M=8, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M,
                                  feature_dim=D, device="cpu", **kw)


def _ids(a, b):
    return [f"m{i}" for i in range(a, b)]


def test_constructor_names_the_three_policies(hmod):
    assert _hf(hmod, overflow="weakest")._overflow == "weakest"
    with pytest.raises(ValueError) as e:
        _hf(hmod, overflow="lru")
    for name in ("'reference'", "'fifo'", "'weakest'"):
        assert name in str(e.value)


def test_append_only_plans_without_a_selection(hmod):
    hf = _hf(hmod, overflow="weakest")
    hf.create_episodic_memories(_ids(0, 5), torch.randn(5, 16))
    assert hf.memory_count == 5 and hf._write_cursor == 0 and stub.CALLS["select"] == 0
    assert [hf.id_to_idx[m] for m in _ids(0, 5)] == [0, 1, 2, 3, 4]


def test_mixed_append_and_evict_takes_the_weakest_of_the_rows_held_before(hmod):
    hf = _hf(hmod, overflow="weakest")
    feats = torch.randn(12, 16)
    hf.create_episodic_memories(_ids(0, 6), feats[:6])
    hf.memory_metadata[:6, 0] = torch.tensor([0.9, 0.2, 0.8, 0.1, 0.2, 0.7])     # rows 3, then 1 and 4 (tie: ring order)
    hf.create_episodic_memories(_ids(6, 11), feats[6:11])          # 2 append (rows 6, 7), 3 evict
    assert hf.memory_count == 8 and hf._write_cursor == 3 and stub.CALLS["select"] == 1
    assert [hf.id_to_idx[m] for m in _ids(6, 11)] == [6, 7, 3, 1, 4]
    assert [hf.id_of_row(r) for r in range(8)] == ["m0", "m9", "m2", "m8", "m10", "m5", "m6", "m7"]
    assert torch.equal(hf.memory_features[[3, 1, 4]], feats[8:11])
    assert torch.equal(hf.memory_metadata[[3, 1, 4], 0], torch.ones(3))
    # the tie between rows 1 and 4 follows the cursor: with the cursor at 3, row 4 goes before row 1
    hf.memory_metadata[:8, 0] = torch.tensor([0.9, 0.2, 0.8, 0.9, 0.2, 0.7, 0.9, 0.9])
    rows, keys = hf.weakest(2, now=NOW)
    assert rows.tolist() == [4, 1] and torch.equal(keys, hf.retention_keys(now=NOW)[rows])
    hf.create_episodic_memory("m11", "e", feats[11])
    assert hf.id_to_idx["m11"] == 4 and hf._write_cursor == 4


def test_equal_keys_are_the_ring(hmod):
    feats = torch.randn(30, 16)
    banks = [_hf(hmod, M=7, overflow=o) for o in ("fifo", "weakest")]
    for hf in banks:
        for a, b in ((0, 5), (5, 9), (9, 12), (12, 18), (18, 19), (19, 30)):
            hf.create_episodic_memories(_ids(a, b), feats[a:b])
    f, w = banks
    assert torch.equal(f.memory_features, w.memory_features) and torch.equal(f.memory_metadata, w.memory_metadata)
    assert f.id_to_idx == w.id_to_idx and f._idx_to_id == w._idx_to_id and f._write_cursor == w._write_cursor


def test_a_run_that_would_evict_more_than_the_bank_holds_is_split(hmod):
    hf = _hf(hmod, M=4, overflow="weakest")
    feats = torch.randn(11, 16)
    hf.create_episodic_memories(_ids(0, 2), feats[:2])
    hf.create_episodic_memories(_ids(2, 11), feats[2:11])          # room for 2, then 7 evictions from a bank of 4
    assert hf.memory_count == 4 and hf._write_cursor == 7
    # runs of at most max_memories rows: [2 append + 2 evict], [4 evict], [1 evict]; equal keys: the ring
    assert stub.CALLS["select"] == 3
    assert [hf.id_of_row(r) for r in range(4)] == ["m8", "m9", "m10", "m7"]
    assert torch.equal(hf.memory_features, feats[[8, 9, 10, 7]])
    with pytest.raises(ValueError):
        hf._plan_slots(9, NOW)                                     # the planner itself refuses rest > count


def test_failed_launch_leaves_the_counters_untouched(hmod, monkeypatch):
    hf = _hf(hmod, M=4, overflow="weakest")
    feats = torch.randn(6, 16)
    hf.create_episodic_memories(_ids(0, 4), feats[:4])
    hf.create_episodic_memory("m4", "e", feats[4])
    before = (hf.memory_count, hf._write_cursor, dict(hf.id_to_idx), list(hf._idx_to_id))

    def boom(*a, **k):
        raise RuntimeError("launch failed")
    monkeypatch.setattr(stub, "bank_write", boom)
    with pytest.raises(RuntimeError):
        hf.create_episodic_memory("bad", "e", feats[5])
    assert (hf.memory_count, hf._write_cursor, hf.id_to_idx, hf._idx_to_id) == before
    monkeypatch.undo()
    monkeypatch.setattr(stub, "bank_select_weakest", boom)
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    with pytest.raises(RuntimeError):
        hf.create_episodic_memory("bad", "e", feats[5])
    assert (hf.memory_count, hf._write_cursor, hf.id_to_idx, hf._idx_to_id) == before


def test_weakest_on_a_sharded_bank_raises(hmod):
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    with pytest.raises(ValueError, match="weakest"):
        ShardedHippocampus(_hf(hmod, overflow="weakest"), 8, ops_module=stub, now_fn=lambda: NOW)
    local = _hf(hmod, overflow="fifo")
    sh = ShardedHippocampus(local, 8, ops_module=stub, now_fn=lambda: NOW)
    sh.write(_ids(0, 3), torch.randn(3, 16))
    local._overflow = "weakest"                                     # switched under a live sharded bank
    with pytest.raises(ValueError, match="weakest"):
        sh.write(_ids(3, 5), torch.randn(2, 16))
    assert sh.memory_count == 3
    local.reinforce(torch.tensor([0, 2]), amount=0.0)               # rows are local: works as on any bank


def test_recall_reinforces_only_when_asked_and_once(hmod):
    hf = _hf(hmod, M=32, overflow="weakest")
    feats = torch.randn(20, 16)
    hf.create_episodic_memories(_ids(0, 20), feats)
    hf.decay_memories(0.5)
    s0, r0 = hf.recall_batch(feats[:3], k=2, now=NOW)
    assert stub.CALLS["reinforce"] == 0 and torch.equal(hf.memory_metadata[:20, 0], torch.full((20,), 0.5))
    s1, r1 = hf.recall_batch(feats[:3], k=2, now=NOW, reinforce=0.25)
    assert stub.CALLS["reinforce"] == 1 and torch.equal(r0, r1) and torch.equal(s0, s1)
    hit = torch.zeros(20, dtype=torch.bool)
    hit[r1.reshape(-1).long()] = True
    assert torch.equal(hf.memory_metadata[:20, 0], torch.where(hit, torch.tensor(0.75), torch.tensor(0.5)))
    hf.reinforce([[0, 0, -1], [0, 99, 1]], amount=0.5, cap=0.9)     # duplicates, -1, out of range
    assert hf.memory_metadata[0, 0].item() == pytest.approx(0.9) and hf.memory_metadata[1, 0].item() == pytest.approx(0.9)
    # the layer helper passes the option through, default off
    from aura_snn_rag_amd.core.language_zone.memory_ops import retrieve_memories
    n = stub.CALLS["reinforce"]
    retrieve_memories(hf, feats[:2], k=2)
    assert stub.CALLS["reinforce"] == n
    retrieve_memories(hf, feats[:2], k=2, reinforce=0.1)
    assert stub.CALLS["reinforce"] == n + 1


def test_reinforce_invalidates_the_cached_score_constants(hmod):
    hf = _hf(hmod, M=32, overflow="weakest")
    hf.create_episodic_memories(_ids(0, 4), torch.randn(4, 16))

    class Ivf:
        rowc_live = True
    hf._ivf = Ivf()
    hf.reinforce(torch.tensor([1]), amount=0.1)
    assert hf._ivf.rowc_live is False
