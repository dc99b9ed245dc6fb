"""Host-side logic of tags and scoped recall on the CPU (``ops`` replaced by tests/cpu_stub_scoped.py, whose
``bank_set_tags`` and ``knn_search_scoped`` restate the rule in torch): tags through every write path and every overflow
policy, through the compactions and a state round trip, ``forget(tags=)``, ``retag``, every argument error, the
pass-through into diverse recall and ``reinforce``, and the plan the host builds for the library."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_scoped as stub

NOW = 1.7e9 + 9.0
STATE_KEYS = {"memory_count", "index_ready", "write_cursor", "centroids_k", "centroids_update_interval", "ids_by_slot",
              "id_to_idx", "slot_time", "implicit_ids"}


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    stub.STAMPS.clear()
    stub.MOVES.clear()
    stub.FIND_SIZES.clear()
    stub.LAST_SCOPED.clear()
    return H


def _hf(H, D=16, M=64, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _ids(a, b, p="m"):
    return [f"{p}{i}" for i in range(a, b)]


def _feats(n, D=16, seed=0):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


def _tags(hf):
    return hf.memory_tags.tolist()


# ------------------------------------------------------------------ tags reach column 3
def test_tags_through_every_write_path(hmod):
    hf = _hf(hmod)
    f = _feats(20)
    hf.create_episodic_memories(_ids(0, 4), f[:4], tags=[3, 1, 4, 1])
    hf.create_episodic_memories(_ids(4, 6), f[4:6], tags=9)                            # one int for every row
    hf.create_episodic_memory("m6", "event", f[6], associated_experts=["x"], tag=5)   # event_id stays unused
    hf.create_episodic_memories(_ids(7, 9), f[7:9])                                    # untagged
    assert hf.bulk_write(f[9:12], tags=np.array([7, 7, 8])) == 3
    hf.write_at(_ids(12, 14), f[12:14], np.array([12, 13]), 2, NOW, tags=torch.tensor([6, 2]))
    assert _tags(hf) == [3, 1, 4, 1, 9, 9, 5, 0, 0, 7, 7, 8, 6, 2]
    assert hf.memory_tags.dtype == torch.int32 and hf.memory_metadata[:14, 3].tolist() == [float(t) for t in _tags(hf)]
    assert stub.CALLS["set_tags"] == 5                                                  # one launch per tagged write
    assert hf.memory_metadata[:14, 0].tolist() == [1.0] * 14                            # nothing else was touched
    # the layer-level store
    from aura_snn_rag_amd.core.language_zone import memory_ops
    memory_ops.store_memory(hf, torch.randn(2, 3, 16), tag=11)
    memory_ops.store_memory(hf, torch.randn(2, 3, 16), tag=[12, 13])
    memory_ops.store_memory(hf, torch.randn(1, 3, 16))
    assert _tags(hf)[14:] == [11, 11, 12, 13, 0]


def test_reference_policy_rewrites_one_slot_and_the_last_row_wins(hmod):
    hf = _hf(hmod, M=4, overflow="reference")
    hf.create_episodic_memories(_ids(0, 9), _feats(9), tags=np.arange(1, 10))
    assert _tags(hf) == [9, 2, 3, 4] and hf.id_of_row(0) == "m8"
    assert stub.STAMPS == [([1, 2, 3, 0], [2, 3, 4, 9])]                               # distinct slots, one launch
    hf.create_episodic_memories(["u"], _feats(1, seed=1))                              # untagged over a tagged slot
    assert _tags(hf) == [0, 2, 3, 4]


def test_fifo_wrap_and_weakest(hmod):
    hf = _hf(hmod, M=4, overflow="fifo")
    hf.create_episodic_memories(_ids(0, 6), _feats(6), tags=np.arange(1, 7))            # wraps onto its own appends
    assert _tags(hf) == [5, 6, 3, 4]
    hf.create_episodic_memories(_ids(6, 9), _feats(3, seed=2), tags=[7, 8, 9])
    assert _tags(hf) == [9, 6, 7, 8]
    hf = _hf(hmod, M=4, overflow="weakest")
    hf.create_episodic_memories(_ids(0, 4), _feats(4), tags=[1, 2, 3, 4])
    hf.memory_metadata[:4, 0] = torch.tensor([0.9, 0.1, 0.8, 0.2])
    hf.create_episodic_memories(_ids(4, 6), _feats(2, seed=3), tags=[5, 6])              # evicts rows 1, then 3
    assert _tags(hf) == [1, 5, 3, 6] and hf.id_of_row(1) == "m4" and hf.id_of_row(3) == "m5"


def test_untagged_writes_leave_the_bank_as_it_was(hmod):
    f = _feats(10)
    a = _hf(hmod, M=8, overflow="fifo")
    a.create_episodic_memories(_ids(0, 10), f)
    a.bulk_write(f[:0])
    assert stub.CALLS["set_tags"] == 0 and stub.CALLS["scoped"] == 0
    assert not bool(a.memory_metadata[:, 3].any())
    b = _hf(hmod, M=8, overflow="fifo")
    b.load_state_dict(a.state_dict())                                                   # same place / grid cells
    b.memory_count = 0
    b.memory_features.zero_(); b.memory_metadata.zero_(); b.memory_locations.zero_()
    b.create_episodic_memories(_ids(0, 10), f, tags=np.arange(10) + 1)
    b.retag(rows=np.arange(8), tag=0)                                                   # tags off again: no trace left
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert set(a.bank_state()) == STATE_KEYS


# ------------------------------------------------------------------ tags travel
def test_tags_survive_forget_prune_consolidate_and_a_round_trip(hmod):
    hf = _hf(hmod, M=32)
    f = _feats(12)
    f[7] = f[2] + 1e-4                                                                  # a near-copy, under another tag
    tags = [1, 2, 3, 1, 2, 3, 4, 9, 5, 5, 6, 7]
    hf.create_episodic_memories(_ids(0, 12), f, tags=tags)
    hf.forget(rows=[0, 4])
    assert _tags(hf) == [2, 3, 1, 3, 4, 9, 5, 5, 6, 7]
    hf.memory_metadata[:10, 0] = torch.tensor([1, 1, .1, 1, 1, 1, 1, .2, 1, 1])
    hf.prune(min_strength=0.5)
    assert _tags(hf) == [2, 3, 3, 4, 9, 5, 6, 7]
    rep = hf.consolidate(similarity=0.99)                                               # scope-blind: 9 merges into 3
    assert rep.n_merged == 1 and _tags(hf) == [2, 3, 3, 4, 5, 6, 7]
    assert not bool(hf.memory_metadata[7:, 3].any())                                    # the freed tail is cleared
    # state round trip: the tags are in the state_dict, bank_state has no new key
    state, bs = hf.state_dict(), hf.bank_state()
    assert set(bs) == STATE_KEYS
    other = _hf(hmod, M=32)
    other.load_state_dict(state)
    other.load_bank_state(bs)
    assert _tags(other) == [2, 3, 3, 4, 5, 6, 7] and other.id_of_row(0) == hf.id_of_row(0)
    _, rows = other.recall_batch(f[:3], k=4, now=NOW, tags=3)
    assert sorted(rows[0].tolist()) == [-1, -1, 1, 2]


def test_forget_by_tags(hmod):
    hf = _hf(hmod)
    f = _feats(9)
    hf.create_episodic_memories(_ids(0, 9), f, tags=[1, 2, 0, 1, 3, 2, 0, 1, 4])
    assert hf.forget(tags=[]).n_removed == 0 and hf.forget(tags=[99]).n_removed == 0 and stub.CALLS["compact"] == 0
    rep = hf.forget(tags=[1, 3], rows=[8])
    assert rep.n_removed == 5 and _tags(hf) == [2, 0, 2, 0]
    assert [hf.id_of_row(r) for r in range(4)] == ["m1", "m2", "m5", "m6"]
    assert hf.forget(tags=0).n_removed == 2 and _tags(hf) == [2, 2]                     # 0: the untagged rows
    with pytest.raises(ValueError):
        hf.forget(tags=[-1])
    assert hf.memory_count == 2


def test_retag(hmod):
    hf = _hf(hmod)
    hf.create_episodic_memories(_ids(0, 6), _feats(6), tags=[1, 1, 2, 2, 3, 3])
    assert hf.retag(rows=torch.tensor([[0, 5], [5, -1], [77, 0]]), tag=8) == 2          # -1, outside, duplicates: ignored
    assert _tags(hf) == [8, 1, 2, 2, 3, 8]
    assert hf.retag(ids=["m1", "m2"], tag=0) == 2 and _tags(hf) == [8, 0, 0, 2, 3, 8]
    assert hf.retag(rows=[3, 4], tag=[5, 6]) == 2 and _tags(hf) == [8, 0, 0, 5, 6, 8]
    before = stub.CALLS["set_tags"]
    with pytest.raises(KeyError):
        hf.retag(ids=["m0", "nobody"], tag=4)
    for bad in (dict(tag=1), dict(rows=[0], tag=1 << 24), dict(rows=[0], tag=-1), dict(rows=[0, 0], tag=[1, 2]),
                dict(rows=[0, 99], tag=[1, 2]), dict(rows=[0], tag=[1, 2]), dict(rows=[0], tag=1.5)):
        with pytest.raises(ValueError):
            hf.retag(**bad)
    assert stub.CALLS["set_tags"] == before and _tags(hf) == [8, 0, 0, 5, 6, 8]
    assert hf.retag(rows=[], tag=3) == 0


# ------------------------------------------------------------------ argument errors
def test_argument_errors(hmod):
    hf = _hf(hmod)
    f = _feats(4)
    for bad in ([1, 2, 3], [1, 2, 3, 1 << 24], [1, 2, 3, -1], [1.0, 2.0, 3.0, 4.0], 1 << 24):
        with pytest.raises(ValueError):
            hf.create_episodic_memories(_ids(0, 4), f, tags=bad)
    with pytest.raises(ValueError):
        hf.bulk_write(f, tags=[1, 2])
    with pytest.raises(ValueError):
        hf.write_at(_ids(0, 2), f[:2], np.array([0, 1]), 2, NOW, tags=[1])
    assert hf.memory_count == 0 and stub.CALLS["set_tags"] == 0
    with pytest.raises(ValueError, match="merge_similarity"):
        hf.create_episodic_memories(_ids(0, 4), f, tags=1, merge_similarity=0.9)
    merging = _hf(hmod, merge_similarity=0.9)
    with pytest.raises(ValueError, match="merge_similarity"):
        merging.create_episodic_memories(_ids(0, 4), f, tags=1)
    merging.create_episodic_memories(_ids(0, 4), f, tags=1, merge_similarity=None)      # tagged, not consolidating
    assert _tags(merging) == [1, 1, 1, 1]

    hf.create_episodic_memories(_ids(0, 4), f, tags=[1, 1, 2, 2])
    with pytest.raises(ValueError, match="use_candidates"):
        hf.recall_batch(f, k=2, tags=1, use_candidates=True)
    with pytest.raises(ValueError, match="use_candidates"):
        hf.recall_batch(f, k=2, min_strength=0.5, use_candidates=True)
    for bad in ([1, 2], 1 << 24, [1, 2, 1 << 24, 0], 1.5):
        with pytest.raises(ValueError):
            hf.recall_batch(f, k=2, tags=bad)
    big = _hf(hmod, M=256)
    big.bulk_write(_feats(200), tags=1, rebuild=False)
    with pytest.raises(ValueError, match="128"):
        big.recall_batch(f, k=129, tags=1)
    assert big.recall_batch(f, k=128, tags=1)[1].shape == (4, 128)
    assert big.recall_batch(f, k=129)[1].shape == (4, 129)                               # the plain recall has no such limit


def test_the_sharded_bank_rejects_the_new_arguments(hmod):
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    sh = ShardedHippocampus(_hf(hmod), 64, ops_module=stub, now_fn=lambda: NOW)
    f = _feats(3)
    with pytest.raises(ValueError, match="tags"):
        sh.write(_ids(0, 3), f, tags=[1, 2, 3])
    with pytest.raises(ValueError, match="tags"):
        sh.bulk_write(f, tags=1)
    sh.write(_ids(0, 3), f)
    for kw in (dict(tags=1), dict(newer_than=0.0), dict(older_than=NOW), dict(min_strength=0.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            sh.recall_batch(f, k=2, **kw)
    assert sh.recall_batch(f, k=2, now=NOW)[1].shape == (3, 2) and stub.CALLS["scoped"] == 0


# ------------------------------------------------------------------ recall
def test_scoped_recall_through_the_bank(hmod):
    hf = _hf(hmod)
    f = _feats(12)
    tags = [1, 2, 1, 2, 1, 2, 0, 0, 3, 3, 3, 1]
    hf.create_episodic_memories(_ids(0, 12), f, tags=tags)
    hf.memory_metadata[:12, 0] = torch.linspace(0.3, 0.9, 12)
    hf.memory_metadata[:12, 1] = torch.tensor(NOW) - 128.0 * torch.arange(12)
    s, r = hf.recall_batch(f[:4], k=5, now=NOW, tags=[1, 2, -1, 7])
    assert stub.CALLS["scoped"] == 1 and stub.LAST_SCOPED["tags"].tolist() == [1, 2, -1, 7]
    assert sorted(r[0].tolist()) == [-1, 0, 2, 4, 11] and r[0, 4] == -1 and s[0, 4] == -float("inf")
    assert sorted(r[1].tolist()) == [-1, -1, 1, 3, 5] and bool((r[2] >= 0).all()) and r[3].tolist() == [-1] * 5
    plain_s, plain_r = hf.recall_batch(f[:4], k=5, now=NOW)
    assert torch.equal(r[2], plain_r[2]) and torch.allclose(s[2], plain_s[2])           # "any" = the plain recall
    # the window is closed at both ends, on the fp32 timestamps
    ts = hf.memory_metadata[:12, 1]
    _, r = hf.recall_batch(f[:1], k=12, now=NOW, newer_than=float(ts[6]), older_than=float(ts[3]))
    assert sorted(x for x in r[0].tolist() if x >= 0) == [3, 4, 5, 6]
    _, r = hf.recall_batch(f[:1], k=12, now=NOW, min_strength=float(hf.memory_metadata[9, 0]), tags=3)
    assert sorted(x for x in r[0].tolist() if x >= 0) == [9, 10]
    # one query through retrieve_similar_memories and the layer functions
    got = hf.retrieve_similar_memories(f[8], k=5, tags=3)
    assert sorted(mid for mid, _ in got) == ["m10", "m8", "m9"]
    from aura_snn_rag_amd.core.language_zone import memory_ops
    feats, scores = memory_ops.retrieve_memories(hf, f[:2], k=4, tags=[3, 0])
    assert feats.shape == (2, 4, 16) and bool((feats[:, 3] == 0).all()) and bool((scores[0, :3] != 0).all())
    assert bool((scores[1, 2:] == 0).all()) and stub.LAST_SCOPED["tags"].tolist() == [3, 0]
    empty = _hf(hmod)
    assert empty.recall_batch(f[:2], k=3, tags=1)[1].shape == (2, 0) and empty.retrieve_similar_memories(f[0], tags=1) == []


def test_scope_passes_into_diverse_recall_and_reinforce(hmod):
    hf = _hf(hmod, M=128)
    f = _feats(60)
    hf.create_episodic_memories(_ids(0, 60), f, tags=[1 + (i % 3) for i in range(60)])
    hf.memory_metadata[:60, 0] = 0.5
    s, r = hf.recall_batch(f[:3], k=4, now=NOW, tags=2, diversity=0.3, max_similarity=0.95)
    assert stub.CALLS["scoped"] == 1 and stub.CALLS["diverse"] == 1 and stub.LAST_SCOPED["k"] == 32   # F = max(32, 4 k)
    assert bool((r >= 0).all()) and bool((hf.memory_tags[r.long().flatten()] == 2).all())
    s, r = hf.recall_batch(f[:3], k=4, now=NOW, tags=[1, 2, 3], min_strength=0.4, reinforce=0.25)
    assert stub.CALLS["scoped"] == 2 and stub.CALLS["reinforce"] == 1
    touched = torch.zeros(60, dtype=torch.bool)
    touched[r.long().flatten()] = True
    assert torch.equal(hf.memory_metadata[:60, 0] == 0.75, touched)
    assert all(int(hf.memory_tags[x]) == t for row, t in zip(r.tolist(), (1, 2, 3)) for x in row)


def test_a_call_without_scope_uses_neither_new_op(hmod, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a new op was used")
    monkeypatch.setattr(stub, "bank_set_tags", boom)
    monkeypatch.setattr(stub, "knn_search_scoped", boom)
    hf = _hf(hmod)
    f = _feats(10)
    hf.create_episodic_memories(_ids(0, 6), f[:6])
    hf.create_episodic_memory("x", "x", f[6])
    hf.bulk_write(f[7:9])
    hf.write_at(["y"], f[9:], np.array([9]), 1, NOW)
    hf.recall_batch(f[:2], k=3, now=NOW)
    hf.recall_batch(f[:2], k=3, now=NOW, reinforce=0.1)
    hf.recall_batch(f[:2], k=3, now=NOW, diversity=0.2)
    hf.retrieve_similar_memories(f[0], k=3)
    hf.forget(rows=[1])
    assert not bool(hf.memory_metadata[:, 3].any())


# ------------------------------------------------------------------ the plan of the library call (pure host code)
def test_the_plan_groups_queries_by_scope():
    from aura_snn_rag_amd import ops
    qt = ops.scoped_query_tags([5, -3, 5, 0, -1, 5], 6)
    assert qt.dtype == np.int32 and qt.tolist() == [5, -1, 5, 0, -1, 5]
    plan, S, T = ops.scoped_plan(qt)
    assert (S, T) == (3, 3) and plan.dtype == np.int32
    assert plan[:3].tolist() == [-1, 0, 5]                                              # "any" first, ascending
    assert plan[3:6].tolist() == [0, 1, 2] and plan[6:9].tolist() == [0, 2, 3] and plan[9:12].tolist() == [2, 1, 3]
    assert plan[12:].tolist() == [1, 4, 3, 0, 2, 5]                                     # stable within a scope
    # a scope of more than 64 queries takes several tiles
    plan, S, T = ops.scoped_plan(ops.scoped_query_tags(7, 150))
    assert (S, T) == (1, 3) and plan[1 + 2 * T:1 + 3 * T].tolist() == [64, 64, 22]
    assert ops.scoped_query_tags(None, 3).tolist() == [-1, -1, -1]
    for bad in ([1, 2], 1 << 24, [0.5, 1.0, 2.0]):
        with pytest.raises(ValueError):
            ops.scoped_query_tags(bad, 3)
    with pytest.raises(ops.AuraDeviceError):
        ops.knn_search_scoped(torch.zeros(4, 8), torch.zeros(4), torch.zeros(4, 4), torch.zeros(1, 8), 1, NOW, 4, tags=1)
    with pytest.raises(ops.AuraDeviceError):
        ops.bank_set_tags(torch.zeros(4, 4), 4, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
