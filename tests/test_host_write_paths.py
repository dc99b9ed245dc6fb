"""The write path's host planning, swept on the CPU: ``create_episodic_memories(ids, feats)`` must leave the bank
exactly as ``create_episodic_memory`` called once per row would, and no call into ``bank_write`` may hand the
parallel kernel a slot twice (``tests/cpu_stub_strict.py`` raises there; on the GPU two waves would then copy
different rows into one slot at the same time, which no CPU stand-in can show by its outcome).

Both sides of every comparison run the same stand-in arithmetic in the same row order, so equality is exact.

Cases that failed through the strict stand-in before ``_store_rows`` looked at the appended run (``'fifo'``,
index off, a batch that appends ``n_app > 0`` rows and overwrites ``rest`` with ``rows held < rest <= 64``):
rows held 0: batches 65, 68, 69, 100, 128; held 1 and 10: 65, 68, 69, 100; held 60: 65, 68; held 63: 65; the
random ``'fifo'`` / index-off sequences that cross the fill in one batch; the same shapes through
``ShardedHippocampus.write`` at world size 1; every ``write_at`` case with ``'fifo'`` and repeated slots."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_ops as plain
from tests import cpu_stub_strict as strict

NOW = 1.7e9 + 5.0
M, D, K, INTERVAL = 64, 8, 4, 16
HELD = (0, 1, 10, 60, 63, 64)
BATCHES = (1, 3, 4, 5, 54, 55, 63, 64, 65, 68, 69, 100, 128, 129, 200)
TENSORS = ("memory_features", "_inv_norm", "memory_metadata", "memory_locations", "centroids", "centroid_counts")


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", strict)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in strict.CALLS:
        strict.CALLS[k] = 0
    return H


def _hf(H, policy, index, m=M):
    hf = H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=m, feature_dim=D,
                                device="cpu", use_centroid_index=index, overflow=policy)
    hf.centroids_k, hf.centroids_update_interval = K, INTERVAL
    hf.update_spatial_state(torch.tensor([0.25, -1.0]))
    return hf


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=g) * (0.25 + 2 * torch.rand(n, 1, generator=g))


def _ids(a, b):
    return [f"m{i}" for i in range(a, b)]


def _assert_same_state(a, b, what):
    for name in TENSORS:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{what}: {name} differs"
    assert a.memory_count == b.memory_count, what
    assert a.id_to_idx == b.id_to_idx, f"{what}: id_to_idx differs"
    assert a._idx_to_id == b._idx_to_id, f"{what}: _idx_to_id differs"


def _assert_same(a, b, what):
    _assert_same_state(a, b, what)
    assert a._write_cursor == b._write_cursor, what
    assert a._index_ready == b._index_ready, what


# ---------------------------------------------------------------------------------- 'reference' and 'fifo'
def _batch_against_one_row_loop(H, policy, index, sizes, seed):
    """``sizes[0]`` rows held before (0: none), then one batch per further size; the twin gets every row alone."""
    a, b = _hf(H, policy, index), _hf(H, policy, index)
    feats = _rows(sum(sizes), seed)
    lo = 0
    for step, n in enumerate(sizes):
        if n == 0:
            continue
        ids, f = _ids(lo, lo + n), feats[lo:lo + n]
        torch.manual_seed(1000 + step)            # the rebuilds draw their initial rows from the global generator
        a.create_episodic_memories(ids, f)
        torch.manual_seed(1000 + step)
        for i in range(n):
            b.create_episodic_memory(ids[i], "e", f[i])
        _assert_same(a, b, f"{policy} index={index} sizes={sizes} after batch {step}")
        lo += n
    assert a.memory_count == min(M, sum(sizes))


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("held", HELD)
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
@pytest.mark.parametrize("policy", ("reference", "fifo"))
def test_batch_equals_one_row_writes(hmod, policy, index, held, batch):
    _batch_against_one_row_loop(hmod, policy, index, (held, batch), seed=held * 1000 + batch)


def _sequence(seed, length=6):
    rng = np.random.RandomState(seed)
    return tuple(int(x) for x in rng.choice(BATCHES, size=length))


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
@pytest.mark.parametrize("policy", ("reference", "fifo"))
def test_batch_sequences_equal_one_row_writes(hmod, policy, index, seed):
    """Several batches in a row: the write cursor is not 0 when a batch wraps."""
    _batch_against_one_row_loop(hmod, policy, index, _sequence(seed), seed=seed)


# ---------------------------------------------------------------------------------- 'weakest'
def _strengths(hf, twin, gen):
    """Unequal keys with ties (steps of 0.1), the same on both banks: without them 'weakest' is the ring."""
    n = hf.memory_count
    if n:
        s = torch.randint(1, 11, (n,), generator=gen).float() / 10.0
        hf.memory_metadata[:n, 0] = s
        twin.memory_metadata[:n, 0] = s


def _replay_run(twin, ids, feats):
    """One run of a 'weakest' batch as the rule states it, on ``twin``'s tensors: appends, then the first
    ``rest`` rows of the eviction order of the keys BEFORE the write; row i goes to planned slot i, in order."""
    m, count, cursor = twin.max_memories, twin.memory_count, twin._write_cursor
    n = len(ids)
    n_app = min(n, m - count)
    rest = n - n_app
    slots = list(range(count, count + n_app))
    if rest:
        keys = strict.bank_retention_keys(twin.memory_metadata, count, NOW)
        victims = strict.eviction_order(keys, cursor % m)[:rest].tolist()
        assert len(set(victims)) == rest and all(0 <= v < count for v in victims)
        slots += victims
    online = twin.use_centroid_index and twin._index_ready
    plain.bank_write(twin.memory_features, twin.memory_locations, twin.memory_metadata, twin._inv_norm, feats,
                     torch.tensor(slots, dtype=torch.int64), twin.current_location, NOW,
                     centroids=twin.centroids if online else None,
                     centroid_counts=twin.centroid_counts if online else None, eff_k=K if online else 0)
    twin.memory_count, twin._write_cursor = count + n_app, cursor + rest
    for mid, s in zip(ids, slots):
        twin.id_to_idx[mid] = s
        twin._idx_to_id[s] = mid
    if twin.use_centroid_index and twin.memory_count % INTERVAL == 0 and twin.memory_count > K:
        twin.rebuild_centroids()


def _weakest_against_replay(H, index, sizes, seed):
    a, twin = _hf(H, "weakest", index), _hf(H, "weakest", index)
    runs = []
    write_rows = a._write_rows

    def logged(ids, feats, now):
        runs.append(len(ids))
        return write_rows(ids, feats, now)
    a._write_rows = logged
    feats = _rows(sum(sizes), seed)
    gen = torch.Generator().manual_seed(seed + 7)
    lo = 0
    for step, n in enumerate(sizes):
        if n == 0:
            continue
        ids, f = _ids(lo, lo + n), feats[lo:lo + n]
        _strengths(a, twin, gen)
        del runs[:]
        torch.manual_seed(1000 + step)
        a.create_episodic_memories(ids, f)
        # a run is the unit of a 'weakest' write: it never evicts more rows than were held before it
        assert sum(runs) == n and max(runs) <= M
        torch.manual_seed(1000 + step)
        at = 0
        for r in runs:
            _replay_run(twin, ids[at:at + r], f[at:at + r])
            at += r
        _assert_same(a, twin, f"weakest index={index} sizes={sizes} after batch {step}")
        lo += n


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("held", HELD)
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
def test_weakest_batch_equals_the_planned_replay(hmod, index, held, batch):
    _weakest_against_replay(hmod, index, (held, batch), seed=held * 1000 + batch)


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
def test_weakest_sequences_equal_the_planned_replay(hmod, index, seed):
    _weakest_against_replay(hmod, index, _sequence(seed), seed=seed)


# ---------------------------------------------------------------------------------- sharded, world size 1
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("held", (0, 10))
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
@pytest.mark.parametrize("policy", ("reference", "fifo"))
def test_sharded_world_of_one_equals_the_unsharded_bank(hmod, policy, index, held, batch):
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    local, hf = _hf(hmod, policy, index), _hf(hmod, policy, index)
    sh = ShardedHippocampus(local, M, ops_module=strict, now_fn=lambda: NOW)
    feats = _rows(held + batch, held * 1000 + batch)
    lo = 0
    for step, n in enumerate((held, batch)):
        if n == 0:
            continue
        ids, f = _ids(lo, lo + n), feats[lo:lo + n]
        torch.manual_seed(1000 + step)
        sh.write(ids, f)
        torch.manual_seed(1000 + step)
        hf.create_episodic_memories(ids, f)
        lo += n
    # (the cursor of a sharded bank is the global one, kept by the wrapper)
    _assert_same_state(local, hf, f"sharded {policy} index={index} held={held} batch={batch}")
    assert sh.memory_count == hf.memory_count and sh._write_cursor == hf._write_cursor
    assert local._index_ready == hf._index_ready


# ---------------------------------------------------------------------------------- write_at, caller-chosen slots
WRITE_AT = (
    # (rows held before, n_app, slots)
    (10, 0, (3, 5, 3, 7, 5, 3)),
    (10, 0, (0, 0, 0, 0)),
    (10, 2, (10, 11, 3, 10, 3, 11, 10)),        # overwrites of slots the same call appends
    (64, 0, tuple(range(64)) + (0, 63, 17)),
)


@pytest.mark.parametrize("held,n_app,slots", WRITE_AT)
@pytest.mark.parametrize("with_cids", (False, True), ids=("no_cids", "cids"))
@pytest.mark.parametrize("policy", ("reference", "fifo", "weakest"))
def test_write_at_with_repeated_slots_last_row_wins(hmod, policy, with_cids, held, n_app, slots):
    hf = _hf(hmod, policy, False)
    base = _rows(held, 5)
    hf.create_episodic_memories(_ids(0, held), base)
    before = {name: getattr(hf, name).clone() for name in TENSORS}
    ids_before = list(hf._idx_to_id)
    n = len(slots)
    feats = _rows(n, 6)
    ids = [f"w{i}" for i in range(n)]
    cids = torch.arange(n, dtype=torch.float32) % 3 if with_cids else None
    hf.write_at(ids, feats, np.array(slots), n_app, NOW + 1.0, cids=cids)
    assert hf.memory_count == held + n_app
    last = {s: i for i, s in enumerate(slots)}
    for s, i in last.items():
        assert torch.equal(hf.memory_features[s], feats[i]), f"slot {s}"
        assert torch.equal(hf._inv_norm[s], 1.0 / feats[i].norm().clamp_min(1e-12))
        want = torch.tensor([1.0, NOW + 1.0, float(cids[i]) if with_cids else -1.0, 0.0])
        assert torch.equal(hf.memory_metadata[s], want), f"slot {s}: {hf.memory_metadata[s]} != {want}"
        assert torch.equal(hf.memory_locations[s], torch.tensor([0.25, -1.0]))
        assert hf._idx_to_id[s] == ids[i]
    assert [hf.id_to_idx[m] for m in ids] == list(slots)
    untouched = [r for r in range(M) if r not in last]
    for name in ("memory_features", "_inv_norm", "memory_metadata", "memory_locations"):
        assert torch.equal(getattr(hf, name)[untouched], before[name][untouched]), name
    assert [hf._idx_to_id[r] for r in untouched] == [ids_before[r] for r in untouched]


def test_strict_stub_fires_on_a_repeated_slot_and_only_for_the_parallel_kernel():
    """The detector itself: it must raise for the calls it is there to catch, and for no others."""
    def state():
        return (torch.zeros(4, D), torch.zeros(4, 2), torch.zeros(4, 4), torch.zeros(4))
    feats, cur = _rows(3, 1), torch.zeros(2)
    rep, ok = torch.tensor([1, 2, 1]), torch.tensor([1, 2, 3])
    cent, counts = torch.randn(256, D), torch.ones(256)
    with pytest.raises(AssertionError, match=r"slots \[1\]"):
        strict.bank_write(*state(), feats, rep, cur, NOW)
    with pytest.raises(AssertionError, match=r"slots \[1\]"):
        strict.bank_write(*state(), feats, rep, cur, NOW, centroids=cent.clone(), centroid_counts=counts.clone(),
                          eff_k=4, distinct_slots=True)
    strict.bank_write(*state(), feats, ok, cur, NOW)
    strict.bank_write(*state(), feats, ok, cur, NOW, centroids=cent.clone(), centroid_counts=counts.clone(), eff_k=4,
                      distinct_slots=True)
    for kw in (dict(distinct_slots=False), dict(distinct_slots=True, serial=True)):
        got = state()
        strict.bank_write(*got, feats, rep, cur, NOW, centroids=cent.clone(), centroid_counts=counts.clone(), eff_k=4, **kw)
        assert torch.equal(got[0][1], feats[2])       # in order: the last row wins
