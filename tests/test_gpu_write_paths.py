"""The write path on the real kernels: a batch equals one-row writes bit for bit, no call hands the parallel
write kernel a slot twice, the derived state (bf16 shadow, inverted lists) follows such writes, the serial
centroid kernel serves repeated slots in row order and agrees with an fp64 replay of its own assignments.

Two detectors, both deterministic: a spy on ``ops.bank_write`` that checks the contract at the call (the same
check as ``tests/cpu_stub_strict.py``; it raises BEFORE the real op runs, so a racing write is never launched),
and comparisons against references.  Every case runs once."""
import math
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from tests import cpu_stub_strict as strict

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
TENSORS = ("memory_features", "_inv_norm", "memory_metadata", "memory_locations", "centroids", "centroid_counts")
# (rows held before, rows in the batch) in units of max_memories / 64: every pair that reached the parallel
# kernel with a repeated slot before _store_rows looked at the appended run ('fifo', index off) ...
TABLE = tuple((h, b) for h, bs in ((0, (65, 68, 69, 100, 128)), (1, (65, 68, 69, 100)), (10, (65, 68, 69, 100)),
                                   (60, (65, 68))) for b in bs)
# ... and the neighbours that take the other branches (pure appends, exact fill, a ring that laps itself,
# a full bank)
AROUND = ((0, 64), (10, 3), (10, 54), (10, 55), (63, 1), (63, 65), (60, 69), (0, 129), (64, 1), (64, 65), (64, 200))
BATCHES = (1, 3, 4, 5, 54, 55, 63, 64, 65, 68, 69, 100, 128, 129, 200)


@pytest.fixture()
def H(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    return H


def _hf(H, M, D, small, **kw):
    hf = H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                device="cuda", **kw)
    if small:
        # a full bank whose size divides the interval rebuilds after every write: kept on purpose at this size
        hf.centroids_k, hf.centroids_update_interval = 4, 16
    else:
        hf.centroids_update_interval = 1000        # does not divide 4096: a full bank writes whole runs
    hf.update_spatial_state(torch.tensor([0.25, -1.0], device="cuda"))
    return hf


@contextmanager
def _spy():
    """``ops.bank_write`` held to its contract for the duration: repeated slots never reach the parallel kernel."""
    import aura_snn_rag_amd.ops as ops
    real = ops.bank_write
    calls = []

    def checked(bank, loc, meta, inv_norm, feats, slots, cur_loc, now, centroids=None, centroid_counts=None,
                eff_k=0, distinct_slots=False, serial=False):
        strict.check_write_contract(slots.cpu(), centroids, distinct_slots, serial)
        calls.append(int(slots.numel()))
        return real(bank, loc, meta, inv_norm, feats, slots, cur_loc, now, centroids=centroids,
                    centroid_counts=centroid_counts, eff_k=eff_k, distinct_slots=distinct_slots, serial=serial)
    ops.bank_write = checked
    try:
        yield calls
    finally:
        ops.bank_write = real


def _rows(n, D, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, D, generator=g) * (0.25 + 2 * torch.rand(n, 1, generator=g))).to(dev).contiguous()


def _ids(a, b):
    return [f"m{i}" for i in range(a, b)]


def _assert_same(a, b, what):
    torch.cuda.synchronize()
    for name in TENSORS:
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{what}: {name} differs"
    assert a.memory_count == b.memory_count and a._write_cursor == b._write_cursor, what
    assert a.id_to_idx == b.id_to_idx, f"{what}: id_to_idx differs"
    assert a._idx_to_id == b._idx_to_id, f"{what}: _idx_to_id differs"
    assert a._index_ready == b._index_ready, what


def _shape(size):
    return (64, 32, True) if size == "small" else (4096, 768, False)


# ---------------------------------------------------------------------------------- 'reference' and 'fifo'
def _batch_against_one_row_loop(H, dev, policy, index, size, sizes, seed):
    M, D, small = _shape(size)
    kw = dict(use_centroid_index=index, overflow=policy)
    a, b = _hf(H, M, D, small, **kw), _hf(H, M, D, small, **kw)
    feats = _rows(sum(sizes), D, seed, dev)
    lo = 0
    for step, n in enumerate(sizes):
        if n == 0:
            continue
        ids, f = _ids(lo, lo + n), feats[lo:lo + n]
        torch.manual_seed(1000 + step)            # the rebuilds draw their initial rows from the global generator
        with _spy():
            a.create_episodic_memories(ids, f)
        torch.manual_seed(1000 + step)
        for i in range(n):
            b.create_episodic_memory(ids[i], "e", f[i])
        _assert_same(a, b, f"{policy} index={index} M={M} sizes={sizes} after batch {step}")
        lo += n
    assert a.memory_count == min(M, sum(sizes))


@pytest.mark.parametrize("held,batch", TABLE + AROUND)
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
@pytest.mark.parametrize("policy", ("reference", "fifo"))
def test_batch_equals_one_row_writes_small(dev, H, policy, index, held, batch):
    _batch_against_one_row_loop(H, dev, policy, index, "small", (held, batch), seed=held * 1000 + batch)


# at 4096 x 768 the rows that share a slot are in flight together; only the table, so that the one-row twin
# stays at a few thousand launches per case ('reference' never took the faulty branch: three pairs of it)
LARGE = [("fifo", h, b) for h, b in TABLE] + [("reference", 0, 65), ("reference", 10, 100), ("reference", 60, 68)]


@pytest.mark.parametrize("policy,held,batch", LARGE)
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
def test_batch_equals_one_row_writes_large(dev, H, policy, index, held, batch):
    _batch_against_one_row_loop(H, dev, policy, index, "large", (64 * held, 64 * batch), seed=held * 1000 + batch)


@pytest.mark.parametrize("size", ("small", "large"))
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
@pytest.mark.parametrize("policy", ("reference", "fifo"))
def test_batch_sequence_equals_one_row_writes(dev, H, policy, index, size):
    """Several batches in a row: the write cursor is not 0 when a batch wraps."""
    rng = np.random.RandomState(3)
    if size == "small":
        sizes = tuple(int(x) for x in rng.choice(BATCHES, size=6))
    else:
        sizes = tuple(64 * int(x) for x in rng.choice((65, 68, 69, 100, 128), size=3))
    _batch_against_one_row_loop(H, dev, policy, index, size, sizes, seed=3)


# ---------------------------------------------------------------------------------- 'weakest'
def _weakest_by_the_rule(H, dev, index, size, sizes, seed):
    """A 'weakest' batch is by design not n one-row writes: every run's victims are the first rows of the eviction
    order rebuilt from the kernel's own keys taken before the run; all slots of a run are distinct."""
    import aura_snn_rag_amd.ops as ops
    M, D, small = _shape(size)
    a = _hf(H, M, D, small, use_centroid_index=index, overflow="weakest")
    feats = _rows(sum(sizes), D, seed, dev)
    gen = torch.Generator().manual_seed(seed + 7)
    write_rows = a._write_rows
    runs = []

    def by_the_rule(ids, f, now):
        count, cursor = a.memory_count, a._write_cursor
        n_app = min(len(ids), M - count)
        rest = len(ids) - n_app
        want = list(range(count, count + n_app))
        if rest:
            keys = ops.bank_retention_keys(a.memory_metadata, count, now).cpu()
            victims = strict.eviction_order(keys, cursor % M)[:rest].tolist()
            assert len(set(victims)) == rest and all(0 <= v < count for v in victims)
            want += victims
        write_rows(ids, f, now)
        runs.append(len(ids))
        assert [a.id_to_idx[m] for m in ids] == want, f"run of {len(ids)} at count {count}, cursor {cursor}"
        assert a._write_cursor == cursor + rest and a.memory_count == count + n_app
        w = torch.tensor(want, device=dev)
        assert torch.equal(a.memory_features[w], f), "a row of the run is not at its planned slot"
        assert [a._idx_to_id[s] for s in want] == list(ids)
    a._write_rows = by_the_rule
    lo = 0
    for step, n in enumerate(sizes):
        if n == 0:
            continue
        if a.memory_count:                        # unequal keys with ties: without them 'weakest' is the ring
            s = torch.randint(1, 11, (a.memory_count,), generator=gen).float() / 10.0
            a.memory_metadata[:a.memory_count, 0] = s.to(dev)
        del runs[:]
        torch.manual_seed(1000 + step)
        with _spy():
            a.create_episodic_memories(_ids(lo, lo + n), feats[lo:lo + n])
        assert sum(runs) == n and max(runs) <= M
        lo += n


@pytest.mark.parametrize("held,batch", TABLE + AROUND)
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
def test_weakest_victims_follow_the_rule_small(dev, H, index, held, batch):
    _weakest_by_the_rule(H, dev, index, "small", (held, batch), seed=held * 1000 + batch)


@pytest.mark.parametrize("held,batch", ((0, 65), (1, 100), (10, 69), (60, 68), (64, 128)))
@pytest.mark.parametrize("index", (False, True), ids=("index_off", "index_on"))
def test_weakest_victims_follow_the_rule_large(dev, H, index, held, batch):
    _weakest_by_the_rule(H, dev, index, "large", (64 * held, 64 * batch), seed=held * 1000 + batch)


@pytest.mark.parametrize("size", ("small", "large"))
def test_weakest_sequence_follows_the_rule(dev, H, size):
    rng = np.random.RandomState(5)
    if size == "small":
        sizes = tuple(int(x) for x in rng.choice(BATCHES, size=6))
    else:
        sizes = tuple(64 * int(x) for x in rng.choice((65, 68, 69, 100, 128), size=3))
    _weakest_by_the_rule(H, dev, True, size, sizes, seed=5)


# ---------------------------------------------------------------------------------- derived state
@pytest.mark.parametrize("policy,index", (("fifo", False), ("reference", False), ("fifo", True), ("reference", True),
                                          ("weakest", True)))
def test_shadow_and_lists_follow_writes_that_repeat_slots(dev, H, policy, index):
    """A bank large enough for the bf16 shadow (and, with more than 512 queries, the inverted lists), brought up
    by a recall, then written by batches that repeat slots in each of the three ways.  After each: the shadow of
    every row held is the rounded normalised row, the recall equals that of a twin without shadows, and every
    row held is listed exactly once."""
    D, M, held = 64, 9000, 8500
    g = torch.Generator().manual_seed(12)
    centres = torch.randn(300, D, generator=g) * 3

    def draw(n):
        return centres[torch.randint(0, 300, (n,), generator=g)] + torch.randn(n, D, generator=g)
    kw = dict(use_centroid_index=index, overflow=policy)
    a, b = _hf(H, M, D, False, **kw), _hf(H, M, D, False, bf16_shadow=False, **kw)
    first = draw(held)
    for hf in (a, b):
        hf.centroids_update_interval = 100000                        # no automatic rebuilds in this test
        torch.manual_seed(1)
        hf.bulk_write(first, rebuild=index)
    now = NOW + 2.0
    q = draw(700 if index else 40).to(dev)                           # 700 > MASKED_SCAN_MAX_QUERIES: the lists

    def same(what):
        b.memory_metadata.copy_(a.memory_metadata); b.centroids.copy_(a.centroids)
        sa, ra = a.recall_batch(q, k=9, now=now)
        sb, rb = b.recall_batch(q, k=9, now=now)
        assert torch.equal(ra, rb) and torch.equal(sa, sb), f"{what}: recall differs from the twin without shadows"
        n = a.memory_count
        if a._shadow is not None:
            assert a._shadow_valid_upto == n
            expect = (a.memory_features * a._inv_norm.unsqueeze(1)).to(torch.bfloat16)
            assert torch.equal(a._shadow[:n], expect[:n]), f"{what}: stale shadow rows"
        if index:
            st = a._ivf
            assert st is not None and st.valid
            listed = st.sorted_rows[st.sorted_rows >= 0]
            assert listed.numel() == n and torch.equal(torch.sort(listed).values,
                                                       torch.arange(n, device=dev, dtype=torch.int32)), \
                f"{what}: the lists do not hold every row exactly once"
    same("after the seeding")
    assert (a._ivf is not None) if index else (a._shadow is not None)
    # appends 500 and overwrites 8600 (> 8500 held): a ring wraps onto the batch's own appends; the reference's
    # mode sends the 8600 to slot 0; then a short run with the cursor off 0; then a ring that laps itself
    at = 0
    for n in (M - held + held + 100, 300, M + 50):
        rows = draw(n)
        if policy == "weakest":
            s = (torch.randint(1, 11, (a.memory_count,), generator=g).float() / 10.0).to(dev)
            for hf in (a, b):
                hf.memory_metadata[:hf.memory_count, 0] = s
        ids = [f"w{at + i}" for i in range(n)]
        with _spy():
            a.create_episodic_memories(ids, rows)
        b.create_episodic_memories(ids, rows)
        at += n
        assert a.id_to_idx == b.id_to_idx and a._write_cursor == b._write_cursor
        assert torch.equal(a.memory_features, b.memory_features) and torch.equal(a._inv_norm, b._inv_norm)
        same(f"after a batch of {n}")
    assert a.memory_count == M


# ---------------------------------------------------------------------------------- the serial kernel, repeated slots
def _bank_state(M, D, k_rows, seed, dev):
    g = torch.Generator().manual_seed(seed)
    cent = torch.zeros(256, D)
    cent[:k_rows] = 0.3 * torch.randn(k_rows, D, generator=g)
    counts = torch.zeros(256)
    counts[:k_rows] = torch.randint(1, 5000, (k_rows,), generator=g).float()
    st = dict(bank=torch.zeros(M, D), loc=torch.zeros(M, 2), meta=torch.zeros(M, 4), inv=torch.zeros(M),
              cent=cent, counts=counts)
    return {k: v.to(dev) for k, v in st.items()}


@pytest.mark.parametrize("D", (50, 768, 1536))
@pytest.mark.parametrize("pattern", ("all_to_slot_0", "random_multiset"))
def test_serial_kernel_with_repeated_slots_equals_one_row_calls(dev, D, pattern):
    from aura_snn_rag_amd import ops
    n, M, eff_k = 150, 40, 256
    a = _bank_state(M, D, eff_k, 11, dev)
    b = {k: v.clone() for k, v in a.items()}
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(n, D, generator=g).to(dev).contiguous()
    slots = torch.zeros(n, dtype=torch.int64) if pattern == "all_to_slot_0" else torch.randint(0, M, (n,), generator=g)
    assert torch.unique(slots).numel() < n
    slots = slots.to(dev)
    cur = torch.tensor([0.25, -1.0], device=dev)

    def write(st, lo, hi):
        ops.bank_write(st["bank"], st["loc"], st["meta"], st["inv"], feats[lo:hi].contiguous(), slots[lo:hi].contiguous(),
                       cur, 1234.0, centroids=st["cent"], centroid_counts=st["counts"], eff_k=eff_k, distinct_slots=False)
    write(a, 0, n)
    for i in range(n):
        write(b, i, i + 1)
    torch.cuda.synchronize()
    for name in ("bank", "inv", "meta", "loc", "cent", "counts"):
        assert torch.equal(a[name], b[name]), f"{name} differs"
    last = {int(s): i for i, s in enumerate(slots.tolist())}
    for s, i in last.items():
        assert torch.equal(a["bank"][s], feats[i])                  # the last row wins


def test_reference_mode_full_bank_with_index_sends_one_batch_to_slot_0(dev, H):
    """overflow='reference', index on, a full bank whose size does NOT divide the interval: one batch of 200 is one
    run, every row to slot 0, through the serial kernel; against the one-row loop."""
    M, D = 100, 32
    kw = dict(use_centroid_index=True, overflow="reference")
    a, b = _hf(H, M, D, True, **kw), _hf(H, M, D, True, **kw)
    feats = _rows(M + 200, D, 9, dev)
    ids = _ids(0, M + 200)
    seen = []
    for hf in (a, b):
        torch.manual_seed(2)
        hf.create_episodic_memories(ids[:M], feats[:M])
    assert a._index_ready and a.memory_count == M
    torch.manual_seed(3)
    with _spy() as calls:
        a.create_episodic_memories(ids[M:], feats[M:])
        seen = list(calls)
    assert seen == [200], "the batch was split: the serial kernel never saw a repeated slot"
    torch.manual_seed(3)
    for i in range(M, M + 200):
        b.create_episodic_memory(ids[i], "e", feats[i])
    _assert_same(a, b, "reference, index on, full bank, batch of 200")
    assert torch.equal(a.memory_features[0], feats[-1])


# ---------------------------------------------------------------------------------- the serial kernel against fp64
REPLAY = [
    # (rows, D, eff_k, clustered, counts_zero)
    (2000, 128, 256, False, False),
    (600, 768, 256, False, False),
    (300, 1030, 200, False, False),
    (600, 1536, 256, False, False),
    (600, 1536, 256, True, False),
    (400, 2048, 64, False, True),
]
U = 2.0 ** -24


def _replay_fp64(cent0, counts0, feats, cids, eff_k):
    """Replay the kernel's OWN centroid ids in fp64 from the same initial table and counts.  Returns the worst
    ``(d[assigned] - min d) / tol``, the number of rows whose two smallest distances lie within ``2 tol`` of each
    other, the replayed table and counts, and the largest number of updates a centroid has had."""
    n, D = feats.shape
    C = cent0[:eff_k].double().clone()
    cnt = counts0[:eff_k].double().clone()
    upd = torch.zeros(eff_k, dtype=torch.int64)
    A = max(float(feats.abs().max()), float(cent0[:eff_k].abs().max()))
    worst, close, m = 0.0, 0, 0
    for i in range(n):
        x = feats[i].double()
        d = (C - x).norm(dim=1)
        tol = 2 * math.sqrt(D) * 5 * U * A * m + (D + 8) * U * float(d.max())
        c = int(cids[i])
        assert 0 <= c < eff_k, f"row {i}: centroid id {c}"
        excess = float(d[c] - d.min())
        worst = max(worst, excess / tol if tol > 0 else (0.0 if excess <= 0 else math.inf))
        two = torch.topk(d, 2, largest=False).values
        close += int(float(two[1] - two[0]) <= 2 * tol)
        cnt[c] += 1
        eta = 1.0 / max(float(cnt[c]), 1.0)
        C[c] = (1 - eta) * C[c] + eta * x
        upd[c] += 1
        m = max(m, int(upd[c]))
    return worst, close, C, cnt, m, A


def _check_against_replay(dev, n, D, eff_k, clustered, counts_zero, serial):
    from aura_snn_rag_amd import ops
    from tests.test_gpu_online_write import _state, _write
    M = n + 10
    st = _state(M, D, eff_k, 11, dev, clustered, counts_zero)
    cent0, counts0 = st["cent"].cpu().clone(), st["counts"].cpu().clone()
    g = torch.Generator().manual_seed(5)
    if clustered:
        pick = torch.randint(0, eff_k, (n,), generator=g)
        feats = cent0[:eff_k][pick] + 0.05 * torch.randn(n, D, generator=g)
    else:
        feats = torch.randn(n, D, generator=g)
    slots = torch.randperm(M, generator=g)[:n]
    _write(ops, st, feats.to(dev).contiguous(), slots.to(dev), eff_k, serial=serial)
    torch.cuda.synchronize()
    cids = st["meta"].cpu()[slots, 2].long()
    worst, close, C, cnt, m, A = _replay_fp64(cent0, counts0, feats, cids, eff_k)
    err = float((st["cent"].cpu()[:eff_k].double() - C).abs().max())
    bound = 5 * U * A * m
    print(f"replay n={n} D={D} k={eff_k} clustered={clustered} counts_zero={counts_zero} serial={serial}: "
          f"worst excess/tol {worst:.3e}, non-discriminating {close}/{n}, centroid error {err:.3e} (bound {bound:.3e}), "
          f"most updates {m}")
    assert worst <= 1.0, f"a row went to a centroid that is not the nearest within the bound: excess/tol {worst}"
    assert torch.equal(st["counts"].cpu()[:eff_k].double(), cnt), "counts differ from the replay"
    assert err <= bound, f"centroid error {err} > {bound}"
    assert close <= 0.10 * n, f"{close} of {n} rows are near-ties within 2 tol: the first assertion decides too little"


@pytest.mark.parametrize("n,D,eff_k,clustered,counts_zero", REPLAY)
def test_serial_kernel_against_fp64_replay(dev, n, D, eff_k, clustered, counts_zero):
    """The one-workgroup serial kernel (the checker the online kernel is held to bit for bit) against an fp64
    replay of the centroid ids it gave, with ``u = 2^-24``, ``A`` the largest magnitude among the rows and the
    initial centroids, ``m`` the most updates any centroid has had so far:

    * every row: ``d[assigned] <= min(d) + tol``, ``tol = 2 sqrt(D) * 5 u A m + (D + 8) u max(d)``.  First term:
      the running mean ``(1 - eta) c + eta x`` rounds five times per element, every value stays within ``A`` and
      ``1 - eta <= 1`` does not amplify what was there, so the fp32 table is within ``5 u A m`` per element of the
      replay, which moves a distance by at most ``sqrt(D)`` times that, for the assigned and for the best centroid.
      Second term: a computed fp32 distance is within ``((D + 2) / 2 + 1) u`` of the exact one relatively, and two
      are compared.  Neither term comes from the kernel; no row is excluded;
    * counts equal the replay's exactly, centroids within ``5 u A m_final`` per element;
    * at most 10 % of the rows have their two smallest fp64 distances within ``2 tol`` (a condition on the inputs:
      otherwise the first assertion would decide too little).

    MI355X, the serial kernel (rows, D, k, clustered, counts_zero): worst excess / tol, rows within 2 tol,
    centroid error against its bound:
      (2000,  128, 256, F, F)   0   26 / 2000   2.8e-7 / 2.3e-5
      ( 600,  768, 256, F, F)   0   23 /  600   2.1e-7 / 2.1e-5
      ( 300, 1030, 200, F, F)   0   14 /  300   2.0e-7 / 1.2e-5
      ( 600, 1536, 256, F, F)   0   39 /  600   3.8e-7 / 1.5e-4
      ( 600, 1536, 256, T, F)   0    0 /  600   3.7e-6 / 4.6e-5
      ( 400, 2048,  64, F, T)   0    9 /  400   1.9e-7 / 5.0e-4
    The kernel chose the fp64 minimiser in every row (excess 0 throughout); the online kernel at D = 1536 gave the
    same figures as the serial one in both cases.  The worst non-discriminating share is 6.5 %."""
    _check_against_replay(dev, n, D, eff_k, clustered, counts_zero, serial=True)


@pytest.mark.parametrize("clustered", (False, True))
def test_online_kernel_against_fp64_replay_above_1024(dev, clustered):
    """The same replay on the online kernel's output at D = 1536 (the unpipelined phase B serves D > 1024): it is
    bit-equal to the serial kernel, so this guards the pair against a shared mistake."""
    _check_against_replay(dev, 600, 1536, 256, clustered, False, serial=False)
