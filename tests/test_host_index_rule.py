"""The rules of tests/index_rule.py anchored on the CPU: the fp64 ranking against torch.cdist, the oracle's own
rebuild_centroids assignment, the fp32 restatement of the segment sums against its fp64 bound, the floors on the share of
decisions forced by their fp64 gap at the seeds the GPU tests use (tests/test_gpu_index_kernels.py) -- a floor is a
property of the inputs and is checked here, on the reference alone; exact ties inside a tie class count towards none --
and the CPU stand-ins of tests/cpu_stub_ops.py against the same rules."""
import numpy as np
import pytest
import torch

from oracle import aura_oracle as O
from tests import cpu_stub_ops as S
from tests import index_rule as R


def _determined(forced):
    """Rank j is pinned when the decisions on both sides of it are forced."""
    left = np.concatenate([np.ones((forced.shape[0], 1), dtype=bool), forced[:, :-1]], 1)
    return left & forced


# ---------------------------------------------------------------------------------------------------------- the key
@pytest.mark.parametrize("D", R.PROBE_DIMS)
def test_probe_forced_ranking_is_cdist_topk(D):
    """Where the decisions are forced the key's ranking is the ranking by distance (cdist in fp64, a stable sort where
    topk would leave the order of the tied zero rows open), and the reference accepts itself with nothing used."""
    table, q = R.probe_case(D)
    key, E, cls = R.probe_reference(D)
    d = torch.cdist(torch.from_numpy(q).double(), torch.from_numpy(table).double())
    by_dist = torch.sort(d, dim=1, stable=True).indices[:, :8].numpy()
    for n in (1, 3, 8):
        ids, forced, ties = R.fp64_ranking(key, E, cls, n)
        pin = _determined(forced)
        assert np.array_equal(ids[pin], by_dist[:, :n][pin])
        bad, worst = R.check_decisions(key, E, cls, ids)
        assert not bad and worst == 0.0, bad
        for nq in (R.PROBE_SMALL_BATCHES if D in R.PROBE_SMALL_BATCH_DIMS else ()) + (R.PROBE_NQ,):   # the GPU tests' cases
            assert forced[:nq].mean() >= R.PROBE_FLOOR, f"D {D} nprobe {n} nq {nq}: forced share {forced[:nq].mean():.4f}"
    assert int((ids[R.PROBE_ZERO_Q] == np.arange(200, 208)).sum()) == 8, "the zero query's nearest are the zero rows, in order"
    assert ids[R.PROBE_EQUAL_Q, 0] == R.PROBE_DUP[0]


def test_probe_rule_rejects_what_it_should():
    """A list with one near pair swapped inside the bound passes; a forced pair swapped, a missing forced row, a repeated
    id and an exact tie in the wrong order do not."""
    key, E, cls = R.probe_reference(40)
    ids, forced, ties = R.fp64_ranking(key, E, cls, 8)
    q = int(np.nonzero(forced[:, 0] & forced[:, 1])[0][0])
    swapped = ids.copy(); swapped[q, [0, 1]] = ids[q, [1, 0]]
    assert R.check_decisions(key, E, cls, swapped)[0]
    dropped = ids.copy(); dropped[q, :7] = ids[q, 1:]; dropped[q, 7] = np.lexsort((np.arange(256), key[q]))[8]
    assert R.check_decisions(key, E, cls, dropped)[0]
    twice = ids.copy(); twice[q, 1] = twice[q, 0]
    assert R.check_decisions(key, E, cls, twice)[0]
    z = ids.copy(); z[R.PROBE_ZERO_Q] = z[R.PROBE_ZERO_Q][::-1]
    assert R.check_decisions(key, E, cls, z)[0], "zero rows out of order"
    e = R.PROBE_EQUAL_Q                                         # rows 7, 20, 100 tie: 7 and 20 share a class, 100 does not
    assert ids[e, :3].tolist() == list(R.PROBE_DUP)
    ok = ids.copy(); ok[e, :3] = [100, 7, 20]
    assert not R.check_decisions(key, E, cls, ok)[0]
    wrong = ids.copy(); wrong[e, :3] = [20, 7, 100]
    assert R.check_decisions(key, E, cls, wrong)[0]


@pytest.mark.parametrize("case", R.ASSIGN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_assign_forced_ranking_is_cdist_argmin(case):
    N, D, k = case
    bank, table = R.assign_case(*case)
    key, E, cls = R.assign_reference(*case)
    ids, forced, ties = R.fp64_ranking(key, E, cls, 1)
    ref = torch.argmin(torch.cdist(torch.from_numpy(bank[:N]).double(), torch.from_numpy(table[:k]).double()), dim=1)
    assert np.array_equal(ids[forced[:, 0], 0], ref.numpy()[forced[:, 0]])
    assert forced.mean() >= R.ASSIGN_FLOOR, f"{case}: forced share {forced.mean():.4f}"
    assert int(ties.sum()) == (1 if k > 9 and N > 4 else 0), "one row, row 4, sits at the repeated centroid"
    bad, worst = R.check_decisions(key, E, cls, ids)
    assert not bad and worst == 0.0, bad
    if k > 40:                                                  # the repeated centroid: only its lowest id is acceptable
        rows = np.nonzero(ids[:, 0] == 3)[0]
        assert rows.size > 0
        other = ids.copy(); other[rows[0], 0] = 9
        assert R.check_decisions(key, E, cls, other)[0]
    # a kernel that ignored k would find the copies of the bank rows behind it
    full = R.key64(bank[:N], table)[0]
    if k < 256:
        copied = np.arange(min(N, 256 - k))
        copied = copied[copied != 2]                            # (the zero row's copy ties with the zero centroid)
        assert bool((full.argmin(1)[copied] >= k).all())


@pytest.mark.parametrize("case", [c for c in R.ASSIGN_CASES if c[0] >= c[2] > 1], ids=lambda c: "x".join(map(str, c)))
def test_oracle_rebuild_assignment_obeys_the_rule(case):
    """OracleBank.rebuild_centroids (oracle/aura_oracle.py: the final cdist + argmin against its own new centroids) on
    the bank rows of the assign cases: every forced row gets the fp64 ranking's centroid."""
    N, D, k = case
    bank, _ = R.assign_case(*case)
    ob = O.OracleBank(N + 5, D, centroids_k=k)
    ob.features[:N] = torch.from_numpy(bank[:N])
    ob.count = N
    ob.metadata[:N, 0] = 1.0
    ob.rebuild_centroids(perm=torch.randperm(N, generator=torch.Generator().manual_seed(1)))
    table = ob.centroids[:k].numpy()
    key, E = R.key64(bank[:N], table)
    cls = R.tie_classes(table)
    ids, forced, ties = R.fp64_ranking(key, E, cls, 1)
    got = ob.metadata[:N, 2].long().numpy()
    f = forced[:, 0]
    assert f.mean() > 0.9 and np.array_equal(got[f], ids[f, 0])


# --------------------------------------------------------------------------------------------------------- the means
def _all_means_cases():
    for D in R.MEANS_DIMS:
        yield f"D{D}", R.means_case(D)
    yield "D8 integers", R.means_case(8, integers=True)
    yield "D260 integers", R.means_case(260, integers=True)
    yield "k256", R.means_case_full()
    yield "k256 D260", R.means_case_full(260, 17)


def test_means_restatement_within_the_fp64_bound():
    for name, (bank, order, seg_off, k) in _all_means_cases():
        assert int(seg_off[0]) == (0 if name.startswith("k256") else R.MEANS_UNLISTED)
        assert sorted(order.tolist()) == list(range(order.size))
        for mean in (True, False):
            for c, e in enumerate(R.means_expected(bank, order, seg_off, k, mean)):
                if e is None:
                    continue
                v32, v64, bound = e
                assert bool((np.abs(v32.astype(np.float64) - v64) <= bound).all()), f"{name} cluster {c} mean={mean}"


def test_means_integer_rows_sum_exactly():
    for D in (8, 260):
        bank, order, seg_off, k = R.means_case(D, integers=True)
        assert float(np.abs(bank).max()) <= 64
        for c in range(k):
            rows = bank[order[seg_off[c]:seg_off[c + 1]]]
            if rows.shape[0]:
                assert np.array_equal(R.segment_sum32(rows).astype(np.int64), rows.astype(np.int64).sum(0))


def test_means_restatement_depends_on_the_order():
    """The restatement is an order, not just a sum: on the real-valued rows another association changes bits (so a
    device that summed otherwise would be seen), and the tail rows go to the first accumulator."""
    bank, order, seg_off, k = R.means_case(100)
    rows = bank[order[seg_off[11]:seg_off[12]]]
    assert rows.shape[0] == 321
    assert not np.array_equal(R.segment_sum32(rows), R.segment_sum32(rows[::-1]))
    assert not np.array_equal(R.segment_sum32(rows), rows.sum(0, dtype=np.float32))
    three = bank[order[seg_off[2]:seg_off[3]]]
    assert np.array_equal(R.segment_sum32(three), (three[0] + three[1]) + three[2])


# --------------------------------------------------------------------------------------------------- the CPU stand-ins
@pytest.mark.parametrize("case", R.ASSIGN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stub_kmeans_assign_obeys_the_rule(case):
    N, D, k = case
    bank, table = R.assign_case(*case)
    key, E, cls = R.assign_reference(*case)
    got = S.kmeans_assign(torch.from_numpy(bank), torch.from_numpy(table), N, k)
    assert got.dtype == torch.int32 and got.numel() == N
    bad, _ = R.check_decisions(key, E, cls, got.numpy()[:, None])
    assert not bad, bad


def test_stub_segment_means_within_the_bound():
    bank, order, seg_off, k = R.means_case(100)
    for sums in (False, True):
        cent = torch.full((k + 4, 100), R.MEANS_SENTINEL)
        S.kmeans_segment_means(torch.from_numpy(bank), torch.from_numpy(order), torch.from_numpy(seg_off), cent, k, sums_only=sums)
        for c, e in enumerate(R.means_expected(bank, order, seg_off, k, not sums)):
            if e is None:
                assert bool((cent[c] == (0.0 if sums else R.MEANS_SENTINEL)).all())
            else:
                assert bool((np.abs(cent[c].double().numpy() - e[1]) <= e[2]).all())
        assert bool((cent[k:] == R.MEANS_SENTINEL).all())


def test_stub_merge_gather_decay():
    g = torch.Generator().manual_seed(5)
    S_, nq, k = 3, 7, 5
    sc = torch.randint(0, 4, (S_, nq, k), generator=g).float().sort(dim=2, descending=True).values   # many equal scores
    ix = torch.randperm(S_ * nq * k, generator=g).reshape(S_, nq, k).to(torch.int32)
    sc[2, :, 3:] = float("-inf"); ix[2, :, 3:] = -1
    ms, mi = S.topk_merge(sc, ix, k)
    for q in range(nq):
        pairs = sorted(((-float(s), int(i)) for s, i in zip(sc[:, q].flatten(), ix[:, q].flatten()) if i >= 0))[:k]
        assert mi[q].tolist() == [p[1] for p in pairs] and ms[q].tolist() == [-p[0] for p in pairs]
    bank = torch.randn(6, 5, generator=g)
    idx = torch.tensor([[0, -1, 6], [11, 5, -2 ** 31]], dtype=torch.int32)
    out = S.bank_gather(bank, idx)
    assert tuple(out.shape) == (2, 3, 5) and torch.equal(out[0, 0], bank[0]) and torch.equal(out[1, 1], bank[5])
    assert bool((out[0, 1:] == 0).all()) and bool((out[1, 0] == 0).all()) and bool((out[1, 2] == 0).all())
    meta = torch.randn(9, 4, generator=g)
    want = meta.clone()
    want[:6, 0] = torch.from_numpy(meta[:6, 0].numpy() * (np.float32(1.0) - np.float32(0.01)))
    S.bank_decay(meta, 0.01, 6)
    assert torch.equal(meta.view(torch.int32), want.view(torch.int32))
