"""The centroid-index kernels held to the rules of tests/index_rule.py on the device: centroid_probe and kmeans_assign to
the fp64 ranking key and its derived bound (every instance: query tile in LDS or not, 16-byte or scalar loads, one, two
and twelve k stages, both sides of the LDS limit, misaligned views), kmeans_segment_means bit for bit to the documented
summation order and within the fp64 bound, kmeans_commit, topk_merge (exactly oracle.merge_topk: ties, short shards, the
32768-query chunk, the largest S k), bank_gather, bank_decay, bank_row_norms, and ivf2_append on a bf16 image.

The inputs, their seeds and the floors on the share of forced decisions are those of tests/index_rule.py; the floors are
asserted on the reference alone in tests/test_host_index_rule.py.  Every case records the worst used share of its bound and
its forced counts (``profiles/index_kernels_parity.json``)."""
import numpy as np
import pytest
import torch

from oracle import aura_oracle as O
from tests import helpers
from tests import index_rule as R

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _misaligned(a, dev):
    """The array on the device as a contiguous view that starts 4 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _record(name, ids, key, E, cls, **extra):
    """Hold ids [nq, n] to the decision rule; the figures are recorded first, so that a failing run leaves them behind."""
    n = ids.shape[1]
    want, forced, ties = R.fp64_ranking(key, E, cls, n)
    bad, worst = R.check_decisions(key, E, cls, ids)
    exact = int((ids == want).all(1).sum())
    helpers.record_parity(f"index {name}", exact, ids.shape[0], forced_decisions=int(forced.sum()),
                          class_ties=int(ties.sum()), decisions=int(forced.size), max_frac_of_bound=round(worst, 4), **extra)
    print(f"\n[index {name}] fp64-exact {exact}/{ids.shape[0]} forced by the gap {int(forced.sum())}/{forced.size}, class ties {int(ties.sum())} "
          f"worst share of the bound {worst:.4f} {extra if extra else ''}")
    assert not bad, f"{name}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------ probe
def _probe(ops, name, q, table, key, E, cls):
    """All the probe assertions for one (queries, table) pair on the device; returns the ids of nprobe = 8."""
    nq = q.shape[0]
    ids8 = ops.centroid_probe(q, table, 8)
    again = ops.centroid_probe(q, table, 8)
    assert ids8.dtype == torch.int32 and tuple(ids8.shape) == (nq, 8)
    assert torch.equal(ids8, again), f"{name}: two calls differ"
    got = ids8.cpu().numpy()
    a, b, c = R.PROBE_DUP
    both = (got == a).any(1) & (got == c).any(1)
    lower_first = int(((got == a).argmax(1) < (got == c).argmax(1))[both].sum())
    _record(f"probe {name} nprobe 8", got, key, E, cls, cross_group_lower_first=f"{lower_first}/{int(both.sum())}")
    D = q.shape[1]
    if D <= 64 or D > 1024:                                     # one stage, or no staged walk: every wave sums k alike,
        assert lower_first == int(both.sum()), f"{name}: row {c} before its copy {a}"   # so the copies' keys are bit-equal
    # the repeated row inside one 32-row group: equal key bits, so the lower row is first and never left out
    has_b = (got == b).any(1)
    assert bool(((got == a).any(1) | ~has_b).all()) and bool(((got == a).argmax(1) < (got == b).argmax(1))[has_b].all()), \
        f"{name}: row {b} before its copy {a}"
    for n in (3, 1):
        ids = ops.centroid_probe(q, table, n)
        assert torch.equal(ids[:, :n], ids8[:, :n]), f"{name}: nprobe {n} is not the prefix of nprobe 8"
        assert bool((ids[:, n:] == -1).all()), f"{name}: columns beyond nprobe {n} are not -1"
        _record(f"probe {name} nprobe {n}", ids[:, :n].cpu().numpy(), key, E, cls)
    return ids8


@pytest.mark.parametrize("D", R.PROBE_DIMS)
def test_centroid_probe(dev, D):
    """300 queries against the 256-row table of index_rule.probe_case at every D of the issue: the decision rule at
    nprobe 8, 3 and 1, -1 beyond nprobe, prefixes, two calls, a query alone against the same query in the batch; the
    zero query returns the zero rows 200 .. 207 in order (exact ties, held by the rule's tie classes), the query that
    equals rows 7, 20 and 100 returns those three first, 7 before 20 (one 32-row group: equal key bits); where 100
    lands among them is recorded per D, and asserted to be behind row 7 at D <= 64 and D > 1024, where every wave
    walks k alike (measured in between, where wave w starts its walk at another stage: the lower row first in 9 of 16
    queries at D = 68, 4 of 13 at 768 and 7 of 19 at 1024).
    Small batches (1, 15, 16, 17: both sides of the 16-query tile) at D = 40 and 768."""
    from aura_snn_rag_amd import ops
    table, q = R.probe_case(D)
    key, E, cls = R.probe_reference(D)
    t, qd = _dev(table, dev), _dev(q, dev)
    ids8 = _probe(ops, f"D{D} nq{R.PROBE_NQ}", qd, t, key, E, cls)
    assert ids8[R.PROBE_ZERO_Q].tolist() == list(range(200, 208)), "the zero query: the zero rows in ascending order"
    first3 = ids8[R.PROBE_EQUAL_Q, :3].tolist()                 # the query that equals rows 7, 20 and 100
    assert sorted(first3) == list(R.PROBE_DUP) and first3.index(R.PROBE_DUP[0]) < first3.index(R.PROBE_DUP[1])
    for i in (0, R.PROBE_ZERO_Q, R.PROBE_BIG_Q, R.PROBE_EQUAL_Q, 150):
        alone = ops.centroid_probe(qd[i:i + 1].clone(), t, 8)
        assert torch.equal(alone[0], ids8[i]), f"D {D}: query {i} alone differs from the batch"
    if D in R.PROBE_SMALL_BATCH_DIMS:
        for nq in R.PROBE_SMALL_BATCHES:
            ids = _probe(ops, f"D{D} nq{nq}", qd[:nq], t, key[:nq], E[:nq], cls)
            assert torch.equal(ids, ids8[:nq]), f"D {D}: the first {nq} queries differ from the batch"
    assert tuple(ops.centroid_probe(qd[:0], t, 8).shape) == (0, 8)


@pytest.mark.parametrize("D", R.PROBE_MISALIGNED_DIMS)
@pytest.mark.parametrize("which", ["queries", "table", "both"])
def test_centroid_probe_misaligned_views(dev, D, which):
    """Offset views (4 bytes past a 16-byte boundary) take the scalar-load instances at a D that is a multiple of 4, on
    either side of the LDS limit; the rule holds as for the aligned arrays."""
    from aura_snn_rag_amd import ops
    table, q = R.probe_case(D)
    key, E, cls = R.probe_reference(D)
    t = _misaligned(table, dev) if which in ("table", "both") else _dev(table, dev)
    qd = _misaligned(q, dev) if which in ("queries", "both") else _dev(q, dev)
    ids8 = _probe(ops, f"D{D} nq{R.PROBE_NQ} misaligned {which}", qd, t, key, E, cls)
    assert ids8[R.PROBE_ZERO_Q].tolist() == list(range(200, 208))


# ----------------------------------------------------------------------------------------------------------- assign
def _assign(ops, name, bank, table, N, k, key, E, cls):
    got = ops.kmeans_assign(bank, table, N, k)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N,)
    assert torch.equal(got, ops.kmeans_assign(bank, table, N, k)), f"{name}: two calls differ"
    ids = got.cpu().numpy().astype(np.int64)
    assert ids.min() >= 0 and ids.max() < k, f"{name}: an id outside [0, {k})"
    _record(f"assign {name}", ids[:, None], key, E, cls)
    return ids


@pytest.mark.parametrize("case", R.ASSIGN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_kmeans_assign(dev, case):
    """count < bank rows; the 256-row table holds copies of bank rows behind k; one zero centroid, one zero bank row;
    centroids 9 and 40 repeat centroid 3 and never win (the rule's tie classes: every row is summed in the same k order,
    so equal rows have equal key bits and the lower id is taken)."""
    from aura_snn_rag_amd import ops
    N, D, k = case
    bank, table = R.assign_case(*case)
    key, E, cls = R.assign_reference(*case)
    ids = _assign(ops, "x".join(map(str, case)), _dev(bank, dev), _dev(table, dev), N, k, key, E, cls)
    for d in (9, 40):
        if k > d:
            assert not bool((ids == d).any()) and bool((ids == 3).any()), f"{case}: centroid {d} won over its copy 3"
    if k > 5 and N > 2:
        assert ids[2] == 5, "the zero row belongs to the zero centroid"
    if case == R.ASSIGN_MISALIGNED:
        off = _assign(ops, "x".join(map(str, case)) + " misaligned bank", _misaligned(bank, dev), _dev(table, dev), N, k,
                      key, E, cls)
        assert np.array_equal(off, ids)


# ------------------------------------------------------------------------------------------------------------ means
def _run_means(ops, dev, bank_d, order, seg_off, k, D, sums):
    cent = torch.full((k + 4, D), R.MEANS_SENTINEL, device=dev)
    ops.kmeans_segment_means(bank_d, _dev(order, dev), _dev(seg_off, dev), cent, k, sums_only=sums)
    return cent.cpu().numpy()


def _check_means(name, bank, order, seg_off, k, got, sums):
    worst = 0.0
    for c, e in enumerate(R.means_expected(bank, order, seg_off, k, not sums)):
        if e is None:
            assert bool((got[c] == (0.0 if sums else R.MEANS_SENTINEL)).all()), f"{name}: empty cluster {c}"
            continue
        v32, v64, bound = e
        err = np.abs(got[c].astype(np.float64) - v64)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(err > 0, err / bound, 0.0))))
        assert np.array_equal(got[c].view(np.int32), v32.view(np.int32)), \
            f"{name}: cluster {c} (len {seg_off[c + 1] - seg_off[c]}) is not the documented order's bits"
        assert bool((err <= bound).all()), f"{name}: cluster {c} outside the fp64 bound"
    assert bool((got[k:] == R.MEANS_SENTINEL).all()), f"{name}: rows beyond k were written"
    return worst


@pytest.mark.parametrize("D", R.MEANS_DIMS)
def test_segment_means_bits_and_bound(dev, D):
    """Built segments (lengths around the 64-row chunk and the 4-row unroll, 37 unlisted rows first, scattered row ids):
    means and sums equal the fp32 restatement bit for bit and lie within the fp64 bound; empty clusters keep the
    sentinel (means) or become zero (sums); rows beyond k are untouched; mean == fl(sum / len); the same segment under
    another id beside other clusters gives the same bits."""
    from aura_snn_rag_amd import ops
    bank, order, seg_off, k = R.means_case(D)
    bank_d = _dev(bank, dev)
    out = {}
    for sums in (False, True):
        out[sums] = _run_means(ops, dev, bank_d, order, seg_off, k, D, sums)
        worst = _check_means(f"D{D} sums={sums}", bank, order, seg_off, k, out[sums], sums)
        helpers.record_parity(f"index means D{D} {'sums' if sums else 'means'}", 1, 1, max_frac_of_bound=round(worst, 4))
    lens = (seg_off[1:] - seg_off[:-1]).astype(np.float32)
    live = lens > 0
    assert np.array_equal((out[True][:k][live] / lens[live, None]).view(np.int32), out[False][:k][live].view(np.int32)), \
        "mean != fl(sum / len)"
    # the segments in reverse cluster order, the unlisted rows now clusters 12 .. 15 of their own
    segs = [order[seg_off[c]:seg_off[c + 1]] for c in range(12)][::-1]
    un = order[:seg_off[0]]
    segs += [un[0:10], un[10:20], un[20:30], un[30:]]
    order2 = np.concatenate(segs).astype(np.int32)
    seg_off2 = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)
    for sums in (False, True):
        moved = _run_means(ops, dev, bank_d, order2, seg_off2, k, D, sums)
        _check_means(f"D{D} moved sums={sums}", bank, order2, seg_off2, k, moved, sums)
        for c in range(12):
            if seg_off[c + 1] > seg_off[c]:
                assert np.array_equal(moved[11 - c].view(np.int32), out[sums][c].view(np.int32)), \
                    f"cluster {c}'s bits changed with its id and its neighbours"


def test_segment_means_integer_rows_and_full_table(dev):
    """Whole-number rows (|x| <= 64) sum exactly; k = 256 with every cluster 65 rows long fills the most partial items
    the workspace formula has to hold (two per cluster)."""
    from aura_snn_rag_amd import ops
    for D in (8, 260):                                          # one and two 256-column slices per row
        bank, order, seg_off, k = R.means_case(D, integers=True)
        got = _run_means(ops, dev, _dev(bank, dev), order, seg_off, k, D, True)
        _check_means(f"integers D{D}", bank, order, seg_off, k, got, True)
        for c in range(k):
            rows = bank[order[seg_off[c]:seg_off[c + 1]]]
            assert np.array_equal(got[c].astype(np.int64), rows.astype(np.int64).sum(0)), f"cluster {c}: not the exact sum"
    for D, length in ((100, 65), (260, 17)):                    # (260, 17): two slices at all 256 clusters
        bank, order, seg_off, k = R.means_case_full(D, length)
        for sums in (False, True):
            got = _run_means(ops, dev, _dev(bank, dev), order, seg_off, k, D, sums)
            _check_means(f"k256 D{D} len{length} sums={sums}", bank, order, seg_off, k, got, sums)


def test_segment_means_empty_call(dev):
    """No rows at all: every cluster is empty.  ``sums_only`` writes zeros to the first k rows (what the docstring says of
    empty clusters); the means leave every row as it was; rows beyond k stay in both."""
    from aura_snn_rag_amd import ops
    bank = torch.randn(8, 12, device=dev)
    order = torch.empty(0, dtype=torch.int32, device=dev)
    seg_off = torch.zeros(6, dtype=torch.int32, device=dev)
    cent = torch.full((7, 12), R.MEANS_SENTINEL, device=dev)
    ops.kmeans_segment_means(bank, order, seg_off, cent, 5)
    assert bool((cent == R.MEANS_SENTINEL).all())
    ops.kmeans_segment_means(bank, order, seg_off, cent, 5, sums_only=True)
    assert bool((cent[:5] == 0).all()) and bool((cent[5:] == R.MEANS_SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------- commit
@pytest.mark.parametrize("N", [0, 1, 257])
@pytest.mark.parametrize("with_counts", [True, False])
def test_kmeans_commit(dev, N, with_counts):
    from aura_snn_rag_amd import ops
    k = 200
    g = torch.Generator().manual_seed(N)
    assign = torch.randint(-1, k, (N,), generator=g).to(torch.int32).to(dev)
    order, seg_off = ops.group_by_cluster(assign, k)
    meta = torch.full((N + 3, 4), float("nan"), device=dev)
    counts = torch.full((256,), float("nan"), device=dev) if with_counts else None
    ops.kmeans_commit(assign, seg_off, meta, counts, k)
    m = meta.cpu()
    assert torch.equal(m[:N, 2], assign.cpu().float())
    assert bool(m[:, [0, 1, 3]].isnan().all()) and bool(m[N:].isnan().all())
    if with_counts:
        want = torch.bincount(assign.cpu()[assign.cpu() >= 0].long(), minlength=k).float()
        assert torch.equal(counts.cpu()[:k], want) and bool(counts.cpu()[k:].isnan().all())


# ------------------------------------------------------------------------------------------------------------ merge
def _shard_lists(S, nq, k, seed, levels, short):
    """Per-shard lists [S, nq, k], each sorted (score descending, then index), indices distinct per query, scores drawn
    from ``levels`` values so that equal scores meet across shards; ``short``: shard s of query q keeps (q + s) % (k + 1)
    real entries and pads with (-inf, -1) -- query 0 then holds fewer than k real entries in all when S < k."""
    g = np.random.default_rng(seed)
    sc = g.integers(0, levels, (S, nq, k)).astype(np.float32) * np.float32(0.25)
    ix = np.argsort(g.random((nq, S * k)), axis=1).astype(np.int32).reshape(nq, S, k).transpose(1, 0, 2).copy()
    o = np.lexsort((ix, -sc), axis=2)
    sc, ix = np.take_along_axis(sc, o, 2), np.take_along_axis(ix, o, 2)
    if short:
        real = (np.arange(nq)[None, :] + np.arange(S)[:, None]) % (k + 1)
        if S < k:
            real[:, 0] = 0
            real[0, 0] = 1
        pad = np.arange(k)[None, None, :] >= real[:, :, None]
        sc[pad], ix[pad] = -np.inf, -1
    return torch.from_numpy(sc), torch.from_numpy(ix)


def _merge_expected(sc, ix, k):
    S, nq, _ = sc.shape
    return O.merge_topk(sc.permute(1, 0, 2).reshape(nq, S * k), ix.permute(1, 0, 2).reshape(nq, S * k).long(), k)


@pytest.mark.parametrize("S,nq,k,short", [(1, 5, 1, False), (8, 50, 32, False), (8, 50, 32, True), (3, 7, 5, False),
                                          (3, 7, 5, True), (2, 32769, 1, False), (2, 32769, 1, True), (8, 3, 1024, False)])
def test_topk_merge_is_the_oracle(dev, S, nq, k, short):
    """Exactly oracle.merge_topk: equal scores across shards go lower index first, short shards are padding, a query with
    fewer than k real entries ends in (-inf, -1); (2, 32769, 1) crosses the 32768-query chunk of the entry point and
    (8, 3, 1024) is the largest S k it accepts (SEL_LDS_KEYS = 8192 keys, k <= SEL_MAX_K = 1024)."""
    from aura_snn_rag_amd import ops
    sc, ix = _shard_lists(S, nq, k, 100 * S + k, 6, short)
    es, ei = _merge_expected(sc, ix, k)
    if S > 1 and not (short and k == 1):                        # (k = 1 and short: one real entry per query)
        real = [sc[:, q][ix[:, q] >= 0] for q in range(min(nq, 8))]
        assert any(r.unique().numel() < r.numel() for r in real), "the case has no equal scores"
    if short and S < k:
        assert bool((ei[0] == -1).any()), "no query with fewer than k real entries"
    gs, gi = ops.topk_merge(sc.to(dev), ix.to(dev), k)
    assert torch.equal(gi.cpu().long(), ei), "merged indices differ from the oracle"
    assert torch.equal(_bits(gs.cpu()), _bits(es)), "merged scores differ from the oracle"


def test_topk_merge_refuses_more_than_its_limit(dev):
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd import _lib
    with pytest.raises(_lib.AuraHipError, match="aura_topk_merge failed: AURA_E_INVAL"):
        ops.topk_merge(torch.zeros(9, 1, 1024, device=dev), torch.zeros(9, 1, 1024, dtype=torch.int32, device=dev), 1024)


# ------------------------------------------------------------------------------------------- gather, decay, row norms
@pytest.mark.parametrize("D", [1, 63, 64, 65, 768])
def test_bank_gather(dev, D):
    """Bits of bank[idx]; -1, rows, rows + 5 and INT32_MIN gather zeros; index 0 and rows - 1 are rows; n in {0, 1, 5}
    and a 2-D index."""
    from aura_snn_rag_amd import ops
    rows = 50
    bank = torch.randn(rows, D, generator=torch.Generator().manual_seed(D))
    bank_d = bank.to(dev)
    for idx in ([], [0], [7, -1, rows, 0, rows - 1], [[rows + 5, 3, -2 ** 31], [rows - 1, 0, -1]]):
        it = torch.tensor(idx, dtype=torch.int32)
        want = torch.zeros(*it.shape, D)
        ok = (it >= 0) & (it < rows)
        want[ok] = bank[it[ok].long()]
        got = ops.bank_gather(bank_d, it.to(dev))
        assert tuple(got.shape) == tuple(it.shape) + (D,) and torch.equal(_bits(got.cpu()), _bits(want))


@pytest.mark.parametrize("count", [0, 1, 256, 257])
def test_bank_decay(dev, count):
    from aura_snn_rag_amd import ops
    meta = torch.randn(300, 4, generator=torch.Generator().manual_seed(count))
    for rate in (0.01, 0.3):
        want = meta.clone()
        want[:count, 0] = torch.from_numpy(meta[:count, 0].numpy() * (np.float32(1.0) - np.float32(rate)))
        got = meta.to(dev)
        ops.bank_decay(got, rate, count)
        assert torch.equal(_bits(got.cpu()), _bits(want)), f"rate {rate}"


@pytest.mark.parametrize("D,offset", [(3, False), (64, False), (770, False), (64, True)])
def test_bank_row_norms(dev, D, offset):
    """inv ||x||_64 - 1 within gamma(D + 4); only rows [row0, row0 + n) are written; a zero row gets 1 / 1e-12f (the
    F.normalize clamp the header documents)."""
    from aura_snn_rag_amd import ops
    g = np.random.default_rng(D)
    x = (g.standard_normal((40, D)) * 10.0 ** g.integers(-3, 4, (40, 1))).astype(np.float32)
    x[9] = 0.0
    bank = _misaligned(x, dev) if offset else _dev(x, dev)
    inv = torch.full((40,), float("nan"), device=dev)
    ops.bank_row_norms(bank, inv, 5, 20)
    got = inv.cpu().numpy()
    assert np.isnan(got[:5]).all() and np.isnan(got[25:]).all()
    assert got[9] == R.INV_OF_ZERO_ROW
    rows = [r for r in range(5, 25) if r != 9]
    rel = np.abs(got[rows].astype(np.float64) * np.linalg.norm(x[rows].astype(np.float64), axis=1) - 1.0)
    helpers.record_parity(f"index row_norms D{D}{' misaligned' if offset else ''}", 1, 1,
                          max_frac_of_bound=round(float(rel.max() / R.row_norm_bound(D)), 4))
    assert bool((rel <= R.row_norm_bound(D)).all())


# ------------------------------------------------------------------------------------------- ivf2_append, bf16 image
def test_ivf2_append_bf16_image(dev):
    """The bf16 twin of test_gpu_half_image's append test on a small layout (600 rows, D = 64, 12 lists, slack 8): new
    rows, rows that already have an entry (holes), rows without a list, and list 11 pushed three rows past its slack --
    legal input that the kernel refuses by dropping the rows and setting the flag.  Afterwards the image rows, rho and
    pos_of_row are a from-scratch bank_shadow_sorted's on the resulting layout, bit for bit, the lists hold exactly the
    rows they should, and the cached row constants are ivf2_row_constants recomputed."""
    from aura_snn_rag_amd import ops
    D, N, M, L, slack = 64, 600, 700, 12, 8
    g = torch.Generator().manual_seed(21)
    bank = torch.zeros(M, D); bank[:N] = torch.randn(N, D, generator=g)
    bank = bank.to(dev).contiguous()
    inv = torch.ones(M, device=dev); ops.bank_row_norms(bank, inv, 0, N)
    cid = torch.randint(-2, L, (N,), generator=g).clamp(min=-1)
    meta = torch.zeros(M, 4, device=dev); meta[:, 0] = 1.0; meta[:, 1] = NOW; meta[:, 2] = -1.0
    meta[:N, 2] = cid.float().to(dev)
    st = ops.build_ivf2(bank[:N], inv[:N], meta[:N, 2], slack=slack, max_rows=M, dtype=torch.bfloat16)
    ns = st["n_sorted"]
    rho = torch.zeros(M, device=dev)
    st["pos_of_row"] = torch.full((M,), -1, dtype=torch.int32, device=dev)
    ops.bank_shadow_sorted(bank, inv, st["sorted_rows"], st["sorted_bf16"], rho, st["pos_of_row"], ns)
    rowc = torch.empty(st["sorted_rows"].numel(), 4, device=dev)
    ops.ivf2_row_constants(meta, rho, st["sorted_rows"], ns, D, NOW, rowc)
    pad_off, len0 = st["pad_off"].cpu().long(), st["list_len"].cpu().long()
    cap = pad_off[1:] - pad_off[:-1]
    free11 = int(cap[11] - len0[11])
    assert 8 <= free11 <= 23 and bool((cap[:10] - len0[:10] >= 8).all())

    listed = torch.nonzero((cid >= 0) & (cid < 10)).flatten()
    rewritten = listed[torch.randperm(listed.numel(), generator=g)[:30]]          # 3 more rows per list 0 .. 9
    dropped = torch.nonzero(cid >= 0).flatten()[-3:]                              # rows that lose their list
    dropped = dropped[~torch.isin(dropped, rewritten)]
    new = torch.arange(N, N + 40)                                                 # 4 more rows per list 0 .. 9
    new_unlisted = torch.arange(N + 40, N + 42)
    push = torch.arange(N + 42, N + 42 + free11 + 3)                              # list 11: three more than it can take
    slots = torch.cat([new, rewritten, dropped, new_unlisted, push])
    assert slots.unique().numel() == slots.numel() and int(slots.max()) < M
    new_cid = torch.cat([torch.arange(40) % 10, torch.arange(30) % 10, torch.full((dropped.numel() + 2,), -1),
                         torch.full((push.numel(),), 11)])
    bank[slots.to(dev)] = torch.randn(slots.numel(), D, generator=g).to(dev)
    meta[slots.to(dev), 2] = new_cid.float().to(dev)
    ops.bank_row_norms(bank, inv, 0, M)                                           # (unchanged rows keep their bits)
    ops.ivf2_append(bank, inv, meta, slots.to(dev), st["sorted_bf16"], st["sorted_rows"], st["pad_off"], st["list_len"],
                    st["pos_of_row"], rho, st["flag"], row_constants=rowc, row_constants_now=NOW)

    assert int(st["flag"].item()) == 1, "the overflow was not flagged"
    assert torch.equal(st["pad_off"].cpu().long(), pad_off)
    sr, pos, ll = st["sorted_rows"].cpu().long(), st["pos_of_row"].cpu().long(), st["list_len"].cpu().long()
    assert int(ll[11]) == int(cap[11]), "list 11 is not back at its capacity"
    lost = push[pos[push] < 0]
    assert lost.numel() == 3, f"{lost.numel()} rows of the overflowing list were dropped, not 3"
    final = torch.full((M,), -1, dtype=torch.long); final[:N] = cid; final[slots] = new_cid; final[lost] = -1
    for c in range(256):
        seg = sr[pad_off[c]:pad_off[c + 1]]
        assert bool((seg[ll[c]:] == -1).all()), f"list {c}: an entry beyond its length"
        held = seg[:ll[c]]
        assert sorted(held[held >= 0].tolist()) == torch.nonzero(final == c).flatten().tolist(), f"list {c}: wrong rows"
    assert int(ll[:10].sum() - len0[:10].sum()) == 70
    # from scratch on the resulting layout
    img2 = torch.zeros_like(st["sorted_bf16"]); rho2 = torch.zeros(M, device=dev)
    pos2 = torch.full((M,), -1, dtype=torch.int32, device=dev)
    ops.bank_shadow_sorted(bank, inv, st["sorted_rows"], img2, rho2, pos2, ns)
    assert torch.equal(st["pos_of_row"], pos2), "pos_of_row is not the layout's reverse map"
    live = st["sorted_rows"][:ns] >= 0                                             # a hole keeps its old bits; never scored
    rows = st["sorted_rows"][:ns][live].long()
    assert torch.equal(_bits(st["sorted_bf16"][:ns][live]), _bits(img2[:ns][live])), "not the rebuilt image"
    assert torch.equal(_bits(rho[rows]), _bits(rho2[rows])), "not the rebuilt rho"
    rowc2 = torch.empty_like(rowc)
    ops.ivf2_row_constants(meta, rho, st["sorted_rows"], ns, D, NOW, rowc2)
    assert torch.equal(_bits(rowc[:ns]), _bits(rowc2[:ns])), "the cached row constants went stale"
