"""The workgroup-per-query refine (coarse_refine_kernel) around its internal switches: the number of re-scoring
rounds, the chunks of a row, and the candidate counts on either side of 512 (one key per thread of the select).
Every case must return the fp32 scan's rows and score bits, through the inverted lists and through the two-stage
full scan, with no overflow flag.

One bank per D (16 384 rows, 256 centroids) holds
  * groups of near-duplicate rows (row + 1e-5 noise, one metadata record) of sizes around the round size R: a query
    aimed at a group keeps about the whole group as survivors, whatever k;
  * a group of exactly identical rows with identical metadata: equal L keys, k = 32 falls inside the tie;
  * eight long lists side by side: with k = 200 (more than the sample groups bound) every row of the probed lists is
    a candidate, 512 < n <= 4096; the ordinary lists give n <= 512;
  * twelve lists of two rows side by side: a query there has n < k candidates and everything survives.
k = 200 on the unclustered bank keeps S >= 200 survivors: several rounds."""
import pytest
import torch

from tests.test_gpu_knn import NOW, _queries

pytestmark = pytest.mark.gpu

N = 16384
R = 48               # survivors per round of coarse_refine_kernel<6, 256, true>: 8 waves x 6 rows (aura_knn_coarse.inl)
GROUPS = (1, 7, R - 1, R, R + 1, 2 * R - 1, 2 * R + 1, 130, 300)
TIE = 60             # identical rows
LONG, LONG_ROWS = 8, 300
TINY, TINY_ROWS = 12, 2
# chunks of 256 floats (this kernel) and of 192 (the other geometries' quarter rows): one short chunk, one exact,
# one + a 32-wide tail, two + tail, all of them
DIMS = (8, 192, 200, 256, 264, 392, 520, 576, 768)


def _clustered_bank(D, g):
    """rows [N, D], meta [N, 4] (centroid id not yet set), centres [256, D], queries aimed at the special rows."""
    centres = torch.randn(256, D, generator=g)
    v = torch.randn(D, generator=g)
    centres[:LONG] = v + 0.5 * torch.randn(LONG, D, generator=g)              # the long lists: neighbours
    u = torch.randn(D, generator=g)
    centres[256 - TINY:] = u + 0.05 * torch.randn(TINY, D, generator=g)        # the tiny lists: close neighbours
    rows, meta, aimed = [], [], []

    def add(x, same_meta=False):
        m = torch.zeros(x.shape[0], 4)
        m[:, 0] = 0.5 + 0.5 * torch.rand(1 if same_meta else x.shape[0], generator=g)
        m[:, 1] = NOW - 7200.0 * torch.rand(1 if same_meta else x.shape[0], generator=g)
        rows.append(x); meta.append(m)

    ordinary = torch.arange(LONG, 256 - TINY)
    for s in GROUPS:                                                            # near-duplicates, one metadata record
        base = centres[ordinary[torch.randint(0, ordinary.numel(), (1,), generator=g)]] + 0.3 * torch.randn(1, D, generator=g)
        add(base + 1e-5 * torch.randn(s, D, generator=g), same_meta=True)
        aimed += [base[0] + 0.02 * torch.randn(D, generator=g) for _ in range(2)]
    base = centres[ordinary[5]] + 0.3 * torch.randn(1, D, generator=g)
    add(base.repeat(TIE, 1), same_meta=True)                                    # exact ties
    aimed += [base[0].clone(), base[0] + 0.02 * torch.randn(D, generator=g)]
    for c in range(LONG):
        add(centres[c] + 0.3 * torch.randn(LONG_ROWS, D, generator=g))
    aimed += [v + 0.3 * torch.randn(D, generator=g) for _ in range(24)]
    for c in range(256 - TINY, 256):
        add(centres[c] + 0.01 * torch.randn(TINY_ROWS, D, generator=g))
    aimed += [u + 0.01 * torch.randn(D, generator=g) for _ in range(2)]
    rest = N - sum(x.shape[0] for x in rows)
    add(centres[ordinary[torch.randint(0, ordinary.numel(), (rest,), generator=g)]] + 0.3 * torch.randn(rest, D, generator=g))
    perm = torch.randperm(N, generator=g)                                       # tied rows are not neighbours
    return torch.cat(rows)[perm].contiguous(), torch.cat(meta)[perm].contiguous(), centres, torch.stack(aimed)


def _gauss_bank(D, g):
    rows = torch.randn(N, D, generator=g)
    meta = torch.zeros(N, 4)
    meta[:, 0] = 0.5 + 0.5 * torch.rand(N, generator=g)
    meta[:, 1] = NOW - 7200.0 * torch.rand(N, generator=g)
    centres = rows[torch.randint(0, N, (256,), generator=g)].clone()
    return rows, meta, centres, torch.empty(0, D)


def _check(ops, dev, kind, D, ks):
    g = torch.Generator().manual_seed(4000 + D + (1 if kind == "gauss" else 0))
    rows, meta, centres, aimed = (_clustered_bank if kind == "cluster" else _gauss_bank)(D, g)
    bank = rows.to(dev).contiguous()
    inv = torch.empty(N, device=dev); ops.bank_row_norms(bank, inv, 0, N)
    meta = meta.to(dev).contiguous()
    cent = centres.to(dev).contiguous()
    if kind == "cluster":
        cid = ops.kmeans_assign(bank, cent, N, 256)
        for c in range(256 - TINY, 256):                                        # the tiny lists keep TINY_ROWS rows each
            members = torch.nonzero(cid == c).flatten()
            cid[members[TINY_ROWS:]] = -1
    else:                                                                       # no structure: lists of ~64 rows drawn by lot
        cid = torch.randint(0, 256, (N,), generator=g).to(dev)
    meta[:, 2] = cid.float()
    lens = torch.bincount(cid[cid >= 0].long(), minlength=256)
    # the preconditions of a zero flag, on the inputs alone
    assert int(torch.topk(lens, 8).values.sum()) <= 4096, "the eight longest lists exceed the refine's candidate slots"
    assert max(GROUPS + (TIE,)) <= 1024
    if kind == "cluster":
        assert int(lens[256 - TINY:].max()) <= TINY_ROWS and int(lens[256 - TINY:].sum()) > 0
    st = ops.build_ivf2(bank, inv, meta[:, 2])
    lists = ops.Ivf2Lists(bank, inv, meta, cent, 8, st["sorted_bf16"], st["rho"], st["sorted_rows"], st["pad_off"],
                          st["list_len"], st["n_sorted"], None, None, st["rho16"])
    nq_big = torch.cuda.get_device_properties(dev).multi_processor_count + 44   # more queries than CUs: <6, 256, true>
    q_all = torch.cat([aimed, _queries(rows, nq_big - aimed.shape[0], g)]).to(dev).contiguous()
    if kind == "cluster":
        small = torch.stack([aimed[2 * GROUPS.index(R + 1)], aimed[2 * len(GROUPS) + 2], aimed[-1]])
    else:
        small = q_all[:3].cpu()
    for q, kk in ((q_all, ks), (small.to(dev).contiguous(), ks[-1:])):          # nq = 3: the one-query-per-CU geometry
        for k in kk:
            what = f"{kind} D={D} nq={q.shape[0]} k={k}"
            s1, r1, o1 = lists.search(q, k, NOW)
            flag = int(o1.item()) & ~ops.KNN_FLAG_NO_CANDIDATES               # (read before the next call resets it)
            s0, r0 = ops.knn_search(bank, inv, meta, q, k, NOW, centroids=cent, nprobe=8, fp32_scan=True)
            assert flag == 0, f"{what}: inverted lists, flag {flag}"
            assert torch.equal(r0, r1), f"{what}: inverted lists, {int((r0 != r1).any(1).sum())} queries differ in rows"
            assert torch.equal(s0, s1), f"{what}: inverted lists, score bits differ"
            s3, r3, o3 = ops.knn_search(bank, inv, meta, q, k, NOW, check_overflow=False, return_flag=True)
            flag = int(o3.item()) & ~ops.KNN_FLAG_NO_CANDIDATES
            s2, r2 = ops.knn_search(bank, inv, meta, q, k, NOW, fp32_scan=True)
            assert flag == 0, f"{what}: full scan, flag {flag}"
            assert torch.equal(r2, r3), f"{what}: full scan, {int((r2 != r3).any(1).sum())} queries differ in rows"
            assert torch.equal(s2, s3), f"{what}: full scan, score bits differ"
    if kind == "cluster" and ks[-1] > 8 * TINY_ROWS:                            # the n < k query did miss rows
        assert bool((r1[-1] < 0).any()) and bool((r1[-1] >= 0).any())


@pytest.mark.parametrize("D", DIMS)
def test_refine_rounds_and_select_paths(dev, D):
    from aura_snn_rag_amd import ops
    _check(ops, dev, "cluster", D, (1, 200, 32))


def test_refine_many_rounds_unclustered(dev):
    """k = 200 on a bank without structure: at least 200 survivors, five rounds or more."""
    from aura_snn_rag_amd import ops
    _check(ops, dev, "gauss", 392, (200,))
