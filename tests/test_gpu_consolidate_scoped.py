"""GPU tests of consolidation within tags (``aura_bank_find_repeats`` by tag and everything above it) against the rule
restated in torch fp64 on the CPU: the cosines of tests/cpu_stub_consolidate.py with every ineligible pair at -inf
(tests/cpu_stub_consolidate_scoped.py), then that stub's ``rule``, ``undecided`` and ``replay_check`` unchanged.

Tolerance: tol = 2 (D + 8) 2^-24, the rule's own (two fp32 evaluations of one cosine).  The replay check holds for every
row; rows that are decided and not tainted (the taint of tests/test_gpu_consolidate.py, on the masked in-batch cosines)
equal the fp64 rule exactly; per case at most 1 % of the rows may be undecided and at least 10 % must be decided
differently from the scope-blind rule (otherwise the data would not tell the two rules apart).  Every call prints its
counts (``SCOPED_COUNTS``): undecided rows, rows that differ from the scope-blind rule, rows that differ from fp64.

End-to-end data: that of tests/test_gpu_consolidate.py (seed 7; 480 groups of 6 near-copies, filled to 20 000 rows).
Copy c of a group carries tag 1 + c % 2, the filler rows tags in {0, 1, 2}: within tags every group keeps two memories,
18 080 = 2 * 480 + 17 120 in all, 1920 merges."""
import json

import numpy as np
import pytest
import torch

from tests import cpu_stub_consolidate_scoped as S
from tests.test_gpu_consolidate import _mixed_batch

R = S
pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
D, N, NQ = 768, 20_000, 600
INF = float("inf")


@pytest.fixture(scope="module")
def H():
    from aura_snn_rag_amd.core import hippocampal as H
    mp = pytest.MonkeyPatch()
    mp.setattr(H.time, "time", lambda: NOW)
    yield H
    mp.undo()


def _hf(H, dim=D, M=N, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(feature_dim=dim, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", **kw)


def _bulk(H, feats, tags, index, **kw):
    hf = _hf(H, dim=feats.shape[1], M=feats.shape[0], use_centroid_index=index, **kw)
    hf.centroids_update_interval = 10 ** 9
    torch.manual_seed(1)
    hf.bulk_write(feats, rebuild=index, tags=tags if isinstance(tags, int) else np.asarray(tags))
    return hf


def tagged(bank, n, seed, T=5):
    g = torch.Generator().manual_seed(1000 + seed)
    bank_tags = torch.randint(0, T, (bank.shape[0],), generator=g)
    src = torch.randint(0, bank.shape[0], (n,), generator=g)
    batch = _mixed_batch(bank, n, seed, copies_of=src)
    same = torch.rand(n, generator=g) < 0.5
    bt = torch.where(same, bank_tags[src], (bank_tags[src] + 1 + torch.randint(0, T - 1, (n,), generator=g)) % T)
    for i in range(20, n, 9):
        if (i // 9) % 2 == 0:
            bt[i] = bt[i - 13]
    return bank_tags, batch, bt


def _case(bank, n, seed):
    """``tagged`` for a batch of n rows (the generator places its degenerate rows up to row 50: 64 rows at the least)."""
    bank_tags, batch, bt = tagged(bank, max(n, 64), seed)
    return bank_tags, batch[:n].contiguous(), bt[:n].contiguous()


def _check_against_the_scoped_rule(hf, bank_tags, batch, bt, tau, tol, what):
    """find_repeats(tags=...) on the device vs the masked fp64 rule; returns (results, undecided, differ from blind)."""
    n = len(batch)
    assert torch.equal(hf.memory_tags.cpu().long(), bank_tags.long())
    st, bl, cs_dev = hf.find_repeats(batch.to(hf.device), tau, now=NOW, tags=bt.to(torch.int32).to(hf.device))
    assert st.dtype == torch.int32 and bl.dtype == torch.int32 and cs_dev.dtype == torch.float32 and not st.is_cuda
    cs0, cb0 = R.cosines(hf.memory_features, hf._inv_norm, hf.memory_count, batch)
    cs, cb = S.mask_cosines(cs0, cb0, bank_tags.long(), S.batch_tags(bt))
    bad = R.degenerate(batch)
    R.replay_check(cs, cb, tau, tol, st, bl, cs_dev, bad=bad)
    rs, rl, _ = R.rule(cs, cb, tau)
    und = R.undecided(cs, cb, tau, tol)
    near = (cb >= tau - tol).tolist()
    taint = und.clone()
    for i in range(n):
        if not taint[i] and any(near[i][j] for j in taint[:i].nonzero().flatten().tolist()):
            taint[i] = True
    ok = (st.long() == rs) & (bl.long() == rl)
    b_s, b_l, _ = R.rule(cs0, cb0, tau)
    blind = int(((b_s != rs) | (b_l != rl)).sum())
    print("SCOPED_COUNTS " + json.dumps(dict(case=what, n=n, N=hf.memory_count, D=batch.shape[1], tau=tau,
                                             undecided=int(und.sum()), differ_from_scope_blind=blind,
                                             differ_from_fp64=int((~ok).sum()), stored=int((rs >= 0).sum()),
                                             in_batch=int((rl >= 0).sum()))))
    assert bool(((st.long() == rs) | und).all()), "a decided row's stored target differs from the fp64 rule"
    assert bool(ok[~taint].all()), "a decided row differs from the fp64 rule"
    has = st >= 0
    assert bool((bank_tags[st[has].long()] == bt[has]).all()), "a stored target of another tag"
    lead = bl >= 0
    assert bool((bt[bl[lead].long()] == bt[lead]).all()), "a leader of another tag"
    return (st, bl, cs_dev), int(und.sum()), blind


# ------------------------------------------------------------------------------------- the scan paths
@pytest.mark.parametrize("dim", [768, 50])
def test_small_bank_dense_scan(H, dev, dim):
    g = torch.Generator().manual_seed(21)
    bank = torch.randn(3000, dim, generator=g)
    sizes = ((256, 1), (1000, 2), (1, 3), (33, 4))
    total = und = blind = 0
    tol = R.tolerance(dim)
    for n, seed in sizes:
        bank_tags, batch, bt = _case(bank, n, seed)
        hf = _bulk(H, bank, bank_tags, False)
        assert hf._ensure_shadow() is None                             # below SHADOW_MIN_ROWS: no image
        for tau in (0.9, 0.95):
            _, u, b = _check_against_the_scoped_rule(hf, bank_tags, batch, bt, tau, tol, f"dense-{dim}")
            total, und, blind = total + n, und + u, blind + b
        assert hf._shadow is None and hf._ivf is None and hf.memory_count == 3000
    assert und <= 0.01 * total, f"{und} of {total} rows undecided"
    assert blind >= 0.10 * total, f"only {blind} of {total} rows tell the scoped rule from the scope-blind one"


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("index", [False, True], ids=["row_shadow", "sorted_image"])
def test_image_scans(H, dev, dim, index):
    g = torch.Generator().manual_seed(21)
    bank = torch.randn(9000, dim, generator=g)
    tol = R.tolerance(dim)
    total = und = blind = 0
    hf = None
    for n, seed in ((1024, 5), (33, 6), (64, 7)):
        bank_tags, batch, bt = _case(bank, n, seed)
        if hf is None:
            hf = _bulk(H, bank, bank_tags, index)
        else:
            hf.retag(rows=torch.arange(9000), tag=bank_tags)           # this seed's bank tags: no image needs upkeep
        for tau in (0.9, 0.95):
            _, u, b = _check_against_the_scoped_rule(hf, bank_tags, batch, bt, tau, tol,
                                                     f"{'sorted_image' if index else 'row_shadow'}-{dim}")
            total, und, blind = total + n, und + u, blind + b
    assert und <= 0.01 * total, f"{und} of {total} rows undecided"
    assert blind >= 0.10 * total, f"only {blind} of {total} rows tell the scoped rule from the scope-blind one"
    if index:
        assert hf._candidate_mode() and hf._ivf is not None and hf._ivf.valid and not hf._unlisted_rows
    else:
        assert hf._shadow is not None and hf._ivf is None


def test_other_scopes_cannot_fill_a_list(H, dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(41)
    base = torch.randn(64, generator=g)
    bank = torch.randn(10_000, 64, generator=g)
    where = torch.randperm(10_000, generator=g)[:4000]
    bank[where] = base + 0.05 * torch.randn(4000, 64, generator=g)
    tags = torch.randint(0, 40, (10_000,), generator=g)
    tags[where] = torch.arange(4000) % 40                              # 100 copies under each of the 40 tags
    hf = _bulk(H, bank, tags, False)
    batch = (base[None, :] * torch.linspace(0.5, 2.0, 64)[:, None]).contiguous().to(dev)
    bt = (torch.arange(64) % 40).to(torch.int32)
    shadow = hf._ensure_shadow()
    assert shadow is not None
    args = (hf.memory_features, hf._inv_norm)
    packed = ops.find_repeats_scoped(*args, hf.memory_metadata, hf.memory_count, batch, bt.to(dev), 0.9, image=shadow,
                                     rho=hf._rho)[3].cpu()
    assert int(packed[3 * 64]) == 0, "100 survivors per row fit a list of 256: rows of other tags must not enter it"
    st = packed[:64].long()
    is_copy = torch.zeros(10_000, dtype=torch.bool)
    is_copy[where] = True
    assert bool((st >= 0).all()) and bool(is_copy[st].all()) and torch.equal(tags[st], bt.long())
    assert bool((packed[64:128] == -1).all())
    # the scope-blind search on the same inputs: 4000 survivors per row, the flag rises (the parent's overflow test)
    blind = ops.find_repeats(*args, hf.memory_count, batch, 0.9, image=shadow, rho=hf._rho)[3].cpu()
    assert int(blind[3 * 64]) != 0
    # 300 copies under ONE tag overflow that tag's lists: the flag rises and the call falls back to the fp32 scan
    more = where[(tags[where] != 7)][:200]
    hf.retag(rows=more, tag=7)
    tags[more] = 7
    packed = ops.find_repeats_scoped(*args, hf.memory_metadata, hf.memory_count, batch, bt.to(dev), 0.9, image=shadow,
                                     rho=hf._rho)[3].cpu()
    assert int(packed[3 * 64]) != 0
    st, bl, cs_dev = hf.find_repeats(batch, 0.9, tags=bt.to(dev))
    cs0, cb0 = R.cosines(hf.memory_features, hf._inv_norm, hf.memory_count, batch.cpu())
    cs, cb = S.mask_cosines(cs0, cb0, tags, bt.long())
    R.replay_check(cs, cb, 0.9, R.tolerance(64), st, bl, cs_dev)       # (best two targets within tol by construction)
    assert bool((st >= 0).all()) and bool(is_copy[st.long()].all()) and torch.equal(tags[st.long()], bt.long())


@pytest.mark.parametrize("mode", ["dense", "row_shadow", "sorted_image"])
def test_exact_duplicates_across_tags_report_the_lowest_row_of_the_tag(H, dev, mode):
    g = torch.Generator().manual_seed(51)
    bank = torch.randn(9000, 64, generator=g)
    dup = {17: [17, 4000, 8999], 300: [300, 301, 7000], 8500: [8500, 8998]}
    for first, rows in dup.items():
        bank[rows] = bank[first].clone()
    tags = torch.randint(0, 5, (9000,), generator=g)
    tags[[17, 4000, 8999]] = torch.tensor([1, 2, 2])
    tags[[300, 301, 7000]] = torch.tensor([0, 3, 3])
    tags[[8500, 8998]] = torch.tensor([1, 1])
    hf = _bulk(H, bank, tags, mode == "sorted_image", bf16_shadow=mode != "dense")
    batch = bank[[8999, 17, 7000, 300, 8998, 8998, 4000, 301]] * 3.0
    bt = [2, 1, 3, 0, 1, 2, 1, 4]
    st, bl, cs = hf.find_repeats(batch.to(dev), 0.99, tags=bt)
    assert st.tolist() == [4000, 17, 301, 300, 8500, -1, 17, -1] and bl.tolist() == [-1] * 8
    assert bool((cs[st >= 0] - 1.0).abs().max() <= R.tolerance(64)) and bool((cs[st < 0] == -INF).all())
    assert (hf._shadow is not None) == (mode == "row_shadow") and (hf._ivf is not None) == (mode == "sorted_image")


def test_one_tag_everywhere_equals_the_unscoped_search(H, dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(61)
    bank = torch.randn(9000, 64, generator=g)
    hf = _bulk(H, bank, 3, True)
    batch = _mixed_batch(bank, 256, 8).to(dev)
    bt = torch.full((256,), 3, dtype=torch.int32, device=dev)
    hf._ensure_norms()
    shadow, ivf = hf._ensure_shadow(), hf._ensure_ivf()
    assert shadow is not None and ivf is not None and not hf._unlisted_rows
    modes = dict(dense={}, row_shadow=dict(image=shadow, rho=hf._rho),
                 sorted_image=dict(image=ivf.sorted_bf16, image_rows=ivf.sorted_rows, n_image=ivf.n_sorted, rho=hf._rho,
                                   lists_flag=ivf.flag))
    for name, kw in modes.items():
        a = ops.find_repeats(hf.memory_features, hf._inv_norm, hf.memory_count, batch, 0.9, **kw)[3].cpu()
        b = ops.find_repeats_scoped(hf.memory_features, hf._inv_norm, hf.memory_metadata, hf.memory_count, batch, bt, 0.9,
                                    **kw)[3].cpu()
        assert int(a[3 * 256]) == 0 and int(a[3 * 256 + 1]) == 0, name
        assert torch.equal(a, b), f"{name}: stored, leader or the cos bits differ from the unscoped search"
        assert int((a[:256] >= 0).sum()) > 50 and int((a[256:512] >= 0).sum()) > 5
    # another tag on the batch: nothing held is eligible, the in-batch walk is unchanged among equal tags
    other = ops.find_repeats_scoped(hf.memory_features, hf._inv_norm, hf.memory_metadata, hf.memory_count, batch,
                                    torch.full_like(bt, 4), 0.9, image=shadow, rho=hf._rho)[3].cpu()
    assert bool((other[:256] == -1).all())


# ------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    fam = torch.randn(40, D, generator=g)
    groups = fam.repeat_interleave(12, 0) + 0.8 * torch.randn(480, D, generator=g)
    copies = groups.repeat_interleave(6, 0) + 0.05 * torch.randn(2880, D, generator=g)
    feats = torch.cat([copies, torch.randn(N - 2880, D, generator=g)])
    label = torch.cat([torch.arange(480).repeat_interleave(6), 480 + torch.arange(N - 2880)])
    perm = torch.randperm(N, generator=g)
    g2 = torch.Generator().manual_seed(70)
    tags = torch.cat([1 + (torch.arange(2880) % 6) % 2, torch.randint(0, 3, (N - 2880,), generator=g2)])
    feats, label, tags = feats[perm].contiguous(), label[perm], tags[perm]
    torch.rand(N, generator=g)                                         # (the strengths of the parent's data)
    q = groups[torch.randint(0, 480, (NQ,), generator=g)] + 0.3 * torch.randn(NQ, D, generator=g)
    return feats, label, tags, q.contiguous()


def _stream(H, data, dev, index, batch):
    feats, label, tags, _ = data
    hf = _hf(H, use_centroid_index=index)
    torch.manual_seed(3)
    reports = []
    for lo in range(0, N, batch):
        rep = hf.create_episodic_memories([f"r{i}" for i in range(lo, min(N, lo + batch))], feats[lo:lo + batch].to(dev),
                                          merge_similarity=0.9, tags=tags[lo:lo + batch].numpy(), merge_within_tags=True)
        reports.append((lo, rep))
    return hf, reports


@pytest.mark.parametrize("index,batch", [(True, 1000), (False, 64)], ids=["on-1000", "off-64"])
def test_a_tagged_stream_keeps_one_memory_per_group_and_tag(H, dev, data, index, batch):
    feats, label, tags, q = data
    hf, reports = _stream(H, data, dev, index, batch)
    assert hf.memory_count == 18_080 and sum(r.n_merged for _, r in reports) == 1920
    origin = torch.tensor([int(hf.id_of_row(r)[1:]) for r in range(hf.memory_count)])        # slot -> stream index
    assert torch.equal(hf.memory_tags.cpu().long(), tags[origin])
    pairs = set(zip(label[origin].tolist(), tags[origin].tolist()))
    assert len(pairs) == 18_080, "two members of one group are held under one tag"
    for lo, rep in reports:
        m = rep.merged.nonzero().flatten()
        if len(m):
            tgt = torch.tensor([int(rep.ids[i][1:]) for i in m.tolist()])
            assert torch.equal(tags[tgt], tags[lo + m]), "a merged pair crosses a tag"
            assert torch.equal(label[tgt], label[lo + m]) and torch.equal(origin[rep.rows[m]], tgt)
    if index:
        assert hf._index_ready and hf._candidate_mode()
    _, rows = hf.recall_batch(q.to(dev), k=8, now=NOW, tags=1)
    rows = rows.cpu().long()
    assert bool((rows >= 0).all()) and bool((tags[origin][rows] == 1).all())
    assert all(len(set(gq.tolist())) == 8 for gq in label[origin][rows])


def test_consolidate_within_tags_leaves_the_streams_bank(H, dev, data):
    feats, label, tags, _ = data
    stream, _ = _stream(H, data, dev, False, 1000)
    hf = _hf(H)
    hf.bulk_write(feats, rebuild=False, tags=tags.numpy())
    assert hf.memory_count == N
    rep = hf.consolidate(0.9, within_tags=True)
    assert (rep.n_before, rep.n_kept, rep.n_merged) == (N, 18_080, 1920) and hf.memory_count == stream.memory_count == 18_080
    assert torch.equal(hf.memory_features, stream.memory_features)      # bit for bit, the cleared tail included
    assert torch.equal(hf.memory_tags, stream.memory_tags)
    kept = torch.from_numpy(rep.old_to_new)
    assert torch.equal(hf.memory_tags.cpu().long()[kept], tags), "a row merged into a memory of another tag"
    # the scope-blind pass on the same rows merges across tags: one memory per group
    blind = _hf(H)
    blind.bulk_write(feats, rebuild=False, tags=tags.numpy())
    assert blind.consolidate(0.9).n_kept == 17_600
