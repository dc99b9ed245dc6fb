"""GPU tests of tags and scoped recall (``aura_bank_set_tags``, ``aura_knn_search_scoped``) and of the host paths above.

Data (``tests/cpu_stub_scoped.scoped_data``, seed 11): D in {768, 100, 50}; N = 6000 held rows (3000 at D = 50) in a bank
of N + 500; randn features; strength 0.25 + 0.75 rand; fp32 timestamps NOW - 128 randint(0, 60); tag 1 has 1 row, tag 2
has 7 (fewer than k), tag 3 has 130 (straddles a 128-row tile), tag 4 about 45 % of the rows, 200 rows untagged, tags
5 .. 40 share the rest; shuffled.  96 queries cycle through the scopes [1, 2, 3, 4, 5, 17, 40, any], k = 8.  The 500 rows
BEYOND ``memory_count`` carry matching tags, full strength, the newest timestamp and copies of the queries as features:
they would win every scope they are let into, so every test below also checks that they are never returned.

The reference of a case is the oracle's ``OracleBank.scores`` over the rows that satisfy the rule (the rule restated with
torch ops, ``cpu_stub_scoped.scope_mask``) followed by ``topk``; ``helpers.topk_equivalent`` must hold (scores within
1e-5, an index may differ only at an oracle near-tie of 2e-6) and at most 2 of the 96 queries may be index-inexact."""
import numpy as np
import pytest
import torch

from oracle import aura_oracle as O
from tests import cpu_stub_scoped as R
from tests.helpers import record_parity, topk_equivalent

pytestmark = pytest.mark.gpu
NOW = R.NOW
K = 8
INF = float("inf")


@pytest.fixture(scope="module")
def H():
    from aura_snn_rag_amd.core import hippocampal as H
    mp = pytest.MonkeyPatch()
    mp.setattr(H.time, "time", lambda: NOW)
    yield H
    mp.undo()


def _hf(H, D, M, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", **kw)


def _fill(H, d, D, N):
    hf = _hf(H, D, N + R.EXTRA_ROWS)
    hf.bulk_write(d["feats"], tags=d["tags"], rebuild=False)
    hf.memory_metadata[:N, 0] = d["strength"].cuda()
    hf.memory_metadata[:N, 1] = d["ts"].cuda()
    hf.memory_locations[:N] = d["locs"].cuda()
    return hf


_BANKS = {}


def _bank(H, D):
    """(hf, the oracle's bank, data) of one D, built once."""
    if D not in _BANKS:
        N = 3000 if D == 50 else 6000
        d = R.scoped_data(D, N)
        hf = _fill(H, d, D, N)
        # the rows beyond memory_count: they match every scope and would beat every held row
        E = R.EXTRA_ROWS
        reps = d["q"][torch.arange(E) % d["q"].shape[0]]
        hf.memory_features[N:] = reps.cuda()
        hf.memory_locations[N:] = d["q_loc"][torch.arange(E) % d["q"].shape[0]].cuda()
        extra_tags = torch.tensor([R.QUERY_SCOPES[i % 7] for i in range(E)], dtype=torch.float32)
        hf.memory_metadata[N:] = torch.stack([torch.ones(E), torch.full((E,), NOW), torch.full((E,), -1.0), extra_tags],
                                             dim=1).cuda()
        hf._inv_norm[N:] = (1.0 / reps.norm(dim=1)).cuda()
        ob = O.OracleBank(max_memories=N, feature_dim=D, spatial_dims=2, use_centroid_index=False)
        ob.features[:N], ob.locations[:N] = d["feats"], d["locs"]
        ob.metadata[:N] = torch.stack([d["strength"], d["ts"], torch.full((N,), -1.0),
                                       torch.from_numpy(d["tags"]).float()], dim=1)
        ob.count = N
        _BANKS[D] = (hf, ob, d, N)
    return _BANKS[D]


def _reference(ob, d, N, k, qtags, with_loc, sel=None, **cond):
    """(rows [nq, k], scores [nq, k], all scores [nq, N], scope sizes): the oracle over the rows the rule admits."""
    sel = range(d["q"].shape[0]) if sel is None else sel
    rows = torch.full((len(sel), k), -1, dtype=torch.int64)
    scores = torch.full((len(sel), k), -INF)
    full = torch.full((len(sel), N), -INF)
    sizes = []
    for j, i in enumerate(sel):
        cand = torch.nonzero(R.scope_mask(ob.metadata, N, int(qtags[j]), **cond)).flatten()
        sizes.append(int(cand.numel()))
        if cand.numel() == 0:
            continue
        sc = ob.scores(d["q"][i], NOW, d["q_loc"][i] if with_loc else None, cand=cand)
        full[j, cand] = sc
        s, p = torch.topk(sc, min(k, cand.numel()))
        rows[j, :s.numel()], scores[j, :s.numel()] = cand[p], s
    return rows, scores, full, sizes


def _hard_properties(hf, N, rows, scores, qtags, sizes, k, **cond):
    """No tolerance: every returned row satisfies the rule and is a held row, padding exactly in the tail."""
    rows, scores = rows.cpu().long(), scores.cpu()
    meta = hf.memory_metadata.cpu()
    assert rows.shape == scores.shape == (len(qtags), k)
    for j in range(rows.shape[0]):
        n_hit = min(k, sizes[j])
        got = rows[j]
        assert bool((got[:n_hit] >= 0).all()) and bool((got[n_hit:] == -1).all()), (j, got.tolist(), sizes[j])
        assert bool((scores[j, n_hit:] == -INF).all()) and bool(torch.isfinite(scores[j, :n_hit]).all())
        assert bool((got[:n_hit] < N).all()), "a row at or beyond memory_count was returned"
        ok = R.scope_mask(meta, N, int(qtags[j]), **cond)
        assert bool(ok[got[:n_hit]].all()), (j, "a returned row is outside the scope")
        assert len(set(got[:n_hit].tolist())) == n_hit
        assert bool((scores[j, :n_hit - 1] >= scores[j, 1:n_hit]).all()) if n_hit > 1 else True


def _case(H, D, name, with_loc=False, k=K, max_inexact=2, **cond):
    hf, ob, d, N = _bank(H, D)
    qtags = d["qtags"]
    s, r = hf.recall_batch(d["q"].cuda(), k=k, now=NOW, tags=qtags, locations=d["q_loc"] if with_loc else None, **cond)
    ref_r, ref_s, full, sizes = _reference(ob, d, N, k, qtags, with_loc, **cond)
    _hard_properties(hf, N, r, s, qtags, sizes, k, **cond)
    exact, n, ok = topk_equivalent(r, s, ref_r, ref_s, full_ref_scores=full)
    print(f"scoped {name}: {exact}/{n} queries index-exact, equivalent={ok}, "
          f"max |score diff| = {float((s.cpu() - ref_s)[torch.isfinite(ref_s)].abs().max()):.3g}")
    record_parity(f"scoped_{name}", exact, n)
    assert ok, f"{name}: scores off by more than 1e-5 or an index differs away from a near-tie"
    assert n - exact <= max_inexact, f"{name}: {n - exact} of {n} queries are index-inexact"
    return s, r, sizes


@pytest.mark.parametrize("D", [768, 100, 50])
def test_scoped_recall_matches_the_oracle(H, D):
    _, _, sizes = _case(H, D, f"D{D}")
    assert sizes[:4] == [1, 7, 130, int(0.45 * (3000 if D == 50 else 6000))]


def test_with_locations(H):
    _case(H, 100, "D100_locations", with_loc=True)


def test_with_min_strength(H):
    _, _, sizes = _case(H, 768, "D768_min_strength", min_strength=0.6)
    assert sizes[3] < int(0.45 * 6000) * 0.7              # the floor really cut the scope


def test_with_a_time_window_closed_at_both_ends(H):
    hf, ob, d, N = _bank(H, 50)
    lo, hi = float(np.float32(NOW - 128.0 * 40)), float(np.float32(NOW - 128.0 * 10))
    ts = d["ts"]
    assert bool((ts == lo).any()) and bool((ts == hi).any()), "the bounds must sit on stored timestamps"
    _, r, sizes = _case(H, 50, "D50_window", newer_than=lo, older_than=hi)
    # rows exactly at either bound are inside: the "any tag" queries' scope counts them
    assert sizes[7] == int(((ts >= lo) & (ts <= hi)).sum())
    got = ts[r.cpu().long().clamp(min=0)][r.cpu() >= 0]
    assert bool((got >= lo).all()) and bool((got <= hi).all())


def test_a_tag_nobody_carries_and_untagged_rows(H):
    hf, ob, d, N = _bank(H, 100)
    q = d["q"][:5].cuda()
    s, r = hf.recall_batch(q, k=K, now=NOW, tags=999)
    assert bool((r == -1).all()) and bool((s == -INF).all())
    s, r = hf.recall_batch(q, k=K, now=NOW, tags=0)       # 0 selects the untagged rows
    assert bool((r >= 0).all()) and bool((hf.memory_tags[r.long().flatten()] == 0).all())
    # more distinct tags than one library call takes: served in chunks, same results
    qq = d["q"][torch.arange(300) % 96].cuda()
    s_many, r_many = hf.recall_batch(qq, k=K, now=NOW, tags=np.arange(300) + 5)
    s_ref, r_ref = hf.recall_batch(qq, k=K, now=NOW, tags=np.where(np.arange(300) + 5 <= 40, np.arange(300) + 5, 999))
    assert torch.equal(r_many, r_ref) and torch.equal(s_many, s_ref)


def test_results_do_not_depend_on_the_batch(H):
    hf, ob, d, N = _bank(H, 768)
    q, qtags = d["q"].cuda(), d["qtags"]
    s, r = hf.recall_batch(q, k=K, now=NOW, tags=qtags)
    for i in (0, 1, 2, 3, 4, 7, 43, 95):                   # every scope kind, one query at a time
        s1, r1 = hf.recall_batch(q[i:i + 1], k=K, now=NOW, tags=int(qtags[i]))
        assert torch.equal(r1[0], r[i]) and torch.equal(s1[0].view(torch.int32), s[i].view(torch.int32)), i
    s2, r2 = hf.recall_batch(q.flip(0).contiguous(), k=K, now=NOW, tags=qtags[::-1].copy())
    assert torch.equal(r2.flip(0), r) and torch.equal(s2.flip(0).view(torch.int32), s.view(torch.int32))
    # ... nor on how many workgroups share a scope's rows
    from aura_snn_rag_amd import ops
    for splits in (1, 3, 64):
        s3, r3 = ops.knn_search_scoped(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, K, NOW, N, tags=qtags,
                                       splits=splits)
        assert torch.equal(r3, r) and torch.equal(s3.view(torch.int32), s.view(torch.int32)), splits


def test_whole_bank_scope_equals_the_plain_exact_recall(H):
    hf, ob, d, N = _bank(H, 768)
    q = d["q"].cuda()
    s, r = hf.recall_batch(q, k=K, now=NOW, min_strength=0.0)
    ps, pr = hf.recall_batch(q, k=K, now=NOW, use_candidates=False)
    exact, n, ok = topk_equivalent(r, s, pr, ps)
    assert ok and n - exact <= 2, (exact, n)


def test_scope_of_a_tag_equals_a_bank_that_holds_only_that_tag(H):
    hf, ob, d, N = _bank(H, 100)
    q = d["q"].cuda()
    s, r = hf.recall_batch(q, k=K, now=NOW, tags=4)
    sub = _fill(H, d, 100, N)
    rep = sub.forget(tags=[t for t in range(41) if t != 4])
    assert sub.memory_count == int(0.45 * N) and rep.n_removed == N - sub.memory_count
    assert bool((sub.memory_tags == 4).all())
    ps, pr = sub.recall_batch(q, k=K, now=NOW, use_candidates=False)
    ids_a = [[hf.id_of_row(x) for x in row] for row in r.tolist()]
    ids_b = [[sub.id_of_row(x) for x in row] for row in pr.tolist()]
    # the same memories: compare through the rows of bank A (old_to_new maps A's rows to B's)
    back = np.full(sub.memory_count, -1, dtype=np.int64)
    back[rep.old_to_new[rep.old_to_new >= 0]] = np.nonzero(rep.old_to_new >= 0)[0]
    exact, n, ok = topk_equivalent(torch.from_numpy(back[pr.cpu().numpy()]), ps, r, s)
    assert ok and n - exact <= 2, (exact, n)
    assert sum(a == b for a, b in zip(ids_a, ids_b)) == exact


@pytest.mark.parametrize("tag,k", [(4, 1), (4, 128), (3, 128)])
def test_limits_of_k(H, tag, k):
    hf, ob, d, N = _bank(H, 768)
    sel = list(range(12))
    q = d["q"][:12].cuda()
    qtags = np.full(12, tag)
    s, r = hf.recall_batch(q, k=k, now=NOW, tags=tag)
    ref_r, ref_s, full, sizes = _reference(ob, d, N, k, qtags, False, sel=sel)
    _hard_properties(hf, N, r, s, qtags, sizes, k)
    exact, n, ok = topk_equivalent(r, s, ref_r, ref_s, full_ref_scores=full)
    print(f"scoped tag {tag} k {k}: {exact}/{n} index-exact")
    assert ok
    with pytest.raises(ValueError, match="128"):
        hf.recall_batch(q, k=129, now=NOW, tags=tag)


def test_tag_stamping_on_the_device(H):
    g = torch.Generator().manual_seed(3)
    # a full bank in the reference's mode rewrites slot 0: the last row's tag stays
    hf = _hf(H, 16, 8, overflow="reference")
    hf.create_episodic_memories([f"m{i}" for i in range(12)], torch.randn(12, 16, generator=g), tags=np.arange(1, 13))
    assert hf.memory_tags.tolist() == [12, 2, 3, 4, 5, 6, 7, 8] and hf.id_of_row(0) == "m11"
    assert hf.memory_metadata[:, 0].tolist() == [1.0] * 8
    # a ring that wraps
    hf = _hf(H, 16, 8, overflow="fifo")
    hf.create_episodic_memories([f"m{i}" for i in range(11)], torch.randn(11, 16, generator=g), tags=np.arange(1, 12))
    assert hf.memory_tags.tolist() == [9, 10, 11, 4, 5, 6, 7, 8]
    hf.create_episodic_memories(["u"], torch.randn(1, 16, generator=g))                 # untagged over a tagged slot
    assert hf.memory_tags.tolist() == [9, 10, 11, 0, 5, 6, 7, 8]
    # bulk_write, retag, and tags moved by the real compaction
    hf = _hf(H, 64, 5000)
    tags = torch.randint(0, 9, (4000,), generator=g).numpy()
    hf.bulk_write(torch.randn(4000, 64, generator=g), tags=tags, rebuild=False)
    assert np.array_equal(hf.memory_tags.cpu().numpy(), tags)
    assert not bool(hf.memory_metadata[4000:].any())
    hf.retag(rows=[5, 6, 4999, -1], tag=77)
    tags[[5, 6]] = 77
    assert np.array_equal(hf.memory_tags.cpu().numpy(), tags)
    rep = hf.forget(tags=[3, 77])
    keep = ~np.isin(tags, [3, 77])
    assert rep.n_removed == int((~keep).sum()) and np.array_equal(hf.memory_tags.cpu().numpy(), tags[keep])


def test_layer_stores_and_retrieves_within_a_tag(H):
    from aura_snn_rag_amd.core.language_zone.memory_ops import BatchedMemoryMixin

    class Layer(BatchedMemoryMixin, torch.nn.Module):
        def __init__(self, hippocampus):
            super().__init__()
            self.hippocampus = hippocampus
            self.query_proj = torch.nn.Identity()

    g = torch.Generator().manual_seed(5)
    hf = _hf(H, 64, 256)
    layer = Layer(hf)
    h = torch.randn(6, 4, 64, generator=g).cuda()
    near = h + 1e-3 * torch.randn(6, 4, 64, generator=g).cuda()
    layer.store_memory(h, tag=1)
    layer.store_memory(near, tag=2)
    hf.bulk_write(torch.randn(100, 64, generator=g), rebuild=False)                     # untagged bystanders
    for tag, own in ((1, h), (2, near)):
        feats, scores = layer.retrieve_memories(h, k=3, tags=tag)
        assert torch.equal(feats[:, 0], own.mean(dim=1)), tag                          # its own copy, not the near one
        _, rows = hf.recall_batch(h.mean(dim=1), k=3, tags=tag)
        assert bool((hf.memory_tags[rows.long().flatten()] == tag).all())
    feats, _ = layer.retrieve_memories(h, k=3)                                          # no scope: both copies compete
    assert feats.shape == (6, 3, 64)
