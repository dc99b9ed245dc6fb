"""GPU tests of diverse recall (``aura_diverse_select`` and everything above it) against the rule restated in
torch fp64 on the CPU (tests/cpu_stub_diverse.py).

Data (seed 7): D = 768; 40 family vectors; 12 groups per family (family + 0.8 randn); 6 near-copies per group
(group + 0.05 randn); filled to 20 000 rows with randn; rows shuffled; strengths 0.5 + 0.5 rand; every timestamp =
now; 600 queries (a group + 0.3 randn).  Cosines are about 0.998 inside a group and about 0.61 between the groups
of a family, far from max_similarity = 0.9 on both sides.

Tolerance: a device cosine differs from the exact one by at most (D + 8) 2^-24 for unit rows (fp32 dot-product
bound plus the two inv_norm roundings); two are compared: tol = 2 (D + 8) 2^-24 = 9.3e-5 at D = 768."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_diverse as R
from tests.cpu_stub_retention import reinforce_reference

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
NOW32 = float(np.float32(NOW))
D, N, NQ = 768, 20_000, 600
TOL = R.tolerance(D)
CONFIGS = [(64, 8, 0.0, 0.9), (64, 8, 0.5, 0.9), (64, 8, 0.5, None), (32, 5, 0.5, None), (128, 32, 0.5, None)]


@pytest.fixture(scope="module")
def H():
    from aura_snn_rag_amd.core import hippocampal as H
    mp = pytest.MonkeyPatch()
    mp.setattr(H.time, "time", lambda: NOW)
    yield H
    mp.undo()


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    fam = torch.randn(40, D, generator=g)
    groups = fam.repeat_interleave(12, 0) + 0.8 * torch.randn(480, D, generator=g)
    copies = groups.repeat_interleave(6, 0) + 0.05 * torch.randn(2880, D, generator=g)
    feats = torch.cat([copies, torch.randn(N - 2880, D, generator=g)])
    label = torch.cat([torch.arange(480).repeat_interleave(6), 480 + torch.arange(N - 2880)])
    perm = torch.randperm(N, generator=g)
    feats, label = feats[perm].contiguous(), label[perm]
    strength = 0.5 + 0.5 * torch.rand(N, generator=g)
    q = groups[torch.randint(0, 480, (NQ,), generator=g)] + 0.3 * torch.randn(NQ, D, generator=g)
    return feats, label, strength, q.contiguous()


def _bank(H, dev, data, index):
    feats, _, strength, _ = data
    hf = H.HippocampalFormation(feature_dim=D, max_memories=N, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                device="cuda", use_centroid_index=index)
    hf.centroids_update_interval = 10 ** 9
    torch.manual_seed(1)
    hf.bulk_write(feats, rebuild=index)
    hf.memory_metadata[:, 0] = strength.to(dev)
    hf.memory_metadata[:, 1] = NOW32
    hf._invalidate_lists()
    return hf


@pytest.fixture(scope="module")
def bank_off(H, dev, data):
    return _bank(H, dev, data, False)


@pytest.fixture(scope="module")
def bank_on(H, dev, data):
    return _bank(H, dev, data, True)


def _select(hf, q, F, k, d, tau):
    from aura_snn_rag_amd import ops
    cs, cr = hf.recall_batch(q, k=F, now=NOW)
    s, r = ops.diverse_select(hf.memory_features, hf._inv_norm, hf.memory_count, cr, cs, k, d, tau)
    return cs, cr, s, r


def _distinct_groups(label, rows):
    return torch.tensor([len(set(label[r[r >= 0].long()].tolist())) for r in rows.cpu()])


# ------------------------------------------------------------------------------------- 1, 2, 3: the rule
@pytest.mark.parametrize("index", [False, True], ids=["index_off", "index_on"])
@pytest.mark.parametrize("F,k,d,tau", CONFIGS)
def test_picks_follow_the_rule(dev, data, bank_off, bank_on, index, F, k, d, tau):
    hf = bank_on if index else bank_off
    q = data[3].to(dev)
    cs, cr, s, r = _select(hf, q, F, k, d, tau)
    if index:
        assert hf._ivf is not None and hf._ivf.valid, "600 queries were expected to run through the inverted lists"
    cos = R.cosines(hf.memory_features, hf._inv_norm, cr, hf.memory_count)
    # 1. every query, no exclusions
    pj = R.replay_check(cr, cs, cos, hf.memory_count, k, d, tau, s, r, TOL)
    assert bool((pj[:, 0] == 0).all()), "the first pick is candidate 0"
    # 2. decided queries: exactly the fp64 picks
    want, margin = R.select_reference(cr, cs, cos, hf.memory_count, k, d, tau)
    decided = margin >= TOL
    same = (pj == want).all(1)
    print(f"F={F} k={k} d={d} tau={tau} index={index}: {int(decided.sum())} of {NQ} queries decided, "
          f"{int(same.sum())} of {NQ} equal to the fp64 picks, {int((pj >= 0).all(1).sum())} full results")
    assert bool(same[decided].all()), f"{int((~same & decided).sum())} decided queries differ from the fp64 picks"
    # the same result through the public call
    s2, r2 = hf.recall_batch(q, k=k, now=NOW, diversity=d, max_similarity=tau, fetch_k=F)
    assert torch.equal(r2, r) and torch.equal(s2.view(torch.int32), s.view(torch.int32))


@pytest.mark.parametrize("F,k", [(64, 8), (32, 5), (128, 32), (33, 33), (96, 7), (1, 1)])
def test_no_diversity_no_limit_is_the_plain_top_k(dev, data, bank_off, F, k):
    q = data[3].to(dev)
    cs, cr, s, r = _select(bank_off, q, F, k, 0.0, None)
    assert torch.equal(r, cr[:, :k]) and torch.equal(s.view(torch.int32), cs[:, :k].contiguous().view(torch.int32))
    s2, r2 = bank_off.recall_batch(q, k=k, now=NOW, diversity=0.0, fetch_k=F)
    sp, rp = bank_off.recall_batch(q, k=k, now=NOW)
    assert torch.equal(r2, rp) and torch.equal(s2.view(torch.int32), sp.view(torch.int32))


# ------------------------------------------------------------------------------------- 4: behaviour
def test_near_copies_leave_the_top_k(dev, data, bank_off, bank_on):
    label, q = data[1], data[3].to(dev)
    _, plain = bank_off.recall_batch(q, k=8, now=NOW)
    repeats = int((_distinct_groups(label, plain) < 8).sum())
    s, r = bank_off.recall_batch(q, k=8, now=NOW, max_similarity=0.9, fetch_k=64)
    groups = _distinct_groups(label, r)
    print(f"plain top-8 repeats a group in {repeats} of {NQ} queries; diverse: {int((groups == 8).sum())} of {NQ} "
          f"hold 8 distinct groups")
    assert repeats >= 590
    assert bool((r >= 0).all()) and bool((groups == 8).all())
    assert torch.equal(r[:, 0], plain[:, 0])
    # the default fetch (max(32, 4 k) = 32 candidates) through the same call
    s32, r32 = bank_off.recall_batch(q, k=8, now=NOW, max_similarity=0.9)
    filled = (r32 >= 0).sum(1).cpu()
    assert bool((_distinct_groups(label, r32) == filled).all())
    # F = k = 8: results run short, picks first, then padding to the end
    s8, r8 = bank_off.recall_batch(q, k=8, now=NOW, max_similarity=0.9, fetch_k=8)
    n8 = (r8 >= 0).sum(1)
    print(f"F = k = 8: {int(n8.min())} to {int(n8.max())} rows per query")
    assert int(n8.min()) >= 1 and int((n8 < 8).sum()) >= 590     # (every query whose plain top-8 repeats a group)
    pad = torch.arange(8, device=dev)[None, :] >= n8[:, None]
    assert bool((r8[pad] == -1).all()) and bool((s8[pad] == float("-inf")).all()) and bool((r8[~pad] >= 0).all())
    assert bool((_distinct_groups(label, r8) == n8.cpu()).all())
    # index on: the candidates are the probed lists' rows; every query with 64 valid candidates
    cs, cr = bank_on.recall_batch(q, k=64, now=NOW)
    so, ro = bank_on.recall_batch(q, k=8, now=NOW, max_similarity=0.9, fetch_k=64)
    full = (cr >= 0).all(1).cpu()
    print(f"index on: {int(full.sum())} of {NQ} queries have 64 valid candidates")
    assert int(full.sum()) > 0 and bool((_distinct_groups(label, ro)[full] == 8).all())


# ------------------------------------------------------------------------------------- 5: invalid candidates
def test_invalid_candidates_are_ignored(dev, data, bank_off):
    from aura_snn_rag_amd import ops
    hf, q = bank_off, data[3][:64].to(dev)
    cs, cr = hf.recall_batch(q, k=48, now=NOW)
    g = torch.Generator().manual_seed(11)
    holes = torch.rand(64, 64, generator=g) < 0.25
    holes[:, 0] = False
    holes[5] = False
    holes[6, 1:] = True                                     # one valid candidate only
    pos = torch.cumsum((~holes).long(), 1) - 1              # where each kept slot takes its candidate from
    keep = ~holes & (pos < 48)
    rows = torch.full((64, 64), -1, dtype=torch.int32)
    scores = torch.full((64, 64), float("-inf"))
    src = pos.clamp(0, 47)
    rows[keep] = cr.cpu().gather(1, src)[keep]
    scores[keep] = cs.cpu().gather(1, src)[keep]
    bad = holes.clone()
    rows[bad & (torch.arange(64)[None, :] % 3 == 0)] = N + 5              # outside the bank
    scores[bad & (torch.arange(64)[None, :] % 3 == 1)] = float("nan")
    rows[bad & (torch.arange(64)[None, :] % 3 == 1)] = 17                 # a real row with a NaN score
    for k, d, tau in ((8, 0.5, 0.9), (8, 0.0, None), (20, 0.5, None)):
        s1, r1 = ops.diverse_select(hf.memory_features, hf._inv_norm, N, rows.to(dev), scores.to(dev), k, d, tau)
        # the same candidates, compacted
        comp_r = torch.full((64, 64), -1, dtype=torch.int32)
        comp_s = torch.full((64, 64), float("-inf"))
        n_ok = keep.sum(1)
        for i in range(64):
            comp_r[i, :n_ok[i]] = rows[i][keep[i]]
            comp_s[i, :n_ok[i]] = scores[i][keep[i]]
        s2, r2 = ops.diverse_select(hf.memory_features, hf._inv_norm, N, comp_r.to(dev), comp_s.to(dev), k, d, tau)
        assert torch.equal(r1, r2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
        cos = R.cosines(hf.memory_features, hf._inv_norm, rows, N)
        R.replay_check(rows, scores, cos, N, k, d, tau, s1, r1, TOL)
        assert int(r1[6, 0]) == int(rows[6, 0]) and bool((r1[6, 1:] == -1).all())
    # a short bank: count < F, and rows at or beyond count are invalid
    count = 40
    cs2, cr2 = ops.knn_search(hf.memory_features, hf._inv_norm, hf.memory_metadata, q, 40, NOW, count=count)
    wide_r = torch.cat([cr2, torch.full((64, 24), -1, dtype=torch.int32, device=dev)], 1).contiguous()
    wide_s = torch.cat([cs2, torch.full((64, 24), float("-inf"), device=dev)], 1).contiguous()
    wide_r[:, 50] = 45                                                      # >= count
    wide_s[:, 50] = 9.0
    s3, r3 = ops.diverse_select(hf.memory_features, hf._inv_norm, count, wide_r, wide_s, 8, 0.5, None)
    s4, r4 = ops.diverse_select(hf.memory_features, hf._inv_norm, count, cr2, cs2, 8, 0.5, None)
    assert torch.equal(r3, r4) and torch.equal(s3.view(torch.int32), s4.view(torch.int32)) and bool((r3 < count).all())


# ------------------------------------------------------------------------------------- 6: reinforce
def test_reinforce_strengthens_exactly_the_returned_rows(dev, data, bank_off):
    hf, q = bank_off, data[3].to(dev)
    before = hf.memory_metadata.clone()
    try:
        s, r = hf.recall_batch(q, k=8, now=NOW, max_similarity=0.9, reinforce=0.1, reinforce_cap=2.0)
        after = hf.memory_metadata.cpu()
    finally:
        hf.memory_metadata.copy_(before)
    want = reinforce_reference(before.cpu(), N, r.cpu(), 0.1, 2.0)
    assert torch.equal(after, want)
    changed = torch.nonzero(after[:, 0] != before.cpu()[:, 0]).squeeze(1)
    assert torch.equal(changed, torch.unique(r[r >= 0]).cpu().long())
    s1, r1 = hf.recall_batch(q, k=8, now=NOW, max_similarity=0.9)            # the selection saw the old strengths
    assert torch.equal(r1, r) and torch.equal(s1, s)


# ------------------------------------------------------------------------------------- 7: small bank, public API
def test_small_fp32_bank_and_the_public_entry_points(dev, H):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    g = torch.Generator().manual_seed(5)
    base = torch.randn(400, 64, generator=g)
    feats = torch.cat([base[:100].repeat_interleave(5, 0) + 0.02 * torch.randn(500, 64, generator=g),
                       torch.randn(1500, 64, generator=g)])
    label = torch.cat([torch.arange(100).repeat_interleave(5), 100 + torch.arange(1500)])
    hf = H.HippocampalFormation(feature_dim=64, max_memories=4096, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                device="cuda", use_centroid_index=False)
    hf.create_episodic_memories([f"m{i}" for i in range(2000)], feats)
    q = (base[:32] + 0.1 * torch.randn(32, 64, generator=g)).to(dev)
    cs, cr = hf.recall_batch(q, k=32, now=NOW)
    s, r = hf.recall_batch(q, k=5, now=NOW, diversity=0.3, max_similarity=0.9)
    cos = R.cosines(hf.memory_features, hf._inv_norm, cr, 2000)
    R.replay_check(cr, cs, cos, 2000, 5, 0.3, 0.9, s, r, R.tolerance(64))
    assert bool((_distinct_groups(label, r) == 5).all())
    _, plain = hf.recall_batch(q, k=5, now=NOW)
    assert bool((_distinct_groups(label, plain) == 1).all())
    ids = hf.retrieve_similar_memories(q[3], None, 5, max_similarity=0.9)
    s3, r3 = hf.recall_batch(q[3:4], k=5, max_similarity=0.9)
    assert [i for i, _ in ids] == [f"m{int(x)}" for x in r3[0]] and len(ids) == 5
    assert hf.retrieve_similar_memories(q[3], None, 5) == hf.retrieve_similar_memories(q[3], k=5)
    mf, ms = MO.retrieve_memories(hf, q, k=5, diversity=0.3, max_similarity=0.9)
    s4, r4 = hf.recall_batch(q, k=5, diversity=0.3, max_similarity=0.9)
    assert mf.shape == (32, 5, 64) and ms.shape == (32, 5)
    assert torch.equal(mf, hf.memory_features[r4.long()]) and torch.equal(ms, s4)
    mf, ms = MO.retrieve_memories(hf, q, k=5, max_similarity=0.9, fetch_k=5)   # five copies fetched: one survives
    assert bool((ms[:, 0] != 0).all()) and bool((ms[:, 1:] == 0).all()) and bool((mf[:, 1:] == 0).all())


# ------------------------------------------------------------------------------------- 8: ABI
def test_abi_rejects_bad_arguments_without_launching(dev, data, bank_off):
    from aura_snn_rag_amd import _lib
    L = _lib.load()
    hf = bank_off
    nq, F, k = 4, 64, 8
    cs, cr = hf.recall_batch(data[3][:nq].to(dev), k=F, now=NOW)
    out_s = torch.full((nq, k), -7.0, device=dev)
    out_r = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(512, dtype=torch.uint8, device=dev)
    need = L.aura_diverse_select_workspace_bytes(nq, F, k)
    assert need >= 0
    assert L.aura_diverse_select_workspace_bytes(nq, 129, k) < 0 and L.aura_diverse_select_workspace_bytes(nq, F, 0) < 0
    assert L.aura_diverse_select_workspace_bytes(nq, F, F + 1) < 0 and L.aura_diverse_select_workspace_bytes(-1, F, k) < 0
    a = dict(bank=hf.memory_features.data_ptr(), inv=hf._inv_norm.data_ptr(), count=N, D=D, rows=cr.data_ptr(),
             scores=cs.data_ptr(), nq=nq, F=F, k=k, d=0.5, tau=0.9, os=out_s.data_ptr(), orr=out_r.data_ptr(),
             ws=ws.data_ptr(), wsb=need)

    def call(**kw):
        b = dict(a, **kw)
        return L.aura_diverse_select(b["bank"], b["inv"], b["count"], b["D"], b["rows"], b["scores"], b["nq"], b["F"],
                                     b["k"], b["d"], b["tau"], b["os"], b["orr"], b["ws"], b["wsb"], None)
    assert call(F=129) == -1 and call(k=F + 1) == -1 and call(k=0) == -1 and call(D=766) == -1 and call(D=4100) == -1
    assert call(D=0) == -1 and call(nq=-1) == -1 and call(count=-1) == -1
    for p in ("bank", "inv", "rows", "scores", "os", "orr"):
        assert call(**{p: None}) == -1, p
    assert call(wsb=need - 1) == -1
    assert call(d=-0.1) == -1 and call(d=1.1) == -1 and call(d=float("nan")) == -1 and call(tau=float("nan")) == -1
    assert call(bank=a["bank"] + 4) == -3
    torch.cuda.synchronize()
    assert bool((out_s == -7.0).all()) and bool((out_r == -7).all()) and not bool(ws.any())
    assert call() == 0
    torch.cuda.synchronize()
    cos = R.cosines(hf.memory_features, hf._inv_norm, cr, N)
    R.replay_check(cr, cs, cos, N, k, 0.5, 0.9, out_s, out_r, TOL)
    assert not bool(ws.any())
