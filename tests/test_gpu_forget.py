"""GPU tests of the bank compaction (``aura_bank_compact``) and of ``forget`` / ``consolidate`` above it.

The mover is compared with the same move in torch (gather everything, then store), bit for bit, on all six arrays.
``forget`` is compared with a fresh bank bulk-written from the survivors, ``consolidate`` with the replay bank that
consolidating writes build from the same rows in chunks of 1024: identical feature bits and ids, no exempted rows.

End-to-end data: that of tests/test_gpu_consolidate.py (seed 7): D = 768; 40 families; 12 groups per family; 6
near-copies per group; filled to 20 000 rows with randn; shuffled.  In fp64 the smallest cosine inside a group is 0.99807
and the largest between two groups 0.67464 (checked below), so at tau 0.9 and 0.95 no decision lies within
tol = 2 (D + 8) 2^-24 = 9.3e-5 of the threshold: the fp64 rule alone decides, 17 600 memories remain, one per group."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_consolidate as R
from tests.cpu_stub_forget import compact_reference

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
D, N, NQ = 768, 20_000, 600
TOL = R.tolerance(D)


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


def _hf(H, dim=D, M=N, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(feature_dim=dim, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                  device="cuda", **kw)


def _bulk(H, feats, index, M=None, **kw):
    hf = _hf(H, dim=feats.shape[1], M=M or feats.shape[0], use_centroid_index=index, **kw)
    hf.centroids_update_interval = 10 ** 9
    torch.manual_seed(1)
    hf.bulk_write(feats, rebuild=index)
    return hf


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------- the mover
ROWS = 6000
SHAPES = {"768-shadow": (768, 2, True), "100": (100, 3, False), "50-scalar": (50, 1, False)}


@pytest.fixture(scope="module")
def arrays(dev):
    out = {}
    for name, (dim, S, sh) in SHAPES.items():
        g = torch.Generator().manual_seed(dim)
        a = [torch.randn(ROWS, dim, generator=g), torch.randn(ROWS, S, generator=g), torch.randn(ROWS, 4, generator=g),
             torch.rand(ROWS, generator=g)]
        if sh:
            a += [torch.randn(ROWS, dim, generator=g).to(torch.bfloat16), torch.rand(ROWS, generator=g)]
        out[name] = [t.to(dev) for t in a]
    return out


def _patterns():
    from aura_snn_rag_amd import ops
    rr = ops.bank_compact_round_rows()
    assert 1000 < rr < ROWS - 1000
    g = np.random.default_rng(3)
    every = np.arange(ROWS)
    pats = {"nothing": (every, 0), "row0": (every[1:], 0), "last": (every[:-1], 0), "every-other": (every[1::2], 0),
            "even-rows": (every[::2], 0),
            "long-run": (np.concatenate([every[:100], every[100 + rr + 50:]]), 0),        # the direct case
            "random-30": (np.nonzero(g.random(ROWS) >= 0.3)[0], 0),
            "middle": (np.nonzero(g.random(ROWS) >= 0.5)[0][:1500] + 0, 0)}
    for n in (rr - 1, rr, rr + 1):
        pats[f"n={n}"] = (1 + np.arange(n), 0)                                            # staged rounds, n at a round
    pats["dst0"] = (6 + np.arange(rr + 1), 5)                                             # a move that starts inside the bank
    return pats


@pytest.mark.parametrize("shape", list(SHAPES))
def test_mover_equals_the_move_in_torch(dev, arrays, shape):
    from aura_snn_rag_amd import ops
    orig = arrays[shape]
    for name, (src, dst0) in _patterns().items():
        if shape == "50-scalar" and name not in ("row0", "random-30", "long-run", "last"):
            continue
        got = [t.clone() for t in orig]
        want = [t.clone() for t in orig]
        compact_reference(want, src, dst0)
        moved = ops.bank_compact(got[0], got[1], got[2], got[3], src, dst0, shadow=got[4] if len(got) > 4 else None,
                                 rho=got[5] if len(got) > 4 else None)
        assert moved == int((src != dst0 + np.arange(src.size)).sum()), name
        for a, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(_bits(x), _bits(y)), f"{shape} / {name}: array {a} differs"
        if name in ("nothing", "last"):
            assert moved == 0 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(got, orig))


def test_mover_staged_then_direct_rounds(dev):
    """More rows than 6000 only because the case needs them: a staged round (rows that shift by one), then -- behind a
    removed run longer than a round -- two direct rounds, the last one partial; D = 64 with the shadow."""
    from aura_snn_rag_amd import ops
    rr, rows = ops.bank_compact_round_rows(), 14_000
    g = torch.Generator().manual_seed(5)
    orig = [torch.randn(rows, 64, generator=g), torch.randn(rows, 2, generator=g), torch.randn(rows, 4, generator=g),
            torch.rand(rows, generator=g), torch.randn(rows, 64, generator=g).to(torch.bfloat16), torch.rand(rows, generator=g)]
    orig = [t.to(dev) for t in orig]
    src = np.concatenate([np.arange(1, 200), np.arange(200 + rr, rows)])
    assert src.size > 2 * rr and src[rr] > 2 * rr - 1
    got, want = [t.clone() for t in orig], [t.clone() for t in orig]
    compact_reference(want, src, 0)
    assert ops.bank_compact(got[0], got[1], got[2], got[3], src, 0, shadow=got[4], rho=got[5]) == src.size
    for a, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(_bits(x), _bits(y)), f"array {a} differs"


def test_mover_refuses_what_the_contract_excludes(dev, arrays):
    from aura_snn_rag_amd import ops
    a = [t.clone() for t in arrays["768-shadow"]]
    keep = [t.clone() for t in a]
    for src, dst0 in (([3, 2], 0), ([2, 2], 0), ([0, 1], 1), ([5, ROWS], 0), ([-1, 4], 0), (np.arange(10), ROWS - 5)):
        with pytest.raises(ValueError):
            ops.bank_compact(a[0], a[1], a[2], a[3], src, dst0, shadow=a[4], rho=a[5])
    with pytest.raises(ValueError):
        ops.bank_compact(a[0], a[1], a[2], a[3], [1], 0, shadow=a[4])
    with pytest.raises(ValueError):
        ops.bank_compact(a[0], a[1][:-1], a[2], a[3], [1], 0)
    assert ops.bank_compact(a[0], a[1], a[2], a[3], [], 0) == 0
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, keep))
    L = ops.lib()
    assert L.aura_bank_compact_workspace_bytes(768, 2, 1) == L.aura_bank_compact_workspace_bytes(768, 2, 1) > 0
    assert L.aura_bank_compact_workspace_bytes(100, 3, 1) < 0 and L.aura_bank_compact_workspace_bytes(0, 2, 0) < 0
    # the C entry point itself: shadow without rho, a move past the end, a workspace that is too small
    src = torch.arange(1, 9, dtype=torch.int32, device=dev)
    nb = L.aura_bank_compact_workspace_bytes(768, 2, 1)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    p = [t.data_ptr() for t in a]
    assert L.aura_bank_compact(p[0], p[1], p[2], p[3], p[4], None, ROWS, 768, 2, src.data_ptr(), 8, 0, base, nb, None) == -1
    assert L.aura_bank_compact(p[0], p[1], p[2], p[3], p[4], p[5], ROWS, 768, 2, src.data_ptr(), 8, ROWS - 7, base, nb, None) == -1
    assert L.aura_bank_compact(p[0], p[1], p[2], p[3], p[4], p[5], ROWS, 768, 2, src.data_ptr(), 8, 0, base, nb - 1, None) == -1
    assert L.aura_bank_compact(p[0], p[1], p[2], p[3], p[4], p[5], ROWS, 768, 2, src.data_ptr(), 8, 0, base + 16, nb, None) == -3
    assert L.aura_bank_compact(p[0], p[1], p[2], p[3], p[4], p[5], ROWS, 768, 2, src.data_ptr(), 0, 0, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, keep))


# ------------------------------------------------------------------------------------- forget
def _kill_set():
    g = torch.Generator().manual_seed(17)
    kill = torch.randperm(N, generator=g)[:3000]
    return torch.unique(torch.cat([kill, torch.tensor([0, 1, 8191, 8192, N - 1])]))


def test_forget_equals_a_fresh_bank_of_the_survivors(H, dev, data):
    feats, _, strength, q = data
    kill = _kill_set()
    alive = torch.ones(N, dtype=torch.bool)
    alive[kill] = False
    surv = alive.nonzero().flatten()
    hf = _bulk(H, feats, False)
    hf.memory_metadata[:N, 0] = strength.to(dev)
    hf.recall_batch(q.to(dev), k=8, now=NOW, use_candidates=False)                # (converts the bf16 shadow)
    assert hf._shadow is not None and hf._shadow_valid_upto == N
    rep = hf.forget(rows=torch.cat([kill, torch.tensor([-1, N, kill[0]])]).to(dev).reshape(1, -1))
    k = surv.numel()
    assert rep.n_removed == kill.numel() and hf.memory_count == k
    want = torch.full((N,), -1, dtype=torch.int64)
    want[surv] = torch.arange(k)
    assert np.array_equal(rep.old_to_new, want.numpy())
    assert hf._shadow_valid_upto == k and hf._norms_valid_upto == k, "the shadow travels with the rows"
    assert not bool(hf.memory_features[k:].any()) and not bool(hf.memory_metadata[k:].any())
    fresh = _bulk(H, feats[surv], False, M=N)
    fresh.memory_metadata[:k, 0] = strength[surv].to(dev)
    s0, r0 = fresh.recall_batch(q.to(dev), k=8, now=NOW, use_candidates=False)
    s1, r1 = hf.recall_batch(q.to(dev), k=8, now=NOW, use_candidates=False)
    assert torch.equal(r0, r1) and torch.equal(_bits(s0), _bits(s1))
    assert torch.equal(_bits(hf.memory_features[:k]), _bits(fresh.memory_features[:k]))
    assert torch.equal(_bits(hf._inv_norm[:k]), _bits(fresh._inv_norm[:k]))
    assert torch.equal(_bits(hf._shadow[:k]), _bits(fresh._shadow[:k])) and torch.equal(_bits(hf._rho[:k]), _bits(fresh._rho[:k]))
    ids = [hf.id_of_row(r) for r in r1[:50].flatten().tolist()]
    assert ids == [f"bulk-{int(surv[r])}" for r in r1[:50].flatten().tolist()]
    assert hf.id_of_row(0) == f"bulk-{int(surv[0])}" and hf.id_of_row(k - 1) == f"bulk-{int(surv[-1])}"
    assert len(hf._implicit_ids) == 1 and isinstance(hf._implicit_ids[0][3], np.ndarray)     # no string per row


def test_forget_with_the_index(H, dev, data):
    feats, _, _, q = data
    kill = _kill_set()
    gone = set(kill.tolist())
    hf = _bulk(H, feats, True)
    assert hf._candidate_mode()
    counts = hf.centroid_counts.clone()
    cids = hf.memory_metadata[:N, 2].clone()
    rep = hf.forget(rows=kill)
    k = hf.memory_count
    assert k == N - kill.numel()
    left = torch.bincount(cids[torch.from_numpy(rep.old_to_new >= 0).to(dev)].long(), minlength=256).float()
    assert torch.equal(hf.centroid_counts, left) and float(counts.sum()) == N
    torch.manual_seed(2)
    hf.rebuild_centroids()
    held = torch.from_numpy(np.nonzero(rep.old_to_new >= 0)[0])
    probe = torch.arange(0, k, 97)
    queries = torch.cat([q, feats[held[probe]]]).to(dev)
    _, rows = hf.recall_batch(queries, k=8, now=NOW)
    assert hf._candidate_mode() and bool((rows >= 0).all())
    origin = held[rows.cpu().long()]
    assert not (set(origin.flatten().tolist()) & gone), "a forgotten memory was recalled"
    assert torch.equal(rows[NQ:, 0].cpu().long(), probe), "a held row is not its own best match"
    assert hf.id_of_row(int(rows[0, 0])) == f"bulk-{int(origin[0, 0])}"


# ------------------------------------------------------------------------------------- consolidate
def test_the_data_leaves_no_decision_near_a_threshold(dev, data):
    """fp64 cosines of every pair (on the device, in chunks): the smallest inside a group, the largest across."""
    feats, label, _, _ = data
    f = feats.to(dev).double()
    f = f / f.norm(dim=1, keepdim=True)
    lab = label.to(dev)
    lo_in, hi_out = 1.0, -1.0
    for a in range(0, N, 2500):
        c = f[a:a + 2500] @ f.t()
        same = lab[a:a + 2500, None] == lab[None, :]
        lo_in = min(lo_in, float(c[same].min()))
        hi_out = max(hi_out, float(c.masked_fill(same, -1.0).max()))
    print(f"smallest cosine inside a group {lo_in:.5f}, largest across groups {hi_out:.5f}, tol {TOL:.2e}")
    assert abs(lo_in - 0.99807) < 5e-5 and abs(hi_out - 0.67464) < 5e-5
    assert lo_in > 0.95 + TOL and hi_out < 0.9 - TOL


_REPLAY = {}


def _replay(H, feats, tau, ids, M=None):
    """The bank consolidating writes leave (chunks of ops.CONSOLIDATE_MAX_BATCH = 1024), built once per case."""
    key = (tau, feats.shape, M)
    if key not in _REPLAY:
        hf = _hf(H, dim=feats.shape[1], M=M or feats.shape[0])
        hf.create_episodic_memories(ids, feats.cuda(), merge_similarity=tau)
        _REPLAY[key] = (hf.memory_count, hf.memory_features[:hf.memory_count].clone(),
                        [hf.id_of_row(r) for r in range(hf.memory_count)])
    return _REPLAY[key]


@pytest.mark.parametrize("index", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("tau", [0.9, 0.95])
def test_consolidate_equals_the_replay(H, dev, data, tau, index):
    from aura_snn_rag_amd import ops
    assert ops.CONSOLIDATE_MAX_BATCH == 1024
    feats, label, _, q = data
    hf = _bulk(H, feats, index)
    torch.manual_seed(4)
    rep = hf.consolidate(tau)
    assert (rep.n_before, rep.n_kept, rep.n_merged) == (N, 17_600, 2400) and hf.memory_count == 17_600
    count, want_f, want_ids = _replay(H, feats, tau, [f"bulk-{i}" for i in range(N)])
    assert count == 17_600
    assert torch.equal(_bits(hf.memory_features[:count]), _bits(want_f)), "feature bits differ from the replay bank"
    ids = [hf.id_of_row(r) for r in range(count)]
    assert ids == want_ids
    assert not bool(hf.memory_features[count:].any()) and not bool(hf.memory_metadata[count:].any())
    # one memory per label, each the first row of its group
    origin = torch.tensor([int(i[5:]) for i in ids])
    held = label[origin]
    first = torch.full((int(label.max()) + 1,), N, dtype=torch.int64).scatter_reduce(0, label, torch.arange(N), "amin")
    assert len(set(held.tolist())) == 17_600 and torch.equal(first[held], origin)
    # every row's new place: its own if kept, else that of the first row of its group
    new_of_origin = torch.full((N,), -1, dtype=torch.int64)
    new_of_origin[origin] = torch.arange(count)
    assert np.array_equal(rep.old_to_new, new_of_origin[first[label]].numpy())
    assert hf._candidate_mode() == index and (not index or not hf._unlisted_rows)
    _, rows = hf.recall_batch(q.to(dev), k=8, now=NOW)
    groups = held[rows.cpu().long()]
    assert bool((rows >= 0).all()) and all(len(set(gq.tolist())) == 8 for gq in groups)


def test_consolidate_dense_path(H, dev):
    g = torch.Generator().manual_seed(23)
    base = torch.randn(50, 100, generator=g)
    rows = torch.cat([base.repeat_interleave(4, 0) + 0.05 * torch.randn(200, 100, generator=g),
                      torch.randn(2800, 100, generator=g)])
    label = torch.cat([torch.arange(50).repeat_interleave(4), 50 + torch.arange(2800)])
    perm = torch.randperm(3000, generator=g)
    rows, label = rows[perm].contiguous(), label[perm]
    hf = _bulk(H, rows, False)
    rep = hf.consolidate(0.9)
    assert hf._shadow is None and rep.n_kept == 2850 and rep.n_merged == 150
    count, want_f, want_ids = _replay(H, rows, 0.9, [f"bulk-{i}" for i in range(3000)])
    assert count == 2850 and torch.equal(_bits(hf.memory_features[:count]), _bits(want_f))
    assert [hf.id_of_row(r) for r in range(count)] == want_ids
    origin = torch.tensor([int(i[5:]) for i in want_ids])
    assert len(set(label[origin].tolist())) == 2850


def test_consolidate_a_wrapped_fifo_ring(H, dev, data):
    feats = data[0][:14_000]
    M = 10_000
    hf = _hf(H, M=M, overflow="fifo")
    ids = [f"r{i}" for i in range(14_000)]
    for lo in range(0, 14_000, 2000):
        hf.create_episodic_memories(ids[lo:lo + 2000], feats[lo:lo + 2000].to(dev))
    assert hf.memory_count == M and hf._write_cursor % M == 4000
    rep = hf.consolidate(0.9)
    count, want_f, want_ids = _replay(H, feats[4000:], 0.9, ids[4000:], M=M)
    assert rep.n_before == M and rep.n_kept == count == hf.memory_count and count < M
    assert torch.equal(_bits(hf.memory_features[:count]), _bits(want_f))
    assert [hf.id_of_row(r) for r in range(count)] == want_ids and hf._write_cursor == 0
    # the oldest held row (r4000, at row 4000 of the ring) is row 0 now; rows map through the rotation
    assert hf.id_of_row(0) == "r4000" and rep.old_to_new[4000] == 0
    place = {mid: r for r, mid in enumerate(want_ids)}
    was = [f"r{r + 10_000}" if r < 4000 else f"r{r}" for r in range(M)]          # what the ring held, by row
    assert all(rep.old_to_new[r] == place[mid] for r, mid in enumerate(was) if mid in place)
    assert sum(mid in place for mid in was) == count and bool((rep.old_to_new >= 0).all())
    hf.create_episodic_memories(["next"], torch.randn(1, D).to(dev))
    assert hf.id_of_row(count) == "next" and hf.memory_count == count + 1
