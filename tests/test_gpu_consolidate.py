"""GPU tests of consolidating writes (``aura_bank_find_repeats``, ``aura_bank_touch`` and everything above them)
against the rule restated in torch fp64 on the CPU (tests/cpu_stub_consolidate.py).

Tolerance: a device cosine differs from the exact one by at most (D + 8) 2^-24 for unit rows; two are compared:
tol = 2 (D + 8) 2^-24 = 9.3e-5 at D = 768.  A row is UNDECIDED when its best cosine lies within tol of tau or its best
two targets within tol of each other; everywhere the replay check holds for every row, decided rows equal the fp64
rule exactly, and on the mixed batches at most 1 % of the rows may be undecided.

End-to-end data: that of tests/test_gpu_diverse.py (seed 7): D = 768; 40 families; 12 groups per family (family + 0.8
randn); 6 near-copies per group (group + 0.05 randn); filled to 20 000 rows with randn; shuffled.  Cosines are about
0.998 inside a group and about 0.61 between the groups of a family, so at tau 0.9 and 0.95 the fp64 rule leaves NO row
undecided and keeps one row per group: 17 600 memories, 2400 merges."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_consolidate as R

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
NOW32 = float(np.float32(NOW))
D, N, NQ = 768, 20_000, 600
TOL = R.tolerance(D)
INF = float("inf")


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


def _mixed_batch(bank, n, seed, copies_of=None):
    """n rows around the threshold: bank rows + s randn for a spread of s (cosines from 1 down to ~0.7), exact copies,
    fresh rows, in-batch near-copies of earlier rows, and the degenerate rows."""
    g = torch.Generator().manual_seed(seed)
    Dm = bank.shape[1]
    src = torch.randint(0, bank.shape[0], (n,), generator=g) if copies_of is None else copies_of
    s = torch.rand(n, 1, generator=g) * 1.0
    rows = bank[src] + s * bank[src].norm(dim=1, keepdim=True) / Dm ** 0.5 * torch.randn(n, Dm, generator=g)
    rows[::7] = bank[src[::7]] * 1.25                                   # exact directions
    rows[3::11] = torch.randn(len(rows[3::11]), Dm, generator=g)        # fresh
    for i in range(20, n, 9):                                           # in-batch near-copies at several distances
        rows[i] = rows[i - 13] + 0.3 * float(torch.rand(1, generator=g)) * torch.randn(Dm, generator=g)
    rows[5] = 0.0
    rows[6, 1] = float("nan")
    rows[8, 0] = float("inf")
    rows[50] = 0.0
    return rows.contiguous()


def _check_against_the_rule(hf, batch, tau, tol, max_undecided=None):
    """find_repeats on the device vs the fp64 rule: the replay check for every row, exact equality for the decided
    rows; returns (device results, number of undecided rows)."""
    st, bl, cs_dev = hf.find_repeats(batch.to(hf.device), tau, now=NOW)
    assert st.dtype == torch.int32 and bl.dtype == torch.int32 and cs_dev.dtype == torch.float32 and not st.is_cuda
    cs, cb = R.cosines(hf.memory_features, hf._inv_norm, hf.memory_count, batch)
    bad = R.degenerate(batch)
    R.replay_check(cs, cb, tau, tol, st, bl, cs_dev, bad=bad)
    rs, rl, rc = R.rule(cs, cb, tau)
    und = R.undecided(cs, cb, tau, tol)
    # an undecided row can change what LATER rows see (it is or is not kept), but only rows that could repeat it: a
    # row is TAINTED when it is undecided or has an earlier tainted row within tol of the threshold or above it.
    # Every other row must equal the fp64 rule exactly.
    near = (cb >= tau - tol).tolist()
    taint = und.clone()
    for i in range(len(batch)):
        if not taint[i] and any(near[i][j] for j in taint[:i].nonzero().flatten().tolist()):
            taint[i] = True
    ok = (st.long() == rs) & (bl.long() == rl)
    stored_ok = (st.long() == rs) | und
    print(f"n={len(batch)} N={hf.memory_count} D={batch.shape[1]} tau={tau}: {int(und.sum())} undecided, "
          f"{int((rs >= 0).sum())} stored repeats, {int((rl >= 0).sum())} in-batch repeats, {int((~ok).sum())} rows differ")
    assert bool(stored_ok.all()), "a decided row's stored target differs from the fp64 rule"
    assert bool(ok[~taint].all()), "a decided row differs from the fp64 rule"
    if max_undecided is not None:
        assert int(und.sum()) <= max_undecided
    return (st, bl, cs_dev), int(und.sum())


# ------------------------------------------------------------------------------------- the scan paths
@pytest.mark.parametrize("dim", [768, 100])
def test_small_bank_dense_scan(H, dev, dim):
    g = torch.Generator().manual_seed(21)
    bank = torch.randn(3000, dim, generator=g)
    hf = _bulk(H, bank, False)
    assert hf._ensure_shadow() is None                                 # below SHADOW_MIN_ROWS: no image
    tol = R.tolerance(dim)
    total = und = 0
    for n, seed in ((256, 1), (1000, 2), (1, 3), (33, 4)):
        batch = _mixed_batch(bank, max(n, 64), seed)[:n] if n < 64 else _mixed_batch(bank, n, seed)
        for tau in (0.9, 0.95):
            _, u = _check_against_the_rule(hf, batch, tau, tol)
            total, und = total + n, und + u
    assert und <= 0.01 * total, f"{und} of {total} rows undecided"
    assert hf._shadow is None and hf._ivf is None and hf.memory_count == 3000


@pytest.fixture(scope="module")
def bank_off(H, dev, data):
    return _bulk(H, data[0], False)


@pytest.fixture(scope="module")
def bank_on(H, dev, data):
    return _bulk(H, data[0], True)


@pytest.mark.parametrize("index", [False, True], ids=["row_shadow", "sorted_image"])
def test_large_bank_image_scan(H, dev, data, bank_off, bank_on, index):
    hf = bank_on if index else bank_off
    feats = data[0]
    total = und = 0
    for n, seed in ((256, 5), (1024, 6), (64, 7)):
        batch = _mixed_batch(feats, n, seed)
        for tau in (0.9, 0.95):
            _, u = _check_against_the_rule(hf, batch, tau, TOL)
            total, und = total + n, und + u
    assert und <= 0.01 * total, f"{und} of {total} rows undecided"
    if index:
        assert hf._candidate_mode() and hf._ivf is not None and hf._ivf.valid and not hf._unlisted_rows
    else:
        assert hf._shadow is not None and hf._ivf is None


def test_sorted_image_with_holes_and_appends(H, dev, data):
    feats, label = data[0], data[1]
    g = torch.Generator().manual_seed(31)
    hf = _bulk(H, feats[:19_000], True, M=19_500, overflow="fifo")
    hf.find_repeats(feats[:8].to(dev), 0.9)                            # packs the lists
    st0 = hf._ivf
    assert st0 is not None and st0.valid and st0.appended == 0
    new = torch.randn(900, D, generator=g)
    hf.create_episodic_memories([f"x{i}" for i in range(900)], new)    # 500 appends, then 400 overwrite slots 0..399
    assert hf.memory_count == 19_500 and hf._ivf is st0 and st0.valid and st0.appended == 900
    holes = int((st0.sorted_rows[:st0.n_sorted] < 0).sum())
    # copies of: overwritten rows (gone: they must find nothing), the rows that replaced them, appended rows,
    # untouched rows.  The overwritten rows are taken among the filler rows: an overwritten member of a group of
    # near-copies leaves five siblings whose cosines to it lie within tol of each other by construction (about
    # 0.9975 +- 5e-5), which the rule cannot decide
    gone = feats[:400][label[:400] >= 480][:100]
    assert gone.shape[0] == 100
    src = torch.cat([gone, new[500:600], new[:100], feats[5000:5100]])
    batch = src * 0.5 + 1e-3 * torch.randn(400, D, generator=g)
    (st, bl, _), u = _check_against_the_rule(hf, batch, 0.95, TOL, max_undecided=4)
    assert hf._ivf is st0 and st0.valid, "the lists were re-packed: the holes were not scanned"
    assert bool((st[:100] == -1).all()), "an overwritten row was found"
    assert holes > 0 and st[100:200].tolist() == list(range(0, 100)) and st[200:300].tolist() == list(range(19_000, 19_100))
    assert st[300:400].tolist() == list(range(5000, 5100))
    # a row the lists DROPPED (a list without a free entry) must not become a missed duplicate: the flag is read
    # with the results, the lists are re-packed and the call repeated
    st0.flag.fill_(1)
    (st2, _, _), _ = _check_against_the_rule(hf, batch, 0.95, TOL, max_undecided=4)
    assert torch.equal(st2, st) and hf._ivf.valid and hf._ivf.appended == 0 and int(hf._ivf.flag) == 0
    # rows without a list (a positioned write): the row-ordered shadow takes over
    hf.write_at(["w"], torch.randn(1, D, generator=g), np.array([7], dtype=np.int64), 0, NOW)
    assert hf._unlisted_rows
    _check_against_the_rule(hf, batch, 0.95, TOL, max_undecided=4)
    assert hf._shadow is not None


def test_overflowing_survivor_lists_fall_back(H, dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(41)
    base = torch.randn(D, generator=g)
    bank = torch.randn(10_000, D, generator=g)
    where = torch.randperm(10_000, generator=g)[:4000]
    bank[where] = base + 0.05 * torch.randn(4000, D, generator=g)
    hf = _bulk(H, bank, False)
    batch = (base[None, :] * torch.linspace(0.5, 2.0, 64)[:, None]).contiguous()
    shadow = hf._ensure_shadow()
    assert shadow is not None
    packed = ops.find_repeats(hf.memory_features, hf._inv_norm, hf.memory_count, batch.to(dev), 0.9, image=shadow,
                              rho=hf._rho)[3].cpu()
    assert int(packed[3 * 64]) != 0, "4000 survivors per row fit no list of 256: the flag must be raised"
    st, bl, cs_dev = hf.find_repeats(batch.to(dev), 0.9)
    cs, cb = R.cosines(hf.memory_features, hf._inv_norm, hf.memory_count, batch)
    R.replay_check(cs, cb, 0.9, TOL, st, bl, cs_dev)                   # (best two targets within tol by construction)
    assert bool((st >= 0).all()) and bool(torch.isin(st.long(), where).all())
    # without near-copies the same bank does not overflow
    packed = ops.find_repeats(hf.memory_features, hf._inv_norm, hf.memory_count, torch.randn(64, D, generator=g).to(dev),
                              0.9, image=shadow, rho=hf._rho)[3].cpu()
    assert int(packed[3 * 64]) == 0 and bool((packed[:64] == -1).all())


@pytest.mark.parametrize("mode", ["dense", "row_shadow", "sorted_image"])
def test_exact_duplicates_report_the_lowest_row(H, dev, mode):
    g = torch.Generator().manual_seed(51)
    bank = torch.randn(9000, 64, generator=g)
    dup = {17: [17, 4000, 8999], 300: [300, 301, 7000], 8500: [8500, 8998]}
    for first, rows in dup.items():
        bank[rows] = bank[first].clone()
    hf = _bulk(H, bank, mode == "sorted_image", bf16_shadow=mode != "dense")
    batch = torch.cat([bank[[8999, 7000, 8998, 4000, 301]] * 3.0, bank[[17]] + 1e-4 * torch.randn(1, 64, generator=g)])
    st, bl, cs = hf.find_repeats(batch.to(dev), 0.99)
    assert st.tolist() == [17, 300, 8500, 17, 300, 17] and bl.tolist() == [-1] * 6
    assert bool((cs[:5] - 1.0).abs().max() <= R.tolerance(64))
    assert (hf._shadow is not None) == (mode == "row_shadow") and (hf._ivf is not None) == (mode == "sorted_image")


def test_touch(H, dev):
    from aura_snn_rag_amd import ops
    hf = _bulk(H, torch.randn(500, 64), False, M=600)
    meta = hf.memory_metadata.clone()
    rows = torch.tensor([3, 3, -1, 499, 500, 10_000, 0], dtype=torch.int32, device=dev)
    ops.bank_touch(hf.memory_metadata, hf.memory_count, rows, NOW + 4096.0)
    want = meta.clone()
    want[[0, 3, 499], 1] = float(np.float32(NOW + 4096.0))
    assert torch.equal(hf.memory_metadata, want)
    hf.touch(torch.tensor([[1, 2]]), now=NOW + 8192.0)
    want[[1, 2], 1] = float(np.float32(NOW + 8192.0))
    assert torch.equal(hf.memory_metadata, want) and hf._slot_time[2] == NOW + 8192.0


# ------------------------------------------------------------------------------------- end to end
def _stream(hf, feats, label, batch, tau, dev):
    """Write ``feats`` in batches with the option on; every batch's find_repeats is compared with the fp64 rule on a
    CPU mirror of the bank (which holds the kept rows in slot order: nothing overflows).  Returns the reports."""
    n = feats.shape[0]
    mirror = torch.zeros(n, feats.shape[1], dtype=torch.float64)      # normalised held rows, fp64
    reports, count = [], 0
    seen = []
    real = hf.find_repeats

    def spy(f, threshold, now=None):
        out = real(f, threshold, now=now)
        seen.append(out)
        return out
    hf.find_repeats = spy
    try:
        for lo in range(0, n, batch):
            f = feats[lo:lo + batch]
            fn = f.double() / f.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
            cs, cb = fn @ mirror[:count].t(), fn @ fn.t()
            rs, rl, rc = R.rule(cs, cb, tau)
            assert not bool(R.undecided(cs, cb, tau, TOL).any()), "the reference data leaves no row undecided"
            rep = hf.create_episodic_memories([f"r{i}" for i in range(lo, lo + len(f))], f.to(dev), merge_similarity=tau)
            st, bl, cd = seen.pop()
            assert not seen
            assert torch.equal(st.long(), rs) and torch.equal(bl.long(), rl), f"batch at {lo}: not the fp64 rule"
            fin = rc > -INF
            assert bool(((cd.double() - rc)[fin].abs() <= TOL).all()) and bool((cd[~fin] == -INF).all())
            kept = (rs < 0) & (rl < 0)
            k = int(kept.sum())
            assert rep.n_stored == k and hf.memory_count == count + k
            inv = hf._inv_norm[count:count + k].cpu().double()
            mirror[count:count + k] = f[kept].double() * inv[:, None]
            count += k
            reports.append((lo, rep))
    finally:
        del hf.find_repeats
    return reports


@pytest.mark.parametrize("index,batch,tau", [(False, 64, 0.9), (True, 64, 0.9), (True, 1000, 0.95), (False, 1000, 0.95)],
                         ids=["off-64-0.9", "on-64-0.9", "on-1000-0.95", "off-1000-0.95"])
def test_a_consolidated_stream_keeps_one_memory_per_group(H, dev, data, index, batch, tau):
    feats, label, _, q = data
    hf = _hf(H, use_centroid_index=index)
    torch.manual_seed(3)
    reports = _stream(hf, feats, label, batch, tau, dev)
    assert hf.memory_count == 17_600 and sum(r.n_merged for _, r in reports) == 2400
    origin = torch.tensor([int(hf.id_of_row(r)[1:]) for r in range(hf.memory_count)])        # slot -> stream index
    held = label[origin]
    assert len(set(held.tolist())) == 17_600, "two members of one group are held"
    for lo, rep in reports:
        m = rep.merged.nonzero().flatten()
        if len(m):
            tgt = torch.tensor([int(rep.ids[i][1:]) for i in m.tolist()])
            assert torch.equal(label[tgt], label[lo + m]), "a merge landed in another group"
            assert torch.equal(origin[rep.rows[m]], tgt)              # the slot that holds the memory the row became
            assert bool((label[lo + m] < 480).all())
    if index:
        assert hf._index_ready and hf._candidate_mode()
    # a plain top-8 recall now returns 8 distinct groups for every query (597 of 600 repeat a group otherwise)
    _, rows = hf.recall_batch(q.to(dev), k=8, now=NOW)
    groups = held[rows.cpu().long()]
    assert bool((rows >= 0).all()) and all(len(set(gq.tolist())) == 8 for gq in groups)


def test_without_the_option_the_stream_is_stored_as_today(H, dev, data):
    """The same 20 000-row stream in batches of 64, index on, without the option -- on a bank built without a
    threshold and on one built with it but switched off per call: every row is stored, in order, both banks equal bit
    for bit.  (That the write receives today's arguments is checked on the host: test_host_consolidate.py.)"""
    feats = data[0]
    ids = [f"r{i}" for i in range(N)]
    banks = []
    for kw, call in ((dict(), dict()), (dict(merge_similarity=0.9), dict(merge_similarity=None))):
        hf = _hf(H, use_centroid_index=True, **kw)
        torch.manual_seed(9)
        for lo in range(0, N, 64):
            assert hf.create_episodic_memories(ids[lo:lo + 64], feats[lo:lo + 64].to(dev), **call) is None
        banks.append(hf)
    a, b = banks
    assert a.memory_count == b.memory_count == N and a.id_to_idx == b.id_to_idx
    for name in ("memory_features", "memory_metadata", "centroids", "centroid_counts", "_inv_norm"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.memory_features.cpu(), feats)                  # every row of the stream was stored, in order
    assert [a.id_of_row(r) for r in (0, 63, 64, N - 1)] == ["r0", "r63", "r64", f"r{N - 1}"]


# ------------------------------------------------------------------------------------- retention
def test_a_repeated_memory_survives_the_eviction(H, dev):
    g = torch.Generator().manual_seed(61)
    base = torch.randn(512, 64, generator=g)
    new = torch.randn(15, 64, generator=g)
    batch = torch.cat([new[:7], base[100:101] * 2.0, new[7:]]).to(dev)
    out = {}
    for tau in (None, 0.95):
        hf = _hf(H, dim=64, M=512, overflow="weakest", merge_similarity=tau, merge_reinforce=0.25)
        hf.create_episodic_memories([f"m{i}" for i in range(512)], base.to(dev))
        hf.decay_memories(0.5)
        hf.memory_metadata[:, 1] = NOW32 - 7200.0
        hf.memory_metadata[100, 0] = 0.01                              # the oldest-looking, weakest memory
        rep = hf.create_episodic_memories([f"n{i}" for i in range(16)], batch)
        out[tau] = (hf, rep)
    hf, rep = out[None]
    assert rep is None and hf.id_of_row(100) == "n0" and "m100" not in [hf.id_of_row(r) for r in range(512)]
    hf, rep = out[0.95]
    assert hf.id_of_row(100) == "m100" and rep.merged.tolist() == [False] * 7 + [True] + [False] * 8
    assert rep.rows[7].item() == 100 and rep.ids[7] == "m100" and (rep.n_stored, rep.n_merged) == (15, 1)
    assert hf.memory_metadata[100, 0].item() == float(np.float32(0.01) + np.float32(0.25))
    assert hf.memory_metadata[100, 1].item() == NOW32 and hf.memory_count == 512
    assert torch.equal(hf.memory_features[100].cpu(), base[100])       # the first observation stands
    assert sorted(hf.id_of_row(int(r)) for r in rep.rows[~rep.merged]) == sorted(f"n{i}" for i in range(16) if i != 7)
