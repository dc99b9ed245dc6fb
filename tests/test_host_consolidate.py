"""Host-side logic of consolidating writes on the CPU (``ops`` replaced by tests/cpu_stub_consolidate.py, which
restates the rule in torch fp64): the rule on hand-made rows, that a call without the option launches nothing new and
writes with today's arguments, the argument errors, the chunking at 1024 rows, the order reinforce -> touch -> write,
the id maps, the report under the three overflow policies, and a rebuild boundary inside a chunk."""
import inspect

import numpy as np
import pytest
import torch

from tests import cpu_stub_consolidate as stub

NOW = 1.7e9 + 5.0


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    stub.FIND_SIZES.clear()
    return H


def _hf(H, D=16, M=64, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _ids(a, b, p="m"):
    return [f"{p}{i}" for i in range(a, b)]


def _unit(*v):
    return torch.tensor(v, dtype=torch.float32)


def _record(monkeypatch, *names):
    """Wrap stub ops so that their calls are logged in order: [(name, args, kwargs), ...]."""
    log = []
    for name in names:
        real = getattr(stub, name)

        def wrapped(*a, _real=real, _name=name, **kw):
            log.append((_name, a, kw))
            return _real(*a, **kw)
        monkeypatch.setattr(stub, name, wrapped)
    return log


def test_the_rule_on_hand_made_rows():
    e = torch.eye(6)
    bank = torch.stack([e[0], e[1], e[1].clone(), 2.0 * e[2]])          # rows 1 and 2 are bit-identical
    inv = 1.0 / bank.norm(dim=1)
    feats = torch.stack([
        e[0] + 0.01 * e[5],                  # 0: repeats stored row 0
        e[3],                                # 1: new, kept
        e[3] + 0.02 * e[4],                  # 2: repeats row 1 of the batch
        e[3] + 0.04 * e[4],                  # 3: repeats the LEADER (row 1), never the repeat (row 2) it is closer to
        torch.zeros(6),                      # 4: norm 0: kept
        _unit(1, float("nan"), 0, 0, 0, 0),  # 5: NaN: kept
        e[1],                                # 6: exact copies: the lowest row
        e[0] + 0.01 * e[5],                  # 7: a copy of row 0 of the batch, which is not kept: the stored row
        _unit(float("inf"), 0, 0, 0, 0, 0),  # 8: Inf: kept
        torch.zeros(6),                      # 9: a second zero row does not repeat the first
        e[4] + e[5],                         # 10: new, kept
    ])
    st, bl, cs = stub.find_repeats_reference(bank, inv, 4, feats, 0.99)
    assert st.tolist() == [0, -1, -1, -1, -1, -1, 1, 0, -1, -1, -1]
    assert bl.tolist() == [-1, -1, 1, 1, -1, -1, -1, -1, -1, -1, -1]
    assert cs[[1, 4, 5, 8, 9, 10]].tolist() == [float("-inf")] * 6
    assert abs(float(cs[6]) - 1.0) < 1e-6 and 0.99 < float(cs[3]) < float(cs[2]) < 1.0
    # the threshold is inclusive and in-batch ties go to the lowest kept row
    f2 = torch.stack([e[0], e[1], (e[0] + e[1])])
    st, bl, cs = stub.find_repeats_reference(bank[:0], inv[:0], 0, f2, 0.5 ** 0.5 - 1e-9)
    assert st.tolist() == [-1, -1, -1] and bl.tolist() == [-1, -1, 0]
    # a degenerate BANK row is nobody's target
    bank2 = torch.stack([torch.zeros(6), _unit(float("nan"), 1, 0, 0, 0, 0), e[2]])
    inv2 = 1.0 / bank2.norm(dim=1).clamp_min(1e-12)
    st, _, _ = stub.find_repeats_reference(bank2, inv2, 3, torch.stack([e[2], torch.zeros(6), e[1]]), 0.9)
    assert st.tolist() == [2, -1, -1]
    stub.replay_check(*stub.cosines(bank, inv, 4, feats), 0.99, stub.tolerance(6), *
                      stub.find_repeats_reference(bank, inv, 4, feats, 0.99), bad=stub.degenerate(feats))


def test_without_the_option_nothing_changes(hmod, monkeypatch):
    log = _record(monkeypatch, "bank_write", "find_repeats", "bank_touch", "bank_reinforce")
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(40, 16, generator=g)
    plain, thr = _hf(hmod), _hf(hmod, merge_similarity=0.999)
    assert plain.merge_similarity is None and (plain.merge_reinforce, plain.merge_cap) == (0.1, 1.0)
    assert (thr.merge_similarity, thr.merge_reinforce, thr.merge_cap) == (0.999, 0.1, 1.0)
    assert plain.create_episodic_memories(_ids(0, 30), feats[:30]) is None
    assert plain.create_episodic_memory("m30", "e", feats[30]) is None
    assert [c[0] for c in log] == ["bank_write", "bank_write"]
    assert stub.CALLS["find_repeats"] == stub.CALLS["touch"] == stub.CALLS["reinforce"] == 0
    # today's arguments: eight positional tensors / numbers and the four keywords of the write path
    assert all(len(a) == 8 and set(kw) == {"centroids", "centroid_counts", "eff_k", "distinct_slots"}
               for _, a, kw in log)
    n_plain = len(log)
    # a bank built with a threshold writes distinct rows with exactly the same arguments ...
    rep = thr.create_episodic_memories(_ids(0, 30), feats[:30])
    thr.create_episodic_memory("m30", "e", feats[30])
    writes = [c for c in log[n_plain:] if c[0] == "bank_write"]
    assert len(writes) == 2 and rep.n_merged == 0 and rep.n_stored == 30
    for (_, a0, k0), (_, a1, k1) in zip(log[:n_plain], writes):
        assert all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a0[4:], a1[4:]))
        assert k0 == k1
    assert torch.equal(plain.memory_features, thr.memory_features) and torch.equal(plain.memory_metadata, thr.memory_metadata)
    # ... and None switches it off per call
    before = stub.CALLS["find_repeats"]
    assert thr.create_episodic_memories(["x"], feats[:1], merge_similarity=None) is None
    assert stub.CALLS["find_repeats"] == before and thr.memory_count == 32
    # signatures: the new arguments are keyword defaults behind the reference's
    p = inspect.signature(hmod.HippocampalFormation.create_episodic_memory).parameters
    assert list(p)[:5] == ["self", "memory_id", "event_id", "features", "associated_experts"]
    p = inspect.signature(hmod.HippocampalFormation.__init__).parameters
    assert p["merge_similarity"].default is None and p["merge_reinforce"].default == 0.1 and p["merge_cap"].default == 1.0


def test_argument_errors(hmod):
    for kw in (dict(merge_similarity=0.0), dict(merge_similarity=-0.5), dict(merge_similarity=1.01),
               dict(merge_similarity=float("nan")), dict(merge_similarity=0.9, merge_reinforce=-0.1),
               dict(merge_similarity=0.9, merge_reinforce=float("nan")), dict(merge_cap=float("nan"))):
        with pytest.raises(ValueError):
            _hf(hmod, **kw)
    hf = _hf(hmod)
    hf.create_episodic_memories(_ids(0, 5), torch.randn(5, 16))
    before = dict(stub.CALLS)
    for tau in (0.0, -1.0, 1.5, float("nan"), "high"):
        with pytest.raises(ValueError):
            hf.create_episodic_memories(["a"], torch.randn(1, 16), merge_similarity=tau)
        with pytest.raises(ValueError):
            hf.find_repeats(torch.randn(1, 16), tau)
    with pytest.raises(ValueError):
        hf.find_repeats(torch.randn(1, 16), None)
    with pytest.raises(ValueError):
        hf.find_repeats(torch.randn(stub.CONSOLIDATE_MAX_BATCH + 1, 16), 0.9)
    hf.merge_reinforce = -1.0                                        # the attributes are checked per call too
    with pytest.raises(ValueError):
        hf.create_episodic_memories(["a"], torch.randn(1, 16), merge_similarity=0.9)
    hf.merge_reinforce = 0.1
    with pytest.raises(ValueError):
        hf.create_episodic_memories(["a", "b"], torch.randn(1, 16), merge_similarity=0.9)
    assert stub.CALLS == before and hf.memory_count == 5            # refused before anything ran
    rep = hf.create_episodic_memories([], torch.zeros(0, 16), merge_similarity=1.0)
    assert rep.n_stored == rep.n_merged == 0 and rep.ids == [] and rep.rows.numel() == 0


def test_chunks_of_1024_see_the_earlier_chunks_rows_as_stored(hmod):
    g = torch.Generator().manual_seed(2)
    base = torch.randn(1100, 16, generator=g)
    feats = torch.cat([base, base[:300] + 1e-4 * torch.randn(300, 16, generator=g)])     # rows 1100.. repeat rows 0..299
    hf = _hf(hmod, M=4096)
    rep = hf.create_episodic_memories(_ids(0, 1400), feats, merge_similarity=0.999)
    assert stub.FIND_SIZES == [1024, 376] and stub.CALLS["find_repeats"] == 2
    assert rep.n_stored == 1100 and rep.n_merged == 300 and hf.memory_count == 1100
    assert not bool(rep.merged[:1100].any()) and bool(rep.merged[1100:].all())
    # rows 0..299 were written by the FIRST chunk: the second chunk finds them in the bank (stored targets)
    assert rep.rows[1100:].tolist() == list(range(300)) and rep.ids[1100:] == _ids(0, 300)
    assert rep.rows[:1100].tolist() == list(range(1100)) and rep.ids[:1100] == _ids(0, 1100)
    assert stub.CALLS["reinforce"] == 1 and stub.CALLS["touch"] == 1      # only the second chunk had stored targets


def test_order_reinforce_and_touch_before_the_write(hmod, monkeypatch):
    g = torch.Generator().manual_seed(3)
    base = torch.randn(10, 16, generator=g)
    hf = _hf(hmod, merge_similarity=0.99, merge_reinforce=0.25, merge_cap=0.9)
    hf.create_episodic_memories(_ids(0, 10), base)
    hf.decay_memories(0.5)
    hf.memory_metadata[:10, 1] = NOW - 1000.0
    log = _record(monkeypatch, "find_repeats", "bank_reinforce", "bank_touch", "bank_write")
    new = torch.randn(3, 16, generator=g)
    batch = torch.stack([base[2] * 3.0, new[0], base[7], base[2], new[1], new[1] * 0.5, new[2]])
    rep = hf.create_episodic_memories(_ids(0, 7, "n"), batch)
    assert [c[0] for c in log] == ["find_repeats", "bank_reinforce", "bank_touch", "bank_write"]
    assert log[1][1][2].tolist() == [2, 7] and log[1][1][3:] == (0.25, 0.9)         # the DISTINCT stored targets, once
    assert log[2][1][2].tolist() == [2, 7] and log[2][1][3] == NOW
    assert torch.equal(log[3][1][4], batch[[1, 4, 6]])                               # the kept rows only
    assert rep.merged.tolist() == [True, False, True, True, False, True, False]
    assert rep.rows.tolist() == [2, 10, 7, 2, 11, 11, 12]
    assert rep.ids == ["m2", "n1", "m7", "m2", "n4", "n4", "n6"] and (rep.n_stored, rep.n_merged) == (3, 4)
    want = torch.full((10,), 0.5)
    want[[2, 7]] = 0.75                                                              # once, not once per repeat
    assert torch.equal(hf.memory_metadata[:10, 0], want)
    ts = torch.full((10,), np.float32(NOW - 1000.0).item())
    ts[[2, 7]] = np.float32(NOW).item()
    assert torch.equal(hf.memory_metadata[:10, 1], ts)
    assert hf._slot_time[2] == NOW and hf._slot_time[7] == NOW
    # in-batch leaders are not reinforced: written at full strength with the current time
    assert hf.memory_metadata[11, 0].item() == 1.0
    # the id maps grow by the kept rows only
    assert hf.memory_count == 13 and len(hf.id_to_idx) == 13 and len(hf.episodic_memories) == 13
    assert all(m not in hf.id_to_idx for m in ("n0", "n2", "n3", "n5"))
    assert [hf.id_of_row(r) for r in (10, 11, 12)] == ["n1", "n4", "n6"]
    assert hf.episodic_memories["n4"].feature_idx == 11
    # the cap: a strength at or above it is left alone
    hf.memory_metadata[2, 0] = 0.95
    hf.create_episodic_memories(["again"], base[2:3])
    assert hf.memory_metadata[2, 0].item() == np.float32(0.95).item() and hf.memory_count == 13


def test_touch_and_find_repeats_are_public(hmod):
    hf = _hf(hmod)
    feats = torch.randn(6, 16)
    hf.create_episodic_memories(_ids(0, 6), feats)
    st, bl, cs = hf.find_repeats(torch.stack([feats[4], torch.randn(16), feats[4]]), 0.99, now=NOW)
    assert st.tolist() == [4, -1, 4] and bl.tolist() == [-1, -1, -1] and cs.dtype == torch.float32
    assert st.dtype == torch.int32 and bl.dtype == torch.int32 and not st.is_cuda
    meta = hf.memory_metadata.clone()
    assert hf.memory_count == 6 and torch.equal(hf.memory_metadata, meta)           # read-only
    hf.touch(torch.tensor([[1, -1], [99, 3]]), now=NOW + 500.0)
    want = meta.clone()
    want[[1, 3], 1] = NOW + 500.0
    assert torch.equal(hf.memory_metadata, want) and hf._slot_time[3] == NOW + 500.0 and hf._slot_time[0] == NOW
    hf.touch([], now=NOW)
    hf.touch([5])
    assert stub.CALLS["touch"] == 2
    empty = _hf(hmod)
    st, bl, cs = empty.find_repeats(torch.stack([feats[0], feats[0]]), 0.9)
    assert st.tolist() == [-1, -1] and bl.tolist() == [-1, 0]
    empty.touch([0])


@pytest.mark.parametrize("policy", ["reference", "fifo", "weakest"])
def test_report_on_a_full_bank(hmod, policy):
    g = torch.Generator().manual_seed(4)
    base = torch.randn(8, 16, generator=g)
    hf = _hf(hmod, M=8, overflow=policy, merge_similarity=0.99, merge_reinforce=0.5)
    hf.create_episodic_memories(_ids(0, 8), base)
    hf.memory_metadata[:8, 0] = torch.tensor([0.9, 0.1, 0.8, 0.7, 0.2, 0.65, 0.5, 0.4])
    new = torch.randn(3, 16, generator=g)
    # repeats of m1 (the weakest) and of m0 (where the ring and the reference write), a kept row and its repeat
    batch = torch.stack([base[1], new[0], new[0] * 2.0, base[0], new[1], new[2]])
    rep = hf.create_episodic_memories(_ids(0, 6, "n"), batch)
    assert rep.merged.tolist() == [True, False, True, True, False, False]
    assert (rep.n_stored, rep.n_merged) == (3, 3) and hf.memory_count == 8
    assert rep.ids == ["m1", "n1", "n1", "m0", "n4", "n5"]
    if policy == "reference":
        # every write goes to slot 0: the last kept row holds it, the earlier ones and m0 were overwritten by this call
        assert rep.rows.tolist() == [1, -1, -1, -1, -1, 0]
        assert hf.id_of_row(0) == "n5" and hf.id_of_row(1) == "m1"
    elif policy == "fifo":
        # the ring writes the kept rows to slots 0, 1, 2: m0 AND m1, both just repeated, are overwritten by this call
        assert rep.rows.tolist() == [-1, 0, 0, -1, 1, 2]
        assert [hf.id_of_row(r) for r in range(3)] == ["n1", "n4", "n5"]
    else:
        # m1 was reinforced to 0.6 (and m0 to the cap) before the victims were chosen: rows 4 (0.2), 7 (0.4) and
        # 6 (0.5) go, in that order; without the reinforcement m1 (0.1) would have been the first
        assert rep.rows.tolist() == [1, 4, 4, 0, 7, 6]
        assert hf.memory_metadata[1, 0].item() == np.float32(0.6).item() and hf.memory_metadata[0, 0].item() == 1.0
        assert [hf.id_of_row(r) for r in (0, 1, 4, 7, 6)] == ["m0", "m1", "n1", "n4", "n5"]
    for r, m in zip(rep.rows.tolist(), rep.ids):
        assert r == -1 or hf.id_of_row(r) == m
    assert all(m not in hf.id_to_idx for m in ("n0", "n2", "n3"))


def test_weakest_keeps_the_memory_that_was_just_repeated(hmod):
    g = torch.Generator().manual_seed(5)
    base = torch.randn(8, 16, generator=g)
    new = torch.randn(2, 16, generator=g)
    batch = torch.stack([new[0], base[3], new[1]])
    out = {}
    for tau in (None, 0.99):
        hf = _hf(hmod, M=8, overflow="weakest", merge_similarity=tau, merge_reinforce=0.5)
        hf.create_episodic_memories(_ids(0, 8), base)
        hf.memory_metadata[:8, 0] = torch.tensor([0.9, 0.8, 0.8, 0.1, 0.7, 0.3, 0.5, 0.9])
        hf.create_episodic_memories(_ids(0, 3, "n"), batch)
        out[tau] = hf
    assert out[None].id_of_row(3) == "n0"                              # without the option the weakest row goes first
    assert out[0.99].id_of_row(3) == "m3" and out[0.99].memory_metadata[3, 0].item() == np.float32(0.6).item()
    assert [out[0.99].id_of_row(r) for r in (5, 6)] == ["n0", "n2"]       # rows 5 (0.3) and 6 (0.5) went instead


def test_a_rebuild_boundary_inside_a_chunk(hmod):
    g = torch.Generator().manual_seed(6)
    base = torch.randn(100, 16, generator=g)
    ids = _ids(0, 100)

    def bank(**kw):
        hf = _hf(hmod, M=400, use_centroid_index=True, **kw)
        hf.centroids_k, hf.centroids_update_interval = 8, 32
        torch.manual_seed(11)                                          # the rebuilds draw from torch's generator
        return hf
    # 20 rows, then a batch of 60 that crosses the boundaries at 32 and 64 with 10 repeats spread through it
    batch = base[20:80].clone()
    rep_at = list(range(3, 60, 6))
    batch[rep_at] = base[:10] * 1.5
    hf = bank(merge_similarity=0.999)
    hf.create_episodic_memories(ids[:20], base[:20])
    rep = hf.create_episodic_memories(_ids(0, 60, "b"), batch)
    kept = [i for i in range(60) if i not in rep_at]
    assert rep.n_merged == 10 and rep.merged.nonzero().flatten().tolist() == rep_at
    assert rep.rows[rep_at].tolist() == list(range(10)) and hf.memory_count == 70 and hf._index_ready
    # the same bank as writing the kept rows alone: the rebuild cadence counts kept rows only
    ref = bank()
    ref.create_episodic_memories(ids[:20], base[:20])
    ref.create_episodic_memories([f"b{i}" for i in kept], batch[kept])
    assert torch.equal(ref.memory_features, hf.memory_features) and torch.equal(ref.centroids, hf.centroids)
    assert torch.equal(ref.memory_metadata[:, 2], hf.memory_metadata[:, 2]) and ref.id_to_idx == hf.id_to_idx
    assert torch.equal(ref.centroid_counts, hf.centroid_counts)


def test_layer_helpers_pass_the_threshold_on(hmod):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    hf = _hf(hmod)
    h = torch.randn(3, 5, 16)
    assert MO.store_memory(hf, h) is None and hf.memory_count == 3 and stub.CALLS["find_repeats"] == 0
    rep = MO.store_memory(hf, h, merge_similarity=0.999)
    assert rep.n_merged == 3 and hf.memory_count == 3 and rep.rows.tolist() == [0, 1, 2]

    class Layer(MO.BatchedMemoryMixin):
        hippocampus = hf
    assert Layer().store_memory(h * 2.0, merge_similarity=0.999).n_merged == 3
    assert Layer().store_memory(torch.randn(2, 5, 16)) is None and hf.memory_count == 5
    built = _hf(hmod, merge_similarity=0.999)
    MO.store_memory(built, h)
    assert MO.store_memory(built, h).n_merged == 3 and built.memory_count == 3          # needs neither argument
    for fn in (MO.store_memory, MO.BatchedMemoryMixin.store_memory):
        assert inspect.signature(fn).parameters["merge_similarity"].default is None
