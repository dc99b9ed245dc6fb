"""Host-side logic of consolidation within tags on the CPU (``ops`` replaced by tests/cpu_stub_consolidate_scoped.py,
which restates the scoped rule in torch fp64 by masking the cosines): the rule on hand-made rows, that nothing changes
while the option is off, the chunking at 1024 rows (a chunk's kept rows carry their tags before the next chunk searches),
``consolidate(within_tags=True)`` against the tagged write stream, and the layer helpers."""
import inspect

import numpy as np
import pytest
import torch

from tests import cpu_stub_consolidate_scoped as stub

NOW = 1.7e9 + 11.0


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    stub.FIND_SIZES.clear()
    stub.MOVES.clear()
    stub.STAMPS.clear()
    stub.SCOPED_FINDS.clear()
    return H


def _hf(H, D=16, M=64, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _ids(a, b, p="m"):
    return [f"{p}{i}" for i in range(a, b)]


def _record(monkeypatch, *names):
    log = []
    for name in names:
        real = getattr(stub, name)

        def wrapped(*a, _real=real, _name=name, **kw):
            log.append((_name, a, kw))
            return _real(*a, **kw)
        monkeypatch.setattr(stub, name, wrapped)
    return log


def test_the_scoped_rule_on_hand_made_rows(hmod):
    e = torch.eye(6)
    bank = torch.stack([e[0] + 0.1 * e[5], e[0], e[1], e[2], e[3]])
    meta = torch.zeros(5, 4)
    meta[:, 3] = torch.tensor([1.0, 2.0, 2.0, 0.0, 7.0])
    inv = 1.0 / bank.norm(dim=1)
    big = 1 << 24
    feats = torch.stack([
        e[0],                    # 0  tag 1: row 1 (tag 2) is the closer copy, row 0 (tag 1, cos 0.995) is the target
        e[1],                    # 1  tag 1: its copy exists only under tag 2: kept
        e[1] + 0.02 * e[4],      # 2  tag 2: the same copy under its own tag: stored row 2
        e[4],                    # 3  tag 3: new, kept
        e[4] + 0.02 * e[5],      # 4  tag 5: an in-batch copy of row 3, which carries another tag: kept
        e[4] + 0.001 * e[5],     # 5  tag 5: the chain skips the kept row 3 (closer, tag 3) and takes row 4
        e[2],                    # 6  tag 0: "untagged" is a scope like any other: stored row 3
        e[2],                    # 7  tag 4: ... and no wildcard: kept
        e[3],                    # 8  tag 9: a tag nobody holds matches nothing (row 4 carries 7): kept
        e[3],                    # 9  tag 2^24: outside the range: kept
        e[3],                    # 10 tag 2^24: ... and not even a row with the same value is its leader: kept
        e[3],                    # 11 tag 9: repeats row 8
    ])
    tags = torch.tensor([1, 1, 2, 3, 5, 5, 0, 4, 9, big, big, 9], dtype=torch.int32)
    st, bl, cs = stub.find_repeats_scoped_reference(bank, inv, meta, 5, feats, tags, 0.99)
    assert st.tolist() == [0, -1, 2, -1, -1, -1, 3, -1, -1, -1, -1, -1]
    assert bl.tolist() == [-1, -1, -1, -1, -1, 4, -1, -1, -1, -1, -1, 8]
    assert abs(float(cs[0]) - 1.0 / 1.01 ** 0.5) < 1e-6 and float(cs[1]) == float("-inf")
    # the scope-blind rule decides these rows differently
    s0, b0, _ = stub.find_repeats_reference(bank, inv, 5, feats, 0.99)
    assert s0.tolist() == [1, 2, 2, -1, -1, -1, 3, 3, 4, 4, 4, 4] and b0.tolist() == [-1] * 4 + [3, 3] + [-1] * 6
    mcs, mcb = stub.scoped_cosines(bank, inv, meta, 5, feats, tags)
    stub.replay_check(mcs, mcb, 0.99, stub.tolerance(6), st, bl, cs)
    # a held row whose column 3 holds no tag is nobody's target; one tag everywhere is the scope-blind rule
    meta[4, 3] = float(big)
    st2, _, _ = stub.find_repeats_scoped_reference(bank, inv, meta, 5, feats[8:9], torch.tensor([big], dtype=torch.int32), 0.99)
    assert st2.tolist() == [-1]
    meta[:, 3] = 3.0
    out = stub.find_repeats_scoped_reference(bank, inv, meta, 5, feats, torch.full((12,), 3, dtype=torch.int32), 0.99)
    assert out[0].tolist() == s0.tolist() and out[1].tolist() == b0.tolist()
    # the same rows through the bank's own entry point
    hf = _hf(hmod, D=6)
    hf.create_episodic_memories(_ids(0, 5), bank, tags=[1, 2, 2, 0, 7])
    h_st, h_bl, h_cs = hf.find_repeats(feats, 0.99, tags=tags)
    assert h_st.tolist() == st.tolist() and h_bl.tolist() == bl.tolist() and torch.equal(h_cs, cs.float())
    assert hf.find_repeats(feats, 0.99)[0].tolist() == s0.tolist()


def test_with_the_option_off_nothing_changes(hmod, monkeypatch):
    log = _record(monkeypatch, "find_repeats", "find_repeats_scoped", "bank_write", "bank_set_tags")
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(20, 16, generator=g)
    hf = _hf(hmod, merge_similarity=0.999)
    assert hf.merge_within_tags is False
    hf.create_episodic_memories(_ids(0, 20), feats)
    hf.find_repeats(feats[:3], 0.9)
    hf.consolidate()
    finds = [c for c in log if c[0] == "find_repeats"]
    assert len(finds) == 2 + 1 and stub.CALLS["find_repeats_scoped"] == 0 and stub.CALLS["set_tags"] == 0
    for _, a, kw in finds:                          # today's arguments: five positionals, no image on this small bank
        assert len(a) == 5 and kw == {} and a[0] is hf.memory_features and a[1] is hf._inv_norm
    # tags together with a consolidating write still raise, with the existing message, before anything runs
    before = dict(stub.CALLS)
    for call in (dict(tags=3), dict(tags=3, merge_within_tags=False)):
        with pytest.raises(ValueError, match="merge_similarity"):
            hf.create_episodic_memories(["a"], feats[:1], **call)
    with pytest.raises(ValueError, match="merge_similarity"):
        hf.create_episodic_memory("a", "e", feats[0], tag=3)
    assert stub.CALLS == before and hf.memory_count == 20
    # the signatures' defaults
    p = inspect.signature(hmod.HippocampalFormation.__init__).parameters
    assert p["merge_within_tags"].default is False
    p = inspect.signature(hmod.HippocampalFormation.find_repeats).parameters
    assert p["tags"].default is None and p["tags"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(hmod.HippocampalFormation.consolidate).parameters
    assert p["within_tags"].default is None and list(p)[:3] == ["self", "similarity", "rebuild"]
    for fn in (hmod.HippocampalFormation.create_episodic_memories, hmod.HippocampalFormation.create_episodic_memory):
        assert inspect.signature(fn).parameters["merge_within_tags"].default is hmod._INSTANCE_DEFAULT


def test_find_repeats_takes_an_int_a_sequence_or_a_tensor(hmod):
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(6, 16, generator=g)
    hf = _hf(hmod)
    hf.create_episodic_memories(_ids(0, 6), feats, tags=[1, 1, 2, 2, 0, 0])
    q = torch.stack([feats[0], feats[2], feats[4], feats[4]])
    for tags in ([1, 1, 0, 1], np.array([1, 1, 0, 1]), torch.tensor([1, 1, 0, 1], dtype=torch.int32),
                 torch.tensor([1, 1, 0, 1])):
        st, bl, cs = hf.find_repeats(q, 0.99, tags=tags)
        assert st.tolist() == [0, -1, 4, -1] and bl.tolist() == [-1] * 4
        assert st.dtype == torch.int32 and cs.dtype == torch.float32
    assert hf.find_repeats(q, 0.99, tags=2)[0].tolist() == [-1, 2, -1, -1]
    assert hf.find_repeats(q, 0.99, tags=0)[0].tolist() == [-1, -1, 4, 4]
    assert hf.find_repeats(q, 0.99, tags=7)[1].tolist() == [-1, -1, -1, 2]          # kept row 2, then its copy
    assert hf.find_repeats(q, 0.99, tags=[1 << 30, -5, 1 << 24, 0])[0].tolist() == [-1, -1, -1, 4]
    assert stub.CALLS["find_repeats_scoped"] == 8 and stub.CALLS["find_repeats"] == 0
    assert all(count == 6 for count, _ in stub.SCOPED_FINDS)
    for bad in ([1, 2], 1.5, torch.tensor([0.5] * 4)):
        with pytest.raises(ValueError):
            hf.find_repeats(q, 0.99, tags=bad)
    # an empty bank: only the batch's own rows, by tag
    empty = _hf(hmod)
    st, bl, _ = empty.find_repeats(torch.stack([feats[0]] * 3), 0.9, tags=[4, 5, 4])
    assert st.tolist() == [-1] * 3 and bl.tolist() == [-1, -1, 0]


def test_a_tagged_merging_write(hmod, monkeypatch):
    g = torch.Generator().manual_seed(3)
    base = torch.randn(6, 16, generator=g)
    hf = _hf(hmod, merge_similarity=0.99, merge_within_tags=True, merge_reinforce=0.25)
    hf.create_episodic_memories(_ids(0, 6), base, tags=[1, 1, 2, 2, 0, 0])
    assert hf.memory_count == 6 and hf.memory_tags.tolist() == [1, 1, 2, 2, 0, 0]
    hf.decay_memories(0.5)
    log = _record(monkeypatch, "find_repeats_scoped", "bank_reinforce", "bank_touch", "bank_write", "bank_set_tags")
    new = torch.randn(2, 16, generator=g)
    batch = torch.stack([base[0] * 2.0,       # tag 1: repeats m0
                         base[0] * 3.0,       # tag 2: m0's copy under another tag: stored
                         base[0] * 0.5,       # tag 2: repeats the row above, not m0
                         new[0],              # tag 1
                         new[0] * 2.0,        # tag 0: stored, untagged rows are a scope
                         base[4]])            # tag 0: repeats m4
    rep = hf.create_episodic_memories(_ids(0, 6, "n"), batch, tags=[1, 2, 2, 1, 0, 0])
    assert [c[0] for c in log] == ["find_repeats_scoped", "bank_reinforce", "bank_touch", "bank_write", "bank_set_tags"]
    assert log[1][1][2].tolist() == [0, 4] and log[2][1][2].tolist() == [0, 4]
    assert rep.merged.tolist() == [True, False, True, False, False, True]
    assert rep.ids == ["m0", "n1", "n1", "n3", "n4", "m4"] and rep.rows.tolist() == [0, 6, 6, 7, 8, 4]
    assert hf.memory_count == 9 and hf.memory_tags.tolist() == [1, 1, 2, 2, 0, 0, 2, 1, 0]
    assert hf.memory_metadata[[0, 4], 0].tolist() == [0.75, 0.75] and hf.memory_metadata[1, 0].item() == 0.5
    # untagged rows are tag 0 and merge only into untagged memories; the write then stamps nothing
    n_stamps = stub.CALLS["set_tags"]
    rep = hf.create_episodic_memories(["u0", "u1"], torch.stack([base[0], base[5] * 4.0]))
    assert rep.merged.tolist() == [False, True] and rep.ids == ["u0", "m5"] and stub.CALLS["set_tags"] == n_stamps
    assert hf.memory_tags.tolist()[-1] == 0 and stub.SCOPED_FINDS[-1][1] == [0, 0]
    # per call, and through the one-row entry point
    plain = _hf(hmod)
    plain.create_episodic_memories(["a"], base[:1], tags=5)
    assert plain.create_episodic_memory("b", "e", base[0] * 2.0, merge_similarity=0.99, tag=6,
                                        merge_within_tags=True).n_merged == 0
    assert plain.create_episodic_memory("c", "e", base[0] * 3.0, merge_similarity=0.99, tag=5,
                                        merge_within_tags=True).ids == ["a"]
    assert plain.memory_tags.tolist() == [5, 6] and stub.CALLS["find_repeats"] == 0


def test_a_chunks_kept_rows_carry_their_tags_before_the_next_chunk_searches(hmod, monkeypatch):
    g = torch.Generator().manual_seed(4)
    base = torch.randn(1100, 16, generator=g)
    tags = torch.randint(1, 4, (1100,), generator=g)
    # rows 1100.. repeat rows 0..299: the first 150 under their source's tag, the others under another one
    feats = torch.cat([base, base[:300] * 1.5])
    rtags = tags[:300].clone()
    rtags[150:] = rtags[150:] % 3 + 1
    all_tags = torch.cat([tags, rtags]).numpy()
    log = _record(monkeypatch, "find_repeats_scoped", "bank_write", "bank_set_tags")
    hf = _hf(hmod, M=4096)
    rep = hf.create_episodic_memories(_ids(0, 1400), feats, merge_similarity=0.999, tags=all_tags, merge_within_tags=True)
    assert [c[0] for c in log] == ["find_repeats_scoped", "bank_write", "bank_set_tags"] * 2
    assert [len(t) for _, t in stub.SCOPED_FINDS] == [1024, 376] and [c for c, _ in stub.SCOPED_FINDS] == [0, 1024]
    # what the second search saw in column 3: the first chunk's tags, already stamped
    assert stub.STAMPS[0][0] == list(range(1024)) and stub.STAMPS[0][1] == tags[:1024].tolist()
    assert rep.n_merged == 150 and rep.n_stored == 1250 and hf.memory_count == 1250
    assert rep.rows[1100:1250].tolist() == list(range(150)) and rep.ids[1100:1250] == _ids(0, 150)
    assert not bool(rep.merged[1250:].any()) and not bool(rep.merged[:1100].any())
    assert hf.memory_tags.tolist() == np.concatenate([all_tags[:1100], all_tags[1250:]]).tolist()
    assert stub.CALLS["find_repeats"] == 0


def _tagged_bank():
    """40 rows over tags 0..2: near-copies inside a tag, the same direction under other tags, degenerate rows."""
    g = torch.Generator().manual_seed(5)
    b = torch.randn(10, 16, generator=g)
    rows = torch.cat([b, b * 2.0, b[:5] * 0.5 + 1e-5 * torch.randn(5, 16, generator=g), torch.zeros(1, 16), b[5:] * 3.0,
                      torch.randn(9, 16, generator=g)])
    tags = np.concatenate([np.arange(10) % 3, (np.arange(10) + 1) % 3, np.arange(5) % 3, [1], (np.arange(5, 10) + 1) % 3,
                           np.arange(9) % 3]).astype(np.int64)
    perm = torch.randperm(rows.shape[0], generator=g)
    return rows[perm].contiguous(), tags[perm.numpy()]


@pytest.mark.parametrize("slab", [7, 1024])
def test_consolidate_within_tags_equals_the_tagged_write_stream(hmod, monkeypatch, slab):
    monkeypatch.setattr(stub, "CONSOLIDATE_MAX_BATCH", slab)
    rows, tags = _tagged_bank()
    n = rows.shape[0]
    hf = _hf(hmod)
    hf.create_episodic_memories(_ids(0, n), rows, tags=tags)
    assert hf.memory_count == n
    rep = hf.consolidate(0.999, within_tags=True)
    stream = _hf(hmod)
    wrep = stream.create_episodic_memories(_ids(0, n), rows, merge_similarity=0.999, tags=tags, merge_within_tags=True)
    k = stream.memory_count
    assert hf.memory_count == k and (rep.n_before, rep.n_kept, rep.n_merged) == (n, wrep.n_stored, wrep.n_merged)
    assert 0 < rep.n_merged < n - 10
    assert torch.equal(hf.memory_features, stream.memory_features)                  # bit for bit, the cleared tail too
    assert hf.memory_tags.tolist() == stream.memory_tags.tolist()
    assert hf.id_to_idx == stream.id_to_idx and [hf.id_of_row(r) for r in range(k)] == [stream.id_of_row(r) for r in range(k)]
    assert rep.old_to_new.tolist() == wrep.rows.tolist()
    # no merged row crossed a tag
    assert all(tags[i] == int(hf.memory_tags[rep.old_to_new[i]]) for i in range(n))
    assert stub.CALLS["find_repeats"] == 0 and all(t.dtype == torch.int32 for t in [hf.memory_tags])
    # the instance default, and within_tags=False is today's scope-blind pass
    own = _hf(hmod, merge_similarity=0.999, merge_within_tags=True)
    own.create_episodic_memories(_ids(0, n), rows, merge_similarity=None, tags=tags)
    assert own.consolidate().n_kept == k
    blind, today = _hf(hmod, merge_within_tags=True), _hf(hmod)
    for bank in (blind, today):
        bank.create_episodic_memories(_ids(0, n), rows, tags=tags)
    before = stub.CALLS["find_repeats_scoped"]
    r0, r1 = blind.consolidate(0.999, within_tags=False), today.consolidate(0.999)
    assert stub.CALLS["find_repeats_scoped"] == before and stub.CALLS["find_repeats"] > 0
    assert r0.old_to_new.tolist() == r1.old_to_new.tolist() and r0.n_kept == r1.n_kept < k
    assert torch.equal(blind.memory_features, today.memory_features)
    assert torch.equal(blind.memory_metadata, today.memory_metadata)


def test_layer_helpers_pass_the_option_on(hmod):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    hf = _hf(hmod)
    h = torch.randn(3, 5, 16)
    MO.store_memory(hf, h, tag=[1, 2, 1])
    with pytest.raises(ValueError, match="merge_similarity"):
        MO.store_memory(hf, h, merge_similarity=0.999, tag=1)
    rep = MO.store_memory(hf, h, merge_similarity=0.999, tag=[2, 2, 1], merge_within_tags=True)
    assert rep.merged.tolist() == [False, True, True] and hf.memory_count == 4 and hf.memory_tags.tolist() == [1, 2, 1, 2]

    class Layer(MO.BatchedMemoryMixin):
        hippocampus = hf
    assert Layer().store_memory(h * 2.0, merge_similarity=0.999, tag=3, merge_within_tags=True).n_merged == 0
    inj = MO.MemoryInjection(hf, 16, num_heads=2)
    assert inj.store_memory(h * 3.0, merge_similarity=0.999, tag=3, merge_within_tags=True).n_merged == 3
    assert hf.memory_count == 7
    # rows 0 and 2 (tag 1) hold different directions; under tag 3 and tag 2 / 1 the same three directions are held
    assert Layer().consolidate_memory(0.999, within_tags=True).n_merged == 0
    assert inj.consolidate_memory(similarity=0.999, within_tags=False).n_merged == 4
    built = _hf(hmod, merge_similarity=0.999, merge_within_tags=True)
    MO.store_memory(built, h, tag=1)
    assert MO.store_memory(built, h, tag=2).n_merged == 0 and MO.store_memory(built, h, tag=1).n_merged == 3
    for fn in (MO.store_memory, MO.BatchedMemoryMixin.store_memory, MO.MemoryInjection.store_memory):
        assert inspect.signature(fn).parameters["merge_within_tags"].default is None
    for fn in (MO.BatchedMemoryMixin.consolidate_memory, MO.MemoryInjection.consolidate_memory):
        p = inspect.signature(fn).parameters
        assert p["within_tags"].default is None and p["similarity"].default is None
