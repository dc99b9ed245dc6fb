"""Host-side logic of per-tag quotas on the CPU (``ops`` replaced by tests/cpu_stub_quota.py, which restates the rule of
``include/aura_hip.h`` in torch): the rule on hand-made metadata, that nothing changes while no quota is set, FIFO inside
a tag of tied keys (the tie origin), a full bank's mixed run, over-quota tags and ``enforce_tag_quotas``, the remap of
the tie origins by a compaction against an fp64 model, the checkpoint round trip, quotas with consolidation within tags,
and the refusals."""
import math

import numpy as np
import pytest
import torch

from tests import cpu_stub_quota as stub

NOW = 1.7e9                    # = 128 * 13281250: on the grid of the stored fp32 timestamps
STEP = 1280.0                  # ten grid steps: keys written a step apart differ by exp(-1280 / 3600) = 0.70


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    clock = {"t": NOW}
    monkeypatch.setattr(H.time, "time", lambda: clock["t"])
    H.clock = clock
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    yield H
    del H.clock


def _hf(H, D=16, M=64, **kw):
    kw.setdefault("use_centroid_index", False)
    kw.setdefault("overflow", "weakest")
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _ids(a, b, p="m"):
    return [f"{p}{i}" for i in range(a, b)]


def _held(hf, tag):
    """ids of the held rows that carry ``tag``, in row order"""
    return [hf.id_of_row(r) for r in np.nonzero(hf.memory_tags.numpy() == tag)[0].tolist()]


def _new_calls():
    return {k: stub.CALLS[k] for k in ("select_scoped", "select_masked", "tag_counts")}


# ---------------------------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_made_metadata(hmod):
    count = 8
    meta = torch.zeros(count, 4)
    meta[:, 0] = torch.tensor([1.0, 0.5, float("nan"), 0.5, -0.0, 0.0, 0.5, 1.0])
    meta[:, 1] = NOW                                      # age 0: key == strength
    meta[:, 3] = torch.tensor([7.0, 7, 7, 7, 7, 7, 3, 3])
    keys = stub.bank_retention_keys(meta, count, NOW)
    tags = stub.held_tags(meta, count)
    # tag 7 from origin 5: the NaN key first; then -0 == +0, row 5 (rotated 0) before row 4 (rotated 7); then the tied 0.5s
    # in ring order from 5 (row 1 -> 4, row 3 -> 6); row 0 last
    assert stub.scope_victims(keys, tags, 7, 5, 6).tolist() == [2, 5, 4, 1, 3, 0]
    assert stub.scope_victims(keys, tags, 7, 0, 6).tolist() == [2, 4, 5, 1, 3, 0]
    # x_t = 0, 1 and held_t; an empty scope; a scope of another tag with its own origin
    scope_tags, origins = [3, 7, 9], [7, 5, 0]
    for in7, q7, want7 in ((1, 7, []), (1, 6, [2]), (6, 6, [2, 5, 4, 1, 3, 0])):
        held, x, victims = stub.scoped_reference(keys, tags, scope_tags, origins, [1, in7, 2], [2, q7, 1])
        assert held.tolist() == [2, 6, 0] and x.tolist() == [1, len(want7), 0]
        assert [v.tolist() for v in victims] == [[6], want7, []]
        # the same through the op and the host's decode: arrival order does not matter, the bitmap names the victims
        packed, bitmap = stub.bank_select_weakest_scoped(meta, count, NOW, scope_tags, origins, [1, in7, 2], [2, q7, 1])
        h2, x2, v2 = stub.scoped_selection_decode(packed, [1, in7, 2])
        assert h2.tolist() == [2, 6, 0] and x2.tolist() == x.tolist() and [v.tolist() for v in v2] == [[6], want7, []]
        assert stub.bitmap_rows(bitmap, count).tolist() == sorted([6] + want7)
    # tag 3 from origin 7: its tied... rows differ in key, so the origin does not matter; from equal keys it would
    meta[6, 0] = 1.0
    keys = stub.bank_retention_keys(meta, count, NOW)
    assert stub.scope_victims(keys, tags, 3, 7, 2).tolist() == [7, 6]
    # the global victims skip the tag victims: the bank's order from cursor 3 is [2, 4, 5, 3, 1, 6, 7, 0]
    assert stub.eviction_order(keys, 3).tolist() == [2, 4, 5, 3, 1, 6, 7, 0]
    assert stub.masked_reference(keys, 3, 3, [2, 5]).tolist() == [4, 3, 1]
    assert stub.tag_counts_reference(meta, count, [0, 3, 7]).tolist() == [0, 2, 6]


def test_off_means_nothing_changes(hmod, monkeypatch):
    H = hmod
    torch.manual_seed(0)
    feats = torch.randn(40, 16)
    tags = np.arange(40) % 3
    plain = _hf(H, M=16)
    keys0 = set(plain.bank_state())
    plain.create_episodic_memories(_ids(0, 12), feats[:12], tags=tags[:12])
    plain.decay(0.3)
    plain.create_episodic_memories(_ids(12, 30), feats[12:30], tags=tags[12:30])     # fills the bank and overflows
    assert _new_calls() == {"select_scoped": 0, "select_masked": 0, "tag_counts": 0}
    assert set(plain.bank_state()) == keys0 and "tag_quota" not in keys0 and plain.tag_quotas == {}
    # the plan of a full bank is the plain 'weakest' plan, tags or no tags
    want, _ = stub.bank_select_weakest(plain.memory_metadata, 16, NOW, plain._write_cursor % 16, 5)
    cur = plain._write_cursor
    for t in (None, tags[:5]):
        slots, n_app, count, cursor = plain._plan_slots(5, NOW) if t is None else plain._plan_slots(5, NOW, tags=t)
        assert slots.tolist() == want.tolist() and (n_app, count, cursor) == (0, 16, cur + 5)
    assert plain._pending_origins is None
    # a bank WITH quotas: an untagged write, and a write of unlimited tags only, launch nothing new and plan alike
    lim = _hf(H, M=16, tag_quota={7: 2})
    lim.create_episodic_memories(_ids(0, 12), feats[:12], tags=tags[:12])
    lim.decay(0.3)
    lim.create_episodic_memories(_ids(12, 30), feats[12:30], tags=tags[12:30])
    lim.create_episodic_memories(_ids(30, 34), feats[30:34])
    plain.create_episodic_memories(_ids(30, 34), feats[30:34])
    assert _new_calls() == {"select_scoped": 0, "select_masked": 0, "tag_counts": 0}
    assert torch.equal(lim.memory_features, plain.memory_features) and torch.equal(lim.memory_metadata, plain.memory_metadata)
    assert lim._write_cursor == plain._write_cursor and lim.id_to_idx == plain.id_to_idx
    assert set(lim.bank_state()) == keys0 | {"tag_quota", "tag_origin"}


@pytest.mark.parametrize("batches", [[1] * 12, [3] * 4, [5, 5, 2]])
def test_fifo_inside_a_tag_under_tied_keys(hmod, batches):
    """The test of the tie origin: ranked from the bank's one cursor, the row just written would be the first of the tied
    rows again and the tag would keep its oldest memories."""
    H = hmod
    hf = _hf(H, M=64, tag_quota={7: 4})
    torch.manual_seed(1)
    hf.create_episodic_memories(_ids(0, 6, "o"), torch.randn(6, 16), tags=[0, 1, 1, 2, 0, 2])
    before = (hf.memory_features[:6].clone(), hf.memory_metadata[:6].clone())
    i = 0
    for b in batches:                                     # 5 > quota: the batch is cut into runs of at most 4
        hf.create_episodic_memories(_ids(i, i + b), torch.randn(b, 16), tags=7)
        i += b
        assert hf.tag_counts() == {7: min(i, 4)}
    assert sorted(_held(hf, 7)) == sorted(_ids(8, 12))
    assert hf.memory_count == 10 and hf._write_cursor == 0               # nobody else's rows, no global victim
    # rows of other tags and untagged rows are bit-identical
    assert torch.equal(hf.memory_features[:6], before[0]) and torch.equal(hf.memory_metadata[:6], before[1])
    assert [hf.id_of_row(r) for r in range(6)] == _ids(0, 6, "o")
    assert all(f"m{j}" not in hf.id_to_idx or hf.id_of_row(hf.id_to_idx[f"m{j}"]) != f"m{j}" for j in range(8))


def test_int_quota_limits_every_tag_but_zero(hmod):
    H = hmod
    hf = _hf(H, M=64, tag_quota=3)
    assert dict(hf.tag_quotas) == {None: 3}
    torch.manual_seed(2)
    tags = np.array([1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 0, 0])
    for i, t in enumerate(tags.tolist()):
        hf.create_episodic_memory(f"m{i}", "e", torch.randn(16), tag=t)
    assert hf.tag_counts() == {1: 3, 2: 3} and hf.tag_counts([0, 1, 5]) == {0: 6, 1: 3, 5: 0}
    assert _held(hf, 1) and sorted(_held(hf, 1)) == ["m12", "m6", "m9"] and sorted(_held(hf, 2)) == ["m10", "m4", "m7"]
    hf.set_tag_quota(0, 2)                                # tag 0 may be named: untagged writes are then limited
    hf.create_episodic_memories(_ids(20, 22), torch.randn(2, 16))
    assert hf.tag_counts([0]) == {0: 6}                   # over its quota: it does not grow, it does not shrink
    rep = hf.enforce_tag_quotas()
    assert rep.n_removed == 4 and hf.tag_counts([0]) == {0: 2} and sorted(_held(hf, 0)) == ["m20", "m21"]


def test_a_full_bank_with_a_mixed_run(hmod):
    H = hmod
    M = 16
    hf = _hf(H, M=M, tag_quota={7: 4, 3: 2})
    torch.manual_seed(3)
    hf.create_episodic_memories(_ids(0, M), torch.randn(M, 16), tags=[7, 1, 7, 0, 3, 7, 1, 0, 7, 3, 1, 0, 1, 1, 0, 0])
    hf.decay(0.5)
    hf.reinforce(torch.tensor([0, 3, 9, 12]), amount=0.25)
    hf._write_cursor = 6
    hf._tag_origin = {7: 3}
    H.clock["t"] = NOW + STEP
    run_tags = np.array([7, 0, 7, 3, 1], dtype=np.int32)
    keys = stub.bank_retention_keys(hf.memory_metadata, M, NOW + STEP)
    slots_w, n_app_w, cursor_w, origins_w, tagv_w, glob_w = stub.rule_run(
        keys, stub.held_tags(hf.memory_metadata, M), run_tags.tolist(), hf._quota_of, {7: 3}, 6, M)
    # by hand: tag 3 holds rows 4 (0.5) and 9 (0.75): victim 4.  tag 7 holds 0 (0.75), 2, 5, 8 (0.5): from origin 3 the
    # tied 0.5s go 5, 8, 2: victims 5, 8.  The two global victims are the first of the bank's order from cursor 6 that
    # are not among them: rows 6, 7 (0.5, rotated 0 and 1).
    assert tagv_w == {3: [4], 7: [5, 8]} and glob_w == [6, 7] and slots_w == [4, 5, 8, 6, 7] and n_app_w == 0
    before = _new_calls()
    slots, n_app, count, cursor = hf._plan_slots(5, NOW + STEP, tags=run_tags)
    assert slots.tolist() == slots_w and (n_app, count, cursor) == (0, M, 6 + 2) and cursor_w == 8
    assert hf._pending_origins == {3: 5, 7: 9} and origins_w == {3: 5, 7: 9}
    after = _new_calls()
    assert (after["select_scoped"] - before["select_scoped"], after["select_masked"] - before["select_masked"]) == (1, 1)
    hf._pending_origins = None
    # the write itself: row i of the run owns slot i of the plan, with its tag; nobody else's row is touched
    meta0, feat0 = hf.memory_metadata.clone(), hf.memory_features.clone()
    f = torch.randn(5, 16)
    hf.create_episodic_memories(_ids(100, 105), f, tags=run_tags)
    assert hf._write_cursor == 8 and hf._tag_origin == {3: 5, 7: 9}
    assert [hf.id_to_idx[f"m{100 + i}"] for i in range(5)] == slots_w
    assert hf.memory_tags[slots_w].tolist() == run_tags.tolist() and torch.equal(hf.memory_features[slots_w], f)
    rest = [r for r in range(M) if r not in slots_w]
    assert torch.equal(hf.memory_metadata[rest], meta0[rest]) and torch.equal(hf.memory_features[rest], feat0[rest])
    assert hf.tag_counts() == {3: 2, 7: 4}
    # no tag victim (the tag is under its quota): the unmasked selection serves, one read fewer launches
    hf.set_tag_quota(9, 5)
    c0 = _new_calls()
    s0 = stub.CALLS["select"]
    hf.create_episodic_memories(["n0"], torch.randn(1, 16), tags=9)
    assert _new_calls()["select_masked"] == c0["select_masked"] and stub.CALLS["select"] == s0 + 1
    assert hf._write_cursor == 9


def test_a_room_and_a_quota_in_one_run(hmod):
    """A bank with room: the tag victims are overwritten, the rest of the run appends (its FIRST rows)."""
    H = hmod
    hf = _hf(H, M=32, tag_quota={7: 2})
    torch.manual_seed(4)
    hf.create_episodic_memories(_ids(0, 4), torch.randn(4, 16), tags=[7, 1, 7, 1])
    hf.create_episodic_memories(_ids(4, 8), torch.randn(4, 16), tags=[1, 7, 0, 7])
    # x_7 = 2 (rows 0, 2), two appends: the run's first two rows take rows 4, 5, the others the victims in order
    assert [hf.id_to_idx[f"m{i}"] for i in range(4, 8)] == [4, 5, 0, 2]
    assert hf.memory_tags[[4, 5, 0, 2]].tolist() == [1, 7, 0, 7] and hf.memory_count == 6
    assert hf.tag_counts() == {7: 2} and hf._tag_origin == {7: 3} and hf._write_cursor == 0


def test_a_reinforced_memory_outlives_weaker_newer_ones(hmod):
    H = hmod
    hf = _hf(H, M=32, tag_quota={7: 3})
    torch.manual_seed(5)
    hf.create_episodic_memories(["a", "b", "c"], torch.randn(3, 16), tags=7)
    hf.decay(0.5)
    hf.reinforce(torch.tensor([hf.id_to_idx["a"]]), amount=0.3)           # a: 0.8, b and c (newer in the ring): 0.5
    gone = []
    for mid in ("d", "e", "f"):
        before = set(_held(hf, 7))
        hf.create_episodic_memory(mid, "e", torch.randn(16), tag=7)
        gone += list(before - set(_held(hf, 7)))
    assert gone == ["b", "c", "a"]


def test_over_quota_neither_grows_nor_shrinks_until_enforced(hmod):
    H = hmod
    hf = _hf(H, M=64, tag_quota={7: 4, 2: 3})
    torch.manual_seed(6)
    hf.bulk_write(torch.randn(10, 16), rebuild=False)
    hf.retag(rows=np.arange(10), tag=7)
    hf.create_episodic_memories(_ids(0, 5, "t"), torch.randn(5, 16), tags=2)   # tag 2: three of them stay
    hf.decay(0.5)
    hf.reinforce(torch.tensor([1, 4, 6]), amount=0.2)
    assert hf.tag_counts() == {2: 3, 7: 10}
    H.clock["t"] = NOW + STEP
    for i in range(3):
        hf.create_episodic_memory(f"w{i}", "e", torch.randn(16), tag=7)
        assert hf.tag_counts() == {2: 3, 7: 10}
    count = hf.memory_count
    keys = stub.bank_retention_keys(hf.memory_metadata, count, NOW + STEP)
    order7 = stub.scope_victims(keys, stub.held_tags(hf.memory_metadata, count), 7, hf._tag_origin.get(7, 0), 10).tolist()
    ids = [hf.id_of_row(r) for r in range(count)]
    rep = hf.enforce_tag_quotas(now=NOW + STEP)
    assert rep.n_removed == 6 and hf.tag_counts() == {2: 3, 7: 4} and hf.memory_count == count - 6
    assert sorted(np.nonzero(rep.old_to_new < 0)[0].tolist()) == sorted(order7[:6])
    for r in range(count):                                # the report's rows match
        if rep.old_to_new[r] >= 0:
            assert hf.id_of_row(int(rep.old_to_new[r])) == ids[r]
    assert sorted(_held(hf, 7)) == sorted(ids[r] for r in order7[6:])     # the last-ranked (strongest) survive
    again = hf.enforce_tag_quotas()
    assert again.n_removed == 0 and again.old_to_new.tolist() == list(range(count - 6))


# ---------------------------------------------------------------------------------------------------------------------
class Model:
    """The bank's retention in fp64 on python lists: rows (id, tag, strength, timestamp), one cursor, tie origins."""

    def __init__(self, M, quotas):
        self.M, self.q, self.rows, self.cursor, self.origin = M, dict(quotas), [], 0, {}

    def keys(self, now):
        return [s * math.exp(-(now - ts) / 3600.0) for _, _, s, ts in self.rows]

    @staticmethod
    def check_keys(keys):
        """the condition of the data: any two keys are bit-equal or at least 1e-3 apart (relative)"""
        k = sorted(keys)
        for a, b in zip(k, k[1:]):
            assert a == b or (b - a) >= 1e-3 * max(abs(a), abs(b)), (a, b)

    def write(self, ids, tags, now):
        """one run"""
        count, keys = len(self.rows), self.keys(now)
        self.check_keys(keys)
        taken = []
        for t in sorted(set(tags)):
            if t not in self.q:
                continue
            in_t = tags.count(t)
            assert in_t <= self.q[t]
            mine = [r for r in range(count) if self.rows[r][1] == t]
            x = min(in_t, max(0, len(mine) + in_t - self.q[t]))
            c = self.origin.get(t, 0)
            v = sorted(mine, key=lambda r: (keys[r], (r - c) % count))[:x]
            if v:
                self.origin[t] = v[-1] + 1
            taken += v
        rem = len(ids) - len(taken)
        n_app = min(rem, self.M - count)
        g = rem - n_app
        free = [r for r in range(count) if r not in taken]
        glob = sorted(free, key=lambda r: (keys[r], (r - self.cursor) % count))[:g]
        self.cursor += g
        evicted = [self.rows[r][0] for r in taken + glob]
        slots = list(range(count, count + n_app)) + taken + glob
        for mid, t, slot in zip(ids, tags, slots):
            row = (mid, t, 1.0, now)
            if slot == len(self.rows):
                self.rows.append(row)
            else:
                self.rows[slot] = row
        return evicted

    def compact(self, kill):
        count = len(self.rows)
        start = self.cursor % self.M if count == self.M else 0
        ring = [(start + i) % count for i in range(count)]
        survivors = [r for r in ring if r not in kill]
        pos = {r: i for i, r in enumerate(ring)}
        self.origin = {t: sum(1 for r in survivors if pos[r] < pos[c % count]) for t, c in self.origin.items()}
        self.rows = [self.rows[r] for r in survivors]
        self.cursor = 0


def _scenario(H, hf):
    """A full, wrapped bank of three tags with decayed and reinforced rows and tie origins in mid-bank; the model beside it."""
    M = hf.max_memories
    model = Model(M, {7: 5, 3: 4})
    g = torch.Generator().manual_seed(7)
    tag_cycle = [7, 3, 0, 1, 7, 1, 0]
    n = 0
    for step, b in enumerate([6, 5, 4, 5, 4, 5, 3, 4, 6, 5, 4, 3]):   # 54 rows into 24: the ring wraps
        now = NOW + step * STEP
        H.clock["t"] = now
        ids, tags = _ids(n, n + b), [tag_cycle[(n + j) % 7] for j in range(b)]
        before = set(hf.id_to_idx[m] for m in hf.id_to_idx if hf.id_of_row(hf.id_to_idx[m]) == m)
        hf.create_episodic_memories(ids, torch.randn(b, 16, generator=g), tags=tags)
        model.write(ids, tags, now)
        n += b
        assert [hf.id_of_row(r) for r in range(hf.memory_count)] == [r[0] for r in model.rows], step
        del before
    return model, n, g


def _continue(H, hf, model, n, g, steps=4, first_step=13):
    tag_cycle = [7, 7, 3, 0, 3, 7]
    for step in range(steps):
        now = NOW + (first_step + step) * STEP
        H.clock["t"] = now
        b = 3 + step % 2
        ids, tags = _ids(n, n + b), [tag_cycle[(n + j) % 6] for j in range(b)]
        held = {hf.id_of_row(r) for r in range(hf.memory_count)}
        hf.create_episodic_memories(ids, torch.randn(b, 16, generator=g), tags=tags)
        evicted = model.write(ids, tags, now)
        now_held = {hf.id_of_row(r) for r in range(hf.memory_count)}
        assert held - now_held == set(evicted), (step, sorted(held - now_held), evicted)
        assert [hf.id_of_row(r) for r in range(hf.memory_count)] == [r[0] for r in model.rows]
        assert hf._tag_origin == model.origin and hf._write_cursor == model.cursor
        n += b
    return n


@pytest.mark.parametrize("how", ["forget", "prune", "consolidate"])
def test_origins_are_remapped_by_a_compaction(hmod, how):
    H = hmod
    hf = _hf(H, M=24, tag_quota={7: 5, 3: 4})
    model, n, g = _scenario(H, hf)
    assert hf.memory_count == 24 and hf._write_cursor % 24 != 0 and any(hf._tag_origin.values())
    assert hf._tag_origin == model.origin and hf._write_cursor == model.cursor
    H.clock["t"] = NOW + 12 * STEP
    if how == "forget":
        kill = [1, 2, 9, 17, 23]
        rep = hf.forget(rows=kill)
    elif how == "prune":
        keys = np.asarray(model.keys(NOW + 12 * STEP))
        model.check_keys(list(keys) + [0.2])
        kill = np.nonzero(keys < 0.2)[0].tolist()
        assert 0 < len(kill) < 20
        rep = hf.prune(min_key=0.2, now=NOW + 12 * STEP)
    else:
        kill = []
        rep = hf.consolidate(similarity=0.999, rebuild=False)          # random rows: nothing merges, the ring is put in order
        assert rep.n_merged == 0
    model.compact(set(kill))
    assert hf.memory_count == len(model.rows) and hf._write_cursor == 0
    assert [hf.id_of_row(r) for r in range(hf.memory_count)] == [r[0] for r in model.rows]
    assert hf._tag_origin == model.origin
    _continue(H, hf, model, n, g)


def test_checkpoint_round_trip_continues_with_the_same_victims(hmod):
    H = hmod
    hf = _hf(H, M=24, tag_quota={7: 5, 3: 4})
    model, n, g = _scenario(H, hf)
    state = hf.bank_state()
    assert state["tag_quota"] == {"default": None, "tags": {7: 5, 3: 4}} and state["tag_origin"] == model.origin
    other = _hf(H, M=24)                                   # quotas and origins travel with the state
    other.load_state_dict(hf.state_dict())
    other.load_bank_state(state)
    assert dict(other.tag_quotas) == {7: 5, 3: 4} and other._tag_origin == hf._tag_origin
    g2 = torch.Generator()
    g2.set_state(g.get_state())
    import copy
    model2 = copy.deepcopy(model)
    _continue(H, hf, model, n, g)
    _continue(H, other, model2, n, g2)
    assert torch.equal(hf.memory_features, other.memory_features) and torch.equal(hf.memory_metadata, other.memory_metadata)
    # a state without quotas leaves a bank's own quotas alone and starts its origins afresh
    plain_state = {k: v for k, v in state.items() if k not in ("tag_quota", "tag_origin")}
    third = _hf(H, M=24, tag_quota={7: 5})
    third.load_state_dict(hf.state_dict())
    third.load_bank_state(plain_state)
    assert dict(third.tag_quotas) == {7: 5} and third._tag_origin == {}


def test_quota_with_consolidation_within_tags(hmod):
    H = hmod
    hf = _hf(H, M=32, tag_quota={7: 3}, merge_similarity=0.99, merge_within_tags=True)
    e = torch.eye(16)
    hf.create_episodic_memories(["a", "b", "c"], e[:3], tags=7)
    assert hf._tag_origin == {} and hf.tag_counts() == {7: 3}
    H.clock["t"] = NOW + STEP
    # a near-copy of "a" and one new row: the copy is merged (not stored, does not count), "a" is reinforced and touched
    # BEFORE the write ranks the tag, so the one victim is "b" although "a" comes first in the tag's ring
    rep = hf.create_episodic_memories(["a2", "d"], torch.stack([e[0] + 0.01 * e[9], e[3]]), tags=7)
    assert rep.n_merged == 1 and rep.ids == ["a", "d"]
    assert sorted(_held(hf, 7)) == ["a", "c", "d"] and hf.tag_counts() == {7: 3}
    assert float(hf.memory_metadata[hf.id_to_idx["a"], 1]) == float(np.float32(NOW + STEP))
    # a batch of copies alone stores nothing and evicts nothing
    c0 = _new_calls()
    rep = hf.create_episodic_memories(["c2", "d2"], torch.stack([e[2], e[3]]), tags=7)
    assert rep.n_merged == 2 and _new_calls() == c0 and sorted(_held(hf, 7)) == ["a", "c", "d"]


def test_more_scopes_than_one_library_call_takes(hmod):
    """A run of 70 limited tags: the stub takes any number, as ``ops.bank_select_weakest_scoped`` does by chunking."""
    H = hmod
    hf = _hf(H, M=256, tag_quota=1)
    torch.manual_seed(8)
    tags = np.arange(1, 71)
    hf.create_episodic_memories(_ids(0, 70), torch.randn(70, 16), tags=tags)
    hf.create_episodic_memories(_ids(70, 140), torch.randn(70, 16), tags=tags[::-1].copy())
    assert hf.memory_count == 70 and set(hf.tag_counts().values()) == {1}
    assert sorted(hf.id_of_row(r) for r in range(70)) == sorted(_ids(70, 140))
    # (row i of a run takes slot i of the plan, so a row need not land on its own tag's victim: the counts are what holds)
    assert sorted(hf.memory_tags.tolist()) == tags.tolist()


def test_refusals(hmod):
    H = hmod
    for policy in ("reference", "fifo"):
        with pytest.raises(ValueError, match="overflow='weakest'"):
            _hf(H, overflow=policy, tag_quota=4)
        hf = _hf(H, overflow=policy)
        with pytest.raises(ValueError, match="overflow='weakest'"):
            hf.set_tag_quota(3, 4)
        hf.set_tag_quota(3, None)                          # removing a limit that is not there is no error
    for bad in (0, -1, 1.5, True, "4"):
        with pytest.raises(ValueError, match="quota must be an integer >= 1"):
            _hf(H, tag_quota=bad)
        with pytest.raises(ValueError, match="quota must be an integer >= 1"):
            _hf(H, tag_quota={3: bad})
    for bad_tag in (-1, 1 << 24, 2.0, "x"):
        with pytest.raises(ValueError, match="tag must be an integer"):
            _hf(H, tag_quota={bad_tag: 4})
    hf = _hf(H, tag_quota={3: 4})
    with pytest.raises(TypeError):
        hf.tag_quotas[3] = 9                               # a read-only view
    with pytest.raises(ValueError, match="at most quota"):
        hf._plan_slots(5, NOW, tags=np.full(5, 3))         # (a run the write path would have cut)
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    with pytest.raises(ValueError, match="tag_quota"):
        ShardedHippocampus(hf, total_rows=64, ops_module=stub)
    sh = ShardedHippocampus(_hf(H, overflow="fifo"), total_rows=64, ops_module=stub)
    with pytest.raises(ValueError, match="tag_quota"):
        sh.set_tag_quota(3, 4)
