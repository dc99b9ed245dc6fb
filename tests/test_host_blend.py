"""Host-side logic of blending merges on the CPU (``ops`` replaced by tests/cpu_stub_blend.py, which restates the rule
of ``include/aura_hip.h`` in torch fp32): the argument errors, that a bank without the option makes no new op call, the
order search -> blend -> reinforce -> touch -> write, that the caller's tensor is never written, a multi-chunk stream
and ``consolidate(blend=)`` against the rule bit for bit (scope-blind and within tags), the reports, the layers and a
checkpoint round trip."""
import inspect

import numpy as np
import pytest
import torch

from tests import cpu_stub_blend as stub

NOW = 1.7e9 + 21.0
TAU = 0.99


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    for log in (stub.FIND_SIZES, stub.MOVES, stub.STAMPS, stub.SCOPED_FINDS, stub.BLENDS):
        log.clear()
    return H


def _hf(H, D=16, M=64, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _ids(a, b, p="m"):
    return [f"{p}{i}" for i in range(a, b)]


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


def _groups(n_groups, copies, extra, D=16, seed=3, noise=0.01):
    """``n_groups`` groups of ``copies`` near-copies (cosine ~0.9999 inside a group, far below TAU between groups) and
    ``extra`` rows of their own, shuffled: ``(rows, label)``."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n_groups, D, generator=g)
    rows = base.repeat_interleave(copies, 0) + noise * torch.randn(n_groups * copies, D, generator=g)
    rows = torch.cat([rows, torch.randn(extra, D, generator=g)])
    label = torch.cat([torch.arange(n_groups).repeat_interleave(copies), n_groups + torch.arange(extra)])
    perm = torch.randperm(rows.shape[0], generator=g)
    return rows[perm].contiguous(), label[perm]


def _model_stream(rows, beta, chunk, tau=TAU, tags=None):
    """The blended stream by the rule alone: chunks of ``chunk`` rows, decisions by the fp64 rule of
    tests/cpu_stub_consolidate.py against the model's current rows (within tags when ``tags`` is given), the blend by
    ``stub.blend_reference``.  Returns ``(held rows [k, D] fp32, stream index of every held row, memories moved)``."""
    D = rows.shape[1]
    bank = torch.zeros(rows.shape[0], D)
    inv = torch.zeros(rows.shape[0])
    meta = torch.zeros(rows.shape[0], 4)
    origin, count, moved = [], 0, 0
    for lo in range(0, rows.shape[0], chunk):
        f = rows[lo:lo + chunk]
        if tags is None:
            st, ld, _ = stub.find_repeats_reference(bank, inv, count, f, tau)
        else:
            st, ld, _ = stub.find_repeats_scoped_reference(bank, inv, meta, count, f,
                                                           torch.as_tensor(tags[lo:lo + chunk], dtype=torch.int32), tau)
        held, batch = stub.blend_reference(bank, f, st.numpy(), ld.numpy(), beta, count)
        moved += len(held) + len(batch)
        for r, g in held.items():
            bank[r] = g
            inv[r] = 1.0 / g.norm().clamp_min(1e-12)
        f = f.clone()
        for j, g in batch.items():
            f[j] = g
        for i in torch.nonzero((st < 0) & (ld < 0)).flatten().tolist():
            bank[count] = f[i]
            inv[count] = 1.0 / f[i].norm().clamp_min(1e-12)
            if tags is not None:
                meta[count, 3] = float(tags[lo + i])
            origin.append(lo + i)
            count += 1
    return bank[:count], origin, moved


def _same_bank(a, b):
    assert a.memory_count == b.memory_count
    n = a.memory_count
    assert [a.id_of_row(r) for r in range(n)] == [b.id_of_row(r) for r in range(n)]
    for name in ("memory_features", "memory_locations", "memory_metadata"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a._inv_norm[:n], b._inv_norm[:n]) and a.id_to_idx == b.id_to_idx


# ------------------------------------------------------------------------------------- the rule itself
def test_the_rule_on_hand_made_rows():
    g = torch.Generator().manual_seed(1)
    bank, feats = torch.randn(5, 8, generator=g), torch.randn(7, 8, generator=g)
    stored = [3, -1, -1, 3, -1, 9, -1]                  # rows 0 and 3 repeat held row 3; row 5 names a row outside
    leader = [-1, -1, 1, -1, 1, -1, 2]                  # rows 2 and 4 follow batch row 1; row 6 names a repeat: ignored
    assert stub.group_keys(stored, leader, 5).tolist() == [3, -1, -3, 3, -3, -1, -1]
    for beta in (0.25, 0.5, 1.0):
        held, batch = stub.blend_reference(bank, feats, stored, leader, beta, 5)
        assert set(held) == {3} and set(batch) == {1}
        b = torch.tensor(beta)
        g3 = bank[3] + b * (feats[0] - bank[3])
        g3 = g3 + b * (feats[3] - g3)
        g1 = feats[1] + b * (feats[2] - feats[1])
        g1 = g1 + b * (feats[4] - g1)
        assert torch.equal(held[3], g3) and torch.equal(batch[1], g1)
    # the order matters away from one half: the chain in descending order ends elsewhere
    held, _ = stub.blend_reference(bank, feats, stored, leader, 0.25, 5)
    rev = stub.blend_step(stub.blend_step(bank[3], feats[3], 0.25), feats[0], 0.25)
    assert not torch.equal(held[3], rev)
    # and it is the update it claims to be: the fp64 value of the same expression, to fp32 rounding
    once = (bank[3].double() + 0.25 * (feats[0].double() - bank[3].double())).float()
    assert torch.allclose(stub.blend_step(bank[3], feats[0], 0.25), once, atol=1e-6)


# ------------------------------------------------------------------------------------- validation
def test_argument_errors(hmod):
    for bad in (0.0, -0.5, 1.5, float("nan"), "x", True):
        with pytest.raises(ValueError, match="merge_blend"):
            _hf(hmod, merge_similarity=0.9, merge_blend=bad)
    with pytest.raises(ValueError, match="merge threshold"):
        _hf(hmod, merge_blend=0.5)                              # blending without a merge threshold
    hf = _hf(hmod)
    f = torch.randn(3, 16, generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="merge threshold"):
        hf.create_episodic_memories(_ids(0, 3), f, merge_blend=0.5)
    with pytest.raises(ValueError, match="merge_blend"):
        hf.create_episodic_memories(_ids(0, 3), f, merge_similarity=0.9, merge_blend=2.0)
    with pytest.raises(ValueError, match="merge_blend"):
        hf.create_episodic_memory("a", "e", f[0], merge_similarity=0.9, merge_blend=0.0)
    assert hf.memory_count == 0 and stub.CALLS["blend"] == 0
    hf.create_episodic_memories(_ids(0, 3), f)
    with pytest.raises(ValueError, match="merge_blend"):
        hf.consolidate(0.9, blend=1.25)
    with pytest.raises(ValueError):
        hf.consolidate(blend=0.5)                               # no threshold anywhere
    assert hf.memory_count == 3 and stub.CALLS["blend"] == 0
    # the keywords are defaults behind the existing ones
    H = hmod.HippocampalFormation
    assert inspect.signature(H.__init__).parameters["merge_blend"].default is None
    assert inspect.signature(H.consolidate).parameters["blend"].default is None
    for fn in (H.create_episodic_memories, H.create_episodic_memory):
        assert inspect.signature(fn).parameters["merge_blend"].default is hmod._INSTANCE_DEFAULT
    assert _hf(hmod, merge_similarity=0.9, merge_blend=1.0).merge_blend == 1.0


def test_the_sharded_bank_refuses_to_blend(hmod):
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    with pytest.raises(ValueError, match="does not blend"):
        ShardedHippocampus(_hf(hmod, merge_similarity=0.9, merge_blend=0.5), 64, ops_module=stub)
    sh = ShardedHippocampus(_hf(hmod), 64, ops_module=stub)
    with pytest.raises(ValueError, match="does not blend"):
        sh.write(_ids(0, 2), torch.randn(2, 16), merge_blend=0.5)
    assert sh.memory_count == 0


# ------------------------------------------------------------------------------------- off means off
def test_without_the_option_no_new_op_is_called(hmod, monkeypatch):
    rows, _ = _groups(6, 3, 10)
    names = ("bank_write", "find_repeats", "bank_touch", "bank_reinforce", "bank_compact", "bank_blend")
    log = _record(monkeypatch, *names)
    a = _hf(hmod, merge_similarity=TAU)
    rep = a.create_episodic_memories(_ids(0, 28), rows)
    assert rep.n_merged == 12 and rep.n_blended == 0
    a.bulk_write(rows[:8] * 2.0)
    crep = a.consolidate()
    assert crep.n_merged == 8 and crep.n_blended == 0
    assert stub.CALLS["blend"] == 0 and "bank_blend" not in [c[0] for c in log]
    # a bank built with a rate, switched off per call (merging off, or the rate None), makes the same calls with the
    # same arguments
    plain = list(log)
    del log[:]
    b = _hf(hmod, merge_similarity=TAU, merge_blend=0.5)
    b.create_episodic_memories(_ids(0, 28), rows, merge_blend=None)
    b.bulk_write(rows[:8] * 2.0)
    b.merge_blend = None                                                 # (consolidate's blend=None is the bank's rate)
    b.consolidate()
    assert [c[0] for c in log] == [c[0] for c in plain] and stub.CALLS["blend"] == 0
    for (_, a0, k0), (_, a1, k1) in zip(plain, log):
        assert len(a0) == len(a1) and k0.keys() == k1.keys()
        for x, y in zip(list(a0) + list(k0.values()), list(a1) + list(k1.values())):
            if isinstance(x, torch.Tensor):
                assert torch.equal(x, y)
            elif isinstance(x, np.ndarray):
                assert np.array_equal(x, y)
            else:
                assert x == y
    _same_bank(a, b)
    # merging switched off per call stores every row, whatever the bank's rate
    c = _hf(hmod, merge_similarity=TAU, merge_blend=0.5)
    assert c.create_episodic_memories(_ids(0, 28), rows, merge_similarity=None) is None
    assert c.memory_count == 28 and stub.CALLS["blend"] == 0


# ------------------------------------------------------------------------------------- the launch order
def test_search_blend_reinforce_touch_write(hmod, monkeypatch):
    g = torch.Generator().manual_seed(5)
    base = torch.randn(4, 16, generator=g)
    hf = _hf(hmod, merge_similarity=TAU, merge_blend=0.25)
    hf.create_episodic_memories(_ids(0, 2), base[:2])
    assert stub.CALLS["blend"] == 0                                      # nothing repeated anything: no launch
    log = _record(monkeypatch, "find_repeats", "bank_blend", "bank_reinforce", "bank_touch", "bank_write")
    batch = torch.stack([base[0] * 1.5 + 0.001 * base[3],               # 0: repeats held row 0
                         base[2],                                        # 1: new, kept
                         base[2] * 2.0 + 0.001 * base[3],                # 2: repeats batch row 1
                         base[3],                                        # 3: new, kept
                         base[0] * 0.5 - 0.001 * base[3]])               # 4: repeats held row 0
    caller = batch.clone()
    held0 = hf.memory_features[0].clone()
    rep = hf.create_episodic_memories(_ids(2, 7), batch)
    assert [c[0] for c in log] == ["find_repeats", "bank_blend", "bank_reinforce", "bank_touch", "bank_write"]
    assert torch.equal(batch, caller), "the caller's tensor was written"
    _, a, kw = log[1]
    assert a[2] == 2 and a[3].tolist() == [0, -1, -1, -1, 0] and a[4].tolist() == [-1, -1, 1, -1, -1] and a[5] == 0.25
    assert kw["feats"].data_ptr() == batch.data_ptr() and kw["out"].data_ptr() != batch.data_ptr()
    assert kw["feats_row0"] == -1 and set(kw) == {"feats", "out", "feats_row0"}
    # the write stores the BLENDED leader and the untouched kept row; the held target moved by the chain 0, then 4
    written = log[4][1][4]
    g1 = stub.blend_step(batch[1], batch[2], 0.25)
    assert torch.equal(written, torch.stack([g1, batch[3]]))
    g0 = stub.blend_step(stub.blend_step(held0, batch[0], 0.25), batch[4], 0.25)
    assert torch.equal(hf.memory_features[:4], torch.stack([g0, base[1], g1, batch[3]]))
    assert hf._inv_norm[0] == 1.0 / g0.norm() and hf._inv_norm[2] == 1.0 / g1.norm()
    assert (rep.n_stored, rep.n_merged, rep.n_blended) == (2, 3, 2) and rep.ids == ["m0", "m3", "m3", "m5", "m0"]
    # metadata: the blend touched nothing; reinforce / touch did what they do without it
    assert hf.memory_metadata[0, 0].item() == 1.0 and hf.memory_metadata[:4, 3].tolist() == [0.0] * 4
    # one row through create_episodic_memory, with the rate given per call
    one = hf.create_episodic_memory("x", "e", base[1] * 3.0, merge_blend=1.0)
    assert one.n_blended == 1 and torch.equal(hf.memory_features[1], stub.blend_step(base[1], base[1] * 3.0, 1.0))
    assert stub.BLENDS[-1][2] == 1.0


# ------------------------------------------------------------------------------------- streams against the rule
@pytest.mark.parametrize("beta", [0.25, 0.5, 1.0])
def test_a_multi_chunk_stream_equals_the_rule(hmod, beta):
    rows, label = _groups(40, 6, 1000, seed=11)                          # 1240 rows: two chunks
    hf = _hf(hmod, M=1300, merge_similarity=TAU, merge_blend=beta)
    rep = hf.create_episodic_memories(_ids(0, 1240), rows)
    want, origin, moved = _model_stream(rows, beta, 1024)
    assert stub.FIND_SIZES == [1024, 216] and stub.CALLS["blend"] == 2
    assert hf.memory_count == 1040 == len(origin) and (rep.n_stored, rep.n_merged) == (1040, 200)
    assert torch.equal(hf.memory_features[:1040], want), "not the rule's bits"
    assert [hf.id_of_row(r) for r in range(1040)] == [f"m{i}" for i in origin]
    assert rep.n_blended == moved == sum(b[4] for b in stub.BLENDS)
    # the second chunk merged into rows the first had blended (a held key that was an in-batch leader before)
    first_half = {int(label[i]) for i in range(1024) if label[i] < 40}
    assert any(int(label[i]) in first_half for i in range(1024, 1240) if label[i] < 40)
    # The memories end nearer their six copies' mean than the first copies were.  With independent noise the squared
    # distance to the mean is proportional to sum (w_i - 1/6)^2 over the chain's weights: 5/6 for the first copy (and
    # for beta = 1, which ends at the last copy), 1/6 at beta = 0.5 and 0.025 at 0.25 -- factors 5 and 34; half the
    # first copies' mean 1 - cos is asked of the average over the 40 groups.
    held_label = label[torch.tensor(origin)]
    cos = torch.nn.functional.cosine_similarity
    d_first = d_got = 0.0
    for gid in range(40):
        mean = rows[label == gid].double().mean(0)
        first = rows[min(i for i in range(1240) if label[i] == gid)].double()
        got = hf.memory_features[int(torch.nonzero(held_label == gid)[0])].double()
        d_first += float(1 - cos(first, mean, dim=0))
        d_got += float(1 - cos(got, mean, dim=0))
    if beta < 1.0:
        assert d_got <= 0.5 * d_first, (d_got, d_first)


@pytest.mark.parametrize("slab", [4, 1024])
def test_consolidate_with_blend_equals_the_blended_stream(hmod, monkeypatch, slab):
    monkeypatch.setattr(stub, "CONSOLIDATE_MAX_BATCH", slab)
    rows, _ = _groups(5, 4, 6, seed=13) if slab == 4 else _groups(40, 6, 1000, seed=14)
    n = rows.shape[0]
    hf = _hf(hmod, M=1300)
    hf.bulk_write(rows, id_prefix="m", rebuild=False)
    rep = hf.consolidate(TAU, blend=0.5)
    fresh = _hf(hmod, M=1300)
    wrep = fresh.create_episodic_memories(_ids(0, n), rows, merge_similarity=TAU, merge_blend=0.5)
    want, origin, moved = _model_stream(rows, 0.5, slab)
    k = len(origin)
    assert hf.memory_count == fresh.memory_count == k and rep.n_merged == wrep.n_merged > 0
    assert torch.equal(hf.memory_features[:k], want) and torch.equal(fresh.memory_features[:k], want)
    assert torch.equal(hf.memory_features, fresh.memory_features)                  # the cleared tail included
    assert torch.equal(hf.memory_metadata[:, :2], fresh.memory_metadata[:, :2])    # strengths and timestamps
    assert torch.equal(hf._inv_norm[:k], fresh._inv_norm[:k])
    assert [hf.id_of_row(r) for r in range(k)] == [fresh.id_of_row(r) for r in range(k)] == [f"m{i}" for i in origin]
    assert rep.old_to_new.tolist() == wrep.rows.tolist()
    assert rep.n_blended == wrep.n_blended == moved > 0
    # every slab was blended in place, above the decided prefix
    slabs = [b for b in stub.BLENDS if b[3] >= 0]
    assert all(b[0] <= b[3] and b[2] == 0.5 for b in slabs) and len(slabs) >= 1
    # the bank's own rate is consolidate's default
    own = _hf(hmod, M=1300, merge_similarity=TAU, merge_blend=0.5)
    own.bulk_write(rows, id_prefix="m", rebuild=False)
    assert own.consolidate().n_blended == moved and torch.equal(own.memory_features, hf.memory_features)


def test_within_tags_the_blend_follows_the_search(hmod, monkeypatch):
    monkeypatch.setattr(stub, "CONSOLIDATE_MAX_BATCH", 16)
    rows, label = _groups(6, 4, 8, seed=17)
    n = rows.shape[0]
    tags = (np.arange(n) % 2 + 1).astype(np.int64)                       # copies of one group fall into both tags
    hf = _hf(hmod, merge_similarity=TAU, merge_blend=0.5, merge_within_tags=True)
    rep = hf.create_episodic_memories(_ids(0, n), rows, tags=tags)
    want, origin, moved = _model_stream(rows, 0.5, 16, tags=tags)
    k = len(origin)
    assert hf.memory_count == k and torch.equal(hf.memory_features[:k], want) and rep.n_blended == moved > 0
    assert hf.memory_tags.tolist() == [int(tags[i]) for i in origin]
    assert stub.CALLS["find_repeats_scoped"] == 2 and stub.CALLS["find_repeats"] == 0
    # a group is held once per tag it arrived under, and no memory moved toward a row of another tag
    blind = _model_stream(rows, 0.5, 16)[1]
    assert k > len(blind)
    # consolidate(within_tags, blend) of the same rows, bulk-written with their tags
    bulk = _hf(hmod)
    bulk.bulk_write(rows, id_prefix="m", rebuild=False, tags=tags)
    crep = bulk.consolidate(TAU, within_tags=True, blend=0.5)
    assert crep.n_kept == k and crep.n_blended == moved and torch.equal(bulk.memory_features[:k], want)
    assert bulk.memory_tags.tolist() == hf.memory_tags.tolist()


# ------------------------------------------------------------------------------------- layers, checkpoints
def test_layers_pass_the_rate_on(hmod):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    g = torch.Generator().manual_seed(19)
    hidden = torch.randn(3, 5, 16, generator=g)
    pooled = hidden.mean(dim=1)
    hf = _hf(hmod, merge_similarity=TAU)

    class Layer(MO.BatchedMemoryMixin):
        hippocampus = hf
    assert Layer().store_memory(hidden).n_blended == 0                               # the bank has no rate
    for layer, scale in ((Layer(), 2.0), (MO.MemoryInjection(hf, 16, num_heads=2), 3.0)):
        before = hf.memory_features[:3].clone()
        rep = layer.store_memory(hidden * scale, merge_blend=0.5)
        assert rep.n_merged == 3 and rep.n_blended == 3
        assert torch.equal(hf.memory_features[:3], stub.blend_step(before, (hidden * scale).mean(dim=1), 0.5))
    rep = MO.store_memory(hf, hidden * 4.0, merge_similarity=0.9, merge_blend=1.0)
    assert rep.n_blended == 3 and stub.BLENDS[-1][2] == 1.0
    hf.bulk_write(pooled * 5.0)
    before = hf.memory_features[:3].clone()
    crep = Layer().consolidate_memory(blend=0.25)
    assert crep.n_merged == 3 and crep.n_blended == 3
    assert torch.equal(hf.memory_features[:3], stub.blend_step(before, pooled * 5.0, 0.25))
    assert MO.MemoryInjection(hf, 16, num_heads=2).consolidate_memory(TAU, blend=0.25).n_blended == 0
    with pytest.raises(ValueError, match="merge_blend"):
        Layer().store_memory(hidden, merge_blend=7.0)


def test_a_checkpoint_round_trip_keeps_the_blended_bank(hmod):
    rows, _ = _groups(8, 5, 20, seed=23)
    hf = _hf(hmod, merge_similarity=TAU, merge_blend=0.5)
    hf.create_episodic_memories(_ids(0, 40), rows[:40])
    other = _hf(hmod, merge_similarity=TAU, merge_blend=0.5)
    other.load_state_dict(hf.state_dict())
    other.load_bank_state(hf.bank_state())
    assert torch.equal(other.memory_features, hf.memory_features) and other.memory_count == hf.memory_count
    # both go on alike: the rest of the stream blends into the same bits
    a = hf.create_episodic_memories(_ids(40, 60), rows[40:])
    b = other.create_episodic_memories(_ids(40, 60), rows[40:])
    assert (a.n_stored, a.n_merged, a.n_blended) == (b.n_stored, b.n_merged, b.n_blended) and a.n_blended > 0
    n = hf.memory_count
    assert other.memory_count == n and other.id_to_idx == hf.id_to_idx
    for name in ("memory_features", "memory_metadata"):
        assert torch.equal(getattr(hf, name), getattr(other, name)), name
    want, origin, _ = _model_stream(rows, 0.5, 40)
    assert torch.equal(hf.memory_features[:len(origin)], want)
