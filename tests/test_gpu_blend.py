"""GPU tests of blending merges (``aura_bank_blend`` and everything above it) against the rule restated in torch fp32
on the CPU (tests/cpu_stub_blend.py): ``g = g + beta * (f - g)`` as ``torch.sub``, ``torch.mul``, ``torch.add``, which is
bit-exact with the kernel by definition.  Everything below is compared on the bits.

Kernel.  Hand-made valid ``stored_target`` / ``batch_leader`` at D = 768 (16-byte accesses, a bf16 shadow with its
watermark inside the bank and a list-sorted image), 100 (16-byte accesses, no image), 50 (4-byte accesses) and 4096 on a
64-row bank (16 KB of LDS per wave), n = 1, 64 and 1024, beta = 0.25, 0.5 and 1: held targets with members at scattered
batch positions on both sides of the shadow's watermark, in-batch leaders with followers, both kinds in one call.  The
derived state is compared with what the library's own kernels compute from the blended bank: ``bank_row_norms``,
``bank_shadow_update`` and ``bank_shadow_sorted`` rebuilt from scratch on copies.

End to end.  The stream of tests/test_gpu_consolidate.py cut to 10 000 rows (seed 7: 480 groups of 6 near-copies at
``group + 0.05 randn``, the rest ``randn``, shuffled), tau = 0.9, beta = 0.5.  The fp64 model
(``cpu_stub_blend.BlendedBank``) first asserts what the device may be judged by: every decision of every chunk lies at
least 0.05 from tau against the model's current (blended) rows (measured on the CPU: 0.098), and no row has two
candidates within tol = 2 (D + 8) 2^-24 of each other.  Then: 7600 kept, 2400 merged, the model's feature bits, every
group's memory at most half as far (1 - cos) from its six copies' mean as the first copy (measured factor: at least
4.09), and every recall path bit-identical to a bank rebuilt from ``state_dict()`` + ``bank_state()``.  The banks of
these tests keep their bf16 images from 2048 rows on (``SHADOW_MIN_ROWS`` lowered on the instance): 7600 rows would
otherwise never reach the image whose upkeep by the blend is the point.

Sequence.  30 seeded steps over a 10 000-row bank (D = 64, 256 centroids, the pool of tests/bank_model.py) that crosses
8192 rows downwards and upwards: blended writes, recalls that reinforce, ``forget``, ``consolidate(blend=)``, a
checkpoint round trip; after every step the model's feature bits and the rebuilt-bank comparison.  There the model asks
for decisions at least 0.01 from tau (half the pool's own gap, ``bank_model.GAP``; tol is 8.6e-6 at D = 64)."""
import numpy as np
import pytest
import torch

from tests import bank_model as B
from tests import cpu_stub_blend as R
from tests import helpers

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
TAU, BETA = 0.9, 0.5
D, N = 768, 10_000
TOL = R.tolerance(D)
_bits = B._bits


@pytest.fixture(scope="module")
def hmod():
    from aura_snn_rag_amd.core import hippocampal as H
    clock = B.Clock()
    mp = pytest.MonkeyPatch()
    mp.setattr(H.time, "time", clock)
    yield H, clock
    mp.undo()


# ------------------------------------------------------------------------------------- the kernel against the rule
def _hand_made(n, N, rng, upto):
    """Valid ``(stored_target, batch_leader)`` for a batch of n rows against N held rows: targets below and at or above
    the shadow's watermark ``upto`` with members at scattered positions, in-batch leaders with followers."""
    stored = np.full(n, -1, dtype=np.int32)
    leader = np.full(n, -1, dtype=np.int32)
    if n == 1:
        stored[0] = int(rng.integers(0, N))
        return stored, leader
    pos = rng.permutation(n)
    lo_rows = rng.choice(np.arange(0, max(1, min(upto, N))), size=3, replace=False)
    hi_rows = rng.choice(np.arange(min(upto, N - 3), N), size=3, replace=False)
    use = 0
    stored[pos[use:use + 4]] = lo_rows[0]; use += 4             # a target with 4 members at scattered positions
    stored[pos[use:use + 2]] = hi_rows[0]; use += 2             # one on the other side of the watermark
    grp = np.sort(pos[use:use + 4]); use += 4                   # an in-batch key with 3 followers
    leader[grp[1:]] = grp[0]
    if n >= 1024:                                               # more of each, of 1 .. 5 members
        for r in (lo_rows[1], lo_rows[2], hi_rows[1], hi_rows[2]):
            k = int(rng.integers(1, 6))
            stored[pos[use:use + k]] = r; use += k
        for _ in range(20):
            k = int(rng.integers(2, 7))
            grp = np.sort(pos[use:use + k]); use += k
            leader[grp[1:]] = grp[0]
    return stored, leader


SHAPES = {768: (3000, 2500), 100: (700, 600), 50: (700, 600), 4096: (64, 64)}          # D: (rows of the bank, held)


@pytest.mark.parametrize("beta", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 64, 1024])
@pytest.mark.parametrize("dim", [768, 100, 50, 4096])
def test_kernel_equals_the_rule(dev, dim, n, beta):
    from aura_snn_rag_amd import ops
    M, held = SHAPES[dim]
    rng = np.random.default_rng([dim, n, int(beta * 100)])
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    bank = torch.randn(M, dim, generator=g).to(dev)
    feats = torch.randn(n, dim, generator=g).to(dev)
    inv = torch.zeros(M, device=dev)
    ops.bank_row_norms(bank, inv, 0, M)
    upto = held // 2 if dim % 8 == 0 else 0                     # the shadow's watermark: inside the held rows
    stored, leader = _hand_made(n, held, rng, upto if upto else held // 2)
    kw, shadow, rho, ivf = {}, None, None, None
    if dim % 8 == 0:
        shadow = torch.zeros(M, dim, dtype=torch.bfloat16, device=dev)
        rho = torch.zeros(M, device=dev)
        ops.bank_shadow_update(bank, inv, shadow, rho, 0, upto)
        kw.update(shadow=shadow, rho=rho, shadow_upto=upto)
    if dim == 768:                                              # a list-sorted image; a fifth of the rows in no list
        cids = torch.from_numpy(rng.integers(-64, 256, size=held).clip(-1)).to(dev)
        ivf = ops.build_ivf2(bank, inv, cids, slack=16, max_rows=M, rho=rho)
        kw.update(sorted_bf16=ivf["sorted_bf16"], sorted_rows=ivf["sorted_rows"], pos_of_row=ivf["pos_of_row"],
                  n_sorted=ivf["n_sorted"])
    before = dict(bank=bank.clone(), rho=None if rho is None else rho.clone(),
                  shadow=None if shadow is None else shadow.clone())
    out = feats.clone()
    st_t, ld_t = torch.from_numpy(stored).to(dev), torch.from_numpy(leader).to(dev)
    ops.bank_blend(bank, inv, held, st_t, ld_t, beta, feats=feats, out=out, **kw)
    torch.cuda.synchronize()
    want_held, want_batch = R.blend_reference(before["bank"], feats, stored, leader, beta, held)
    assert len(want_held) >= 1 and (n == 1 or len(want_batch) >= 1)
    want_bank, want_out = before["bank"].cpu().clone(), feats.cpu().clone()
    for r, row in want_held.items():
        want_bank[r] = row
    for j, row in want_batch.items():
        want_out[j] = row
    assert torch.equal(_bits(bank.cpu()), _bits(want_bank)), "bank rows: not the rule's bits"
    assert torch.equal(_bits(out.cpu()), _bits(want_out)), "blended batch rows: not the rule's bits"
    # 1/||row||: bank_row_norms on a copy of the blended bank
    inv2 = torch.zeros(M, device=dev)
    ops.bank_row_norms(bank.clone(), inv2, 0, M)
    assert torch.equal(_bits(inv), _bits(inv2)), "inv_norm: not bank_row_norms' bits"
    if shadow is not None:
        # the shadow below the watermark: bank_shadow_update on a copy; at or above it nothing was touched
        sh2, rho2 = before["shadow"].clone(), before["rho"].clone()
        ops.bank_shadow_update(bank, inv, sh2, rho2, 0, upto)
        if ivf is not None:                                     # the image: rebuilt from scratch over the same layout
            img2 = torch.zeros_like(ivf["sorted_bf16"])
            ops.bank_shadow_sorted(bank, inv, ivf["sorted_rows"], img2, rho2, None, ivf["n_sorted"])
            ns = ivf["n_sorted"]
            assert torch.equal(_bits(ivf["sorted_bf16"][:ns]), _bits(img2[:ns])), "the sorted image: not the rebuilt bits"
        assert torch.equal(_bits(shadow), _bits(sh2)), "the shadow: not bank_shadow_update's bits"
        assert torch.equal(_bits(rho), _bits(rho2)), "rho: not the conversion kernels' bits"
        assert torch.equal(_bits(shadow[upto:]), _bits(before["shadow"][upto:])), "a row at or above the watermark moved"
        above = [r for r in want_held if r >= upto]
        below = [r for r in want_held if r < upto]
        assert n == 1 or (above and below), "targets on both sides of the watermark"
        if ivf is None and above:
            assert torch.equal(_bits(rho[above]), _bits(before["rho"][above]))
        if below:
            assert not torch.equal(_bits(shadow[below]), _bits(before["shadow"][below])), "the shadow did not follow"


def test_entries_out_of_range_are_ignored(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(4)
    bank, feats = torch.randn(40, 64, generator=g).to(dev), torch.randn(8, 64, generator=g).to(dev)
    inv = torch.zeros(40, device=dev)
    ops.bank_row_norms(bank, inv, 0, 40)
    # held rows: 30.  Row 0 names a row outside the held set, row 2 a leader that is not earlier, row 4 a leader that
    # is itself a repeat, row 6 a negative leader below -1; rows 1 and 5 are a valid pair around them.
    stored = np.array([30, 7, -1, -1, -1, 7, -1, -5], dtype=np.int32)
    leader = np.array([-1, -1, 2, -1, 1, -1, -9, 3], dtype=np.int32)
    b0, out = bank.clone(), feats.clone()
    ops.bank_blend(bank, inv, 30, torch.from_numpy(stored).to(dev), torch.from_numpy(leader).to(dev), 0.5, feats=feats,
                   out=out)
    held, batch = R.blend_reference(b0, feats, stored, leader, 0.5, 30)
    assert set(held) == {7} and set(batch) == {3}
    want, want_out = b0.cpu().clone(), feats.cpu().clone()
    want[7], want_out[3] = held[7], batch[3]
    assert torch.equal(_bits(bank.cpu()), _bits(want)) and torch.equal(_bits(out.cpu()), _bits(want_out))
    for bad in (dict(beta=0.0), dict(beta=1.5), dict(out=feats), dict(rho=torch.zeros(40, device=dev)),
                dict(feats_row0=10), dict(sorted_bf16=torch.zeros(48, 64, dtype=torch.bfloat16, device=dev))):
        args = dict(beta=0.5, feats=feats, out=out)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.bank_blend(bank, inv, 30, torch.from_numpy(stored).to(dev), torch.from_numpy(leader).to(dev), **args)


@pytest.mark.parametrize("dim,beta", [(768, 0.25), (100, 0.5), (50, 1.0)])
def test_a_slab_of_the_bank_is_blended_in_place(dev, dim, beta):
    """``feats_row0 >= 0``: the batch is bank rows [row0, row0 + n), the held rows lie below; blended leaders are
    written where they stand, with their norms and shadow rows."""
    from aura_snn_rag_amd import ops
    M, held, row0, n = 2200, 900, 1000, 1024
    rng = np.random.default_rng([dim, 7])
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    bank = torch.randn(M, dim, generator=g).to(dev)
    inv = torch.zeros(M, device=dev)
    ops.bank_row_norms(bank, inv, 0, M)
    stored, leader = _hand_made(n, held, rng, held // 2)
    kw = {}
    if dim % 8 == 0:
        shadow, rho = ops.make_shadow(bank, inv)
        kw = dict(shadow=shadow, rho=rho, shadow_upto=M)
    b0 = bank.clone()
    ops.bank_blend(bank, inv, held, torch.from_numpy(stored).to(dev), torch.from_numpy(leader).to(dev), beta,
                   feats_row0=row0, **kw)
    want_held, want_batch = R.blend_reference(b0, b0[row0:row0 + n], stored, leader, beta, held)
    want = b0.cpu().clone()
    for r, row in want_held.items():
        want[r] = row
    for j, row in want_batch.items():
        want[row0 + j] = row
    assert len(want_batch) >= 21 and torch.equal(_bits(bank.cpu()), _bits(want)), "the slab: not the rule's bits"
    inv2 = torch.zeros(M, device=dev)
    ops.bank_row_norms(bank, inv2, 0, M)
    assert torch.equal(_bits(inv), _bits(inv2))
    if kw:
        sh2, rho2 = ops.make_shadow(bank, inv)
        assert torch.equal(_bits(kw["shadow"]), _bits(sh2)) and torch.equal(_bits(kw["rho"]), _bits(rho2))


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
    feats, label = feats[perm].contiguous(), label[perm]
    q = groups[torch.randint(0, 480, (32,), generator=g)] + 0.3 * torch.randn(32, D, generator=g)
    return feats, label, q.contiguous()


_MODELS = {}


def _model(data, dev, batch, tags=None):
    """The fp64 model of the stream in batches of ``batch`` (computed once per batch size), with the conditions under
    which the device may be judged asserted from the model alone."""
    key = (batch, tags is not None)
    if key not in _MODELS:
        feats = data[0]
        m = R.BlendedBank(D, N, device=dev, tol=TOL)
        for lo in range(0, N, batch):
            m.write(feats[lo:lo + batch], list(range(lo, min(N, lo + batch))), TAU, BETA,
                    None if tags is None else tags[lo:lo + batch])
        print(f"model batch={batch} tags={tags is not None}: {m.count} kept, {m.merged} merged, {m.moved} blends, "
              f"smallest distance of a decision from tau {m.min_margin:.4f}, {m.near_ties} near-ties")
        assert m.min_margin >= 0.05, f"a decision lies {m.min_margin} from tau"
        assert m.near_ties == 0, "two candidate targets of a row lie within tol of each other"
        _MODELS[key] = m
    return _MODELS[key]


def _hf(H, dim=D, M=N, **kw):
    kw.setdefault("use_centroid_index", False)
    hf = H.HippocampalFormation(feature_dim=dim, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                device="cuda", **kw)
    hf.SHADOW_MIN_ROWS = 2048                           # the images live from 2048 rows on (see the module docstring)
    return hf


def _rebuilt(hf, make):
    new = make()
    new.load_state_dict(hf.state_dict())
    new.load_bank_state(hf.bank_state())
    return new


def _same_recalls(hf, fresh, q, now, indexed):
    """Every recall path of ``hf`` against the bank rebuilt from its checkpoint, bit for bit; then the derived state."""
    n = hf.memory_count
    loc = torch.zeros(q.shape[0], hf.memory_locations.shape[1], device=q.device)
    paths = [("two-stage", q, dict(use_candidates=False)),
             ("dense", q, dict(use_candidates=False, locations=loc)),
             ("scoped", q, dict(min_strength=0.5)),
             ("scoped tag 0", q, dict(tags=0)),
             ("diverse", q, dict(diversity=0.3, max_similarity=0.9, fetch_k=32))]
    if indexed:
        assert hf._candidate_mode() and fresh._candidate_mode()
        paths.append(("index", q, dict(use_candidates=True)))
        if q.is_cuda:                                   # more than MASKED_SCAN_MAX_QUERIES queries: the inverted lists
            paths.append(("lists", q.repeat(17, 1), dict(use_candidates=True)))
    for name, qq, kw in paths:
        s1, r1 = hf.recall_batch(qq, k=8, now=now, **kw)
        s2, r2 = fresh.recall_batch(qq, k=8, now=now, **kw)
        assert torch.equal(r1, r2), f"{name}: rows differ from the bank rebuilt from the checkpoint"
        assert torch.equal(_bits(s1), _bits(s2)), f"{name}: score bits differ from the bank rebuilt from the checkpoint"
    hf._ensure_norms(); fresh._ensure_norms()
    assert torch.equal(_bits(hf._inv_norm[:n]), _bits(fresh._inv_norm[:n])), "_inv_norm differs from the rebuilt bank's"
    if hf._shadow is not None and fresh._shadow is not None:
        u = min(hf._shadow_valid_upto, fresh._shadow_valid_upto, n)
        assert torch.equal(_bits(hf._shadow[:u]), _bits(fresh._shadow[:u])), "the bf16 shadow differs from the rebuilt bank's"
        assert torch.equal(_bits(hf._rho[:u]), _bits(fresh._rho[:u])), "rho differs from the rebuilt bank's"
    return len(paths)


def _nearer_the_mean(data, model, held_feats):
    """1 - cos of every group's memory to its six copies' mean against the first copy's: the largest ratio."""
    feats, label, _ = data
    origin = torch.tensor(model.origin)
    held_label = label[origin]
    cos = torch.nn.functional.cosine_similarity
    worst = 0.0
    for gid in range(480):
        members = torch.nonzero(label == gid).flatten()
        mean = feats[members].double().mean(0)
        first = feats[members.min()].double()
        row = torch.nonzero(held_label == gid).flatten()
        assert row.numel() == 1 and int(origin[row]) == int(members.min()), "one memory per group: its first copy's slot"
        got = held_feats[int(row)].double()
        worst = max(worst, float(1 - cos(got, mean, dim=0)) / float(1 - cos(first, mean, dim=0)))
    return worst


@pytest.mark.parametrize("index", [False, True], ids=["exact", "index"])
@pytest.mark.parametrize("batch", [256, 1024])
def test_a_blended_stream(dev, hmod, data, batch, index):
    H, clock = hmod
    clock.now = NOW
    feats, label, q = data
    model = _model(data, dev, batch)
    assert model.count == 7600 and model.merged == 2400
    make = lambda: _hf(H, use_centroid_index=index, merge_similarity=TAU, merge_blend=BETA)   # noqa: E731
    hf = make()
    torch.manual_seed(3)
    n_merged = n_blended = 0
    for lo in range(0, N, batch):
        rep = hf.create_episodic_memories([f"r{i}" for i in range(lo, min(N, lo + batch))], feats[lo:lo + batch].to(dev))
        n_merged, n_blended = n_merged + rep.n_merged, n_blended + rep.n_blended
    assert hf.memory_count == 7600 and n_merged == 2400 and n_blended == model.moved
    assert [hf.id_of_row(r) for r in (0, 7599)] == [f"r{model.origin[0]}", f"r{model.origin[-1]}"]
    held = hf.memory_features[:7600].cpu()
    same = (_bits(held) == _bits(model.feats[:7600])).all(1)
    helpers.record_parity(f"blended stream batch={batch} {'index' if index else 'exact'}", int(same.sum()), 7600,
                          merged=n_merged, blends=n_blended, min_margin=round(model.min_margin, 4))
    assert bool(same.all()), f"{int((~same).sum())} of 7600 rows differ from the model's bits"
    worst = _nearer_the_mean(data, model, held)
    print(f"blended stream batch={batch} index={index}: largest (1 - cos to the mean) / (the first copy's) = {worst:.4f}")
    assert worst <= 0.5, f"a group's memory is {worst} times as far from its copies' mean as the first copy"
    assert hf._shadow is not None or hf._ivf is not None, "no bf16 image was live: the blend's upkeep was not exercised"
    if index:
        assert hf._ivf is not None and hf._index_ready
    _same_recalls(hf, _rebuilt(hf, make), q.to(dev), NOW, index)


def test_consolidate_with_blend_leaves_the_streams_bits(dev, hmod, data):
    H, clock = hmod
    clock.now = NOW
    feats, _, q = data
    model = _model(data, dev, 1024)
    make = lambda: _hf(H, use_centroid_index=False)                                          # noqa: E731
    hf = make()
    hf.bulk_write(feats.to(dev), rebuild=False)
    hf._ensure_shadow()                                  # a live shadow travels with the rows and follows the blend
    rep = hf.consolidate(TAU, blend=BETA)
    assert (rep.n_before, rep.n_kept, rep.n_merged, rep.n_blended) == (N, 7600, 2400, model.moved)
    same = (_bits(hf.memory_features[:7600].cpu()) == _bits(model.feats[:7600])).all(1)
    helpers.record_parity("consolidate(blend) of the bulk-written stream", int(same.sum()), 7600, merged=rep.n_merged,
                          blends=rep.n_blended)
    assert bool(same.all()), f"{int((~same).sum())} of 7600 rows differ from the model's bits"
    assert [hf.id_of_row(r) for r in (0, 7599)] == [f"bulk-{model.origin[0]}", f"bulk-{model.origin[-1]}"]
    assert not bool(hf.memory_features[7600:].any())
    _same_recalls(hf, _rebuilt(hf, make), q.to(dev), NOW, False)


def test_a_blended_stream_within_tags(dev, hmod, data):
    H, clock = hmod
    clock.now = NOW
    feats, label, q = data
    tags = (np.arange(N) % 2 + 1).astype(np.int64)       # every group's copies fall into both tags
    model = _model(data, dev, 1024, tags=tags)
    make = lambda: _hf(H, merge_similarity=TAU, merge_blend=BETA, merge_within_tags=True)    # noqa: E731
    hf = make()
    n_blended = 0
    for lo in range(0, N, 1024):
        rep = hf.create_episodic_memories([f"r{i}" for i in range(lo, min(N, lo + 1024))], feats[lo:lo + 1024].to(dev),
                                          tags=tags[lo:lo + 1024])
        n_blended += rep.n_blended
    k = model.count
    assert 7600 < k < N and hf.memory_count == k and n_blended == model.moved
    same = (_bits(hf.memory_features[:k].cpu()) == _bits(model.feats[:k])).all(1)
    helpers.record_parity("blended stream within tags batch=1024", int(same.sum()), k, blends=n_blended,
                          min_margin=round(model.min_margin, 4))
    assert bool(same.all()), f"{int((~same).sum())} of {k} rows differ from the model's bits"
    assert hf.memory_tags.cpu().tolist() == model.tag[:k].tolist()
    # consolidate(within_tags, blend) of the same rows bulk-written with their tags
    bulk = _hf(H)
    bulk.bulk_write(feats.to(dev), rebuild=False, tags=tags)
    rep = bulk.consolidate(TAU, within_tags=True, blend=BETA)
    assert rep.n_kept == k and rep.n_blended == model.moved
    assert torch.equal(_bits(bulk.memory_features[:k].cpu()), _bits(model.feats[:k]))
    _same_recalls(hf, _rebuilt(hf, make), q.to(dev), NOW, False)


# ------------------------------------------------------------------------------------- a short seeded sequence
SEQ_D, SEQ_M, SEQ_STEPS, LIVE = 64, 10_000, 30, 8192


def _sequence_plan():
    """30 steps; sizes chosen so that the bank crosses 8192 rows downwards (a forget) and upwards (blended writes)."""
    return [("bulk", 9500), ("consolidate",), ("write", 300), ("recall",), ("forget", 1200), ("write", 64), ("recall",),
            ("write", 1500), ("checkpoint",), ("write", 300), ("bulk", 400), ("consolidate",), ("recall",),
            ("forget", 2000), ("write", 7), ("write", 1100), ("write", 1), ("recall",), ("bulk", 300), ("consolidate",),
            ("checkpoint",), ("write", 300), ("forget", 1500), ("write", 64), ("recall",), ("write", 500),
            ("consolidate",), ("write", 300), ("recall",), ("write", 33)]


def test_a_seeded_sequence(dev, hmod):
    H, clock = hmod
    run_sequence(H, clock, dev)


def run_sequence(H, clock, dev):
    """The sequence on ``dev`` (the CPU with ``H.ops`` replaced by tests/cpu_stub_blend.py replays it without a GPU)."""
    clock.now = B.T0
    pool = B.pool_for(SEQ_D, 22_000, 400, 0, dev)
    q = pool.queries
    rng = np.random.default_rng(29)
    torch.manual_seed(29)

    def make():
        hf = H.HippocampalFormation(feature_dim=SEQ_D, max_memories=SEQ_M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                    device=str(dev), use_centroid_index=True, merge_similarity=B.TAU, merge_blend=BETA)
        hf.centroids_update_interval = 1024
        return hf

    hf = make()
    model = R.BlendedBank(SEQ_D, SEQ_M, device=dev, tol=R.tolerance(SEQ_D))
    plan = _sequence_plan()
    assert len(plan) == SEQ_STEPS
    counts, next_id, live_blends, checked = [], 0, 0, 0
    for step, op in enumerate(plan):
        clock.now = B.T0 + 128.0 * (step + 1)
        kind = op[0]
        if kind in ("bulk", "write"):
            n = op[1]
            f = pool.take(n)
            names = list(range(next_id, next_id + n))
            next_id += n
            if kind == "bulk":
                hf.bulk_write(f, id_prefix="b", first_index=names[0], rebuild=(step == 0))
                model.bulk(f, names)
            else:
                image = hf._shadow is not None or (hf._ivf is not None and hf._ivf.valid)
                rep = hf.create_episodic_memories([f"w{i}" for i in names], f)
                before = model.moved
                model.write(f, names, B.TAU, BETA)
                assert rep.n_blended == model.moved - before and hf.memory_count == model.count, f"step {step}: {op}"
                live_blends += int(image and rep.n_blended > 0)
        elif kind == "consolidate":
            before = model.moved
            rep = hf.consolidate(blend=BETA)
            model.consolidate(B.TAU, BETA)
            assert (rep.n_kept, rep.n_blended) == (model.count, model.moved - before), f"step {step}: {op}"
        elif kind == "forget":
            kill = rng.choice(model.count, size=op[1], replace=False)
            hf.forget(rows=kill)
            model.forget(kill)
        elif kind == "recall":
            hf.recall_batch(q, k=8, now=clock.now, reinforce=0.05)
        elif kind == "checkpoint":
            hf = _rebuilt(hf, make)
        counts.append(model.count)
        n = model.count
        assert model.min_margin >= 0.01 and model.near_ties == 0, f"step {step} {op}: the model's decisions are too " \
            f"close to call ({model.min_margin} from tau, {model.near_ties} near-ties)"
        assert hf.memory_count == n, f"step {step}: {op}"
        same = (_bits(hf.memory_features[:n].cpu()) == _bits(model.feats[:n])).all(1)
        assert bool(same.all()), f"step {step} {op}: {int((~same).sum())} of {n} rows differ from the model's bits"
        assert not bool(hf.memory_features[n:].any())
        checked += _same_recalls(hf, _rebuilt(hf, make), q, clock.now, hf._candidate_mode())
    print(f"sequence: counts {counts}; smallest distance of a decision from tau {model.min_margin:.4f}; "
          f"{model.near_ties} near-ties; {model.moved} blends, {live_blends} blending writes over a live image")
    helpers.record_parity("blend sequence D=64 index", checked, checked, blends=model.moved,
                          min_margin=round(model.min_margin, 4))
    down = any(a >= LIVE > b for a, b in zip(counts, counts[1:]))
    up = any(a < LIVE <= b for a, b in zip(counts, counts[1:]))
    assert down and up, f"the bank never crossed {LIVE} rows both ways: {counts}"
    assert live_blends >= 3, "too few blending writes met a live bf16 image"
