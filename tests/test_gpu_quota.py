"""GPU tests of per-tag quotas: ``aura_bank_tag_counts``, ``aura_bank_select_weakest_scoped`` and
``aura_bank_select_weakest_masked`` checked EXACTLY (same rows, same order) against the rule restated in
tests/cpu_stub_quota.py, from the kernel's own keys; a stream of tagged writes with quotas through the bank; and the C
ABI's argument checks.

The rule (``include/aura_hip.h``, "Per-tag quotas"): a tag's eviction order is (key, (r - origin) mod count) ascending
over ITS rows, a NaN key first; x = min(incoming, max(0, held + incoming - quota)); the global victims are the bank's
eviction order with the tag victims left out."""
import numpy as np
import pytest
import torch

from tests import cpu_stub_quota as Q

pytestmark = pytest.mark.gpu
NOW = 1.7e9 + 777.0
NOW32 = float(np.float32(NOW))


def _meta(count, S, seed):
    """Strengths from four values and timestamps from three buckets (thresholds fall inside ties), a NaN, a negative
    strength and +-0; tags: S == 1 -> one scope that is the whole bank; else scope 0 empty, scope 1 a single row, the
    other scopes share the rows with a tag nobody asks for and with untagged rows."""
    g = torch.Generator().manual_seed(seed)
    meta = torch.zeros(count, 4)
    meta[:, 0] = torch.tensor([0.25, 0.5, 0.75, 1.0])[torch.randint(0, 4, (count,), generator=g)]
    meta[:, 1] = torch.tensor(NOW32) - 128.0 * torch.tensor([0.0, 7.0, 30.0])[torch.randint(0, 3, (count,), generator=g)]
    meta[:, 2] = -1
    if count > 8:
        meta[3, 0], meta[4, 0], meta[5, 0], meta[6, 0] = float("nan"), -0.5, 0.0, -0.0
    scope_tags = [5 + 3 * s for s in range(S)]
    if S == 1:
        meta[:, 3] = float(scope_tags[0])
    else:
        pool = torch.tensor(scope_tags[2:] + [4, 0], dtype=torch.float32) if S > 2 else torch.tensor([4.0, 0.0])
        meta[:, 3] = pool[torch.randint(0, pool.numel(), (count,), generator=g)]
        meta[count // 2, 3] = float(scope_tags[1])
    return meta, scope_tags


def _want(keys, tags, scope_tags, origins, incoming, quotas):
    """The rule, with one sort per distinct origin."""
    orders = {c: Q.eviction_order(keys, c) for c in set(origins)}
    held, xs, victims = [], [], []
    for t, c, n_in, q in zip(scope_tags, origins, incoming, quotas):
        mine = orders[c][tags[orders[c]] == t]
        x = min(n_in, max(0, mine.numel() + n_in - q))
        held.append(mine.numel()); xs.append(x); victims.append(mine[:x].tolist())
    return held, xs, victims


@pytest.mark.parametrize("S", [1, 3, 64, 65])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097, 100_003])
def test_scoped_and_masked_selection_are_exact(dev, count, S):
    from aura_snn_rag_amd import ops
    meta, scope_tags = _meta(count, S, seed=count + S)
    meta_d = meta.to(dev)
    keys = ops.bank_retention_keys(meta_d, count, NOW).cpu()
    tags = Q.held_tags(meta, count)
    got_counts = ops.bank_tag_counts(meta_d, count, scope_tags).cpu()
    assert got_counts.tolist() == Q.tag_counts_reference(meta, count, scope_tags).tolist()
    held_t = got_counts.tolist()
    for shift in range(4):
        # origins 0, count // 2, count - 1 and x = 0, 1, held, held // 2, dealt over the scopes (shifted per round)
        origins = [(0, count // 2, count - 1)[(s + shift) % 3] for s in range(S)]
        incoming, quotas = [], []
        for s in range(S):
            h, mode = held_t[s], (s + shift) % 4
            if mode == 0:
                n_in, q = 2, h + 2                       # x = 0
            elif mode == 1:
                n_in, q = 1, max(h, 1)                   # x = 1 (0 for an empty scope)
            elif mode == 2:
                n_in, q = max(h, 1), max(h, 1)           # x = held
            else:
                n_in, q = h // 2 + 1, h + 1              # x = held // 2
            incoming.append(n_in); quotas.append(q)
        w_held, w_x, w_vic = _want(keys, tags, scope_tags, origins, incoming, quotas)
        packed, bitmap = ops.bank_select_weakest_scoped(meta_d, count, NOW, scope_tags, origins, incoming, quotas)
        held, x, vic = ops.scoped_selection_decode(packed.cpu(), incoming)
        assert held.tolist() == w_held == held_t and x.tolist() == w_x, (count, S, shift)
        assert [v.tolist() for v in vic] == w_vic, (count, S, shift)
        taken = sorted(r for v in w_vic for r in v)
        assert Q.bitmap_rows(bitmap, count).tolist() == taken
        # the global victims skip them
        free = count - len(taken)
        for cursor in (0, count - 1):
            for n in sorted(m for m in {1, free // 3, free} if 1 <= m <= free):
                rows, k = ops.bank_select_weakest_masked(meta_d, count, NOW, cursor, n, bitmap)
                want = Q.masked_reference(keys, cursor, n, taken)
                assert torch.equal(rows.cpu(), want), (count, S, shift, cursor, n)
                assert torch.equal(k.cpu().view(torch.int32), keys[want].view(torch.int32))
    if S == 1:
        assert held_t == [count]                         # the scope that is the whole bank
    else:
        assert held_t[:2] == [0, 1]                      # the empty scope and the scope of a single row


@pytest.mark.parametrize("count", [1, 65, 4097, 100_003])
def test_masked_selection_with_a_clear_bitmap_is_the_unmasked_one(dev, count):
    from aura_snn_rag_amd import ops
    meta, _ = _meta(count, 3, seed=count)
    meta_d = meta.to(dev)
    clear = torch.zeros((count + 31) // 32, dtype=torch.int32, device=dev)
    for cursor in (0, count // 2):
        for n in sorted({1, max(1, count // 7), count}):
            a = ops.bank_select_weakest(meta_d, count, NOW, cursor, n)
            b = ops.bank_select_weakest_masked(meta_d, count, NOW, cursor, n, clear)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    meta_d[:, 0], meta_d[:, 1] = 1.0, NOW32              # a bank of equal keys: the ring
    n = max(1, count // 3)
    a = ops.bank_select_weakest(meta_d, count, NOW, count // 2, n)
    b = ops.bank_select_weakest_masked(meta_d, count, NOW, count // 2, n, clear)
    assert torch.equal(a[0], b[0]) and a[0].cpu().tolist() == [(count // 2 + i) % count for i in range(n)]


def test_tag_counts_equal_bincount(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(5)
    count = 70_001
    meta = torch.zeros(count + 7, 4)
    meta[:, 3] = torch.randint(0, 200, (count + 7,), generator=g).float()
    meta[11, 3], meta[12, 3], meta[13, 3] = -3.0, float(1 << 24), float("nan")     # no tag at all
    want = torch.bincount(Q.held_tags(meta, count).clamp(min=0)[Q.held_tags(meta, count) >= 0], minlength=200)
    scope_tags = list(range(0, 200, 2)) + [100_000]      # 101 scopes: two library calls; one tag nobody carries
    got = ops.bank_tag_counts(meta.to(dev), count, sorted(scope_tags)).cpu()
    assert got.tolist() == [int(want[t]) if t < 200 else 0 for t in sorted(scope_tags)]
    assert ops.bank_tag_counts(meta.to(dev), 0, [1, 2]).tolist() == [0, 0]


@pytest.mark.parametrize("index", [False, True])
def test_a_stream_of_tagged_writes_with_quotas(dev, monkeypatch, index):
    """10 000 x 64, across the 8192-row threshold of the bf16 images and past a full bank.  After every run: the counts
    respect the quotas, the victims are those the rule names from the kernel's keys, and recall (scoped and plain) is
    bit-identical to a bank rebuilt from ``state_dict()`` + ``bank_state()``."""
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core import hippocampal as H
    clock = {"t": NOW}
    monkeypatch.setattr(H.time, "time", lambda: clock["t"])
    M, D = 10_000, 64
    quotas = {1: 300, 2: 60, 3: 1500, 4: 5}

    def make():
        return H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                      device="cuda", use_centroid_index=index, overflow="weakest", tag_quota=quotas)
    hf = make()
    g = torch.Generator().manual_seed(9)
    queries = torch.randn(12, D, generator=g).to(dev)
    q_tags = [1, 2, 3, 4, 5, 0, -1, 1, 2, 3, 4, -1]
    runs = {"n": 0, "tag_victims": 0, "global": 0}
    real_plan, real_write = hf._plan_slots, hf._write_rows

    def plan(n, now=None, tags=None):
        count = hf.memory_count
        if tags is None or count == 0:
            return real_plan(n, now, tags=tags)
        keys = ops.bank_retention_keys(hf.memory_metadata, count, now).cpu()
        held = Q.held_tags(hf.memory_metadata.cpu(), count)
        want = Q.rule_run(keys, held, tags.tolist(), hf._quota_of, dict(hf._tag_origin), hf._write_cursor, M)
        slots, n_app, new_count, cursor = real_plan(n, now, tags=tags)
        assert slots.tolist() == want[0] and (n_app, cursor) == (want[1], want[2]), f"run {runs['n']}: victims differ"
        assert {**hf._tag_origin, **(hf._pending_origins or {})} == want[3]
        runs["tag_victims"] += sum(len(v) for v in want[4].values())
        runs["global"] += len(want[5])
        return slots, n_app, new_count, cursor

    def write(*a, **kw):
        real_write(*a, **kw)
        runs["n"] += 1
        counts = hf.tag_counts()
        assert all(counts[t] <= quotas[t] for t in quotas), (runs["n"], counts)
        other = make()
        other.load_state_dict(hf.state_dict())
        other.load_bank_state(hf.bank_state())
        now = clock["t"]
        for kw2 in ({"tags": q_tags}, {}):
            s0, r0 = hf.recall_batch(queries, k=5, now=now, **kw2)
            s1, r1 = other.recall_batch(queries, k=5, now=now, **kw2)
            assert torch.equal(r0, r1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)), (runs["n"], kw2)

    monkeypatch.setattr(hf, "_plan_slots", plan)
    monkeypatch.setattr(hf, "_write_rows", write)
    probs = torch.tensor([0.45, 0.15, 0.05, 0.2, 0.004, 0.146])     # tags 0 and 5 are unlimited: they fill the bank
    n = 0
    for step, b in enumerate([3000, 3000, 2500, 2500, 2000, 1500, 900, 700]):   # 16 100 rows into 10 000
        clock["t"] = NOW + 128.0 * 3 * step
        tags = torch.multinomial(probs, b, replacement=True, generator=g).numpy().astype(np.int32)
        hf.create_episodic_memories([f"m{i}" for i in range(n, n + b)], torch.randn(b, D, generator=g), tags=tags)
        n += b
        if step == 2:
            hf.decay(0.4)
            hf.reinforce(torch.arange(0, hf.memory_count, 7), amount=0.3)
    print(f"quota stream (index={index}): {runs}")
    assert hf.memory_count == M and runs["tag_victims"] > 1000 and runs["global"] > 100
    # (a quota is a cap, not a reservation: global victims may have taken rows of a tag under its quota)
    assert all(c <= quotas[t] for t, c in hf.tag_counts().items())


def test_abi_rejects_bad_arguments_without_launching(dev):
    from aura_snn_rag_amd import _lib
    L = _lib.load()
    count, S = 1000, 3
    meta = _meta(count, S, seed=1)[0].to(dev)
    before = meta.clone()
    params = torch.tensor([[5, 8, 11], [0, 1, 2], [2, 2, 2], [1, 1, 1]], dtype=torch.int32, device=dev)
    out = torch.full((2 * S + 12,), -7, dtype=torch.int64, device=dev)
    bitmap = torch.zeros((count + 31) // 32, dtype=torch.int32, device=dev)
    cnt = torch.full((S,), -7, dtype=torch.int32, device=dev)
    nbytes = L.aura_bank_select_weakest_scoped_workspace_bytes(count, S)
    assert nbytes > 8 * count
    assert L.aura_bank_select_weakest_scoped_workspace_bytes(0, S) < 0
    assert L.aura_bank_select_weakest_scoped_workspace_bytes(count, 0) < 0
    assert L.aura_bank_select_weakest_scoped_workspace_bytes(count, 65) < 0
    assert L.aura_bank_select_weakest_masked_workspace_bytes(count, 0) < 0
    assert L.aura_bank_select_weakest_masked_workspace_bytes(count, 10) == L.aura_bank_select_weakest_workspace_bytes(count, 10)
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    m, p, o, bm = meta.data_ptr(), params.data_ptr(), out.data_ptr(), bitmap.data_ptr()

    def scoped(meta_p=m, count_=count, tags_p=p, org_p=p + 12, in_p=p + 24, q_p=p + 36, S_=S, cap=6, held_p=o,
               x_p=o + 8 * S, slots_p=o + 16 * S, comp_p=o + 16 * S + 48, bm_p=bm, ws_p=base, ws_bytes=nbytes):
        return L.aura_bank_select_weakest_scoped(meta_p, count_, NOW, tags_p, org_p, in_p, q_p, S_, cap, held_p, x_p,
                                                 slots_p, comp_p, bm_p, ws_p, ws_bytes, None)
    assert scoped(count_=0) == -1 and scoped(S_=0) == -1 and scoped(S_=65) == -1 and scoped(cap=-1) == -1
    assert scoped(ws_bytes=nbytes - 1) == -1
    for name in ("meta_p", "tags_p", "org_p", "in_p", "q_p", "held_p", "x_p", "slots_p", "comp_p", "bm_p", "ws_p"):
        assert scoped(**{name: None}) == -1, name
    assert scoped(ws_p=base + 4) == -3 and scoped(meta_p=m + 4) == -3

    def counts(meta_p=m, count_=count, tags_p=p, S_=S, out_p=cnt.data_ptr()):
        return L.aura_bank_tag_counts(meta_p, count_, tags_p, S_, out_p, None)
    assert counts(meta_p=None) == -1 and counts(tags_p=None) == -1 and counts(out_p=None) == -1
    assert counts(count_=-1) == -1 and counts(S_=0) == -1 and counts(S_=65) == -1 and counts(meta_p=m + 4) == -3

    n = 10
    slots = torch.full((n,), -7, dtype=torch.int64, device=dev)
    keys = torch.full((n,), -7.0, device=dev)
    mb = L.aura_bank_select_weakest_masked_workspace_bytes(count, n)

    def masked(meta_p=m, count_=count, cursor=0, n_=n, bm_p=bm, s_p=slots.data_ptr(), k_p=keys.data_ptr(), ws_p=base,
               ws_bytes=mb):
        return L.aura_bank_select_weakest_masked(meta_p, count_, NOW, cursor, n_, bm_p, s_p, k_p, ws_p, ws_bytes, None)
    assert masked(n_=0) == -1 and masked(n_=count + 1) == -1 and masked(count_=0) == -1 and masked(cursor=-1) == -1
    assert masked(ws_bytes=mb - 1) == -1 and masked(ws_p=base + 4) == -3
    for name in ("meta_p", "bm_p", "s_p", "k_p", "ws_p"):
        assert masked(**{name: None}) == -1, name
    torch.cuda.synchronize()
    assert torch.equal(meta.view(torch.int32), before.view(torch.int32))          # (bits: the table holds a NaN)
    assert bool((out == -7).all()) and bool((cnt == -7).all())
    assert bool((slots == -7).all()) and bool((keys == -7.0).all()) and not bool(bitmap.any()) and not bool(ws.any())
    # and the same calls with good arguments work
    assert scoped() == 0 and counts() == 0 and masked() == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 1, int((meta[:, 3] == 11).sum())] and out[:S].tolist() == cnt.tolist()
