"""Replay on the GPU: the uniforms against the NumPy Philox bit for bit, the draw keys against the rule in fp64 within
the bound the number formats give, the selection exactly from the kernel's own keys (fp32 ties are real: the sample is
the top n of ``bank_replay_keys`` by (d descending, row ascending), never compared with fp64 directly), the product
paths (``HippocampalFormation.replay``, the layers) and the ABI's refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import cpu_stub_replay as R

pytestmark = pytest.mark.gpu

NOW = 1.7e9
NOW32 = float(np.float32(NOW))
COUNTS = [1, 63, 64, 65, 4097, 100_003]
PRIORITIES = ["key", "strength", "uniform"]
ALPHAS = [0.0, 1.0, 2.5]
# tags: 9 = an empty scope, 11 = a single row, 0 / 3 / 5 / 7 shared, 13 = carried but never asked for
SCOPES = [{}, {"tags": [9]}, {"tags": 11}, {"tags": [0, 3, 5], "older_than": NOW32 - 128.0},
          {"tags": 7, "min_strength": 0.5, "newer_than": NOW32 - 128.0}]


def _meta(count, seed):
    """Strengths from a handful of values plus a NaN, a negative, +0, -0 and +inf; timestamps from three 128-s buckets
    plus one NaN; tags as listed above."""
    g = torch.Generator().manual_seed(seed)
    meta = torch.zeros(count, 4)
    meta[:, 0] = torch.tensor([0.05, 0.25, 0.5, 0.75, 1.0, 2.0])[torch.randint(0, 6, (count,), generator=g)]
    meta[:, 1] = torch.tensor(NOW32) - 128.0 * torch.randint(0, 3, (count,), generator=g).float()
    meta[:, 2] = -1
    meta[:, 3] = torch.tensor([0.0, 3.0, 5.0, 7.0, 13.0])[torch.randint(0, 5, (count,), generator=g)]
    if count > 8:
        meta[2, 0], meta[3, 0], meta[4, 0], meta[5, 0], meta[6, 0] = float("nan"), -0.5, 0.0, -0.0, float("inf")
        meta[7, 1] = float("nan")
        meta[count // 2, 3] = 11.0
    return meta


_CACHE = {}


def _bank(count, dev):
    """(host metadata, device metadata), built once per count and left unchanged"""
    if count not in _CACHE:
        m = _meta(count, seed=count)
        _CACHE[count] = (m, m.to(dev))
    return _CACHE[count]


def _top_n(d, n):
    """The rule's step 6 from per-row keys on the device: rows int32 [n], keys [n], eligible."""
    order = torch.sort(d, descending=True, stable=True).indices[:n]      # (stable: equal keys keep the lower row first)
    keys = d[order]
    ok = keys > -math.inf
    return torch.where(ok, order.to(torch.int32), torch.full_like(order, -1, dtype=torch.int32)), keys, (d > -math.inf).sum()


@pytest.mark.parametrize("count", COUNTS)
def test_uniforms_match_numpy_philox_exactly(dev, count):
    from aura_snn_rag_amd import ops
    _, meta = _bank(count, dev)
    rows = np.arange(count, dtype=np.uint64)
    for seed in (2024, (1 << 32) + 5):
        for draw in (0, (1 << 33) + 7):
            _, u = ops.bank_replay_keys(meta, count, NOW, seed=seed, draw=draw, return_uniforms=True)
            want = R.uniforms(R.random_words(rows, seed, draw))[0]
            assert np.array_equal(u.cpu().numpy().astype(np.int64), want), (seed, draw)


@pytest.mark.parametrize("priority", PRIORITIES)
@pytest.mark.parametrize("count", COUNTS)
def test_keys_against_the_rule_in_fp64(dev, count, priority):
    """|d - (alpha (ln s + a32) - ln(-ln u))| <= 2^-23 (4 alpha (|ln s| + |a|) + 4 |ln(-ln u)| + 3): the 3-ulp bound on
    logf plus the three roundings; a32 in NumPy fp32 (correctly rounded on both sides), u exact."""
    from aura_snn_rag_amd import ops
    host, meta = _bank(count, dev)
    m = host.numpy()
    seed, draw = 99, 12345
    worst = 0.0
    for alpha in ALPHAS:
        for scope in (SCOPES[0], SCOPES[3]):
            d, q = ops.bank_replay_keys(meta, count, NOW, priority=priority, alpha=alpha, seed=seed, draw=draw,
                                        return_uniforms=True, **scope)
            d = d.cpu().numpy()
            lw32 = R.log_priority(m, count, NOW, priority)
            ok = R.in_scope(m, count, **scope) & np.isfinite(lw32)
            assert np.array_equal(d > -np.inf, ok) and np.all(np.isneginf(d[~ok])), (alpha, scope)
            u = (q.cpu().numpy().astype(np.float64) + 0.5) * 2.0 ** -23
            with np.errstate(all="ignore"):
                ln_s = np.log(m[:, 0].astype(np.float64)) if priority != "uniform" else np.zeros(count)
                a32 = (-(np.float32(NOW) - m[:, 1]) / np.float32(3600.0)).astype(np.float64) if priority == "key" \
                    else np.zeros(count)
                g = np.log(-np.log(u))
                want = alpha * (ln_s + a32) - g
                tol = 2.0 ** -23 * (4 * alpha * (np.abs(ln_s) + np.abs(a32)) + 4 * np.abs(g) + 3)
            if ok.any():
                ratio = float(np.max(np.abs(d[ok].astype(np.float64) - want[ok]) / tol[ok]))
                worst = max(worst, ratio)
    print(f"count={count} {priority}: max |d - fp64| / tolerance = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("count", COUNTS)
def test_selection_is_exactly_the_top_n_of_the_kernels_keys(dev, count):
    from aura_snn_rag_amd import ops
    _, meta = _bank(count, dev)
    seen = set()
    for n in sorted({1, max(1, count // 7), count}):
        for priority in PRIORITIES:
            for alpha in ALPHAS:
                for si, scope in enumerate(SCOPES):
                    kw = dict(priority=priority, alpha=alpha, seed=7, draw=(1 << 40) + n, **scope)
                    d = ops.bank_replay_keys(meta, count, NOW, **kw)
                    rows, keys, eligible = ops.bank_replay(meta, count, NOW, n, **kw)
                    w_rows, w_keys, w_elig = _top_n(d, n)
                    assert rows.dtype == torch.int32 and rows.shape == (n,) and keys.shape == (n,)
                    assert torch.equal(rows, w_rows), (n, kw)
                    assert torch.equal(keys.view(torch.int32), w_keys.view(torch.int32)), (n, kw)
                    e = int(eligible)
                    assert e == int(w_elig) and int((rows >= 0).sum()) == min(n, e)
                    seen.add("0" if e == 0 else "1" if e == 1 else "<n" if e < n else ">=n")
    if count > 8:
        assert seen == {"0", "1", "<n", ">=n"}


@pytest.mark.parametrize("count", [65, 100_003])
def test_alpha_0_strength_equals_uniform_where_both_admit(dev, count):
    from aura_snn_rag_amd import ops
    _, meta = _bank(count, dev)
    a = ops.bank_replay_keys(meta, count, NOW, priority="strength", alpha=0.0, seed=3, draw=4)
    b = ops.bank_replay_keys(meta, count, NOW, priority="uniform", alpha=0.0, seed=3, draw=4)
    both = (a > -math.inf) & (b > -math.inf)
    assert int(both.sum()) == int((a > -math.inf).sum()) < count and bool((b > -math.inf).all())
    assert torch.equal(a[both].view(torch.int32), b[both].view(torch.int32))
    # and the prefix property on the device: the first 8 of a draw of 64 are the draw of 8
    r8 = ops.bank_replay(meta, count, NOW, 8, seed=3, draw=4)
    r64 = ops.bank_replay(meta, count, NOW, 64, seed=3, draw=4)
    assert torch.equal(r8[0], r64[0][:8]) and torch.equal(r8[1], r64[1][:8])


@pytest.mark.parametrize("index", [False, True])
def test_product_replay(dev, index):
    from aura_snn_rag_amd.core import hippocampal as H
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    M, D = 10_000, 32

    def make():
        return H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                      device="cuda", use_centroid_index=index, replay_seed=5)
    hf = make()
    g = torch.Generator().manual_seed(21)
    for b in range(0, M, 2500):
        hf.create_episodic_memories([f"m{i}" for i in range(b, b + 2500)], torch.randn(2500, D, generator=g),
                                    tags=torch.randint(0, 6, (2500,), generator=g).numpy().astype(np.int32))
    hf.decay(0.3)                                           # strengths 0.7, 0.9, 0.95 and 1.0 through the bank's own methods
    hf.reinforce(torch.arange(0, M, 3), amount=0.2)
    hf.reinforce(torch.arange(0, M, 7), amount=0.25)
    now = float(hf.memory_metadata[0, 1].item()) + 640.0
    queries = torch.randn(16, D, generator=g).to(dev)
    hf.recall_batch(queries, k=5, now=now)                  # (whatever recall derives from the bank exists now)
    # the sample is the rule rebuilt from replay_keys; the counter numbers the calls
    for kw in ({}, {"tags": [2, 4], "alpha": 2.0}, {"priority": "strength", "min_strength": 0.93}):
        d = hf.replay_keys(now=now, **kw)
        n = 1500
        s = hf.replay(n, now=now, **kw)
        w_rows, w_keys, w_elig = _top_n(d, n)
        assert torch.equal(s.rows, w_rows) and torch.equal(s.keys, w_keys) and int(s.eligible) == int(w_elig)
        valid = s.rows >= 0
        assert torch.equal(s.features[valid], hf.memory_features[s.rows[valid].long()]) and not bool(s.features[~valid].any())
        assert s.features.shape == (n, D)
    assert int(s.eligible) < n and hf.bank_state()["replay_draws"] == 3     # (the last scope pads)
    inj = MO.MemoryInjection(hf, D, num_heads=2)

    class Layer(MO.BatchedMemoryMixin):
        hippocampus = hf

    want = hf.replay(64, draw=9, now=now, tags=1)
    for owner in (inj, Layer()):
        feats, rows = owner.replay_memories(64, draw=9, now=now, tags=1)
        assert torch.equal(rows, want.rows) and torch.equal(feats, want.features)
    # reinforce through replay: the existing method patches the derived state, so a following recall equals that of a
    # bank rebuilt from the checkpoint, bit for bit
    before = hf.memory_metadata.clone()
    s = hf.replay(2000, draw=11, now=now, reinforce=0.1, reinforce_cap=2.0)
    changed = torch.nonzero((hf.memory_metadata != before).any(dim=1)).flatten()
    assert torch.equal(changed, torch.sort(s.rows.long()).values) and changed.numel() == 2000
    other = make()
    other.load_state_dict(hf.state_dict())
    other.load_bank_state(hf.bank_state())
    s0, r0 = hf.recall_batch(queries, k=5, now=now)
    s1, r1 = other.recall_batch(queries, k=5, now=now)
    assert torch.equal(r0, r1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
    assert other.replay(10, now=now).rows.tolist() == hf.replay(10, now=now).rows.tolist()


def test_abi_rejects_bad_arguments_without_launching(dev):
    from aura_snn_rag_amd import _lib
    L = _lib.load()
    count, n = 1000, 10
    meta = _meta(count, seed=1).to(dev)
    rows = torch.full((n,), -7, dtype=torch.int32, device=dev)
    keys = torch.full((n,), -7.0, device=dev)
    elig = torch.full((1,), -7, dtype=torch.int64, device=dev)
    out_d = torch.full((count,), -7.0, device=dev)
    nbytes = L.aura_bank_replay_workspace_bytes(count, n)
    assert nbytes > 4 * count
    assert L.aura_bank_replay_workspace_bytes(count, 0) < 0 and L.aura_bank_replay_workspace_bytes(count, count + 1) < 0
    assert L.aura_bank_replay_workspace_bytes(-1, 1) < 0 and L.aura_bank_replay_workspace_bytes(0, 5) == 0
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    good = (ctypes.c_int32 * 3)(3, 5, 7)
    many = (ctypes.c_int32 * 65)(*range(65))
    nan = float("nan")

    def replay(meta_p=meta.data_ptr(), count_=count, prio=0, alpha=1.0, tags=good, n_tags=3, cond=0, n_=n,
               r_p=rows.data_ptr(), k_p=keys.data_ptr(), e_p=elig.data_ptr(), ws_p=base, ws_bytes=nbytes):
        return L.aura_bank_replay(meta_p, count_, NOW, prio, alpha, tags, n_tags, cond, 0.0, 0.0, 0.0, 1, 2, n_, r_p, k_p,
                                  e_p, ws_p, ws_bytes, None)

    def rkeys(meta_p=meta.data_ptr(), count_=count, prio=0, alpha=1.0, tags=good, n_tags=3, cond=0, d_p=out_d.data_ptr()):
        return L.aura_bank_replay_keys(meta_p, count_, NOW, prio, alpha, tags, n_tags, cond, 0.0, 0.0, 0.0, 1, 2, d_p,
                                       None, None)
    for f in (replay, rkeys):
        assert f(alpha=-0.5) == -1 and f(alpha=16.5) == -1 and f(alpha=nan) == -1, f
        assert f(prio=3) == -1 and f(prio=-1) == -1 and f(cond=8) == -1 and f(count_=-1) == -1
        assert f(tags=many, n_tags=65) == -1 and f(n_tags=-1) == -1 and f(tags=None) == -1
        assert f(tags=(ctypes.c_int32 * 3)(3, 3, 7)) == -1 and f(tags=(ctypes.c_int32 * 3)(5, 3, 7)) == -1
        assert f(tags=(ctypes.c_int32 * 3)(-1, 3, 7)) == -1 and f(tags=(ctypes.c_int32 * 3)(3, 5, 1 << 24)) == -1
        assert f(meta_p=None) == -1 and f(meta_p=meta.data_ptr() + 4) == -3
    assert replay(n_=0) == -1 and replay(n_=count + 1) == -1
    assert replay(ws_bytes=nbytes - 1) == -1 and replay(ws_p=base + 4) == -3
    for name in ("r_p", "k_p", "e_p", "ws_p"):
        assert replay(**{name: None}) == -1, name
    assert rkeys(d_p=None) == -1
    torch.cuda.synchronize()
    assert bool((rows == -7).all()) and bool((keys == -7.0).all()) and int(elig) == -7 and bool((out_d == -7.0).all())
    assert not bool(ws.any())
    # the same calls with good arguments work, 64 tags included; an empty bank gets the padding alone
    assert replay() == 0 and rkeys() == 0 and replay(tags=many, n_tags=64) == 0 and replay(tags=None, n_tags=0) == 0
    torch.cuda.synchronize()
    d = out_d.clone()
    assert replay() == 0
    torch.cuda.synchronize()
    assert int(elig) == int((d > -math.inf).sum()) and sorted(rows.tolist()) == sorted(_top_n(d, n)[0].tolist())
    rows.fill_(-7); keys.fill_(-7.0); elig.fill_(-7)
    assert replay(count_=0, ws_p=None, ws_bytes=0) == 0 and rkeys(count_=0) == 0
    torch.cuda.synchronize()
    assert rows.tolist() == [-1] * n and bool(torch.isneginf(keys).all()) and int(elig) == 0
