"""Replay on the CPU (``ops`` replaced by tests/cpu_stub_replay.py, which restates the rule of ``include/aura_hip.h`` in
NumPy): the generator's known answers, the exactness of the uniforms, the properties the rule promises (prefix, scope
filter, padding), the draw counter and its checkpoint key, reinforce / touch on exactly the drawn rows, an aged bank, the
refusals, and the distribution of the draw itself against ``p / sum p`` (seeded: deterministic checks)."""
import math

import numpy as np
import pytest
import torch

from tests import cpu_stub_replay as stub

NOW = 1.7e9                    # = 128 * 13281250: on the grid of the stored fp32 timestamps
DAY = 86400.0


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


def _hf(H, D=16, M=256, **kw):
    kw.setdefault("use_centroid_index", False)
    return H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                  device="cpu", **kw)


def _filled(H, n=100, seed=0, **kw):
    """a bank of n rows, tags 0..4 in turn, strengths in (0.05, 1], written at NOW"""
    g = torch.Generator().manual_seed(seed)
    hf = _hf(H, **kw)
    hf.create_episodic_memories([f"m{i}" for i in range(n)], torch.randn(n, 16, generator=g),
                                tags=np.arange(n) % 5)
    hf.memory_metadata[:n, 0] = 0.05 + 0.95 * torch.rand(n, generator=g)
    return hf


# ---------------------------------------------------------------------------------------------------------------------
# the generator and the uniforms
def test_philox_known_answers():
    """the Random123 vectors of Philox4x32-10"""
    F = 0xFFFFFFFF
    for counter, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in stub.philox4x32_10(counter, key)) == want
    # the rule's packing: row and draw as 64-bit halves, the seed as the key
    assert int(stub.random_words(0, 0, 0)) == 0x6627e8d5
    assert int(stub.random_words((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1)) == 0x408f276d
    assert int(stub.random_words(0x85a308d3243f6a88, 0x299f31d0a4093822, 0x0370734413198a2e)) == 0xd16cfe09


def test_uniforms_are_exact_and_never_0_or_1():
    x = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0x80000000, 0x6627e8d5], dtype=np.uint64)
    q, u = stub.uniforms(x)
    assert u.dtype == np.float32
    assert q.tolist() == [0, 0, 1, (1 << 23) - 1, 1 << 22, 0x6627e8d5 >> 9]
    # a 24-bit odd numerator over 2^24: the fp32 value IS the rational
    assert [float(v) for v in u] == [(2 * int(k) + 1) / 2.0 ** 24 for k in q]
    assert float(u[0]) == 2.0 ** -24 and float(u[3]) == 1.0 - 2.0 ** -24
    allq = np.arange(0, 1 << 23, 4099, dtype=np.uint64) << np.uint64(9)
    q2, u2 = stub.uniforms(allq)
    assert np.array_equal(u2.astype(np.float64) * 2.0 ** 24, 2.0 * q2 + 1.0)
    assert u2.min() > 0.0 and u2.max() < 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the properties of the rule, through HippocampalFormation.replay
def test_prefix_and_scope_filter_properties(hmod):
    hf = _filled(hmod)
    a = hf.replay(8, draw=3, now=NOW)
    b = hf.replay(64, draw=3, now=NOW)
    assert a.rows.dtype == torch.int32 and a.keys.dtype == torch.float32 and a.rows.shape == (8,)
    assert torch.equal(a.rows, b.rows[:8]) and torch.equal(a.keys, b.keys[:8])
    assert int(b.eligible) == 100 and len(set(b.rows.tolist())) == 64
    assert torch.all(b.keys[:-1] >= b.keys[1:])
    # the sample equals the rule rebuilt from replay_keys
    d = hf.replay_keys(draw=3, now=NOW)
    rows, keys, elig = stub.sample_from_keys(d.numpy(), 64)
    assert b.rows.tolist() == rows.tolist() and np.array_equal(b.keys.numpy(), keys) and elig == 100
    # the sample of a scope = the full-bank order filtered to the scope
    full = hf.replay(100, draw=3, now=NOW)
    tags = hf.memory_tags.numpy()
    for scope in (2, [1, 4], [0]):
        s = hf.replay(100, draw=3, now=NOW, tags=scope)
        want = [r for r in full.rows.tolist() if tags[r] in np.atleast_1d(scope)]
        assert int(s.eligible) == len(want) == 20 * np.atleast_1d(scope).size
        assert s.rows.tolist() == want + [-1] * (100 - len(want))
        kf = dict(zip(full.rows.tolist(), full.keys.tolist()))
        assert s.keys.tolist() == [kf[r] for r in want] + [-math.inf] * (100 - len(want))
    strong = hf.replay(100, draw=3, now=NOW, min_strength=0.5)
    st = hf.memory_metadata[:100, 0].numpy()
    assert [r for r in strong.rows.tolist() if r >= 0] == [r for r in full.rows.tolist() if st[r] >= np.float32(0.5)]
    # a pair's key does not depend on alpha's scope companions, nor eligibility on alpha
    assert int(hf.replay(5, draw=3, now=NOW, alpha=0.0).eligible) == 100


def test_padding_features_and_clamp(hmod):
    hf = _filled(hmod, n=30)
    hf.memory_metadata[[3, 8], 0] = torch.tensor([0.0, float("nan")])          # two rows no priority can draw
    s = hf.replay(12, draw=0, now=NOW, tags=4)                               # tag 4: rows 4, 9, ..., 29 -> six rows
    assert int(s.eligible) == 6 and s.rows[6:].tolist() == [-1] * 6 and sorted(s.rows[:6].tolist()) == [4, 9, 14, 19, 24, 29]
    assert torch.all(torch.isinf(s.keys[6:])) and torch.all(s.keys[6:] < 0)
    assert torch.equal(s.features[:6], hf.memory_features[s.rows[:6].long()]) and not s.features[6:].any()
    assert hf.replay(12, draw=0, now=NOW, tags=4, return_features=False).features is None
    big = hf.replay(1000, draw=0, now=NOW)                                    # clamped to memory_count
    assert big.rows.shape == (30,) and int(big.eligible) == 28 and big.rows[28:].tolist() == [-1, -1]
    assert int(hf.replay(1000, draw=0, now=NOW, priority="uniform").eligible) == 30
    assert int(hf.replay(3, draw=0, now=NOW, tags=9).eligible) == 0             # a tag nobody carries
    empty = _hf(hmod).replay(5)
    assert empty.rows.shape == (0,) and empty.keys.shape == (0,) and empty.features.shape == (0, 16)
    assert int(empty.eligible) == 0 and stub.CALLS["replay"] == 5           # (the empty bank reaches no op)


def test_draw_counter_and_bank_state(hmod):
    hf = _filled(hmod, replay_seed=77)
    assert "replay_draws" not in hf.bank_state()
    fixed = [hf.replay(10, draw=5, now=NOW).rows.tolist() for _ in range(2)]
    assert fixed[0] == fixed[1] and "replay_draws" not in hf.bank_state()     # an explicit draw advances nothing
    seq = [hf.replay(10, now=NOW).rows.tolist() for _ in range(3)]
    assert seq[0] != seq[1] != seq[2] and hf.bank_state()["replay_draws"] == 3
    assert seq == [hf.replay(10, draw=i, now=NOW).rows.tolist() for i in range(3)]
    assert hf.replay(10, draw=5, now=NOW).rows.tolist() == fixed[0]
    assert hf.replay(10, draw=5, now=NOW, seed=78).rows.tolist() != fixed[0]    # another seed, another draw
    # replay_keys(draw=None) shows the draw the next call will make, and numbers nothing
    d = hf.replay_keys(now=NOW)
    assert hf.bank_state()["replay_draws"] == 3
    nxt = hf.replay(10, now=NOW)
    assert nxt.rows.tolist() == stub.sample_from_keys(d.numpy(), 10)[0].tolist()
    # the counter travels: a new object continues the sequence
    state = hf.bank_state()
    other = _hf(hmod, replay_seed=77)
    other.load_state_dict(hf.state_dict())
    other.load_bank_state(state)
    assert other.bank_state()["replay_draws"] == 4
    assert other.replay(10, now=NOW).rows.tolist() == hf.replay(10, now=NOW).rows.tolist()
    assert other.replay(10, now=NOW).rows.tolist() == hf.replay(10, draw=5, now=NOW).rows.tolist()
    # a state without the key resets the counter
    del state["replay_draws"]
    other.load_bank_state(state)
    assert "replay_draws" not in other.bank_state()


def test_reinforce_and_touch_reach_exactly_the_drawn_rows(hmod):
    hf = _filled(hmod)
    hf.memory_metadata[:100, 0] *= 0.5                                        # room below the cap
    before = hf.memory_metadata.clone()
    calls = dict(stub.CALLS)
    s = hf.replay(16, draw=1, now=NOW, reinforce=0.25)
    drawn = s.rows.long()
    want = before.clone()
    want[drawn, 0] = torch.minimum(before[drawn, 0] + 0.25, torch.tensor(1.0))
    assert torch.equal(hf.memory_metadata, want)
    assert stub.CALLS["reinforce"] == calls["reinforce"] + 1 and stub.CALLS["touch"] == calls["touch"]
    # the draw was final before the strengths moved: it is the draw of the bank as it was
    assert s.rows.tolist() == stub.sample_from_keys(stub.draw_keys(before, 100, NOW, draw=1), 16)[0].tolist()
    later = NOW + 1280.0
    before = hf.memory_metadata.clone()
    s = hf.replay(16, draw=2, now=later, touch=True, tags=[1, 2])
    drawn = s.rows.long()
    want = before.clone()
    want[drawn, 1] = later
    assert torch.equal(hf.memory_metadata, want) and stub.CALLS["touch"] == calls["touch"] + 1
    assert stub.CALLS["reinforce"] == calls["reinforce"] + 1
    assert np.all(hf._slot_time[drawn.numpy()] == later)
    # padding rows reach neither
    before = hf.memory_metadata.clone()
    s = hf.replay(30, draw=2, now=later, tags=3, reinforce=0.1, reinforce_cap=2.0, touch=True)
    assert int(s.eligible) == 20 and (s.rows < 0).sum() == 10
    changed = torch.nonzero((hf.memory_metadata != before).any(dim=1)).flatten().tolist()
    assert changed == sorted(r for r in s.rows.tolist() if r >= 0)


def test_an_aged_key_bank_still_draws(hmod):
    hf = _filled(hmod)
    hf.memory_metadata[:100, 1] = torch.tensor(NOW - 6 * DAY) - 128.0 * torch.arange(100)
    now = NOW
    assert not hf.retention_keys(now=now).any()                               # expf underflows: every key is 0
    s = hf.replay(20, draw=0, now=now)
    assert int(s.eligible) == 100 and len(set(s.rows.tolist())) == 20 and s.rows.min() >= 0
    assert torch.isfinite(s.keys).all()
    # and recency still counts: lw = ln(s) - age / 3600 in the log domain
    lw = stub.log_priority(hf.memory_metadata.numpy(), 100, now, "key")
    assert np.isfinite(lw).all() and lw.max() < -140.0


def test_layers_replay_memories(hmod):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    hf = _filled(hmod)
    inj = MO.MemoryInjection(hf, 16, num_heads=2)

    class Layer(MO.BatchedMemoryMixin):
        hippocampus = hf

    want = hf.replay(12, draw=4, now=NOW, tags=1)
    for owner in (inj, Layer()):
        feats, rows = owner.replay_memories(12, draw=4, now=NOW, tags=1)
        assert torch.equal(rows, want.rows) and torch.equal(feats, want.features)


def test_refusals(hmod):
    hf = _filled(hmod)
    calls = stub.CALLS["replay"]
    bad = [dict(priority="recency"), dict(alpha=-0.1), dict(alpha=16.5), dict(alpha=float("nan")),
           dict(tags=list(range(65))), dict(tags=-1), dict(tags=[1, 1 << 24]), dict(tags=[]), dict(tags=1.5),
           dict(seed=-1), dict(seed=1 << 64), dict(draw=-1), dict(draw=1 << 64), dict(newer_than=float("nan")),
           dict(min_strength=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            hf.replay(4, now=NOW, **kw)
        with pytest.raises(ValueError):
            hf.replay_keys(now=NOW, **kw)
    with pytest.raises(ValueError):
        hf.replay(-1)
    with pytest.raises(ValueError):
        _hf(hmod, replay_seed=-3)
    assert "replay_draws" not in hf.bank_state() and stub.CALLS["replay"] == calls   # refused before any draw
    # the argument checks of the op itself (host code): the limits are inclusive, 64 tags are a union, repeats collapse
    assert stub._replay_args("t", "key", 16.0, list(range(64)), None, None, None, (1 << 64) - 1, (1 << 64) - 1)[0][3] == 64
    assert stub.replay_scope_tags([5, 3, 5, 0]).tolist() == [0, 3, 5]
    assert stub.replay_scope_tags(None).size == 0
    with pytest.raises(ValueError):
        stub.bank_replay(hf.memory_metadata, 100, NOW, 101)
    with pytest.raises(ValueError):
        stub.bank_replay(hf.memory_metadata, 100, NOW, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the distribution, from the rule alone
SEED, DRAWS = 2024, 20000


def _meta_with_priorities(p):
    """timestamps at NOW, so that 'key' equals 'strength': lw = ln(p)"""
    meta = np.zeros((len(p), 4), dtype=np.float32)
    meta[:, 0] = np.asarray(p, dtype=np.float32)
    meta[:, 1] = np.float32(NOW)
    return meta


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.0, 2.0])
def test_first_pick_distribution(alpha):
    """Chi-square of the first picks of draws 0..19 999 over 16 rows with lw = ln(0.05 (i + 1)) against p / sum p,
    p = exp(alpha lw); the bar is the 99.9 % quantile at 15 degrees of freedom.  (In fp64 the rule gives 13.7, 17.9, 17.7
    and 21.7 at alpha = 1, 0.5, 0 and 2.)"""
    w = 0.05 * (np.arange(16) + 1.0)
    meta = _meta_with_priorities(w)
    d = stub.draw_keys(meta, 16, NOW, "key", alpha, seed=SEED, draw=np.arange(DRAWS))
    assert d.shape == (DRAWS, 16) and np.array_equal(d, stub.draw_keys(meta, 16, NOW, "strength", alpha, seed=SEED,
                                                                        draw=np.arange(DRAWS)))
    first = np.argmax(d, axis=1)                                     # (argmax: the lower row on equal keys)
    p = np.exp(alpha * np.log(w.astype(np.float32).astype(np.float64)))
    expect = DRAWS * p / p.sum()
    chi2 = float(np.sum((np.bincount(first, minlength=16) - expect) ** 2 / expect))
    print(f"alpha={alpha}: chi2={chi2:.2f}")
    assert chi2 < 37.70


def test_ordered_pair_distribution():
    """The ordered first two of n = 2 over 5 rows, lw = ln of 0.1, 0.2, 0.4, 0.8, 1.0, alpha = 1, against
    p_i / S * p_j / (S - p_i): 20 cells, the 99.9 % quantile at 19 degrees of freedom.  (In fp64 the rule gives 25.05.)"""
    w = np.array([0.1, 0.2, 0.4, 0.8, 1.0])
    meta = _meta_with_priorities(w)
    d = stub.draw_keys(meta, 5, NOW, "key", 1.0, seed=SEED, draw=np.arange(DRAWS))
    order = np.argsort(-d.astype(np.float64), axis=1, kind="stable")[:, :2]
    # the same two through the op, for a few draws
    for k in (0, 1, 19999):
        assert stub.bank_replay(torch.from_numpy(meta), 5, NOW, 2, seed=SEED, draw=k)[0].tolist() == order[k].tolist()
    counts = np.zeros((5, 5))
    np.add.at(counts, (order[:, 0], order[:, 1]), 1)
    p = w.astype(np.float32).astype(np.float64)
    S = p.sum()
    chi2 = 0.0
    for i in range(5):
        for j in range(5):
            if i != j:
                e = DRAWS * p[i] / S * p[j] / (S - p[i])
                chi2 += (counts[i, j] - e) ** 2 / e
    assert counts.trace() == 0
    print(f"ordered pairs: chi2={chi2:.2f}")
    assert chi2 < 43.82
