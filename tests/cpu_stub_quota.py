"""Per-tag quotas in torch on the CPU: ``bank_tag_counts``, ``bank_select_weakest_scoped`` and
``bank_select_weakest_masked`` on top of ``tests/cpu_stub_consolidate_scoped.py`` (which brings every other stand-in)
-- TEST INFRASTRUCTURE ONLY.

They restate the rule of ``include/aura_hip.h`` ("Per-tag quotas") literally, with ``eviction_order`` and
``ordered_bits`` of ``tests/cpu_stub_retention.py``:
  a tag's eviction order = its rows of [0, count) by (key, (r - origin) mod count) ascending, a NaN key first
  x = min(incoming, max(0, held + incoming - quota))            (never more than held)
  the masked global selection = the bank's eviction order with the rows of the bitmap left out.
``rule_run`` is the whole rule for one run (steps 1 - 4), from keys the caller supplies."""
import numpy as np
import torch

from tests.cpu_stub_consolidate_scoped import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_consolidate_scoped import (CALLS, LAST, FIND_SIZES, MOVES, STAMPS, SCOPED_FINDS,  # noqa: F401
                                               KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError,
                                               CONSOLIDATE_MAX_BATCH, CONSOLIDATE_MAX_IMAGE_DIM, TAG_LIMIT, held_tags)
from tests.cpu_stub_retention import eviction_order, ordered_bits, bank_retention_keys

CALLS["tag_counts"] = 0
CALLS["select_scoped"] = 0
CALLS["select_masked"] = 0
QUOTA_MAX_SCOPES = 64
I64_MAX = torch.iinfo(torch.int64).max


def tag_counts_reference(meta, count, scope_tags):
    t = held_tags(meta, count)
    return torch.tensor([int((t == int(s)).sum()) for s in scope_tags], dtype=torch.int64)


def scope_victims(keys, tags, tag, origin, x):
    """The first ``x`` rows of tag ``tag``'s eviction order (``keys`` fp32 [count], ``tags`` int64 [count])."""
    order = eviction_order(keys, origin)
    return order[tags[order] == int(tag)][:int(x)]


def scoped_reference(keys, tags, scope_tags, origins, incoming, quotas):
    """``(held [S], x [S], [victims of scope s in its eviction order])`` from the rule."""
    held, xs, victims = [], [], []
    for t, c, n_in, q in zip(scope_tags, origins, incoming, quotas):
        h = int((tags == int(t)).sum())
        x = min(int(n_in), max(0, h + int(n_in) - int(q)), h)
        held.append(h)
        xs.append(x)
        victims.append(scope_victims(keys, tags, t, c, x))
    return torch.tensor(held, dtype=torch.int64), torch.tensor(xs, dtype=torch.int64), victims


def masked_reference(keys, cursor, n, masked_rows):
    """The first ``n`` rows of the bank's eviction order among the rows not in ``masked_rows``."""
    order = eviction_order(keys, cursor)
    if len(masked_rows):
        keep = torch.ones(keys.numel(), dtype=torch.bool)
        keep[torch.as_tensor(masked_rows, dtype=torch.int64)] = False
        order = order[keep[order]]
    return order[:int(n)]


def rule_run(keys, tags, run_tags, quota_of, origins, cursor, M):
    """Steps 1 - 4 for one run.  ``keys`` fp32 [count] and ``tags`` int64 [count] of the rows held before the run,
    ``run_tags`` the run's tags (ints), ``quota_of(t)`` -> quota or None, ``origins`` {tag: origin} (missing: 0).
    Returns ``(slots list, n_app, new cursor, new origins, tag victims per scope {tag: rows}, global victims)``."""
    count, n = keys.numel(), len(run_tags)
    limited = sorted({int(t) for t in run_tags if quota_of(int(t)) is not None})
    new_origins = dict(origins)
    tag_victims, taken = {}, []
    for t in limited:
        in_t = sum(1 for u in run_tags if int(u) == t)
        assert in_t <= quota_of(t), "a run holds at most q(t) rows of a limited tag"
        held = int((tags == t).sum()) if count else 0
        x = min(in_t, max(0, held + in_t - quota_of(t)))
        v = scope_victims(keys, tags, t, origins.get(t, 0), x) if x else torch.zeros(0, dtype=torch.int64)
        tag_victims[t] = v.tolist()
        if x:
            new_origins[t] = int(v[-1]) + 1
            taken += v.tolist()
    rem = n - len(taken)
    n_app = min(rem, M - count)
    g = rem - n_app
    glob = masked_reference(keys, cursor, g, taken).tolist() if g else []
    slots = list(range(count, count + n_app)) + taken + glob
    return slots, n_app, cursor + g, new_origins, tag_victims, glob


def _signed_comp(keys, rows, origin, count):
    """The composites as the library writes them: ordered key and rotated row, top bit flipped (signed-sortable)."""
    o = ordered_bits(keys[rows])
    rot = (rows - int(origin) % count) % count
    return ((o - 0x80000000) << 32) | rot


def bank_tag_counts(meta, count, scope_tags):
    CALLS["tag_counts"] += 1
    t = np.asarray(scope_tags, dtype=np.int64).reshape(-1)
    assert t.size == 0 or (np.all(np.diff(t) > 0) and t[0] >= 0 and t[-1] < TAG_LIMIT)
    return tag_counts_reference(meta, count, t.tolist()).to(torch.int32)


def bank_select_weakest_scoped(meta, count, now, scope_tags, origins, incoming, quotas, bitmap=None):
    CALLS["select_scoped"] += 1
    t = np.asarray(scope_tags, dtype=np.int64).reshape(-1)
    S = t.size
    assert count >= 1 and S >= 1 and np.all(np.diff(t) > 0) and t[0] >= 0 and t[-1] < TAG_LIMIT
    o, n_in, q = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (origins, incoming, quotas))
    assert o.size == n_in.size == q.size == S and np.all(o >= 0) and np.all(n_in >= 0) and np.all(q >= 1)
    keys = bank_retention_keys(meta, count, now)
    CALLS["keys"] -= 1
    held, xs, victims = scoped_reference(keys, held_tags(meta, count), t.tolist(), o.tolist(), n_in.tolist(), q.tolist())
    T = int(n_in.sum())
    packed = torch.empty(2 * S + 2 * T, dtype=torch.int64)
    packed[:S], packed[S:2 * S] = held, xs
    packed[2 * S:2 * S + T] = -1
    packed[2 * S + T:] = I64_MAX
    words = (count + 31) // 32
    if bitmap is None:
        bitmap = torch.zeros(words, dtype=torch.int32)
    assert bitmap.dtype == torch.int32 and bitmap.numel() >= words
    off = 0
    for s in range(S):
        v = victims[s]
        if v.numel():
            perm = torch.flip(torch.arange(v.numel()), dims=[0])          # an arrival order that is not the eviction order
            packed[2 * S + off:2 * S + off + v.numel()] = v[perm]
            packed[2 * S + T + off:2 * S + T + off + v.numel()] = _signed_comp(keys, v, int(o[s]), count)[perm]
            for r in v.tolist():
                w = int(bitmap[r >> 5]) | (1 << (r & 31))
                bitmap[r >> 5] = w - (1 << 32) if w >= (1 << 31) else w
        off += int(n_in[s])
    return packed, bitmap


def scoped_selection_decode(packed, incoming):
    p = packed.numpy() if isinstance(packed, torch.Tensor) else np.asarray(packed)
    n_in = np.asarray(incoming, dtype=np.int64).reshape(-1)
    S, T = n_in.size, int(n_in.sum())
    held, x = p[:S].copy(), p[S:2 * S].copy()
    victims, o = [], 0
    for s in range(S):
        m = int(n_in[s])
        seg = slice(2 * S + o, 2 * S + o + m)
        comp = p[2 * S + T + o:2 * S + T + o + m]
        victims.append(p[seg][np.argsort(comp, kind="stable")[:int(x[s])]].astype(np.int64))
        o += m
    return held, x, victims


def bitmap_rows(bitmap, count):
    """The rows of [0, count) whose bit is set."""
    b = bitmap.detach().cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    bits = (b[:, None] >> np.arange(32)[None, :]) & 1
    return np.nonzero(bits.reshape(-1)[:count])[0]


def bank_select_weakest_masked(meta, count, now, cursor, n, bitmap):
    CALLS["select_masked"] += 1
    assert 1 <= n <= count and cursor >= 0 and bitmap.dtype == torch.int32
    keys = bank_retention_keys(meta, count, now)
    CALLS["keys"] -= 1
    rows = masked_reference(keys, cursor, n, bitmap_rows(bitmap, count).tolist())
    assert rows.numel() == n, "fewer unmasked rows than asked for"
    return rows, keys[rows]
