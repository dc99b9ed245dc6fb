"""Replay in NumPy on the CPU: ``bank_replay_keys`` and ``bank_replay`` on top of ``tests/cpu_stub_quota.py`` (which
brings every other stand-in) -- TEST INFRASTRUCTURE ONLY.

They restate the rule of ``include/aura_hip.h`` ("Replay") literally, Philox in uint64 arithmetic and the keys in fp32:
  x   = word 0 of Philox4x32-10, counter (row lo, row hi, draw lo, draw hi), key (seed lo, seed hi)
  u   = ((x >> 9) + 0.5) * 2^-23
  lw  = log(strength) + -(now32 - timestamp) / 3600 ('key') | log(strength) ('strength') | 0 ('uniform')
  d   = alpha * lw - log(-log(u)), a zero written as +0; eligible = in scope and lw finite
  sample = the first min(n, #eligible) eligible rows by (d descending, row ascending), then -1 / -inf.
The argument checks are those of ``aura_snn_rag_amd.ops`` itself (host code that needs no library)."""
import numpy as np
import torch

from aura_snn_rag_amd.ops import REPLAY_MAX_ALPHA, REPLAY_MAX_TAGS, REPLAY_PRIORITIES, _replay_args, replay_scope_tags  # noqa: F401
from tests.cpu_stub_quota import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_quota import (CALLS, LAST, FIND_SIZES, MOVES, STAMPS, SCOPED_FINDS,  # noqa: F401
                                  KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError,
                                  CONSOLIDATE_MAX_BATCH, CONSOLIDATE_MAX_IMAGE_DIM, TAG_LIMIT, QUOTA_MAX_SCOPES)

CALLS["replay"] = 0
CALLS["replay_keys"] = 0

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """All four output words (uint64 arrays holding 32-bit values) for ``counter`` (4 broadcastable arrays of 32-bit
    values) and ``key`` (2 ints)."""
    c = [np.asarray(w, dtype=np.uint64) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                   # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def random_words(rows, seed, draw):
    """x of the rule for ``rows`` and ``draw`` (broadcastable integer arrays) under ``seed``: uint64 holding 32 bits."""
    r, d, s = np.asarray(rows, dtype=np.uint64), np.asarray(draw, dtype=np.uint64), int(seed)
    return philox4x32_10((r & MASK, r >> S32, d & MASK, d >> S32), (s & 0xFFFFFFFF, s >> 32))[0]


def uniforms(x):
    """``(x >> 9 as int64, u fp32)``; every operation below is exact in fp32."""
    q = (np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.int64)
    return q, (q.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def row_tags(meta, count):
    """int64 [count]: the tag of every row as ``aura_row_tag`` reads column 3 (-2: no tag)."""
    w = np.asarray(meta[:count, 3], dtype=np.float32)
    ok = (w > np.float32(-1.0)) & (w < np.float32(16777216.0))
    return np.where(ok, np.trunc(np.where(ok, w, 0)).astype(np.int64), -2)


def log_priority(meta, count, now, priority):
    """fp32 [count]: lw of the rule."""
    m = np.asarray(meta[:count], dtype=np.float32)
    with np.errstate(all="ignore"):
        if priority == "uniform":
            return np.zeros(count, dtype=np.float32)
        lw = np.log(m[:, 0])
        if priority == "key":
            lw = lw + -(np.float32(now) - m[:, 1]) / np.float32(3600.0)
    assert lw.dtype == np.float32
    return lw


def in_scope(meta, count, tags=None, newer_than=None, older_than=None, min_strength=None):
    m = np.asarray(meta[:count], dtype=np.float32)
    ok = np.ones(count, dtype=bool)
    t = replay_scope_tags(tags)
    if t.size:
        ok &= np.isin(row_tags(meta, count), t.astype(np.int64))
    with np.errstate(invalid="ignore"):
        if newer_than is not None:
            ok &= m[:, 1] >= np.float32(newer_than)
        if older_than is not None:
            ok &= m[:, 1] <= np.float32(older_than)
        if min_strength is not None:
            ok &= m[:, 0] >= np.float32(min_strength)
    return ok


def gumbel_keys(lw, alpha, u):
    """fp32: d of the rule from lw, alpha and u (broadcastable), zeros as +0."""
    with np.errstate(all="ignore"):
        d = np.float32(alpha) * np.asarray(lw, dtype=np.float32) - np.log(-np.log(np.asarray(u, dtype=np.float32)))
    assert d.dtype == np.float32
    return np.where(d == 0, np.float32(0.0), d)


def draw_keys(meta, count, now, priority="key", alpha=1.0, tags=None, newer_than=None, older_than=None,
              min_strength=None, seed=0, draw=0):
    """fp32 [count] (``draw`` an int) or [len(draw), count] (an array of draws): d, ``-inf`` where not eligible."""
    meta = meta.detach().cpu().numpy() if isinstance(meta, torch.Tensor) else np.asarray(meta)
    lw = log_priority(meta, count, now, priority)
    ok = in_scope(meta, count, tags, newer_than, older_than, min_strength) & np.isfinite(lw)
    dr = np.asarray(draw, dtype=np.uint64)
    rows = np.arange(count, dtype=np.uint64)
    x = random_words(rows if dr.ndim == 0 else rows[None, :], seed, dr if dr.ndim == 0 else dr[:, None])
    d = gumbel_keys(lw, alpha, uniforms(x)[1])
    return np.where(ok, d, np.float32(-np.inf)).astype(np.float32)


def sample_from_keys(d, n):
    """``(rows int32 [n], keys fp32 [n], eligible)`` from per-row keys ``d`` (``-inf``: not eligible)."""
    d = np.asarray(d, dtype=np.float32)
    order = np.argsort(-d.astype(np.float64), kind="stable")            # d descending, equal d -> the lower row
    elig = int(np.sum(d > -np.inf))
    take = order[:min(n, elig)]
    rows = np.full(n, -1, dtype=np.int32)
    keys = np.full(n, -np.inf, dtype=np.float32)
    rows[:take.size], keys[:take.size] = take, d[take]
    return rows, keys, elig


def bank_replay_keys(meta, count, now, *, priority="key", alpha=1.0, tags=None, newer_than=None, older_than=None,
                     min_strength=None, seed=0, draw=0, return_uniforms=False):
    assert 0 <= count <= meta.shape[0]
    _replay_args("bank_replay_keys", priority, alpha, tags, newer_than, older_than, min_strength, seed, draw)
    CALLS["replay_keys"] += 1
    d = torch.from_numpy(draw_keys(meta, count, now, priority, alpha, tags, newer_than, older_than, min_strength, seed,
                                   draw))
    if not return_uniforms:
        return d
    q = uniforms(random_words(np.arange(count, dtype=np.uint64), seed, draw))[0]
    return d, torch.from_numpy(q.astype(np.int32))


def bank_replay(meta, count, now, n, *, priority="key", alpha=1.0, tags=None, newer_than=None, older_than=None,
                min_strength=None, seed=0, draw=0):
    if not (1 <= n <= count <= meta.shape[0]):
        raise ValueError(f"bank_replay: need 1 <= n <= count (n={n}, count={count})")
    _replay_args("bank_replay", priority, alpha, tags, newer_than, older_than, min_strength, seed, draw)
    CALLS["replay"] += 1                            # (a refused call does not count)
    d = draw_keys(meta, count, now, priority, alpha, tags, newer_than, older_than, min_strength, seed, draw)
    rows, keys, elig = sample_from_keys(d, n)
    return torch.from_numpy(rows), torch.from_numpy(keys), torch.tensor(elig, dtype=torch.int64)
