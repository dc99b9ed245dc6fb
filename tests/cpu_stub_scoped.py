"""``bank_set_tags`` and ``knn_search_scoped`` in torch on the CPU, on top of ``tests/cpu_stub_forget.py`` -- TEST
INFRASTRUCTURE ONLY -- and the data of the scoped-recall tests.

The rule (``include/aura_hip.h``, ``aura_knn_search_scoped``): row ``r < count`` is in query ``i``'s scope iff
``tags[i] < 0 or int(meta[r][3]) == tags[i]``, ``meta[r][1] >= float32(newer_than)``, ``meta[r][1] <=
float32(older_than)`` and ``meta[r][0] >= min_strength`` (a condition given as None is not applied); the result is the top
``k`` of the scope by the combined score, descending, equal scores to the lower row, padded with ``-inf`` / ``-1``."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.cpu_stub_forget import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_forget import (CALLS, LAST, FIND_SIZES, MOVES, KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE,  # noqa: F401
                                   AuraDeviceError, CONSOLIDATE_MAX_BATCH, CONSOLIDATE_MAX_IMAGE_DIM, tolerance,
                                   compact_reference)

CALLS["set_tags"] = 0
CALLS["scoped"] = 0
STAMPS = []                                        # (slots, tags) of every stub bank_set_tags call
LAST_SCOPED = {}                                   # arguments of the most recent stub knn_search_scoped

TAG_LIMIT = 1 << 24
SCOPED_MAX_K = 128
INF = float("inf")


def bank_set_tags(meta, count, slots, tags):
    CALLS["set_tags"] += 1
    assert slots.dtype == torch.int64 and tags.dtype == torch.int32 and slots.shape == tags.shape and slots.dim() == 1
    s, t = slots.tolist(), tags.tolist()
    assert len(set(s)) == len(s), "bank_set_tags: the slots must be distinct"
    assert all(0 <= x < count for x in s), "bank_set_tags: a slot outside the held rows"
    assert all(0 <= x < TAG_LIMIT for x in t), "bank_set_tags: a tag outside [0, 2^24)"
    STAMPS.append((s, t))
    meta[slots, 3] = tags.to(meta.dtype)


def scoped_query_tags(tags, nq):
    if tags is None:
        return np.full(nq, -1, dtype=np.int32)
    if isinstance(tags, torch.Tensor):
        tags = tags.detach().cpu().numpy()
    t = np.asarray(tags)
    if t.dtype.kind not in "iu":
        raise ValueError(f"tags must be integers, got dtype {t.dtype}")
    t = t.astype(np.int64)
    if t.ndim == 0:
        t = np.full(nq, int(t), dtype=np.int64)
    t = t.reshape(-1)
    if t.size != nq:
        raise ValueError(f"{t.size} tags for {nq} queries")
    if t.size and int(t.max()) >= TAG_LIMIT:
        raise ValueError(f"tags must be below 2^24 = {TAG_LIMIT}")
    return np.where(t < 0, -1, t).astype(np.int32)


def scope_mask(meta, count, tag=-1, newer_than=None, older_than=None, min_strength=None):
    """bool [rows of meta]: the rule for ONE query tag, restated with torch ops on any device."""
    m = meta.detach()
    ok = torch.zeros(m.shape[0], dtype=torch.bool, device=m.device)
    ok[:count] = True
    if tag is not None and tag >= 0:
        ok &= m[:, 3].to(torch.int32) == int(tag)
    if newer_than is not None:
        ok &= m[:, 1] >= torch.tensor(float(np.float32(newer_than)), dtype=torch.float32, device=m.device)
    if older_than is not None:
        ok &= m[:, 1] <= torch.tensor(float(np.float32(older_than)), dtype=torch.float32, device=m.device)
    if min_strength is not None:
        ok &= m[:, 0] >= torch.tensor(float(np.float32(min_strength)), dtype=torch.float32, device=m.device)
    return ok


def knn_search_scoped(bank, inv_norm, meta, queries, k, now, count, tags=None, newer_than=None, older_than=None,
                      min_strength=None, loc=None, q_loc=None, check_flag=True, splits=None):
    CALLS["scoped"] += 1
    nq = queries.shape[0]
    if not (1 <= k <= min(count, SCOPED_MAX_K)):
        raise ValueError(f"knn_search_scoped: k={k} must be in [1, min(count, {SCOPED_MAX_K})]")
    qt = scoped_query_tags(tags, nq)
    LAST_SCOPED.clear()
    LAST_SCOPED.update(k=k, now=now, count=count, tags=qt.copy(), newer_than=newer_than, older_than=older_than,
                       min_strength=min_strength, q_loc=q_loc, check_flag=check_flag)
    scores = torch.full((nq, k), -INF)
    rows = torch.full((nq, k), -1, dtype=torch.int32)
    m_norm = F.normalize(bank[:count], dim=1)
    temporal = torch.exp(-(now - meta[:count, 1]) / 3600.0)
    for i in range(nq):
        sim = torch.mm(F.normalize(queries[i:i + 1], dim=1), m_norm.t()).squeeze(0)
        sp = torch.zeros_like(sim)
        if q_loc is not None:
            sp = 1.0 / (1.0 + torch.norm(loc[:count] - q_loc[i], dim=1))
        comb = (0.5 * sim + 0.3 * sp + 0.2 * temporal) * meta[:count, 0]
        cand = torch.nonzero(scope_mask(meta, count, int(qt[i]), newer_than, older_than, min_strength)[:count]).flatten()
        if cand.numel():
            order = torch.sort(-comb[cand], stable=True).indices[:k]        # equal scores: the lower row first
            scores[i, :order.numel()], rows[i, :order.numel()] = comb[cand][order], cand[order].to(torch.int32)
    return scores, rows


# ---- the data of tests/test_gpu_scoped.py (and of the host tests that want the same scopes)
NOW = 1.7e9 + 777.0
QUERY_SCOPES = [1, 2, 3, 4, 5, 17, 40, -1]       # the 96 queries cycle through these (-1: any tag)
EXTRA_ROWS = 500                                  # rows of the bank beyond the held ones


def scoped_data(D, N, nq=96, seed=11):
    """Features, strengths, fp32 timestamps, locations, tags (shuffled) and queries: tag 1 has 1 row, tag 2 has 7 (fewer
    than k = 8), tag 3 has 130 (straddles a 128-row tile), tag 4 about 45 % of the rows, 200 rows are untagged and tags
    5 .. 40 share the rest evenly (about 80 rows each at N = 6000)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(N, D, generator=g)
    strength = 0.25 + 0.75 * torch.rand(N, generator=g)
    ts = (NOW - 128.0 * torch.randint(0, 60, (N,), generator=g).double()).float()
    locs = torch.randn(N, 2, generator=g)
    n4 = int(0.45 * N)
    sizes = {1: 1, 2: 7, 3: 130, 4: n4, 0: 200}
    rest = N - sum(sizes.values())
    tags = [t for t, n in sizes.items() for _ in range(n)]
    tags += [5 + (i % 36) for i in range(rest)]
    tags = torch.tensor(tags, dtype=torch.int64)[torch.randperm(N, generator=g)]
    q = torch.randn(nq, D, generator=g)
    q_loc = torch.randn(nq, 2, generator=g)
    qtags = np.asarray([QUERY_SCOPES[i % len(QUERY_SCOPES)] for i in range(nq)], dtype=np.int64)
    return dict(feats=feats, strength=strength, ts=ts, locs=locs, tags=tags.numpy(), q=q, q_loc=q_loc, qtags=qtags)
