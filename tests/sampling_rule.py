"""The rule of ``include/aura_hip.h`` ("Next token") in NumPy -- TEST INFRASTRUCTURE ONLY.

Two sides.  The fp32 side restates what contains no transcendental and is therefore checked for equality: the cleaning,
the correctly rounded penalty and temperature divisions (NumPy's fp32 ``/`` and ``*`` are correctly rounded), the
ranking by (z descending, id ascending), the blocked prefix sum of given terms and the nucleus from given prefix sums.
The fp64 side gives what the device's ``expf`` / ``logf`` are measured against: ``exp``, prefix sums and
``-log(-log u)``.  The Philox words and the uniforms come from ``tests/cpu_stub_replay.py``.

Everything is vectorised over rows: ``z`` is [N, V]."""
import numpy as np

from tests.cpu_stub_replay import philox4x32_10, uniforms

MAX_K, MAX_V, BLOCK = 1024, 131072, 16
FLT_MAX = np.finfo(np.float32).max
RULES = ("divide", "signed")
NINF = np.float32(-np.inf)


# ------------------------------------------------------------------------------------------------------ fp32 side
def clean(z):
    """Step 1: NaN -> -inf, +inf -> FLT_MAX; -0 -> +0 (it counts as +0 wherever values are ranked or returned)."""
    z = np.array(z, dtype=np.float32, copy=True)
    z[np.isnan(z)] = NINF
    z[z > FLT_MAX] = FLT_MAX
    return z + np.float32(0.0)


def _clamp(z):
    z = np.where(z > FLT_MAX, FLT_MAX, z).astype(np.float32)
    return z + np.float32(0.0)


def penalise(z, seen, penalty, rule="divide"):
    """Steps 1 and 2 on fp32 ``z`` [N, V] with ``seen`` [N, V] (anything non-zero counts) or None."""
    assert rule in RULES
    z = clean(z)
    p = np.float32(penalty)
    if seen is None or p == np.float32(1.0):
        return z
    with np.errstate(over="ignore", invalid="ignore"):
        q = z / p
        if rule == "signed":
            q = np.where(z < 0, z * p, q)
    assert q.dtype == np.float32
    return np.where(np.asarray(seen) != 0, _clamp(q), z).astype(np.float32)


def temper(z, temperature):
    """Step 4: a correctly rounded division, +inf back to FLT_MAX."""
    with np.errstate(over="ignore"):
        q = np.asarray(z, dtype=np.float32) / np.float32(temperature)
    assert q.dtype == np.float32
    return _clamp(q)


def greedy(z):
    """Step 3 on penalised ``z`` [N, V]: the argmax, equal z -> the lower id; -1 for a row without a z > -inf."""
    tok = np.argmax(z, axis=1).astype(np.int64)                  # (the first of equal maxima)
    return np.where(z[np.arange(z.shape[0]), tok] > NINF, tok, -1)


def rank(z, top_k):
    """Step 5: ``(ids int32 [N, k'], z [N, k'])``, the first k' = min(top_k, V) tokens by (z descending, id ascending)."""
    k = min(int(top_k), z.shape[1])
    order = np.argsort(-z, axis=1, kind="stable")[:, :k]         # stable: equal z keep the lower id first
    return order.astype(np.int32), np.take_along_axis(z, order, axis=1)


def prefix_sums32(e):
    """The rule's blocked inclusive prefix sum of fp32 terms [N, k] in rank order (blocks of 16 ranks)."""
    e = np.asarray(e, dtype=np.float32)
    N, k = e.shape
    c = np.zeros((N, k), dtype=np.float32)
    base = np.zeros(N, dtype=np.float32)
    for b0 in range(0, k, BLOCK):
        run = np.zeros(N, dtype=np.float32)
        for j in range(b0, min(k, b0 + BLOCK)):
            run = run + e[:, j]
            c[:, j] = base + run
        base = base + run
    assert c.dtype == np.float32
    return c


def kept_from_cum(c, top_p):
    """Step 6 from given prefix sums [N, k] (fp32): bool [N, k].  An empty row (S == 0 with nothing finite) is the
    caller's to mask."""
    c = np.asarray(c, dtype=np.float32)
    tp = np.float32(top_p)
    keep = np.ones(c.shape, dtype=bool)
    if tp >= np.float32(1.0):
        return keep
    thr = tp * c[:, -1]
    assert thr.dtype == np.float32
    keep[:, 1:] = c[:, :-1] <= thr[:, None]
    return keep


def words(ids, streams, seed, step):
    """x of step 7 for token ``ids`` [N, k], ``streams`` [N] and ``step`` (an int or [N]) under ``seed``."""
    ids = np.asarray(ids).astype(np.uint64)
    st = np.asarray(streams, dtype=np.uint64).reshape(-1, 1)
    sp = np.asarray(step, dtype=np.uint64).reshape(-1, 1)
    m = np.uint64(0xFFFFFFFF)
    s = int(seed)
    return philox4x32_10((ids & m, st & m, sp & m, sp >> np.uint64(32)), (s & 0xFFFFFFFF, s >> 32))[0]


def gumbel32(u):
    with np.errstate(all="ignore"):
        g = -np.log(-np.log(np.asarray(u, dtype=np.float32)))
    assert g.dtype == np.float32
    return g


def argmax_kept(d, ids, live):
    """The token of step 7 from draw keys ``d`` [N, k], their ``ids`` and the ranks that may win (``live``): the
    largest d, equal d -> the lower id; -1 for a row where nothing may win."""
    d = np.where(live, np.asarray(d, dtype=np.float64), -np.inf)
    ids = np.asarray(ids).astype(np.int64)
    best = d.max(axis=1, keepdims=True)
    tie = live & (d == best)
    tok = np.where(tie, ids, np.iinfo(np.int64).max).min(axis=1)
    return np.where(live.any(axis=1), tok, -1)


def sample(z, seen=None, streams=None, *, penalty=1.0, rule="divide", temperature=1.0, top_k=50, top_p=0.9, seed=0,
           step=0):
    """The whole rule for rows ``z`` [N, V] in fp32 (NumPy's own exp / log stand in for expf / logf: the stub's
    arithmetic, not the device's bits).  ``step`` may be [N].  Returns a dict: ``token`` int64 [N] and, unless greedy,
    the inspection outputs ``ids``, ``z``, ``cum``, ``d``, ``kept``, ``n_kept`` (``top_k=0``: ``d`` [N, V] only)."""
    z = np.asarray(z, dtype=np.float32)
    N, V = z.shape
    streams = np.arange(N) if streams is None else np.asarray(streams)
    zp = penalise(z, seen, penalty, rule)
    if np.float32(temperature) == 0:
        return dict(token=greedy(zp))
    zt = temper(zp, temperature)
    if top_k == 0:
        assert np.float32(top_p) >= 1
        ids = np.broadcast_to(np.arange(V, dtype=np.int32), (N, V))
        live = zt > NINF
        with np.errstate(invalid="ignore"):
            d = np.where(live, zt + gumbel32(uniforms(words(ids, streams, seed, step))[1]), NINF).astype(np.float32)
        return dict(token=argmax_kept(d, ids, live), d=d)
    ids, zk = rank(zt, top_k)
    empty = ~(zk[:, :1] > NINF)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(empty, np.float32(0), np.exp(zk - zk[:, :1])).astype(np.float32)
    c = prefix_sums32(e)
    kept = kept_from_cum(c, top_p) & ~empty
    with np.errstate(invalid="ignore"):
        d = np.where(kept, zk + gumbel32(uniforms(words(ids, streams, seed, step))[1]), NINF).astype(np.float32)
    return dict(token=argmax_kept(d, ids, kept & (zk > NINF)), ids=ids, z=zk, cum=c, d=d, kept=kept,
                n_kept=kept.sum(axis=1).astype(np.int32))


# ------------------------------------------------------------------------------------------------------ fp64 side
def exp64(zk):
    """e64_j = exp(z_j - z_0) in fp64 from fp32 candidates [N, k] (an empty row gives zeros)."""
    zk = np.asarray(zk, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(zk - zk[:, :1])
    return np.where(np.isnan(e), 0.0, e)


def cum64(zk):
    return np.cumsum(exp64(zk), axis=1)


def kept_count64(zk, top_p):
    """How many ranks step 6 keeps in fp64 for ``top_p`` (a float: the tests scale it by 1 -+ eps)."""
    c = cum64(zk)
    if top_p >= 1:
        return np.full(c.shape[0], c.shape[1])
    return 1 + np.sum(c[:, :-1] <= top_p * c[:, -1:], axis=1)


def gumbel64(q):
    """-log(-log u) in fp64 with u exactly ((x >> 9) + 0.5) 2^-23 from the 23-bit integers ``q``."""
    u = (np.asarray(q, dtype=np.float64) + 0.5) * 2.0 ** -23
    return -np.log(-np.log(u))


def softmax64(zk, kept):
    """The exact distribution of the draw: softmax of the kept candidates' z, zero elsewhere."""
    e = np.where(kept, exp64(zk), 0.0)
    return e / e.sum(axis=1, keepdims=True)
