"""The rules of the centroid-index kernels (probe, assign, segment means, row norms) restated in NumPy, with the inputs
the host and the GPU tests share.  Test infrastructure: nothing here is measured on a device.

``u = 2^-24`` and ``gamma(n) = n u / (1 - n u)``.

Ranking key   ``aura_centroid_probe`` and ``aura_kmeans_assign`` rank the table rows c for a query x by
              ``key(x, c) = sum c_i^2 - 2 sum x_i c_i`` (the query's own norm is common to every row and never enters).
              ``key64`` is that expression in fp64 on the fp32 inputs; a computed key lies within
              ``E(x, c) = gamma(K) (sum c_i^2 + 2 sum |x_i c_i|)`` of it.
  K           counts the roundings the longest path through a term can meet, in every instance of either kernel:
              * the dot product is an accumulation of D products in some order (MFMA 16x16x4 steps in the probe, 32x32x2
                steps in assign, a k walk that starts at another stage per wave): a product rounds once and is then
                carried through at most D - 1 additions: D roundings, whatever the order (padding columns add exact zeros);
              * the squares are an fmaf chain per lane -- at most ceil(D / 4) links in the probe, ceil(D / 64) in
                ``row_norm2_kernel`` -- followed by the lane additions: two in the probe, six in the butterfly of
                ``row_norm2_kernel``.  A chain of D squares plus six additions covers both: D + 6;
              * ``fmaf(-2, dot, norm)`` (probe) and ``norm - 2 dot`` with an exact doubling (assign) round once more.
              So no term meets more than D + 7 roundings and ``(1 + u)^(D + 7) - 1 <= gamma(D + 7)``: K = D + 8 holds with
              one to spare.  (For D >= 8 the dot product's D + 1 is the longest path; the uniform D + 8 is kept so that
              the one formula also covers D = 3 and 4, where the butterfly is.)
Decisions     A returned list p_0 .. p_{n-1} is acceptable iff the ids are distinct and inside the table, for j < j'
              ``key64(p_j) <= key64(p_j') + E(p_j) + E(p_j')``, and for every row c that was not returned
              ``key64(c) >= key64(p_{n-1}) - E(c) - E(p_{n-1})``.
  exact ties  Rows of one *tie class* whose key64 are equal must come out lower id first (and a row left out must have a
              higher id than the last returned row of its class with the same key).  A class holds rows whose computed
              keys are bit-equal by construction: rows with the same bits that are summed in the same order.  For
              assign every row is summed alike (``tie_classes(table)``); for the probe the k walk depends on the row's
              32-row group, so only duplicates inside one group share a class (``tie_classes(table, group=32)``) --
              and all-zero rows, whose sums are exact zeros in any order, share one class everywhere.
  forced      The fp64 ranking (key ascending, then id) has n adjacent decisions per query: between ranks j and j + 1
              for j < n.  A decision is *forced* when the fp64 gap exceeds the two bounds, and only then.  Only forced
              decisions prove that the kernel's arithmetic agrees with fp64; the tests keep floors on their share (probe
              90 %, assign 99 %) and the floors are checked on the reference alone (test_host_index_rule).  Exact ties
              inside one class are counted apart (``class_ties``): they test the tie-break, not the key, and count
              towards no floor.  The inputs are built for the floors: the table rows and the queries share a mean, so
              that the non-zero rows have negative keys and come before the 56 zero rows (whose keys are all 0); the
              repeated centroid of assign stands apart and one bank row is placed at it.
Segment sums  ``segment_sum32`` restates the documented order of ``kmeans_partial_kernel`` / ``kmeans_reduce_kernel`` in
              float32: per chunk of 64 rows four accumulators take rows r, r+1, r+2, r+3 while four remain, the rest go
              to the first, ``s = (a0 + a1) + (a2 + a3)``; the chunks are added in order from zero; the mean divides by
              ``float(len)``.  The device must equal it bit for bit.  ``segment_bound64`` is the fp64 statement that
              guards the restatement: the sum within ``gamma(len + 2) sum |x|``, the mean within that over len.
Row norms     ``inv = 1 / max(||x||, 1e-12)``: ``|inv ||x||_64 - 1| <= gamma(D + 4)`` (the chain and butterfly of the
              squares, halved by the root, then the root and the reciprocal), ``1 / 1e-12f`` for a zero row.
Merge         ``oracle.aura_oracle.merge_topk`` is the rule; nothing is restated here."""
import functools

import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def key_K(D):
    return D + 8


# ------------------------------------------------------------------------------------------------------ ranking key
def key64(x, table):
    """(key64 [nq, T], E [nq, T]) of fp32 queries x [nq, D] against fp32 rows table [T, D]."""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(table, dtype=np.float64)
    dot = x @ c.T
    adot = np.abs(x) @ np.abs(c).T
    n2 = (c * c).sum(1)
    return n2[None, :] - 2.0 * dot, gamma(key_K(x.shape[1])) * (n2[None, :] + 2.0 * adot)


def tie_classes(table, group=None):
    """Class label per row: the lowest id among the rows with the same bits (inside the row's ``group``-row block when
    ``group`` is given); every all-zero row is in class -1."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    cls = np.arange(t.shape[0])
    first = {}
    for i in range(t.shape[0]):
        if not t[i].any():
            cls[i] = -1
            continue
        k = (t[i].tobytes(), None if group is None else i // group)
        cls[i] = first.setdefault(k, i)
    return cls


def fp64_ranking(key, E, cls, n):
    """The fp64 ranking's first n ids per query [nq, n], which of its n adjacent decisions are forced by the gap
    [nq, n] (decisions that do not exist, n == T, count as forced) and which are exact ties inside one class [nq, n]."""
    nq, T = key.shape
    ids = np.broadcast_to(np.arange(T), key.shape)
    order = np.lexsort((ids, key), axis=1)                                  # key ascending, then id
    m = min(T, n + 1)
    o = order[:, :m]
    k = np.take_along_axis(key, o, 1)
    e = np.take_along_axis(E, o, 1)
    c = cls[o]
    forced = np.ones((nq, n), dtype=bool)
    gap = k[:, 1:] - k[:, :-1]
    forced[:, :m - 1] = gap > e[:, 1:] + e[:, :-1]
    ties = np.zeros((nq, n), dtype=bool)
    ties[:, :m - 1] = (gap == 0) & (c[:, 1:] == c[:, :-1])
    return order[:, :n], forced, ties


def check_decisions(key, E, cls, ids):
    """Hold returned ids [nq, n] to the decision rule.  Returns (problems, worst): a list of strings (empty: accepted)
    and the worst used share of a bound among the decisions that went against fp64."""
    key = np.asarray(key); E = np.asarray(E); ids = np.asarray(ids).astype(np.int64)
    nq, T = key.shape
    n = ids.shape[1]
    bad = []
    if ids.min() < 0 or ids.max() >= T:
        return [f"ids outside [0, {T})"], float("inf")
    srt = np.sort(ids, axis=1)
    if n > 1 and bool((srt[:, 1:] == srt[:, :-1]).any()):
        bad.append("ids repeat")
    kp = np.take_along_axis(key, ids, 1)
    ep = np.take_along_axis(E, ids, 1)
    cp = cls[ids]
    worst = 0.0

    def share(excess, room):
        nonlocal worst
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(excess > 0, excess / room, 0.0)                     # room == 0 with an excess: inf
        if s.size:
            worst = max(worst, float(np.nanmax(s)))

    for j in range(n):
        for j2 in range(j + 1, n):
            room = ep[:, j] + ep[:, j2]
            excess = kp[:, j] - kp[:, j2]
            share(excess, room)
            v = np.nonzero((excess > room) | ((excess == 0) & (cp[:, j] == cp[:, j2]) & (ids[:, j] > ids[:, j2])))[0]
            if v.size:
                q = int(v[0])
                bad.append(f"{v.size} queries order ranks {j}, {j2} against the rule (query {q}: ids {ids[q].tolist()})")
    out = np.ones((nq, T), dtype=bool)
    np.put_along_axis(out, ids, False, 1)
    room = E + ep[:, -1:]
    excess = kp[:, -1:] - key
    share(np.where(out, excess, 0.0), room)
    tie = (excess == 0) & (cls[None, :] == cp[:, -1:]) & (np.arange(T)[None, :] < ids[:, -1:])
    v = np.nonzero((out & ((excess > room) | tie)).any(1))[0]
    if v.size:
        q = int(v[0])
        c = int(np.nonzero(out[q] & ((excess[q] > room[q]) | tie[q]))[0][0])
        bad.append(f"{v.size} queries leave out a row the rule requires (query {q}: row {c}, ids {ids[q].tolist()})")
    return bad, worst


# ---------------------------------------------------------------------------------------------------- segment sums
def segment_sum32(rows):
    """float32 sum of rows [len, D] (in segment order) in the kernels' documented order."""
    rows = np.asarray(rows, dtype=np.float32)
    total = np.zeros(rows.shape[1], dtype=np.float32)
    for c0 in range(0, rows.shape[0], 64):
        chunk = rows[c0:c0 + 64]
        cnt = chunk.shape[0]
        a = np.zeros((4, rows.shape[1]), dtype=np.float32)
        n4 = cnt // 4 * 4
        for r in range(0, n4, 4):
            a[0] += chunk[r]; a[1] += chunk[r + 1]; a[2] += chunk[r + 2]; a[3] += chunk[r + 3]
        for r in range(n4, cnt):
            a[0] += chunk[r]
        total = total + ((a[0] + a[1]) + (a[2] + a[3]))
    return total


def segment_mean32(rows):
    return segment_sum32(rows) / np.float32(rows.shape[0])


def segment_bound64(rows, mean):
    """(fp64 value [D], bound [D]) of the sum (``mean`` False) or the mean of rows [len, D]."""
    x = np.asarray(rows, dtype=np.float64)
    n = x.shape[0]
    s, b = x.sum(0), gamma(n + 2) * np.abs(x).sum(0)
    return (s / n, b / n) if mean else (s, b)


def row_norm_bound(D):
    return gamma(D + 4)


INV_OF_ZERO_ROW = np.float32(1.0) / np.float32(1e-12)


# ----------------------------------------------------------------------------------------------------- shared inputs
PROBE_DIMS = (4, 40, 50, 60, 64, 68, 768, 1024, 1028, 1030, 2048)
PROBE_SMALL_BATCH_DIMS = (40, 768)           # nq in {1, 15, 16, 17} besides 300
PROBE_SMALL_BATCHES = (1, 15, 16, 17)
PROBE_MISALIGNED_DIMS = (64, 1028)           # an offset view (base 4 bytes past a 16-byte boundary): scalar loads
PROBE_NQ = 300
PROBE_ZERO_Q, PROBE_BIG_Q, PROBE_EQUAL_Q = 20, 24, 28    # the special queries (behind the small batches)
PROBE_DUP = (7, 20, 100)                     # rows 20 (same 32-row group) and 100 (another group) repeat row 7
PROBE_FLOOR = 0.90
ASSIGN_CASES = ((1, 4, 1), (127, 3, 31), (128, 32, 32), (129, 33, 33), (1000, 100, 200), (2000, 768, 256),
                (300, 1028, 7))
ASSIGN_MISALIGNED = (128, 32, 32)
ASSIGN_FLOOR = 0.99
MEANS_DIMS = (4, 8, 100, 256, 260, 768)
MEANS_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 321)     # clusters 0 .. 11 of k = 16; 12 .. 15 are empty
MEANS_UNLISTED = 37                          # rows with id -1: seg_off[0]
MEANS_SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def probe_case(D):
    """(table [256, D], queries [300, D]) fp32.  Table: rows 0 .. 199 Gaussian, 200 .. 255 zero (the reference keeps the
    rows beyond centroids_k zero), rows 20 and 100 copies of row 7.  Queries, all of scale s = max(1, 0.45 sqrt(D)): the
    even ones s times a Gaussian, the odd ones s times (a centroid plus 0.3 noise), every twentieth of those row 7, the
    repeated one; then the zero query, a query of norm 1e3 and a query bit-equal to row 7 (behind the first 17 queries:
    the small batches hold ordinary queries only).  The scale is there for the floor: key(c) = |c|^2 - 2 x.c is about
    D - 2 s sqrt(D) z, negative for the dozens of rows with z > 1.1, so the nearest rows of every query but the zero
    query are non-zero rows that compete through the key's arithmetic.  At unit scale the 56 zero rows (key 0) are the
    nearest of most queries once D >= 40 and most decisions are ties of 0 against 0."""
    g = np.random.default_rng(1000 + D)
    scale = np.float32(max(1.0, 0.45 * np.sqrt(D)))
    table = np.zeros((256, D), dtype=np.float32)
    table[:200] = g.standard_normal((200, D)).astype(np.float32)
    table[PROBE_DUP[1]] = table[PROBE_DUP[0]]
    table[PROBE_DUP[2]] = table[PROBE_DUP[0]]
    q = g.standard_normal((PROBE_NQ, D)).astype(np.float32)
    which = g.integers(0, 200, PROBE_NQ)
    near = np.arange(PROBE_NQ) % 2 == 1
    which[np.nonzero(near)[0][10::20]] = PROBE_DUP[0]
    q[near] = table[which[near]] + np.float32(0.3) * q[near]
    q *= scale
    q[PROBE_ZERO_Q] = 0.0
    big = q[PROBE_BIG_Q].astype(np.float64)
    q[PROBE_BIG_Q] = (big * (1e3 / np.linalg.norm(big))).astype(np.float32)
    q[PROBE_EQUAL_Q] = table[PROBE_DUP[0]]
    return table, q


@functools.lru_cache(maxsize=None)
def probe_reference(D):
    """(key64, E, tie classes) of probe_case(D)."""
    table, q = probe_case(D)
    k, e = key64(q, table)
    return k, e, tie_classes(table, group=32)


@functools.lru_cache(maxsize=None)
def assign_case(N, D, k):
    """(bank [N + 5, D], table [256, D]) fp32; the call assigns rows [0, N) to the first k table rows.  Centroids are
    Gaussians of scale 3; centroid 5 is zero, centroids 9 and 40 repeat centroid 3 (each where k reaches it), which
    stands apart at four times the others' norm so that only the row placed at it, row 4, is undecided between the
    copies; table rows >= k are copies of bank rows, so that a kernel that ignored k would choose them.  Bank rows by
    i % 4: 0 and 2 a centroid (never 3, 9 or 40) plus unit noise, 1 a unit Gaussian, 3 a centroid plus noise of the
    centroids' own scale; row 2 is zero."""
    g = np.random.default_rng(2000 + 7 * N + D)
    table = (3.0 * g.standard_normal((256, D))).astype(np.float32)
    if k > 5:
        table[5] = 0.0
    if k > 9:
        table[3] *= np.float32(4.0)
    for d in (9, 40):
        if k > d:
            table[d] = table[3]
    bank = g.standard_normal((N + 5, D)).astype(np.float32)
    which = g.integers(0, k, N + 5)
    if k > 9:
        which[np.isin(which, (3, 9, 40))] = 0
    i = np.arange(N + 5)
    bank[i % 2 == 0] += table[which[i % 2 == 0]]
    bank[i % 4 == 3] = table[which[i % 4 == 3]] + np.float32(3.0) * bank[i % 4 == 3]
    if N > 2:
        bank[2] = 0.0
    if k > 9 and N > 4:
        bank[4] = table[3] + g.standard_normal(D).astype(np.float32)
    table[k:] = bank[np.arange(256 - k) % N]
    return bank, table


@functools.lru_cache(maxsize=None)
def assign_reference(N, D, k):
    bank, table = assign_case(N, D, k)
    key, e = key64(bank[:N], table[:k])
    return key, e, tie_classes(table[:k])


def means_layout(lengths, unlisted, seed, extra_rows=3):
    """(order int32 [n], seg_off int32 [k + 1], rows M) for built segments: ``unlisted`` rows with no cluster first, then
    cluster c's ``lengths[c]`` rows; the row ids are a shuffle of [0, n), so every segment lists scattered rows in no
    order."""
    g = np.random.default_rng(seed)
    n = unlisted + int(sum(lengths))
    order = g.permutation(n).astype(np.int32)
    seg_off = (unlisted + np.concatenate([[0], np.cumsum(lengths)])).astype(np.int32)
    return order, seg_off, n + extra_rows


@functools.lru_cache(maxsize=None)
def means_case(D, integers=False):
    """(bank [M, D], order, seg_off, k = 16) for MEANS_LENGTHS.  Real rows: Gaussians times 10^(-2 .. 2) per row, so that
    the order of the additions shows in the last bits; ``integers``: whole numbers in [-64, 64] (every partial sum is
    exact in fp32)."""
    lengths = MEANS_LENGTHS + (0, 0, 0, 0)
    order, seg_off, M = means_layout(lengths, MEANS_UNLISTED, 3000 + D)
    g = np.random.default_rng(4000 + D)
    if integers:
        bank = g.integers(-64, 65, (M, D)).astype(np.float32)
    else:
        bank = (g.standard_normal((M, D)) * 10.0 ** g.integers(-2, 3, (M, 1))).astype(np.float32)
    return bank, order, seg_off, 16


@functools.lru_cache(maxsize=None)
def means_case_full(D=100, length=65):
    """k = 256 with every cluster ``length`` rows long.  65: 512 partial items, the most per row the workspace formula
    must hold.  (16640 x D stays under the largest tensor of these tests, 2000 x 2048, only for D <= 246: the two column
    slices of ``kmeans_reduce_kernel`` at all 256 clusters are reached with D = 260 and 17-row clusters.)"""
    order, seg_off, M = means_layout((length,) * 256, 0, 3500 + D)
    g = np.random.default_rng(4500 + D)
    return g.standard_normal((M, D)).astype(np.float32), order, seg_off, 256


def means_expected(bank, order, seg_off, k, mean):
    """Per cluster c < k: None when empty, else (fp32 restatement [D], fp64 value [D], bound [D])."""
    out = []
    for c in range(k):
        rows = bank[order[seg_off[c]:seg_off[c + 1]]]
        if rows.shape[0] == 0:
            out.append(None)
            continue
        v32 = segment_mean32(rows) if mean else segment_sum32(rows)
        out.append((v32,) + segment_bound64(rows, mean))
    return out
