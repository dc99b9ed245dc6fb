"""The rule of ``include/aura_hip.h`` ("Poisson bridge") in NumPy -- TEST INFRASTRUCTURE ONLY.

The generator in exact integers (``philox4x32_10`` of ``tests/cpu_stub_replay.py``), the probability in fp64 with its
derived fp32 bound, the decision ``u < q`` and the rate exactly as the rule states them, and an fp32 restatement of the
projection for the CPU stand-in.  The rate is ``count * fl(1 / T)``, the bits of torch's mean on the GPU; torch's mean on
the CPU is ``count / T``, which differs in the last bit for some (count, T), so the CPU stand-in takes torch's.

The bound of ``q``.  z = fl(dot_K + b) with dot_K a chain of K fmaf: the chain's error is at most K e sum|x_k W_k| to first
order (every partial sum is bounded by sum|x_k W_k|, e = 2^-24 the unit roundoff), the bias add rounds once more, and the
second-order terms are covered by entering K + 8 for K + 1 ("Row linear"'s form):
    dz = |z - z64| <= (K + 8) e (sum_k |x_k W_k| + |b|).
The sigmoid's slope is at most 1/4 everywhere, so the dot's share of the error of q is at most dz / 4.  The sigmoid's own
roundings: E = expf(-z) has 1 ulp = 2 e relative error, 1 + E rounds once (e), so fl(1 + E) has relative error at most
2 e E / (1 + E) + e <= 3 e, and the division rounds once more (e): at most 4 e relative, entered as 4.5 e for the second
order, on q64 + dz / 4.  Where E overflows (z < -88.7) the kernel's q is exactly 0 and q64 < 2^-126, and where q is
subnormal its rounding is absolute: one term of 2^-126 covers both.
    |q - q64| <= dz / 4 + 4.5 e (q64 + dz / 4) + 2^-126."""
import numpy as np

from tests.cpu_stub_replay import philox4x32_10

E24 = 2.0 ** -24
TINY = 2.0 ** -126
MAX_K, MAX_H, MAX_T = 256, 4096, 64


def key_of(seed):
    s = int(seed)
    return s & 0xFFFFFFFF, s >> 32


def words(c, j, p, s, seed):
    """The four words (uint64 arrays holding 32 bits) of counter (c, j, p, s) under ``seed``; broadcastable arrays."""
    return philox4x32_10((c, j, p, s), key_of(seed))


def uniform_of(word):
    """``u = ((word >> 9) + 0.5) * 2^-23`` in fp32 (every operation exact)."""
    q = (np.asarray(word, dtype=np.uint64) >> np.uint64(9)).astype(np.int64)
    return (q.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def row_addresses(N, streams=None, rows_per_stream=None, start=0):
    """``(stream uint64 [N], position uint64 [N])`` of every row: row ``n = b S + i`` has stream ``streams[b]`` and
    position ``start[b] + i``; the default is stream ``n``, one row each."""
    if streams is None:
        streams, S = np.arange(N, dtype=np.uint64), 1
    else:
        streams, S = np.asarray(streams, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF), int(rows_per_stream)
    B = N // S
    assert B * S == N and streams.shape == (B,)
    st = np.broadcast_to(np.asarray(start, dtype=np.int64), (B,)).astype(np.uint64)
    i = np.arange(S, dtype=np.uint64)
    return np.repeat(streams, S), (st[:, None] + i[None, :]).reshape(N) & np.uint64(0xFFFFFFFF)


def uniforms(H, T, stream, position, seed):
    """fp32 [N, T, H]: u of the rule for every (row, timestep, channel)."""
    stream, position = np.asarray(stream, dtype=np.uint64), np.asarray(position, dtype=np.uint64)
    N, groups = stream.shape[0], (T + 3) // 4
    c = np.arange(H, dtype=np.uint64)[None, None, :]
    j = np.arange(groups, dtype=np.uint64)[None, :, None]
    w = words(c, j, position[:, None, None], stream[:, None, None], seed)            # 4 x [N, groups, H]
    u = np.stack([uniform_of(x) for x in w], axis=2)                                    # [N, groups, 4, H]
    return np.ascontiguousarray(u.reshape(N, 4 * groups, H)[:, :T])


def spikes_of(q, u):
    """fp32 [N, T, H]: ``u < q`` (false for a NaN q) from the fp32 probabilities ``q`` [N, H]."""
    q = np.asarray(q, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (u < q[:, None, :]).astype(np.float32)


def rate_of(spikes):
    """fp32 [N, H]: ``float(count) * fl(1 / float(T))``: the sum times the rounded reciprocal, as torch's device mean."""
    T = spikes.shape[1]
    out = spikes.sum(axis=1, dtype=np.float64).astype(np.float32) * (np.float32(1.0) / np.float32(T))
    assert out.dtype == np.float32
    return out


def probability64(x, W, b=None):
    """``(q64, bound)`` [N, H]: the fp64 probability on the fp32 inputs and the derived bound of the kernel's fp32 q
    (see the module's docstring).  Rows that are not finite give NaN bounds."""
    x64, W64 = np.asarray(x, dtype=np.float64), np.asarray(W, dtype=np.float64)
    K = x64.shape[1]
    with np.errstate(all="ignore"):
        z = x64 @ W64.T
        mag = np.abs(x64) @ np.abs(W64).T
        if b is not None:
            z = z + np.asarray(b, dtype=np.float64)
            mag = mag + np.abs(np.asarray(b, dtype=np.float64))
        q = 1.0 / (1.0 + np.exp(-z))
        dz = (K + 8) * E24 * mag
        bound = dz / 4 + 4.5 * E24 * (q + dz / 4) + TINY
    return q, bound


def dot_order(K):
    """The k order of the rule's chain: per block of eight, b, b + 4, b + 1, b + 5, b + 2, b + 6, b + 3, b + 7 (below K)."""
    order = []
    for b in range(0, K, 8):
        order += [k for k in (b, b + 4, b + 1, b + 5, b + 2, b + 6, b + 3, b + 7) if k < K]
    return order


def probability32(x, W, b=None):
    """fp32 [N, H]: the rule's op sequence with the fmaf chain emulated through fp64 (the product is exact there; the
    sum is rounded twice, so the last bit may differ from the device's: for the stand-in, not for bits)."""
    x, W = np.asarray(x, dtype=np.float32), np.asarray(W, dtype=np.float32)
    t = np.zeros((x.shape[0], W.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in dot_order(x.shape[1]):
            t = (x[:, k].astype(np.float64)[:, None] * W[:, k].astype(np.float64)[None, :] + t).astype(np.float32)
        z = t if b is None else t + np.asarray(b, dtype=np.float32)
        q = np.float32(1.0) / (np.float32(1.0) + np.exp(-z))
    assert q.dtype == np.float32
    return q


def bridge(x, W, b, T, seed, streams=None, rows_per_stream=None, start=0, q=None):
    """``(rate, q, spikes)`` of the rule; ``q`` given: the decision on those probabilities (a kernel's own)."""
    N, H = np.asarray(x).shape[0], np.asarray(W).shape[0]
    s, p = row_addresses(N, streams, rows_per_stream, start)
    q = probability32(x, W, b) if q is None else np.asarray(q, dtype=np.float32)
    spikes = spikes_of(q, uniforms(H, T, s, p, seed))
    return rate_of(spikes), q, spikes
