"""The place-code rule of ``include/aura_hip.h`` ("Place code") restated in NumPy, as test infrastructure: the winners by
a stable sort on ``(-value, cell)`` with -0 = +0 and NaN above +inf, everything else in fp64 on the given fp32 inputs,
and the magnitude sums the tolerances are stated in.  Nothing here is measured on a device."""
import numpy as np

U22, U23, U24 = 2.0 ** -22, 2.0 ** -23, 2.0 ** -24
TENTH = float(np.float32(0.1))                     # the rule's 0.1f


def winners(z, k):
    """``idx`` [N, k] int32: per row of the fp32 logits ``z`` [N, P] the top ``k`` cells -- larger value first, -0.0 and
    +0.0 equal, any NaN above +inf (all NaNs equal), equal values to the lower cell -- in ascending cell index."""
    z = np.asarray(z, dtype=np.float32)
    N, P = z.shape
    assert 1 <= k <= P
    nan = np.isnan(z)
    v = np.where(nan, 0.0, z.astype(np.float64))
    v = np.where(v == 0.0, 0.0, v)                 # -0.0 -> +0.0
    cell = np.broadcast_to(np.arange(P), (N, P))
    out = np.empty((N, k), np.int32)
    for n in range(N):
        # lexsort: the LAST key is the primary one.  NaN first, then descending value, then ascending cell.
        order = np.lexsort((cell[n], -v[n], ~nan[n]))
        out[n] = np.sort(order[:k])
    return out


def sigmoid64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float32).astype(np.float64)))


def rule(z, e, w2t, b2, k):
    """``dict(idx [N, k] int32, act [N, k], out [N, D], dense [N, P], mag [N, D])``, the last four fp64:
    ``act = 1 / (1 + exp(-z))`` at the winners, ``out = e + 0.1f (sum_j act_j W2t[j] + b2)``, ``dense`` zero except
    ``act`` at the winners, ``mag = sum_j |act_j W2t[j]| + |b2|``."""
    z = np.asarray(z, dtype=np.float32)
    e64, w64, b64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (e, w2t, b2))
    N, P = z.shape
    idx = winners(z, k)
    act = sigmoid64(np.take_along_axis(z, idx.astype(np.int64), axis=1))
    out = np.empty_like(e64)
    mag = np.empty_like(e64)
    with np.errstate(invalid="ignore"):
        for n in range(N):
            rows = w64[idx[n]]                                             # [k, D]
            out[n] = e64[n] + TENTH * (act[n] @ rows + b64)
            mag[n] = np.abs(act[n]) @ np.abs(rows) + np.abs(b64)
    dense = np.zeros((N, P), np.float64)
    np.put_along_axis(dense, idx.astype(np.int64), act, axis=1)
    return dict(idx=idx, act=act, out=out, dense=dense, mag=mag)


def out_bound(k, mag, out64):
    """``|out - out_64| <= 0.1 (k + 2) 2^-24 mag + 2^-23 |out_64|``: k fused steps, the bias add, the scaling, and the
    residual add relative to the result."""
    return 0.1 * (k + 2) * U24 * mag + U23 * np.abs(out64)


def backward(g_out, g_dense, idx, act, w2t):
    """``(g_z [N, P] fp64, absdot [N, k] fp64)`` from the fp32 inputs of the backward launch:
    ``g_z[n, j] = (0.1f <g_out[n], W2t[j]> + g_dense[n, j]) act (1 - act)`` at the winners, 0 elsewhere;
    ``absdot = sum_d |g_out[n, d] W2t[j, d]|``."""
    g64, w64, a64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (g_out, w2t, act))
    idx = np.asarray(idx).astype(np.int64)
    N, k = idx.shape
    P = w64.shape[0]
    g_z = np.zeros((N, P), np.float64)
    absdot = np.empty((N, k), np.float64)
    for n in range(N):
        rows = w64[idx[n]]
        g_act = TENTH * (rows @ g64[n])
        if g_dense is not None:
            g_act = g_act + np.asarray(g_dense[n], dtype=np.float32).astype(np.float64)[idx[n]]
        g_z[n, idx[n]] = g_act * a64[n] * (1.0 - a64[n])
        absdot[n] = np.abs(rows) @ np.abs(g64[n])
    return g_z, absdot


def g_z_bound(D, absdot, g_z64_at_winners, g_dense_at_winners=None):
    """``|g_z - g_z64| <= (D + 3) 2^-24 * 0.1 * absdot * 0.25 + 2^-23 |g_z64|`` at the winners (any order of the D-term
    dot product, its scaling and the two products with ``act (1 - act) <= 1/4``).  With a ``g_dense`` term, its add
    rounds once more relative to the larger of the two addends: ``+ 2^-24 (0.1 absdot + |g_dense|) * 0.25``."""
    b = (D + 3) * U24 * 0.1 * absdot * 0.25 + U23 * np.abs(g_z64_at_winners)
    if g_dense_at_winners is not None:
        b = b + U24 * (0.1 * absdot + np.abs(g_dense_at_winners)) * 0.25
    return b
