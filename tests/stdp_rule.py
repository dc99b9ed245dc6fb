"""The STDP rule of ``include/aura_hip.h`` ("STDP") restated in NumPy, as test infrastructure: the traces in fp32
exactly as written (two roundings per step), ``dW`` in fp64 from those fp32 traces, and the per-element magnitude sum
``S`` that the tolerances are stated in.  Nothing here is measured on a device."""
import numpy as np

U24 = 2.0 ** -24
U23 = 2.0 ** -23


def traces(pre, post, lambda_pre, lambda_post, x0=None, y0=None):
    """``pre`` [B, T, I], ``post`` [B, T, O] (any float dtype; taken to fp32, which is exact for fp32 and bf16 values).
    Returns ``(x [B, T, I], y_before [B, T, O], x_final [B, I], y_final [B, O])``, all fp32: ``x`` includes its step,
    ``y_before`` is the post trace at its step before the step's own spike, ``fl(lambda_post * y[t-1])``."""
    pre = np.asarray(pre, dtype=np.float32)
    post = np.asarray(post, dtype=np.float32)
    B, T, I = pre.shape
    O = post.shape[2]
    lp, lq = np.float32(lambda_pre), np.float32(lambda_post)
    x = np.zeros((B, I), np.float32) if x0 is None else np.asarray(x0, dtype=np.float32).copy()
    y = np.zeros((B, O), np.float32) if y0 is None else np.asarray(y0, dtype=np.float32).copy()
    xs = np.empty((B, T, I), np.float32)
    yb = np.empty((B, T, O), np.float32)
    for t in range(T):
        x = (lp * x).astype(np.float32) + pre[:, t]           # fp32 product, then fp32 sum: two roundings
        yb[:, t] = (lq * y).astype(np.float32)                # y at step t before the step's own spike
        y = yb[:, t] + post[:, t]
        xs[:, t] = x
    assert x.dtype == np.float32 and y.dtype == np.float32
    return xs, yb, x, y


def expand_pre(pre, T):
    """A time-invariant ``pre`` [B, I] as [B, T, I]."""
    pre = np.asarray(pre)
    return np.repeat(pre[:, None, :], T, axis=1)


def rule(pre, post, lambda_pre, lambda_post, a_plus, a_minus, x0=None, y0=None):
    """``(dW [O, I] fp64, S [O, I] fp64, x_final fp32, y_final fp32)`` with the amplitudes as their fp32 values."""
    xs, yb, xf, yf = traces(pre, post, lambda_pre, lambda_post, x0, y0)
    pre64 = np.asarray(pre, dtype=np.float32).astype(np.float64)
    post64 = np.asarray(post, dtype=np.float32).astype(np.float64)
    B = pre64.shape[0]
    ap, am = float(np.float32(a_plus)), float(np.float32(a_minus))
    ltp = np.einsum("bto,bti->oi", post64, xs.astype(np.float64))
    ltd = np.einsum("bto,bti->oi", yb.astype(np.float64), pre64)
    dw = (ap * ltp - am * ltd) / B
    s = (abs(ap) * np.einsum("bto,bti->oi", np.abs(post64), np.abs(xs).astype(np.float64))
         + abs(am) * np.einsum("bto,bti->oi", np.abs(yb).astype(np.float64), np.abs(pre64))) / B
    return dw, s, xf, yf


def dw_bound(B, T, s):
    """``|dW_dev - dW_64| <= (2 B T + 8) 2^-24 S``: any summation order of the 2 B T terms plus the operand and output
    scalings."""
    return (2 * B * T + 8) * U24 * s


def apply(w, dw, lr, w_min, w_max):
    """``W'`` in fp64 from the fp32 weights and the fp64 ``dW`` (``lr`` as its fp32 value)."""
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.clip(w64 + float(np.float32(lr)) * dw, w_min, w_max)


def w_bound(B, T, s, lr, w, w_new):
    """``|W'_dev - W'_64| <= lr * dw_bound + 2^-23 max(|W|, |W'|)``; the clamp is 1-Lipschitz, so nothing is excluded."""
    w64 = np.abs(np.asarray(w, dtype=np.float64))
    return abs(float(np.float32(lr))) * dw_bound(B, T, s) + U23 * np.maximum(w64, np.abs(w_new))


def to_bf16_exact(a):
    """Round an fp32 array to the nearest bf16 value (ties to even), returned as fp32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def spikes(rng, shape, density, levels=8):
    """Multi-bit spikes as the GIF loops emit them: 0 with probability ``1 - density``, else a level in 1 .. levels."""
    on = rng.random(shape) < density
    return (on * rng.integers(1, levels + 1, shape)).astype(np.float32)
