"""The row-linear rule of ``include/aura_hip.h`` ("Row linear") restated in NumPy, as test infrastructure: once in fp64
with the bounds, once in fp32 in the rule's own summation order.  Nothing here is measured on a device.
``u = 2^-24`` (half an ulp of a value in [1, 2)).

prologue  The LayerNorm is the one of "Theta-gamma" with the same row sum (a lane's elements in ascending order, then
          six butterfly steps), so ``tests/theta_gamma_rule.norm`` gives xh in fp64 and its bound ``dxh`` (its
          ``y_bound``: ``|gamma| dn + 2u |xh|``).  Without a prologue ``dxh = 0``.
dot       A sum of K products in any order errs by at most ``(K - 1) u' sum|xh_k w_k|`` with ``u' = u / (1 - K u)``; the
          fused multiply-add rounds once per term, so ``K u`` covers the chain and the butterfly; the bias adds one
          rounding of the result: ``(K + 8) u (sum_k |xh_k w_k| + |b|)`` has the slack for the second-order terms at
          K <= 8192 (K u < 5e-4).  The computed xh differs from the fp64 one by at most dxh, which moves the sum by
          ``sum_k |w_k| dxh_k`` and enters the first term through ``|xh| <= |xh64| + dxh``:
              dt = (K + 8) u (sum_k (|xh64_k| + dxh_k) |w_k| + |b|) + sum_k |w_k| dxh_k.
GELU      ``g(t) = 0.5 t (1 + erf(t / sqrt 2))``, ``|g'| <= 1.13``: the error of t arrives as ``1.13 dt``.  The evaluation:
          ``c = fl(1 / sqrt 2)`` and the product ``fl(t c)`` are each within u relatively, erf' <= 1.1284: the argument
          moves erf by at most ``1.6 u |t|``; erff itself is within 16 ulp of a value of at most 1 (the OpenCL limit the
          device function keeps): ``2^-19``; ``1 + erf <= 2`` rounds by at most 2u; ``0.5 t`` is exact; the last product
          rounds by ``u |g|``:
              dg = 1.13 dt + 0.5 |t| (2^-19 + 5u (1 + |t|)) + u |g|.
residual  one more rounding: ``u |y|`` (and the same u |y| once more as slack for the rounding of the fp64 sum's own
          comparison against fp32 storage)."""
import math

import numpy as np

from tests import theta_gamma_rule as TG

U24 = 2.0 ** -24
E_ERF = 2.0 ** -19
INV_SQRT2_F32 = np.float32(0.70710678118654752440)
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(t):
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return 0.5 * t * (1.0 + _erf(t / math.sqrt(2.0)))


def linear64(x, weights, biases=None, norm=None, eps=1e-5, gelu=False, residual=None):
    """The rule in fp64 on the fp32 inputs: ``dict(y=[..], bound=[..], xh, xh_bound)``; ``weights`` / ``biases`` lists."""
    x = np.asarray(x, dtype=np.float32)
    R, K = x.shape
    biases = [None] * len(weights) if biases is None else biases
    with np.errstate(invalid="ignore", over="ignore"):
        if norm is not None:
            f = TG.norm(x, norm[0], norm[1], eps)
            xh, dxh = f["y"], f["y_bound"]
        else:
            xh, dxh = x.astype(np.float64), np.zeros((R, K))
        ys, bounds = [], []
        for W, b in zip(weights, biases):
            W64 = np.asarray(W, dtype=np.float32).astype(np.float64)
            b64 = np.zeros(W64.shape[0]) if b is None else np.asarray(b, dtype=np.float32).astype(np.float64)
            t = xh @ W64.T + b64[None, :]
            dt = (K + 8) * U24 * ((np.abs(xh) + dxh) @ np.abs(W64).T + np.abs(b64)[None, :]) + dxh @ np.abs(W64).T
            if gelu:
                g = gelu64(t)
                dt = 1.13 * dt + 0.5 * np.abs(t) * (E_ERF + 5.0 * U24 * (1.0 + np.abs(t))) + U24 * np.abs(g)
                t = g
            if residual is not None:
                t = t + np.asarray(residual, dtype=np.float32).astype(np.float64)
            ys.append(t)
            bounds.append(dt + 2.0 * U24 * np.abs(t))
    return dict(y=ys, bound=bounds, xh=xh, xh_bound=dxh)


# ------------------------------------------------------------------------------------------------ fp32, the rule's order
def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _butterfly(s):
    """[.., 64] fp32 lane values -> [..] by the xor butterfly 32, 16, 8, 4, 2, 1."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = (s + s[..., lanes ^ off]).astype(np.float32)
    return s[..., 0]


def _lanes(v):
    """[.., K] -> ([.., steps, 64, 4], K): lane l's elements are [.., :, l, :] in ascending k; zeros pad the tail."""
    K = v.shape[-1]
    steps = -(-K // 256)
    p = np.zeros(v.shape[:-1] + (steps * 256,), dtype=v.dtype)
    p[..., :K] = v
    return p.reshape(v.shape[:-1] + (steps, 64, 4)), K


def row_sum32(v):
    """``sum_K`` of the rule: fp32 adds, a lane's elements in ascending k from 0, then the butterfly.  (A padded zero
    adds nothing: s + 0 = s.)"""
    p, _ = _lanes(_f32(v))
    s = np.zeros(p.shape[:-3] + (64,), dtype=np.float32)
    for i in range(p.shape[-3]):
        for j in range(4):
            s = (s + p[..., i, :, j]).astype(np.float32)
    return _butterfly(s)


def norm32(x, gamma, beta, eps):
    """The prologue in fp32 as the rule rounds it: ``(xh, mu, rstd)``."""
    x, gamma, beta = _f32(x), _f32(gamma), _f32(beta)
    K = np.float32(x.shape[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        mu = (row_sum32(x) / K).astype(np.float32)
        d = (x - mu[..., None]).astype(np.float32)
        var = (row_sum32((d * d).astype(np.float32)) / K).astype(np.float32)
        rstd = (np.float32(1.0) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
        n = (d * rstd[..., None]).astype(np.float32)
        return ((n * gamma).astype(np.float32) + beta).astype(np.float32), mu, rstd


def dot32(xh, W):
    """[R, K] x [N, K] -> [R, N] in the rule's order.  The fused multiply-add is formed in fp64 (the product of two fp32
    numbers is exact there) and rounded to fp32: a second rounding that can differ from the device's single one in the
    last bit of rare cases, so this restatement is for bounds and known answers, not for bit comparison."""
    xp, _ = _lanes(_f32(xh))
    wp, _ = _lanes(_f32(W))
    t = np.zeros((xp.shape[0], wp.shape[0], 64), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(xp.shape[-3]):
            for j in range(4):
                prod = xp[:, None, i, :, j].astype(np.float64) * wp[None, :, i, :, j].astype(np.float64)
                t = (prod + t.astype(np.float64)).astype(np.float32)
        return _butterfly(t)


def gelu32(t):
    t = _f32(t)
    with np.errstate(invalid="ignore"):
        e = _erf((t * INV_SQRT2_F32).astype(np.float32).astype(np.float64)).astype(np.float32)
        return ((np.float32(0.5) * t).astype(np.float32) * (np.float32(1.0) + e).astype(np.float32)).astype(np.float32)


def linear32(x, weights, biases=None, norm=None, eps=1e-5, gelu=False, residual=None):
    """The rule in fp32: ``dict(y=[..], xh)``."""
    x = _f32(x)
    biases = [None] * len(weights) if biases is None else biases
    xh = norm32(x, norm[0], norm[1], eps)[0] if norm is not None else x
    ys = []
    with np.errstate(invalid="ignore", over="ignore"):
        for W, b in zip(weights, biases):
            t = dot32(xh, W)
            if b is not None:
                t = (t + _f32(b)[None, :]).astype(np.float32)
            if gelu:
                t = gelu32(t)
            if residual is not None:
                t = (t + _f32(residual)).astype(np.float32)
            ys.append(t)
    return dict(y=ys, xh=xh)
