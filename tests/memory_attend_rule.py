"""The memory-attend rule of ``include/aura_hip.h`` ("Memory attend") restated in NumPy, as test infrastructure: in fp64
on the fp32 inputs, with a bound derived from the number formats.  Nothing here is measured on a device.

Result: with ``e = 2^-24``, ``ds`` the score's bound, ``p`` the fp64 softmax and ``j`` running over the ``H M`` pairs ``(h, m)``,

    eta_m = ds_m + 2e (mx - s_m + ds_m + max_k ds_k)
    A_m   = expm1(eta_m) + 2e exp(eta_m)
    Z     = 2e (M - 1) (1 + max_k A_k),        B = sum_k p_k A_k + Z
    dp_m  = p_m (A_m (1 - p_m) + sum_{k != m} p_k A_k + Z) / (1 - B)  (+ 2e of p_m and of itself, + tiny)
    dy    = (sum_j |U_j| dp_j + 2e H M sum_j (p_j + dp_j) |U_j| + 2e |bo + acc| + 2e |y|) (1 + 2^-12)

Derivation.  Every fp32 rounding behind the dot product is entered at a whole ulp, ``2e`` relatively, not at the half
ulp that round-to-nearest guarantees: the GPU test asks every element to stay within HALF its bound, and a single
rounding may use its half ulp in full (``tests/row_linear_epilogue_rule.py`` does the same, for the same reason).

scores    ``s = fl(s0 + dot)`` with the LayerNorm prologue, the fmaf chain and the butterfly of "Row linear" (K = D, the
          bias is s0): ``tests/row_linear_rule.linear64`` gives s in fp64 and its bound ``ds``, which holds the
          LayerNorm's error ``dxh`` carried through ``sum_k |G_k| dxh_k``, the chain and the rounding of the add.
softmax   The device subtracts its own maximum ``c`` (of the computed scores) before the exponential.  A softmax does
          not depend on the shift, so measure against ``E_m = exp(s64_m - c)`` and ``S = sum_m E_m``, ``p_m = E_m / S``.
          The argument ``fl(s_m - c)`` differs from ``s64_m - c`` by the score's error and one rounding of a number
          of magnitude at most ``mx64 - s64_m + ds_m + max_k ds_k``: that is ``eta_m``.  expf is within 1 ulp (the
          documented accuracy of the device function; ``2e`` relatively), so the computed ``e_m = E_m (1 + a_m)`` with
          ``|a_m| <= exp(eta_m) (1 + 2e) - 1 = A_m``: the ``exp(ds)`` factor.  The sum over m in ascending order rounds
          M - 1 times, each at most ``2e`` of a partial sum that is at most the whole one: ``sum = S (1 + b)`` with
          ``|b| <= sum_k p_k A_k + Z = B``.  Then
              e_m / sum - p_m = p_m (a_m - b) / (1 + b),   a_m - b = a_m (1 - p_m) - sum_{k != m} p_k a_k - (the sum's roundings):
          the ``p (1 - p)``-type sensitivity: a weight near one barely moves, whatever its score's error.  The
          quotient rounds once more: ``2e`` of the result.  Where expf underflows (a score 87 or more below the
          maximum) the computed e_m is zero or subnormal and ``a_m`` is no small number; its absolute error is below
          ``2^-125``, and against ``S >= exp(-2 max ds)`` that moves every weight of the head by at most ``tiny = (M + 1)
          2^-125 exp(2 max ds)``, which is added to every dp.
sum       ``acc`` adds ``fl(p_j U_j)`` over the H M pairs in order: a weight's error arrives as ``|U_j| dp_j``; a term
          is rounded once as a product and takes part in at most H M - 1 roundings of partial sums, each at most ``2e``
          of ``sum_j |p_j U_j|``: ``2e H M sum_j (p_j + dp_j) |U_j|`` covers both.
y         ``fl(bo + acc)`` and ``fl(x + .)`` round once each: ``2e |bo + acc|`` and ``2e |y|``.  The factor
          ``1 + 2^-12`` holds the second-order terms (products of the above: ``2e H M <= 2^-13``).
Without a bias ``bo + acc`` is acc itself and its rounding does not happen; the term stays in the bound (it can only
widen it by ``2e |acc|``, far below the rest)."""
import numpy as np

from tests import row_linear_rule as RULE

E24 = 2.0 ** -24
TINY = 2.0 ** -125


def finish32(p, U, x, bo=None):
    """Steps 4 of the rule in fp32 for given weights ``p`` [R, H, M] (taken as they are): ``acc`` adds ``fl(p U)`` over
    (h, m) in ascending order from zero, then ``y = fl(x + fl(bo + acc))``.  Bit for bit what the device makes of the
    same p: for the known answers (a uniform p = 1/M with M a power of two, a one-hot p)."""
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    p, U, x = f32(p), f32(U), f32(x)
    R, H, M, D = U.shape
    acc = np.zeros((R, D), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(H):
            for m in range(M):
                acc = (acc + (p[:, h, m, None] * U[:, h, m, :]).astype(np.float32)).astype(np.float32)
        if bo is not None:
            acc = (f32(bo)[None, :] + acc).astype(np.float32)
        return (x + acc).astype(np.float32)


def attend32(x, gamma, beta, G, s0, U, bo=None, eps=1e-5):
    """The rule in fp32 as it rounds (NumPy's exp in place of the device's expf, and ``tests/row_linear_rule.dot32``'s
    twice-rounded fmaf: for the bound's own test and for known answers, not for bits): ``dict(y, p)``."""
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    x, G, s0 = f32(x), f32(G), f32(s0)
    R, H, M, D = G.shape
    xh = RULE.norm32(x, gamma, beta, eps)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.stack([(s0[r].reshape(H * M) + RULE.dot32(xh[r:r + 1], G[r].reshape(H * M, D))[0]).astype(np.float32)
                      for r in range(R)]).reshape(R, H, M)
        e = np.exp((s - s.max(axis=2, keepdims=True)).astype(np.float32)).astype(np.float32)
        total = np.zeros((R, H), dtype=np.float32)
        for m in range(M):
            total = (total + e[:, :, m]).astype(np.float32)
        p = (e / total[:, :, None]).astype(np.float32)
    return dict(y=finish32(p, U, x, bo), p=p)


def attend64(x, gamma, beta, G, s0, U, bo=None, eps=1e-5):
    """The rule in fp64 on the fp32 inputs: ``dict(y, bound, p, dp, s, ds)`` with y, bound [R, D] and p, dp, s, ds
    [R, H, M]."""
    f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    x32 = np.asarray(x, dtype=np.float32)
    G64, s064, U64 = f64(G), f64(s0), f64(U)
    R, H, M, D = G64.shape
    b64 = np.zeros(D) if bo is None else f64(bo)
    s = np.empty((R, H, M))
    ds = np.empty((R, H, M))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            lin = RULE.linear64(x32[r:r + 1], [np.asarray(G, dtype=np.float32)[r].reshape(H * M, D)],
                                [np.asarray(s0, dtype=np.float32)[r].reshape(H * M)], norm=(gamma, beta), eps=eps)
            s[r] = lin["y"][0].reshape(H, M)
            ds[r] = lin["bound"][0].reshape(H, M)
        mx = s.max(axis=2, keepdims=True)
        E = np.exp(s - mx)
        p = E / E.sum(axis=2, keepdims=True)
        dmax = ds.max(axis=2, keepdims=True)
        eta = ds + 2.0 * E24 * (mx - s + ds + dmax)
        cap = np.minimum(eta, 700.0)
        A = np.expm1(cap) + 2.0 * E24 * np.exp(cap)
        Z = 2.0 * E24 * (M - 1) * (1.0 + A.max(axis=2, keepdims=True))
        pA = (p * A).sum(axis=2, keepdims=True)
        B = pA + Z
        moved = p * (A * (1.0 - p) + (pA - p * A) + Z) / np.where(B < 1.0, 1.0 - B, np.nan)
        dp = moved + 2.0 * E24 * (p + moved) + (M + 1) * TINY * np.exp(np.minimum(2.0 * dmax, 700.0))
        acc = np.einsum("rhm,rhmd->rd", p, U64)
        absU = np.abs(U64)
        dacc = np.einsum("rhm,rhmd->rd", dp, absU) + 2.0 * E24 * H * M * np.einsum("rhm,rhmd->rd", p + dp, absU)
        t = b64[None, :] + acc
        y = x32.astype(np.float64) + t
        bound = (dacc + 2.0 * E24 * np.abs(t) + 2.0 * E24 * np.abs(y)) * (1.0 + 2.0 ** -12)
    return dict(y=y, bound=bound, p=p, dp=dp, s=s, ds=ds)
