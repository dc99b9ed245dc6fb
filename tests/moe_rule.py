"""The MoE-zone rule of ``include/aura_hip.h`` ("MoE zone") restated in NumPy, as test infrastructure: in fp64 on the
fp32 inputs with bounds derived from the number formats, and in fp32 as it rounds.  Nothing here is measured on a device.

Conventions.  ``e = 2^-24``.  Every fp32 rounding is entered at a whole ulp, ``2e`` relatively, not at the half ulp that
round-to-nearest guarantees: the tests ask every element to stay within HALF its bound, and a single rounding may use its
half ulp in full (``tests/memory_attend_rule.py`` does the same).  A dot product over K terms, in any order of
summation, fused or not, errs by at most ``2e K sum_k |a_k w_k|`` (K roundings of partial sums that are each at most the
sum of magnitudes): the bounds hold for the kernel's MFMA order, for the fp32 restatement's and for a library GEMM's.

Route.
  pre     ``fl(bW + fl(dot + bU))``: ``dpre = 2e Dm sum|x U| + 2e |dot + bU| + 2e |pre|``.
  g       tanh is 1-Lipschitz: the argument's error arrives unamplified; the device's tanhf is budgeted at 2 ulp,
          ``4e |g|``, and NumPy's fp32 tanh lies within that: ``dg = dpre + 4e |g|``.
  h       ``fl(dt g)`` with dt the fp32 of the module's dt: ``dh = |dt| dg + 2e |h|``.
  z       ``dz = sum_j |G_ej| dh_j + 2e Hr sum_j |G_ej h_j| + 2e |z|``.
  temp    exact without ``attn_gain``.  With it, ``fl(T / fl(gain + 1e-6f))`` rounds twice: a relative ``4e`` (``(1 + 2e)^2``
          is below ``1 + 4e (1 + 2^-20)``; the slack is in the final factor); the clamp is 1-Lipschitz.
          ``z / temp`` rounds once more: ``dz' = (dz + (4e + 2e) |z|) / temp``.
  softmax as ``tests/memory_attend_rule.py`` derives it: with ``eta = dz' + 2e (mx - z + dz' + max dz')`` the exponential
          errs relatively by ``A = expm1(eta) + 2e exp(eta)`` (expf within 1 ulp), the sum rounds at most
          ``R = max(E - 1, 6)`` times (the device's butterfly: six levels, adding +0 is exact; an ascending sum: E - 1),
          and ``dp = p (A (1 - p) + sum_{k != m} p_k A_k + Z) / (1 - B) + 2e (p + that) + tiny``, ``Z = 2e R (1 + max A)``,
          ``B = sum p A + Z``.
  top-k   an order between two experts is open when their probabilities are closer than the sum of their bounds.
  weights ``s = sum_top p`` rounds k - 1 times and once for ``+ 1e-8f``: ``ds = sum_top dp + 2e k (s + 1e-8)``;
          ``dw = dp_r / den + p_r ds / den^2 + 2e w``, times ``1 + 2^-12`` for the second-order terms.
Expert layer (inputs exact: the row of x, or integer spikes).
  c       ``dc = 2e K sum|a W_s| + 2e |c|``.
  i       ``di = sum_m |W_g[n, m]| dc_m + 2e Hh sum|c W_g| + 2e |i|``.
  GIF     from ``v = 0`` the membrane is ``fl(0 decay) + i = i``; the clamp to ``+-2 L theta`` is 1-Lipschitz (its limit is
          computed from fp32 constants; where |i| is within ``di`` of it the quotient is |2L| (1 - 1e-6), far from an
          integer's floor for L <= 64, and the spike count is L either way); ``t = fl(theta + 1e-6f)`` and the division
          round once each: ``dnv = di / t + 4e |nv|``.  The spike count is ``clamp(floor(nv), 0, L)``: a neuron is OPEN
          when ``nv64`` is within ``dnv`` of a deciding integer 1..L; then ``floor(nv64 - dnv)`` and ``floor(nv64 + dnv)``
          (clamped) are both admissible.  First order in the sense that ``dnv`` is evaluated at the fp64 values.
  y       ``dy = 2e Hh sum|s W_r| + 2e |y|`` on exact spikes.
Combine   restated exactly in fp32 (``combine32``); against fp64: ``sum_j (|w_j| dy_j + |y_j| dw_j) + 2e (k + 1) sum_j |w_j y_j|``.
Every bound carries a final factor ``1 + 2^-12`` for products of the above."""
import numpy as np

E24 = 2.0 ** -24
TINY = 2.0 ** -125
SLACK = 1.0 + 2.0 ** -12
F32_1EM6 = np.float32(1e-6)
F32_1EM8 = np.float32(1e-8)


def _f32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32))


def _f64(v):
    return _f32(v).astype(np.float64)


# ---- route ---------------------------------------------------------------------------------------------------------

def topk_order(p, k):
    """The top ``k`` of every row of ``p`` by (value descending, expert id ascending), NaN first: int64 [N, k]."""
    p = np.asarray(p)
    key = np.where(np.isnan(p), np.inf, p)
    # a stable sort of the negated key keeps the lower id first among equals
    return np.argsort(-key, axis=1, kind="stable")[:, :k].astype(np.int64)


def weights32(p, idx):
    """Step 7 in fp32, bit for bit, on given fp32 probabilities and their ranked experts."""
    p = _f32(p)
    top = np.take_along_axis(p, idx, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        s = top[:, 0].copy()
        for r in range(1, idx.shape[1]):
            s = (s + top[:, r]).astype(np.float32)
        return (top / (s + F32_1EM8).astype(np.float32)[:, None]).astype(np.float32)


def _temp(temperature, attn_gain, dtype):
    T = dtype(np.float32(temperature))
    if attn_gain is None:
        return T
    g = np.asarray(_f32(attn_gain), dtype=dtype)
    t = T / (g + dtype(F32_1EM6))
    # fminf(fmaxf(t, 0.1f), 5.0f): a NaN gives 0.1
    lo, hi = dtype(np.float32(0.1)), dtype(np.float32(5.0))
    t = np.where(np.isnan(t), lo, t)
    return np.minimum(np.maximum(t, lo), hi)[:, None]


def route32(x, U, bU, bW, gate_w, gate_b, dt, k, temperature=1.0, attn_gain=None):
    """The route in fp32 as it rounds (NumPy's matmul, tanh and exp in place of the device's chains and functions: for
    the stubs and the bound's own test, not for bits): ``dict(indices, weights, probs)``."""
    x, U, bU, bW, G, gb = map(_f32, (x, U, bU, bW, gate_w, gate_b))
    with np.errstate(invalid="ignore", over="ignore"):
        pre = (bW[None, :] + ((x @ U.T).astype(np.float32) + bU[None, :])).astype(np.float32)
        h = (np.float32(dt) * np.tanh(pre).astype(np.float32)).astype(np.float32)
        z = ((h @ G.T).astype(np.float32) + gb[None, :]).astype(np.float32)
        z = (z / _temp(temperature, attn_gain, np.float32)).astype(np.float32)
        ex = np.exp((z - z.max(axis=1, keepdims=True)).astype(np.float32)).astype(np.float32)
        s = np.zeros(x.shape[0], dtype=np.float32)
        for e in range(G.shape[0]):
            s = (s + ex[:, e]).astype(np.float32)
        p = (ex / s[:, None]).astype(np.float32)
    idx = topk_order(p, k)
    return dict(indices=idx, weights=weights32(p, idx), probs=p)


def route64(x, U, bU, bW, gate_w, gate_b, dt, k, temperature=1.0, attn_gain=None):
    """The route in fp64 on the fp32 inputs: ``dict(indices, weights, dweights, probs, dprobs, order_margin)``.
    ``order_margin`` [N]: the smallest ``|p_a - p_b| - (dp_a + dp_b)`` over the pairs (rank r, rank r + 1), r < k, of
    the row: negative where the row's top-k order is open."""
    x, U, bU, bW, G, gb = map(_f64, (x, U, bU, bW, gate_w, gate_b))
    N, Dm = x.shape
    Hr, E = U.shape[0], G.shape[0]
    dt64 = float(np.float32(dt))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dot = x @ U.T
        inner = dot + bU[None, :]
        pre = bW[None, :] + inner
        dpre = 2 * E24 * Dm * (np.abs(x) @ np.abs(U).T) + 2 * E24 * np.abs(inner) + 2 * E24 * np.abs(pre)
        g = np.tanh(pre)
        dg = dpre + 4 * E24 * np.abs(g)
        h = dt64 * g
        dh = abs(dt64) * dg + 2 * E24 * np.abs(h)
        z0 = h @ G.T + gb[None, :]
        dz0 = dh @ np.abs(G).T + 2 * E24 * Hr * (np.abs(h) @ np.abs(G).T) + 2 * E24 * np.abs(z0)
        temp = _temp(temperature, attn_gain, np.float64)
        rel = 0.0 if attn_gain is None else 4 * E24
        z = z0 / temp
        # a logit of -inf (a bias of -inf) is -inf in every precision: no error, and its exponential is an exact zero
        gone = np.isneginf(z)
        dz = np.where(gone, 0.0, (dz0 + (rel + 2 * E24) * np.abs(z0)) / np.abs(temp))
        mx = z.max(axis=1, keepdims=True)
        Ex = np.exp(z - mx)
        p = Ex / Ex.sum(axis=1, keepdims=True)
        dmax = dz.max(axis=1, keepdims=True)
        eta = np.where(gone, 0.0, np.minimum(dz + 2 * E24 * (mx - z + dz + dmax), 700.0))
        A = np.expm1(eta) + 2 * E24 * np.exp(eta)
        R = max(E - 1, 6)
        Z = 2 * E24 * R * (1.0 + A.max(axis=1, keepdims=True))
        pA = (p * A).sum(axis=1, keepdims=True)
        B = pA + Z
        moved = p * (A * (1.0 - p) + (pA - p * A) + Z) / np.where(B < 1.0, 1.0 - B, np.nan)
        dp = (moved + 2 * E24 * (p + moved) + (E + 1) * TINY * np.exp(np.minimum(2 * dmax, 700.0))) * SLACK
        idx = topk_order(p, k)
        full = topk_order(p, E)
        ps, dps = np.take_along_axis(p, full, axis=1), np.take_along_axis(dp, full, axis=1)
        if E > 1:
            last = min(k, E - 1)
            gaps = (ps[:, :last] - ps[:, 1:last + 1]) - (dps[:, :last] + dps[:, 1:last + 1])
            margin = gaps.min(axis=1)
        else:
            margin = np.full(N, np.inf)
        top, dtop = ps[:, :k], dps[:, :k]
        s = top.sum(axis=1, keepdims=True)
        den = s + float(F32_1EM8)
        ds = dtop.sum(axis=1, keepdims=True) + 2 * E24 * k * den
        w = top / den
        dw = (dtop / den + top * ds / den ** 2 + 2 * E24 * w) * SLACK
    return dict(indices=idx, weights=w, dweights=dw, probs=p, dprobs=dp, order_margin=margin)


# ---- experts -------------------------------------------------------------------------------------------------------

def gif_limits(gif):
    """``(t, L)`` of a layer's ``(decay, L, alpha, threshold)``: the fp32 divisor ``fl(theta + 1e-6f)`` and L."""
    thr = np.float32(gif[3])
    return np.float32(thr + F32_1EM6), float(gif[1])


def layer64(a, Ws, bs, Wg, bg, gif):
    """One expert layer in fp64 on exact inputs ``a`` [P, K]: ``dict(nv, dnv, spikes, lo, hi, open)``; ``lo``/``hi`` the
    admissible spike counts of every neuron, ``open`` where they differ."""
    a, Ws, bs, Wg, bg = map(_f64, (a, Ws, bs, Wg, bg))
    K, Hh = Ws.shape[1], Ws.shape[0]
    t32, L = gif_limits(gif)
    t, thr = float(t32), float(np.float32(gif[3]))
    with np.errstate(invalid="ignore", over="ignore"):
        c = a @ Ws.T + bs[None, :]
        dc = 2 * E24 * K * (np.abs(a) @ np.abs(Ws).T) + 2 * E24 * np.abs(c)
        i = c @ Wg.T + bg[None, :]
        di = dc @ np.abs(Wg).T + 2 * E24 * Hh * (np.abs(c) @ np.abs(Wg).T) + 2 * E24 * np.abs(i)
        cl = 2.0 * L * thr
        v = np.minimum(np.maximum(i, -cl), cl)
        nv = v / t
        dnv = (di / t + 4 * E24 * np.abs(nv)) * SLACK
        count = lambda q: np.minimum(np.maximum(np.floor(q), 0.0), L)
        spikes, lo, hi = count(nv), count(nv - dnv), count(nv + dnv)
    return dict(nv=nv, dnv=dnv, spikes=spikes, lo=lo, hi=hi, open=lo != hi, i=i, di=di)


def readout64(s, Wr, br):
    """``y`` in fp64 from exact spikes ``s`` [P, Hh]: ``dict(y, bound)``."""
    s, Wr, br = map(_f64, (s, Wr, br))
    y = s @ Wr.T + br[None, :]
    return dict(y=y, bound=(2 * E24 * Wr.shape[1] * (np.abs(s) @ np.abs(Wr).T) + 2 * E24 * np.abs(y)) * SLACK)


def expert32(x, params, gifs):
    """``SNNExpert.predict`` in fp32 as it rounds (NumPy's matmul: for the stubs and the bound's own test, not for
    bits).  ``params`` the flat list of ``ops.moe_expert_table``: ``(y [P, Dm], [spikes of every layer])``."""
    a = _f32(x)
    trace = []
    layers = (len(params) - 2) // 4
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(layers):
            Ws, bs, Wg, bg = (_f32(t) for t in params[4 * l:4 * l + 4])
            c = ((a @ Ws.T).astype(np.float32) + bs[None, :]).astype(np.float32)
            i = ((c @ Wg.T).astype(np.float32) + bg[None, :]).astype(np.float32)
            t32, L = gif_limits(gifs[l])
            thr = np.float32(gifs[l][3])
            cl = np.float32(np.float32(np.float32(L) * thr) * np.float32(2.0))
            v = np.minimum(np.maximum(i, -cl), cl)
            a = np.minimum(np.maximum(np.floor((v / t32).astype(np.float32)), np.float32(0.0)), np.float32(L))
            trace.append(a)
        Wr, br = _f32(params[-2]), _f32(params[-1])
        return ((a @ Wr.T).astype(np.float32) + br[None, :]).astype(np.float32), trace


def expert64(x, params, gifs):
    """``SNNExpert.predict`` in fp64, every layer on the fp64 rule's own spikes: ``dict(y, bound, open)`` with ``open``
    [P] the rows that have an open neuron in any layer (their ``y`` is one of several admissible ones)."""
    a = _f64(x)
    layers = (len(params) - 2) // 4
    open_rows = np.zeros(a.shape[0], dtype=bool)
    for l in range(layers):
        r = layer64(a, *params[4 * l:4 * l + 4], gifs[l])
        open_rows |= r["open"].any(axis=1)
        a = r["spikes"]
    out = readout64(a, params[-2], params[-1])
    return dict(y=out["y"], bound=out["bound"], open=open_rows)


# ---- combine -------------------------------------------------------------------------------------------------------

def combine32(y, weights, indices):
    """``out[token] = sum_j fl(w_j y_j)`` over the token's slots in ascending expert id, from the first product, bit
    for bit: ``y`` [N, k, Dm], ``weights`` [N, k], ``indices`` [N, k]."""
    y, w = _f32(y), _f32(weights)
    order = np.argsort(np.asarray(indices), axis=1, kind="stable")
    with np.errstate(invalid="ignore", over="ignore"):
        out = None
        for r in range(order.shape[1]):
            slot = order[:, r]
            rows = np.arange(y.shape[0])
            p = (w[rows, slot][:, None] * y[rows, slot]).astype(np.float32)
            out = p if out is None else (out + p).astype(np.float32)
    return out


def combine64(y, dy, w, dw):
    """The weighted sum in fp64 and its bound: ``y``, ``dy`` [N, k, Dm], ``w``, ``dw`` [N, k]."""
    y, dy, w, dw = (np.asarray(v, dtype=np.float64) for v in (y, dy, w, dw))
    k = y.shape[1]
    out = (w[:, :, None] * y).sum(axis=1)
    bound = (np.abs(w)[:, :, None] * dy + np.abs(y) * dw[:, :, None]).sum(axis=1) + \
        2 * E24 * (k + 1) * (np.abs(w)[:, :, None] * np.abs(y)).sum(axis=1)
    return dict(out=out, bound=bound * SLACK)
