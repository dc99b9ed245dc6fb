"""The theta-gamma rule of ``include/aura_hip.h`` ("Theta-gamma") restated in NumPy, as test infrastructure.  The phases
``a`` and ``g`` are formed in fp32 exactly as the rule rounds them; everything after them is fp64 on those fp32 numbers,
together with the bounds.  Nothing here is measured on a device.  ``u = 2^-24`` (half an ulp of a value in [1, 2)),
``E = 2^-21`` (4 ulp of a value below 1: the OpenCL limit for sin and cos, which the device functions keep).

pe        ``q = sa + 0.5 (A sg)``, ``A = (ca + 1) 0.5``.  The computed sa, ca, sg are each within E.  ``ca + 1 <= 2`` rounds
          by at most 2u and the halving is exact: A is within ``0.5 E + u``.  ``A sg`` (both at most 1): ``(0.5 E + u) + E``
          and one rounding u; halved exactly: ``0.75 E + u``.  Adding sa: ``1.75 E + u`` and a rounding of at most 2u
          (|q| <= 1.5).  So q is within ``1.75 E + 3u``, which the stated ``1.75 E + 9u`` covers; times amp, and the last
          product rounds by ``u |pe|``:   ``|pe - pe_64| <= |amp| (1.75 E + 9u) + u |pe_64|``.
d_amp     is q: the same bound with amp = 1 (the last term is then slack).
d_theta   ``amp (ca - (0.25 sa) sg)``: ca within E; ``0.25 sa`` exact, times sg: ``0.25 (E + E)`` and a rounding of 0.25u; the
          difference is at most 1.25 and rounds by at most 2u: ``1.5 E + 2.25u``, covered by the same form.
d_gamma   ``amp ((0.5 A) cg)``: ``0.5 ((0.5 E + u) + E)`` and two roundings of at most u: ``0.75 E + 2.5u``, covered.
mean      a sum of D numbers whose longest chain has ``T_D - 1`` additions (a lane's elements, then six butterfly
          steps) errs by at most ``(T_D - 1) u sum|h|``; divided by D and rounded once more:  ``T_D u A``, ``A = mean|h|``.
rstd      ``var + eps`` from the computed mean: each ``(h - mu)^2`` carries 3u relative, the sum ``T_D - 1`` more, the
          division and the add of eps one each; moving the mean by ``dmu`` adds exactly ``dmu^2``, which is
          ``(T_D u A rstd)^2`` relative.  Square root and reciprocal halve that and round twice:
          ``|rstd - rstd_64| <= rstd ((T_D / 2 + 4) u + (T_D u A rstd)^2)``.
n, y      ``n = (h - mu) rstd``: ``dmu rstd <= T_D u A rstd``, two roundings and rstd's relative error on |n|.  The stated
          ``dn = (T_D + 8) u (A rstd + 2 |n|)`` covers it (the second-order term while ``T_D^2 u A rstd |n| <= 8``: at the
          tested 1e3 spreads of offset and |n| <= 8 it is below 1).  ``y = n w + b``: ``|w| dn`` and two roundings relative
          to the result:   ``|y - y_64| <= |w| dn + 2u |y_64|``.
g_x       ``rstd (wg - c1 - n c2)``: each of the three terms with its rounding and the ``T_D`` of its row mean, rstd's own
          relative error, all inside ``(T_D + 10) u (|wg| + mean|wg| + |n| mean|wg n|)``; the forward's error in n enters
          through ``n c2`` and through c2 itself:  the stated bound (``g_x_bound``).
sums      a sum over tokens whose longest chain has ``T_N - 1`` additions, each term a rounded product:
          ``(T_N + 3) u S`` with S the sum of the absolute terms, plus what the factors' own bounds propagate.
``dh`` (optional everywhere) widens ``dn`` by what a perturbation of every h by at most ``dh`` does to n,
``rstd (2 + |n|) dh``: used where two fp32 evaluations with different tables are compared."""
import numpy as np

U24 = 2.0 ** -24
E = 2.0 ** -21
TWO_PI = np.float32(2.0 * np.pi)


def ratio(theta_freq, gamma_freq):
    return np.float32(float(gamma_freq) / float(theta_freq))


def phases(pos, th, ga, max_seq_len, r):
    """``(a, g)`` fp32 [R, D] from fp32 positions [R], rounded as the rule rounds them."""
    pos, th, ga = (np.asarray(v, dtype=np.float32) for v in (pos, th, ga))
    denom = np.float32(max(int(max_seq_len) - 1, 1))
    phi = ((pos / denom).astype(np.float32) * TWO_PI).astype(np.float32)[:, None]
    a = (phi + th[None, :]).astype(np.float32)
    g = ((phi * np.float32(r)).astype(np.float32) + ga[None, :]).astype(np.float32)
    return a, g


def table(pos, th, ga, amp, max_seq_len, r):
    """``dict(a, g fp32; pe, d_theta, d_gamma, d_amp fp64 [R, D])``."""
    a, g = phases(pos, th, ga, max_seq_len, r)
    a64, g64 = a.astype(np.float64), g.astype(np.float64)
    m = np.asarray(amp, dtype=np.float32).astype(np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        sa, ca, sg, cg = np.sin(a64), np.cos(a64), np.sin(g64), np.cos(g64)
        A = (ca + 1.0) * 0.5
        q = sa + 0.5 * (A * sg)
        return dict(a=a, g=g, pe=q * m, d_amp=q + 0.0 * m, d_theta=m * (ca - 0.25 * sa * sg), d_gamma=m * 0.5 * A * cg)


def pe_bound(amp, value64):
    """``|amp| (1.75 E + 9u) + u |value|`` for pe, d_theta and d_gamma; d_amp takes ``amp = 1``."""
    m = np.abs(np.asarray(amp, dtype=np.float64))
    return m * (1.75 * E + 9.0 * U24) + U24 * np.abs(value64)


def elements_per_lane(D):
    return -(-(D // 4) // 64) * 4 if D % 4 == 0 else -(-D // 64)


def T_D(D):
    """Additions on the longest chain of a row sum plus one: a lane's elements, six butterfly steps."""
    return elements_per_lane(D) + 7


def groups(N):
    return max(1, min(1024, -(-N // 16)))


def T_N(N):
    """The same for a sum over tokens: a wave's run of tokens, three waves, a run of groups, seven more runs."""
    G = groups(N)
    return -(-N // (4 * G)) + 3 + -(-G // 8) + 7 + 1


def norm(h, w, b, eps, dh=0.0):
    """LayerNorm of the fp32 rows ``h`` [N, D] in fp64: ``dict(y, mean, rstd, n, A, dn, y_bound, mean_bound,
    rstd_bound)``."""
    h64 = np.asarray(h, dtype=np.float32).astype(np.float64)
    w64, b64 = (np.asarray(v, dtype=np.float32).astype(np.float64)[None, :] for v in (w, b))
    D = h64.shape[1]
    t = T_D(D)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = h64.mean(1, keepdims=True)
        var = ((h64 - mean) ** 2).mean(1, keepdims=True)
        rstd = 1.0 / np.sqrt(var + float(eps))
        n = (h64 - mean) * rstd
        y = n * w64 + b64
        A = np.abs(h64).mean(1, keepdims=True)
        dn = (t + 8) * U24 * (A * rstd + 2.0 * np.abs(n)) + rstd * (2.0 + np.abs(n)) * dh
        return dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], n=n, A=A, dn=dn,
                    y_bound=np.abs(w64) * dn + 2.0 * U24 * np.abs(y),
                    mean_bound=(t * U24 * A + dh)[:, 0],
                    rstd_bound=(rstd * ((t / 2 + 4) * U24 + (t * U24 * A * rstd) ** 2 + rstd * dh * 2.0))[:, 0])


def norm_backward(h, w, g_y, eps, dh=0.0):
    """``dict(g_x, g_x_bound, n, dn)`` fp64 for the fp32 rows ``h``, weight ``w`` and output gradient ``g_y``."""
    f = norm(h, w, np.zeros_like(np.asarray(w, dtype=np.float32)), eps, dh)
    n, dn, rstd = f["n"], f["dn"], f["rstd"][:, None]
    D = n.shape[1]
    wg = np.asarray(w, dtype=np.float32).astype(np.float64)[None, :] * np.asarray(g_y, dtype=np.float32).astype(np.float64)
    c1 = wg.mean(1, keepdims=True)
    c2 = (wg * n).mean(1, keepdims=True)
    g_x = rstd * (wg - c1 - n * c2)
    m = lambda v: np.abs(v).mean(1, keepdims=True)
    bound = rstd * ((T_D(D) + 10) * U24 * (np.abs(wg) + m(wg) + np.abs(n) * m(wg * n)) + dn * np.abs(c2)
                    + np.abs(n) * (np.abs(wg) * dn).mean(1, keepdims=True)) + 2.0 * U24 * np.abs(g_x)
    return dict(g_x=g_x, g_x_bound=bound, n=n, dn=dn)


def token_sum(f64, df, g64, dg, T):
    """``(sum_t f g, bound)`` over axis 0 for factors known within ``df`` and ``dg``: ``(T + 3) u S`` plus the
    propagated bounds."""
    f64, g64 = np.broadcast_arrays(np.asarray(f64, np.float64), np.asarray(g64, np.float64))
    S = np.abs(f64 * g64).sum(0)
    return (f64 * g64).sum(0), (T + 3) * U24 * S + (df * np.abs(g64) + np.abs(f64) * dg + df * dg).sum(0)
