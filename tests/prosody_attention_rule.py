"""The prosody-attention rule of ``include/aura_hip.h`` ("Prosody attention") restated in NumPy, as test infrastructure:
fp32 wherever the rule rounds, fp64 for the transcendentals on the fp32 phases, together with the bounds.  Nothing here
is measured on a device.  ``u = 2^-24`` (half an ulp of a value in [1, 2)).

channels  ``amp = |sin(phase)|``, ``pitch = |cos(phase)|`` on the fp32 phase ``fl(float(id) c)``: the device functions keep
          OpenCL's 4 ulp for sin and cos, and an ulp of a value below 1 is at most 2^-23:  ``E = 2^-21``.  The boundary
          channel is a comparison of such a sine with 0.8f; it is exact for every id whose fp64 sine is further than E
          from 0.8f (``boundary_margin``).
LIF, salience (no smoothing), the division, the selection: exact fp32 operations in a fixed order: no tolerance.
smoothing ``m`` products ``fl(kw sal)`` (each within ``u |kw sal|``) and ``m - 1`` additions: any order of the additions, and
          a fused multiply-add in place of product and addition, stays within ``m u max|kw sal| m = m u max|sal|`` of
          any other (``smooth_bound``).  m = 2 is exact: the halving is exact and one addition rounds alike everywhere.
          After the division by ``den = max + 1e-6`` an error e of the numerator and e of the maximum give at most
          ``(e / den) (1 + |sal| / den)`` and one rounding (``normalized_bound``).
avg       k values of magnitude at most ``max|sal|`` added in some order and divided:  ``k u max|sal|`` (``avg_bound``).
mu        ``min_gain + range tanh(gain_up avg)``: OpenCL's 5 ulp for tanh, an ulp below 1 at most 2^-23: ``T = 5 * 2^-23``
          times ``|range|``; the product of gain_up and avg, the product with the range and the final addition round once
          each, relative to numbers of at most ``M = max(|min_gain| + |range|, |range| |gain_up avg|)`` (tanh has slope at
          most 1):  ``|range| T + 3 u M`` (``mu_bound``).  Where the avg itself is only known within ``d_avg`` (another
          summation order), ``|range| |gain_up| d_avg`` more.
gains     ``fl(mu fl(1 + sal))`` from the kernel's own mu and salience: exact; from a mu within ``d_mu``:
          ``d_mu |1 + sal| + 2 u |gains|``."""
import numpy as np

U24 = 2.0 ** -24
E = 2.0 ** -21
T = 5.0 * 2.0 ** -23
F32 = np.float32
C_AMP, C_PITCH, C_BOUND = F32(0.1), F32(0.05), F32(0.3)
THRESH = F32(0.8)
EPS = F32(1e-6)


def phases(ids):
    """The three fp32 phases of integer ids (any shape)."""
    f = np.asarray(ids).astype(np.float32)
    return f * C_AMP, f * C_PITCH, f * C_BOUND


def channels(ids):
    """``(amp64, pitch64, boundary, margin)``: fp64 channels on the fp32 phases, the boundary as fp32 0 / 1, and the
    distance of the boundary sine from the threshold."""
    pa, pp, pb = (p.astype(np.float64) for p in phases(ids))
    sb = np.sin(pb)
    return np.abs(np.sin(pa)), np.abs(np.cos(pp)), (sb > float(THRESH)).astype(np.float32), np.abs(sb - float(THRESH))


def lif(x, decay, v0=None, lengths=None):
    """The rule's LIF on fp32 ``x`` [B, S] with one fp32 decay: ``(spikes [B, S], v_out [B])``."""
    x = np.asarray(x, dtype=np.float32)
    B, S = x.shape
    d = F32(decay)
    v = np.zeros(B, np.float32) if v0 is None else np.asarray(v0, dtype=np.float32).copy()
    lens = np.full(B, S) if lengths is None else np.clip(np.asarray(lengths).astype(np.int64), 0, S)
    spikes = np.zeros((B, S), np.float32)
    one = F32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(S):
            live = t < lens
            nv = (d * v).astype(np.float32) + x[:, t]
            s = (nv >= one).astype(np.float32)
            nv = (nv - s).astype(np.float32)
            spikes[:, t] = np.where(live, s, F32(0))
            v = np.where(live, nv, v).astype(np.float32)
    return spikes, v


def salience(s_amp, s_pitch, s_bound, weights):
    w = np.asarray(weights, dtype=np.float32)
    return ((w[0] * s_amp).astype(np.float32) + (w[1] * s_pitch).astype(np.float32)).astype(np.float32) \
        + (w[2] * s_bound).astype(np.float32)


def smooth(sal, m, lengths=None):
    """The tap rule: products rounded, added left to right from the first, zero outside [0, len)."""
    sal = np.asarray(sal, dtype=np.float32)
    B, S = sal.shape
    lens = np.full(B, S) if lengths is None else np.clip(np.asarray(lengths).astype(np.int64), 0, S)
    live = np.arange(S)[None, :] < lens[:, None]
    if m <= 1:
        return np.where(live, sal, F32(0))
    kw = F32(1.0) / F32(m)
    h = m // 2
    pad = np.zeros((B, S + 2 * m), np.float32)
    pad[:, m:m + S] = np.where(live, sal, F32(0))
    prod = (kw * pad).astype(np.float32)
    out = None
    for j in range(m):
        tap = prod[:, m - h + j:m - h + j + S]
        out = tap.copy() if out is None else (out + tap).astype(np.float32)
    return np.where(live, out, F32(0)).astype(np.float32)


def normalize(sal, lengths=None):
    sal = np.asarray(sal, dtype=np.float32)
    B, S = sal.shape
    lens = np.full(B, S) if lengths is None else np.clip(np.asarray(lengths).astype(np.int64), 0, S)
    out = sal.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            n = int(lens[b])
            if n > 0:
                den = F32(sal[b, :n].max()) + EPS
                out[b, :n] = sal[b, :n] / den
    return out


def key(sal):
    """The monotone selection key: unsigned order is value order, -0 = +0, every NaN the largest."""
    u = np.asarray(sal, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where(u == 0x80000000, 0, u)
    k = np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, 0xFFFFFFFF, k)


def winners(sal, k, lengths=None):
    """``(winners int32 [B, k] padded with -1, avg fp32 [B])`` on the fp32 salience given."""
    sal = np.asarray(sal, dtype=np.float32)
    B, S = sal.shape
    lens = np.full(B, S) if lengths is None else np.clip(np.asarray(lengths).astype(np.int64), 0, S)
    win = np.full((B, k), -1, np.int32)
    avg = np.zeros(B, np.float32)
    for b in range(B):
        n = int(lens[b])
        ke = min(k, n)
        if ke == 0:
            continue
        order = np.argsort(-key(sal[b, :n]), kind="stable")[:ke]
        win[b, :ke] = order
        s = sal[b, order[0]]
        with np.errstate(invalid="ignore", over="ignore"):
            for r in order[1:]:
                s = F32(s + sal[b, r])
            avg[b] = F32(s) / F32(ke)
    return win, avg


def mu64(avg, gain_up, min_gain, max_gain):
    """``(mu fp64, bound)`` from the fp32 avg: the phase and the range in fp32 as the rule rounds them, the rest fp64."""
    avg = np.asarray(avg, dtype=np.float32)
    g = (F32(gain_up) * avg).astype(np.float32).astype(np.float64)
    rng = float(F32(max_gain) - F32(min_gain))
    mu = float(F32(min_gain)) + rng * np.tanh(g)
    M = np.maximum(abs(float(F32(min_gain))) + abs(rng), abs(rng) * np.abs(g))
    return mu, abs(rng) * T + 3.0 * U24 * M


def gains32(mu, sal):
    """``fl(mu fl(1 + sal))`` on fp32 mu [B] and salience [B, S]."""
    mu = np.asarray(mu, dtype=np.float32)[:, None]
    return (mu * (F32(1.0) + np.asarray(sal, dtype=np.float32)).astype(np.float32)).astype(np.float32)


def smooth_bound(raw, m):
    """Per row [B, 1]: ``m u max|raw|`` (0 for m <= 2)."""
    mx = np.abs(np.asarray(raw, dtype=np.float64)).max(axis=1, keepdims=True) if raw.shape[1] else 0.0
    return (0.0 if m <= 2 else m * U24) * mx


def normalized_bound(smoothed, e):
    """The bound on the normalised salience when the smoothed one (and with it its maximum) is within ``e`` [B, 1]."""
    s = np.asarray(smoothed, dtype=np.float64)
    den = np.abs(s.max(axis=1, keepdims=True) + float(EPS))
    res = np.abs(s) / den
    return (e / den) * (1.0 + res) + 2.0 * U24 * res


def avg_bound(k, max_abs):
    return k * U24 * max_abs


def forward(amp, pitch, bound, decay, weights, k, m=1, normalize_salience=True, gain_up=1.8, min_gain=0.5,
            max_gain=2.5, lengths=None, v0=None):
    """The whole rule on given fp32 channels: a dict of fp32 arrays, plus ``mu64`` and ``mu_bound``."""
    B, S = np.asarray(amp).shape
    v0 = np.zeros((B, 3), np.float32) if v0 is None else np.asarray(v0, dtype=np.float32)
    sp, vo = [], []
    for c, x in enumerate((amp, pitch, bound)):
        s, v = lif(x, np.asarray(decay, dtype=np.float32)[c], v0[:, c], lengths)
        sp.append(s)
        vo.append(v)
    raw = salience(sp[0], sp[1], sp[2], weights)
    sm = smooth(raw, m, lengths)
    sal = normalize(sm, lengths) if normalize_salience else sm
    win, avg = winners(sal, k, lengths)
    m64, mb = mu64(avg, gain_up, min_gain, max_gain)
    mu = m64.astype(np.float32)
    return dict(spikes=np.stack(sp), v_out=np.stack(vo, axis=1), raw=raw, smoothed=sm, salience=sal, winners=win,
                avg=avg, mu=mu, mu64=m64, mu_bound=mb, gains=gains32(mu, sal))
