"""The decode-attention rule of ``include/aura_hip.h`` ("Decode attention") in NumPy -- TEST INFRASTRUCTURE ONLY.

``step64`` evaluates one step in fp64 on the fp32 inputs as given (plain softmax: the exact function); ``step32`` restates
the kernel's fp32 order of operations (unit dots, butterflies, slots, blocks of four, chunk merge) with NumPy's fp32
``exp`` / ``tanh`` in place of the device's, so it is a second fp32 evaluation of the same order, not a bit reference.
``ctx_bound`` / ``scale_bound`` bound any such evaluation against fp64.  Both steps append to the caches they are given
(in place), leave inactive rows alone and return ``ctx``, ``scale`` and the new ``lengths``.

Where the bounds come from, u = 2^-24 (half an ulp of a rounded result), every operation rounded once:

scale.  The gate's pre-activation g is four rounded products, three adds and the bias: |dg| <= 5 u (sum|Wp p| + |bp|).
  sig = 1 / (1 + expf(-g)) has slope <= 1/4 and four operations on values <= 2 (expf within 1 ulp = 2 u relative, which
  costs e / (1 + e)^2 * 2 u <= u / 2): |d sig| <= dg / 4 + 4 u, and fl(1 + sig) adds 2 u.  tanhf is within 5 * 2^-23 = 10 u
  (the header's figure for the accurate device function): fl(1 + fl(0.2 tanhf)) is within 4 u, the 0.05 factor within 2 u.
  The memory gate's dot has ceil(D / 256) units of four products per lane, 6 butterfly adds, the bias: T_D = 4 ceil(D /
  256) + 9, |dm| <= T_D u (sum|wm x| + |bm|); fl(1 + fl(0.5 sig(m))) is within dm / 8 + 4 u.  Every factor is >= 1, so an
  absolute error of a factor is at most that relative error; three products add 3 u:
      E_s = dg / 4 + dm / 8 + 24 u                          (relative; absent factors contribute nothing but are kept)

scores.  q' = fl(q s) (u), a unit's four products and three adds (4 u), log2 GP butterfly adds, isq = fl(1 / sqrt(dh))
  (u), the product with it (u): with A_t = isq sum_i |q'_i K_ti|,
      |dz_t| <= (E_s + (log2 GP + 7) u) A_t =: Dz_t,  Dz = max_t Dz_t.
  Perturbing every score by at most Dz changes a softmax weight by a factor within exp(+-2 Dz).

weights and sums.  Position t enters as expf(fl(z_t - m)) and is later multiplied by expf of differences of running
  maxima (block rescales, slot merge, chunk merge).  The differences telescope: their sum is at most zmax - z_t, each
  is rounded relative to itself, so the exponents of position t carry at most (zmax - z_t) u in all, a relative error
  of the weight.  Besides that: at most 256 / R adds and 64 / R rescales in the slot (expf 2 u + product u each), log2 R
  slot merges and L / 256 chunk merges (expf, product, add: 4 u each), the product p V (u), the final division (u) and
  slack: T1 = 256 / R + 3 * 64 / R + 4 log2 R + 4 (L / 256 + 1) + 8.  The denominator l carries the same, weighted:
  Z = sum_t w_t (zmax - z_t).  So
      |ctx_d - ctx64_d| <= sum_t w_t |V_td| (expm1(2 Dz) + ((zmax - z_t) + Z) u + 2 T1 u).
  R = 64 / GP slots, GP the power of two >= dh / 4.  The L + 1 terms enter through w_t: the bound is a weighted mean of
  |V|, so it does not grow with L beyond the chunk merges.
"""
import math

import numpy as np

U = 2.0 ** -24
CHUNK = 256
f32 = np.float32


def gp_of(dh):
    g, gp = dh // 4, 1
    while gp < g:
        gp *= 2
    return gp


def slots_of(dh):
    return 64 // gp_of(dh)


def active_rows(lengths, cap, n_chunks=None):
    lim = cap if n_chunks is None else min(cap, CHUNK * n_chunks)
    L = np.asarray(lengths)
    return (L >= 0) & (L < lim)


# ------------------------------------------------------------------------------------------------------------ scale
def scale64(B, H, prosody=None, Wp=None, bp=None, wm=None, bm=None, x=None):
    """s [B, H] in fp64 on the fp32 inputs as given."""
    s = np.ones((B, H))
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    if prosody is not None:
        p = prosody.astype(np.float64)
        g = p @ Wp.astype(np.float64).T + bp.astype(np.float64)
        s = s * (1.0 + sig(g)) * (1.0 + 0.2 * np.tanh(p[:, 0:1])) * (1.0 + 0.05 * np.tanh(p[:, 1:2]))
    if wm is not None:
        m = x.astype(np.float64) @ wm.astype(np.float64).reshape(-1) + float(np.asarray(bm).reshape(-1)[0])
        s = s * (1.0 + 0.5 * sig(m))[:, None]
    return s


def _sig32(a):
    with np.errstate(over="ignore"):
        return (f32(1.0) / (f32(1.0) + np.exp(-a, dtype=f32))).astype(f32)


def _dot_D32(w, x):
    """dot_D of the header: lane l owns the units l, l + 64, .., ascending; then the xor butterfly."""
    D = w.shape[0]
    lanes = np.zeros(64, f32)
    prod = (w * x).astype(f32)
    for l in range(64):
        d = f32(0.0)
        for u in range(l, D // 4, 64):
            for e in range(4):
                d = f32(d + prod[4 * u + e])
        lanes[l] = d
    for off in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[np.arange(64) ^ off]).astype(f32)
    return lanes[0]


def scale32(B, H, prosody=None, Wp=None, bp=None, wm=None, bm=None, x=None):
    s = np.ones((B, H), f32)
    if prosody is not None:
        for b in range(B):
            p = prosody[b]
            fa = f32(f32(1.0) + f32(f32(0.2) * np.tanh(p[0], dtype=f32)))
            fv = f32(f32(1.0) + f32(f32(0.05) * np.tanh(p[1], dtype=f32)))
            for h in range(H):
                g = f32(Wp[h, 0] * p[0])
                for j in (1, 2, 3):
                    g = f32(g + f32(Wp[h, j] * p[j]))
                g = f32(g + bp[h])
                s[b, h] = f32(f32(f32(f32(1.0) + _sig32(g)) * fa) * fv)
    if wm is not None:
        w = wm.reshape(-1)
        for b in range(B):
            m = f32(_dot_D32(w, x[b]) + f32(np.asarray(bm).reshape(-1)[0]))
            s[b] = (s[b] * f32(f32(1.0) + f32(f32(0.5) * _sig32(m)))).astype(f32)
    return s


def scale_bound(B, H, prosody=None, Wp=None, bp=None, wm=None, bm=None, x=None):
    """E_s [B, H]: the relative error bound of an fp32 scale against ``scale64``."""
    e = np.full((B, H), 24.0 * U)
    if prosody is not None:
        dg = 5.0 * U * (np.abs(prosody.astype(np.float64)) @ np.abs(Wp.astype(np.float64)).T + np.abs(bp.astype(np.float64)))
        e = e + dg / 4.0
    if wm is not None:
        D = wm.size
        T_D = 4 * math.ceil(D / 256) + 9
        dm = T_D * U * (np.abs(x.astype(np.float64)) @ np.abs(wm.astype(np.float64)).reshape(-1)
                        + abs(float(np.asarray(bm).reshape(-1)[0])))
        e = e + dm[:, None] / 8.0
    return e


# ------------------------------------------------------------------------------------------------------------- steps
def _heads(a, H):
    B, D = a.shape
    return a.reshape(B, H, D // H)


def step64(q, k_new, v_new, K, V, lengths, prosody=None, Wp=None, bp=None, wm=None, bm=None, x=None, n_chunks=None,
           advance=True, with_bound=False):
    """One step in fp64.  K, V [B, H, cap, dh] fp32 are appended to in place.  Returns a dict: ctx [B, D] fp64, scale
    [B, H] fp64 (0 on inactive rows), lengths (new, int32) and, with ``with_bound``, bound [B, D]."""
    B, H, cap, dh = K.shape
    L = np.asarray(lengths, np.int32).copy()
    act = active_rows(L, cap, n_chunks)
    s = scale64(B, H, prosody, Wp, bp, wm, bm, x)
    Es = scale_bound(B, H, prosody, Wp, bp, wm, bm, x) if with_bound else None
    qh, kh, vh = _heads(q, H), _heads(k_new, H), _heads(v_new, H)
    ctx = np.zeros((B, H, dh))
    bound = np.zeros((B, H, dh))
    gp, R = gp_of(dh), slots_of(dh)
    isq32 = f32(1.0) / np.sqrt(f32(dh))
    for b in range(B):
        if not act[b]:
            s[b] = 0.0
            continue
        n = int(L[b])
        K[b, :, n], V[b, :, n] = kh[b], vh[b]
        for h in range(H):
            Kt, Vt = K[b, h, :n + 1].astype(np.float64), V[b, h, :n + 1].astype(np.float64)
            qs = qh[b, h].astype(np.float64) * s[b, h]
            z = (Kt @ qs) / math.sqrt(dh)
            w = np.exp(z - z.max())
            w = w / w.sum()
            ctx[b, h] = w @ Vt
            if with_bound:
                q32 = (qh[b, h] * f32(s[b, h])).astype(f32).astype(np.float64)
                A = float(isq32) * (np.abs(Kt) @ np.abs(q32))
                Dz = float(np.max((Es[b, h] + (math.log2(gp) + 7) * U) * A))
                T1 = 256 // R + 3 * (64 // R) + 4 * math.log2(R) + 4 * (n // CHUNK + 1) + 8
                gap = z.max() - z
                rel = math.expm1(2.0 * Dz) + (gap + float(w @ gap)) * U + 2.0 * T1 * U
                bound[b, h] = (w * rel) @ np.abs(Vt)
        if advance:
            L[b] += 1
    out = {"ctx": ctx.reshape(B, H * dh), "scale": s, "lengths": L}
    if with_bound:
        out["bound"] = bound.reshape(B, H * dh)
        out["scale_bound"] = Es * np.abs(s)
    return out


def _exp32(a):
    with np.errstate(under="ignore"):
        return np.exp(f32(a), dtype=f32)


def _merge32(a, b):
    """The symmetric merge of two (m, l, acc); an empty side has m = -inf."""
    (ma, la, aa), (mb, lb, ab) = a, b
    M = max(ma, mb)
    ea = f32(0.0) if ma == -np.inf else _exp32(f32(ma - M))
    eb = f32(0.0) if mb == -np.inf else _exp32(f32(mb - M))
    return M, f32(f32(la * ea) + f32(lb * eb)), ((aa * ea).astype(f32) + (ab * eb).astype(f32)).astype(f32)


def _scores32(qs, Kt, dh, isq):
    """z_t of the header for the rows Kt [n, dh]: unit dots, then the butterfly over GP units."""
    gp, G = gp_of(dh), dh // 4
    prod = (Kt * qs[None, :]).astype(f32).reshape(-1, G, 4)
    unit = prod[:, :, 0]
    for e in (1, 2, 3):
        unit = (unit + prod[:, :, e]).astype(f32)
    lanes = np.zeros((Kt.shape[0], gp), f32)
    lanes[:, :G] = unit
    off = gp // 2
    while off >= 1:
        lanes = (lanes + lanes[:, np.arange(gp) ^ off]).astype(f32)
        off //= 2
    return (lanes[:, 0] * isq).astype(f32)


def step32(q, k_new, v_new, K, V, lengths, prosody=None, Wp=None, bp=None, wm=None, bm=None, x=None, n_chunks=None,
           advance=True):
    """One step in the kernel's fp32 order.  Same conventions as ``step64``; ctx and scale are fp32."""
    B, H, cap, dh = K.shape
    L = np.asarray(lengths, np.int32).copy()
    act = active_rows(L, cap, n_chunks)
    s = scale32(B, H, prosody, Wp, bp, wm, bm, x)
    qh, kh, vh = _heads(q, H), _heads(k_new, H), _heads(v_new, H)
    ctx = np.zeros((B, H, dh), f32)
    R = slots_of(dh)
    isq = f32(f32(1.0) / np.sqrt(f32(dh)))
    empty = lambda: (f32(-np.inf), f32(0.0), np.zeros(dh, f32))
    for b in range(B):
        if not act[b]:
            s[b] = 0.0
            continue
        n = int(L[b])
        K[b, :, n], V[b, :, n] = kh[b], vh[b]
        for h in range(H):
            qs = (qh[b, h] * s[b, h]).astype(f32)
            z = _scores32(qs, K[b, h, :n + 1], dh, isq)
            total = None
            for c in range(n // CHUNK + 1):
                t0, end = c * CHUNK, min(c * CHUNK + CHUNK, n + 1)
                slots = []
                for r in range(R):
                    m, l, acc = empty()
                    pos = np.arange(t0 + r, end, R)
                    for i in range(0, len(pos), 4):
                        blk = pos[i:i + 4]
                        mn = max(m, f32(z[blk].max()))
                        al = f32(1.0) if m == mn else _exp32(f32(m - mn))
                        l, acc = f32(l * al), (acc * al).astype(f32)
                        for t in blk:
                            p = _exp32(f32(z[t] - mn))
                            l = f32(l + p)
                            acc = (acc + (p * V[b, h, t]).astype(f32)).astype(f32)
                        m = mn
                    slots.append((m, l, acc))
                off = 1
                while off < R:                                          # slot r pairs with r ^ off: symmetric
                    slots = [_merge32(slots[r], slots[r ^ off]) for r in range(R)]
                    off *= 2
                total = slots[0] if total is None else _merge32(total, slots[0])
            ctx[b, h] = (total[2] / total[1]).astype(f32)
        if advance:
            L[b] += 1
    return {"ctx": ctx.reshape(B, H * dh), "scale": s, "lengths": L}


def forward64(hidden, weights, H, prosody=None, use_memory=True):
    """The module's causal forward in fp64 from its ``state_dict`` (NumPy arrays): hidden [B, S, D] -> [B, S, D]."""
    W = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    hid = np.asarray(hidden, np.float64)
    B, S, D = hid.shape
    dh = D // H
    lin = lambda n, t: t @ W[n + ".weight"].T + W[n + ".bias"]
    q, k, v = (lin(n, hid).reshape(B, S, H, dh).transpose(0, 2, 1, 3) for n in ("q_proj", "k_proj", "v_proj"))
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    if prosody is not None:
        p = np.asarray(prosody, np.float64)
        gain = sig(lin("prosody_gate", p)).transpose(0, 2, 1)[..., None]
        q = q * (1.0 + gain) * (1.0 + 0.2 * np.tanh(p[..., 0]))[:, None, :, None] \
            * (1.0 + 0.05 * np.tanh(p[..., 1]))[:, None, :, None]
    if use_memory:
        q = q * (1.0 + 0.5 * sig(lin("memory_gate", hid)))[:, None, :, :]
    z = q @ k.transpose(0, 1, 3, 2) / math.sqrt(dh)
    z = np.where(np.tril(np.ones((S, S), bool)), z, -np.inf)
    w = np.exp(z - z.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    ctx = (w @ v).transpose(0, 2, 1, 3).reshape(B, S, D)
    return lin("o_proj", ctx)
