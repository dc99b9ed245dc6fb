"""The surrogate-gradient rules of ``csrc/aura_train.hip`` (GIF, prosody GIF, LIF step) and of
``aura_addition_linear_backward`` restated in CPU torch, as test infrastructure: no GPU, no product code.

Forward.  The loop in fp32 exactly as the forward rounds it (for bf16 tensors every op's fp32 result is rounded to
bf16, Python scalars enter as fp32), returning the spikes, the final state and the two documented saves: the
pre-clamp potential ``a_t`` and the threshold ``theta_{t-1}`` it was computed with.

Backward.  A reverse pass over T that recomputes ``te, cl, b, d, n, s`` (and the per-step ``scale``, ``ae`` of the
prosody form) in fp32 from the saves, with the forward's roundings: the clamp side, the floor and the surrogate
window are decided on those fp32 numbers.  Every gradient product and sum after that is fp64.  Beside every
gradient the same recurrence runs on the absolute value of every term: its result M bounds the size of everything
that was added up on the way to that element.

Bounds.  ``u = 2^-24``.  A computed gradient is the exact one with every operation's result multiplied by some
``(1 + delta)``, ``|delta| <= u``; an element reached through at most K such operations lies within
``gamma_K M``, ``gamma_K = K u / (1 - K u)`` (K u M and its second-order remainder), plus K roundings in the
subnormal range.  K counts the roundings on the longest chain from an incoming gradient to the element:

GIF step   (``gif_bwd_kernel``; k = roundings already on gv / gth)
           gs_tot = gs + alpha gth - thp gv           product, sum, (product,) difference          k + 3
           tri    = 1 - 2 |n - rint n|                n - rint n and the doubling are exact           1
           gn     = gs_tot sur                                                                     k + 5
           gb     = gv + gn / d                       quotient, sum                                k + 7
           gth'   = ... + (-gn b / (d d)) + gcl 2L    product, square, quotient, sum, then the
                                                      clamp term's sum after it                    k + 10
           gh = ga = gb;  gv' = ga decay                                                           k + 8
prosody    (``prosody_bwd_kernel``) gathers the three theta terms in gte first and adds ``gte scale``:
           one product and one sum more                                                 gth'       k + 12
           gh = ga g                                                                               k + 8
autograd   (the oracle) performs the same operations node by node and accumulates the five uses of theta
           in another order: ``-gn ((b / d) / d)`` is three operations, the ``+ 1e-6`` node and the
           accumulation add at most three sums after it                                            k + 12
So ``K_STEP = 12`` roundings per time step travelled covers both kernels and the reference's graph:
           g_h[t]            K_STEP (T - t)
           g_v0, g_theta0    K_STEP T
g_gains[t] each channel's three terms: ``gth (s - (thp - thr0)) alpha`` k + 4, ``gte thp (-strength)`` k + 12,
           ``ga x`` k + 8; at most 3 VEC <= 24 sums inside a lane, one float atomic per lane (at most H, in any
           order), one more for what the buffer held:    K_STEP (T - t) + 25 + H
LIF step   g_s = gs - gm thr (2); den = |sl pre| + 1 (2, both terms positive); den den carries den's error twice
           and rounds (5); sl / . (1); g_s . (1); gm + . (1):  g_x  2 + 5 + 3 = 10;  g_mem_prev = beta g_x  11;
           raw_slope = -g_s |pre| sgn / (den2 den2): 2 + 1 + 5 + 1 = 9;  its sum over B rows  9 + B.
           (In the GIF steps d and te are the forward's own fp32 numbers, exact for both sides: d d rounds once.)
bf16       the backward kernels do the fp32 arithmetic above on the bf16-rounded forward values and round the
           result once: ``2^-8 |got|`` more for a bf16 output (``g_gains`` and ``raw_slope`` stay fp32).  The
           reference's bf16 autograd rounds every node to bf16 instead: the same K with ``u = 2^-8``.
AdditionLinear   a sum of T signed copies of g (no product is rounded): ``(T + 2) u sum|g|``.

The oracle's own fp32 autograd reached 12.9 u M at T = 32 (K = 384) on the CPU: a plausibility check for the
count, not its source.  Nothing here is measured on a device."""
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U24 = 2.0 ** -24
U8 = 2.0 ** -8
K_STEP = 12
K_GAINS = 25                # + H
K_LIF = dict(g_x=10, g_mem_prev=11, raw_slope=9)    # slope sum: 9 + B
TINY = 2.0 ** -149


def rb(x):
    return x.to(BF16).to(F32)


def _rounder(dtype):
    return rb if dtype == BF16 else (lambda x: x)


def f32s(x):
    """A Python scalar as the kernels receive it: rounded to fp32."""
    return float(torch.tensor(float(x), dtype=F32))


def bound(K, M, u=U24, want=None, out_dtype=F32):
    """``gamma_K M`` (+ one rounding of the result for a bf16 output).  K: a number or a tensor broadcast to M."""
    K = torch.as_tensor(K, dtype=F64)
    gamma = torch.where(K * u < 1.0, K * u / (1.0 - K * u).clamp_min(TINY), torch.full_like(K, float("inf")))
    b = torch.where(M > 0, gamma * M, torch.zeros_like(M)) + K * TINY
    if out_dtype == BF16:
        b = b + U8 * (want.abs() + b)
    return b


def worst_ratio(got, rule, u=U24, out_dtype=F32):
    """max over EVERY element of |got - want| / bound for a ``(want, M, K)`` triple; a NaN counts as infinite."""
    want, M, K = rule
    got = got.detach().cpu().to(F64)
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if got.numel() == 0:
        return 0.0
    err = (got - want).abs()
    ratio = torch.where(err > 0, err / bound(K, M, u=u, want=want, out_dtype=out_dtype), torch.zeros_like(err))
    return float(torch.where(torch.isnan(got), torch.full_like(ratio, float("inf")), ratio).max())


# ---- GIF and prosody GIF --------------------------------------------------------------------------------------

def _step_consts(gains, t, alpha, strength, r):
    """(g, raw, scale, ae) [rows, 1] fp32 of step t, rounded as the forward rounds them."""
    g = gains[:, t].to(F32).unsqueeze(1)
    raw = r(1.0 - r(strength * r(g - 1.0)))
    return g, raw, torch.clamp(raw, 0.5, 1.5), r(alpha * g)


def _mid(a, th, L, scale, prosody, r):
    """fp32 (te, cl, b, d, n, s) of one step from (a, theta_prev)."""
    te = r(th * scale) if scale is not None else th
    cl = r(r(L * te) * 2.0)
    b = torch.minimum(torch.maximum(a, -cl), cl)
    d = te if prosody else r(th + 1e-6)
    n = r(b / d)
    s = torch.clamp(torch.floor(n), 0, L)
    return te, cl, b, d, n, s


def gif_forward(h, v0, th0, decay, L, alpha, thr0, gains=None, strength=0.0, prosody=False):
    """``dict(spikes, v, theta, save_a, save_theta, n)``: tensors of h's dtype (n fp32, [rows, T, H])."""
    dtype = h.dtype
    r = _rounder(dtype)
    v, th = v0.to(F32), th0.to(F32)
    mod = prosody and gains is not None
    S, A, TH, N = [], [], [], []
    for t in range(h.shape[1]):
        x = h[:, t].to(F32)
        scale, ae = None, alpha
        if mod:
            g, _, scale, ae = _step_consts(gains, t, alpha, strength, r)
            x = r(x * g)
        a = r(r(v * decay) + x)
        te, cl, b, d, n, s = _mid(a, th, L, scale, prosody, r)
        A.append(a); TH.append(th); S.append(s); N.append(n)
        v = r(b - r(s * te))
        if alpha > 0:
            th = r(r(th + r(ae * s)) - r(ae * r(th - thr0)))
    st = lambda xs: torch.stack(xs, dim=1) if xs else h.new_zeros(h.shape, dtype=F32)
    return dict(spikes=st(S).to(dtype), v=v.to(dtype), theta=th.to(dtype), save_a=st(A).to(dtype),
                save_theta=st(TH).to(dtype), n=st(N))


def gif_backward(save_a, save_theta, g_spikes, g_v, g_theta, decay, L, alpha, thr0, h=None, gains=None,
                 strength=0.0, prosody=False):
    """fp64 BPTT.  Returns ``dict(g_h, g_v0, g_theta0, g_gains)`` of ``(value, M, K)`` triples (g_gains None
    without gains); K is a tensor broadcastable to the value."""
    dtype = save_a.dtype
    r = _rounder(dtype)
    rows, T, H = save_a.shape
    mod = prosody and gains is not None
    D = lambda x: x.to(F64)
    dec, al, st, th0 = f32s(decay), f32s(alpha), f32s(strength), f32s(thr0)
    Lf = float(L)
    gv, gth = D(g_v).clone(), D(g_theta).clone()
    Mv, Mth = gv.abs(), gth.abs()
    gh, Mh = torch.zeros(rows, T, H, dtype=F64), torch.zeros(rows, T, H, dtype=F64)
    gg = torch.zeros(rows, T, dtype=F64) if mod else None
    Mg = torch.zeros(rows, T, dtype=F64) if mod else None
    zero = torch.zeros(rows, H, dtype=F64)
    for t in range(T - 1, -1, -1):
        a, thp = save_a[:, t].to(F32), save_theta[:, t].to(F32)
        g = raw = scale = None
        ae = torch.full((rows, 1), al, dtype=F64)
        if mod:
            g, raw, scale, ae32 = _step_consts(gains, t, alpha, strength, r)
            ae = D(ae32)
        te, cl, b, d, n, s = _mid(a, thp, L, scale, prosody, r)
        lo, hi = a < -cl, a > cl
        inside = ~(lo | hi)
        window = (n >= 0.0) & (n <= Lf + 1.0)
        te, b, d, n, s, thp = D(te), D(b), D(d), D(n), D(s), D(thp)
        tri = torch.clamp(1.0 - 2.0 * (n - torch.round(n)).abs(), 0.0, 1.0)
        sur = torch.where(window, tri, zero)
        gs = D(g_spikes[:, t])
        gs_tot, Ms = gs - te * gv, gs.abs() + te.abs() * Mv
        gthp, Mthp = gth.clone(), Mth.clone()
        acc, Macc = zero.clone(), zero.clone()
        if al > 0.0:
            gs_tot, Ms = gs_tot + ae * gth, Ms + ae.abs() * Mth
            gthp, Mthp = gthp - ae * gth, Mthp + ae.abs() * Mth
            if mod:
                acc = acc + gth * (s - (thp - th0)) * al
                Macc = Macc + Mth * (s + thp.abs() + abs(th0)) * al
        gte, Mte = -s * gv, s * Mv
        gn, Mn = gs_tot * sur, Ms * sur
        gb, Mb = gv + gn / d, Mv + Mn / d.abs()
        gte, Mte = gte - gn * b / (d * d), Mte + Mn * b.abs() / (d * d)
        ga, Ma = torch.where(inside, gb, zero), torch.where(inside, Mb, zero)
        gcl = torch.where(lo, -gb, torch.where(hi, gb, zero))
        gte, Mte = gte + gcl * (2.0 * Lf), Mte + torch.where(inside, zero, Mb) * (2.0 * Lf)
        if mod:
            sc = D(scale)
            gthp, Mthp = gthp + gte * sc, Mthp + Mte * sc
            live = (raw >= 0.5) & (raw <= 1.5)
            acc = acc + torch.where(live, gte * thp * (-st), zero)
            Macc = Macc + torch.where(live, Mte * thp.abs() * abs(st), zero)
            x = D(h[:, t])
            acc, Macc = acc + ga * x, Macc + Ma * x.abs()
            gg[:, t], Mg[:, t] = acc.sum(dim=1), Macc.sum(dim=1)
            gh[:, t], Mh[:, t] = ga * D(g), Ma * D(g).abs()
        else:
            gthp, Mthp = gthp + gte, Mthp + Mte
            gh[:, t], Mh[:, t] = ga, Ma
        gv, Mv = ga * dec, Ma * abs(dec)
        gth, Mth = gthp, Mthp
    steps = (T - torch.arange(T, dtype=F64))                  # steps travelled when g_h[t] is written
    out = dict(g_h=(gh, Mh, (K_STEP * steps).view(1, T, 1)), g_v0=(gv, Mv, torch.tensor(float(K_STEP * T))),
               g_theta0=(gth, Mth, torch.tensor(float(K_STEP * T))), g_gains=None)
    if mod:
        out["g_gains"] = (gg, Mg, (K_STEP * steps + K_GAINS + H).view(1, T))
    return out


# ---- LIF step -------------------------------------------------------------------------------------------------

def lif_forward(x, mem, beta, thr):
    """``dict(spikes, mem, pre)`` of x's dtype: mm = beta mem + x; pre = mm - thr; s = pre > 0; mem' = mm - s thr."""
    dtype = x.dtype
    r = _rounder(dtype)
    x, mem, beta, thr = (t.to(F32) for t in (x, mem, beta, thr))
    mm = r(r(beta * mem) + x)
    pre = r(mm - thr)
    s = (pre > 0).to(F32)
    return dict(spikes=s.to(dtype), mem=r(mm - s * thr).to(dtype), pre=pre.to(dtype))


def lif_backward(pre, g_spk, g_mem, beta, thr, slope):
    """``dict(g_x, g_mem_prev, raw_slope, slope_sum)`` of ``(value, M, K)``; the comment above ``lif_bwd_kernel``
    and ``LearnableSurrogateFn.backward``: sign(0) = 0."""
    pr, gs, gm, bt, th, sl = (t.to(F64) for t in (pre, g_spk, g_mem, beta, thr, slope))
    g_s, M_s = gs - gm * th, gs.abs() + gm.abs() * th.abs()
    den = (sl * pr).abs() + 1.0
    g_m, M_m = gm + g_s * (sl / (den * den)), gm.abs() + M_s * (sl.abs() / (den * den))
    ap = pr.abs()
    den2 = sl * ap + 1.0
    raw, M_raw = -g_s * ap * torch.sign(pr) / (den2 * den2), M_s * ap / (den2 * den2)
    B = pr.shape[0]
    return dict(g_x=(g_m, M_m, K_LIF["g_x"]), g_mem_prev=(bt * g_m, bt.abs() * M_m, K_LIF["g_mem_prev"]),
                raw_slope=(raw, M_raw, K_LIF["raw_slope"]),
                slope_sum=(raw.sum(dim=0), M_raw.sum(dim=0), K_LIF["raw_slope"] + B))


# ---- AdditionLinear -------------------------------------------------------------------------------------------

def addition_linear_backward(x, w, g):
    """``dict(g_x, g_w)`` of ``(value fp64, bound)``: g_x[b][k] = -sum_o g[b][o] sgn(x[b][k] - w[o][k]),
    g_w[o][k] = +sum_b (the same); sgn(0) = 0 for +0 and -0.  Bound ``(T + 2) u sum|g|`` over the reduction."""
    B, OUT = g.shape
    sg = torch.sign(x.to(F64).unsqueeze(1) - w.to(F64).unsqueeze(0))          # [B, OUT, IN], exact sign
    g64 = g.to(F64)
    g_x = -(g64.unsqueeze(2) * sg).sum(dim=1)
    g_w = (g64.unsqueeze(2) * sg).sum(dim=0)
    bx = ((OUT + 2) * U24 * g64.abs().sum(dim=1, keepdim=True)).expand_as(g_x)
    bw = ((B + 2) * U24 * g64.abs().sum(dim=0).unsqueeze(1)).expand_as(g_w)
    return dict(g_x=(g_x, bx), g_w=(g_w, bw))
