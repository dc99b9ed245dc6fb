"""Inputs shared by tests/test_host_surrogate_rule.py (CPU) and tests/test_gpu_surrogate.py: the host test anchors
the rule of tests/surrogate_rule.py in the oracle on exactly the tensors the GPU tests feed the kernels.

Random cases are pushed away from the surrogate window's two discontinuities (n = 0 and n = L + 1) by
``keep_distance``; the hand-made cases stand on the decision points themselves and every number in them is a
short dyadic fraction, so that (where the effective threshold is a power of two) each operation of the backward
pass is exact in fp32 as in fp64."""
import functools
import math
from collections import namedtuple

import torch

from tests import surrogate_rule as R

F32, BF16 = torch.float32, torch.bfloat16
DECAY = math.exp(-0.1)
THR0 = 1.0
STRENGTH = 0.3
NEAR = 1e-4
ONE_GRID_PASS = 2048 * 256

# kind: "gif", "prosody" (gains: with / without)
Case = namedtuple("Case", "name kind dtype rows T H L alpha gains")


def _c(kind, dtype, rows, T, H, L, alpha, gains=False):
    name = (f"{kind}{'-gains' if gains else ''}-{'f32' if dtype == F32 else 'bf16'}-{rows}x{T}x{H}-L{L}-a{alpha}")
    return Case(name, kind, dtype, rows, T, H, L, alpha, gains)


def _kinds():
    return (("gif", False), ("prosody", True), ("prosody", False))


# vector and scalar instance by shape: H 24 (VEC 4 / 8), 13 (scalar), 20 (VEC 4 in fp32, scalar in bf16)
INSTANCE_CASES = [_c(k, dt, 5, 6, H, 8, 0.05, g) for k, g in _kinds() for dt in (F32, BF16) for H in (24, 13, 20)]
# T = 1; alpha = 0 with and without gains; L = 1, 2, 16; bf16 L = 256 (the documented limit)
EDGE_CASES = ([_c(k, dt, 3, 1, 24, 4, 0.05, g) for k, g in _kinds() for dt in (F32, BF16)] +
              [_c(k, dt, 4, 5, 24, 8, 0.0, g) for k, g in _kinds() for dt in (F32, BF16)] +
              [_c(k, F32, 4, 5, 13, L, 0.05, g) for k, g in _kinds() for L in (1, 2, 16)] +
              [_c(k, BF16, 4, 5, 24, 256, 0.05, g) for k, g in _kinds()])
SMALL_CASES = INSTANCE_CASES + EDGE_CASES
# second grid pass: more than 2048 x 256 work items at T = 1
BIG_CASES = [_c(k, dt, 4100, 1, H, 8, 0.05, g) for k, g in _kinds()
             for dt, H in ((F32, 129), (F32, 516), (BF16, 129), (BF16, 1032))]

LIF_CASES = [(dt, B, C) for dt in (F32, BF16) for B, C in ((5, 24), (7, 13), (6, 20), (1, 4))]
LIF_BIG_CASES = [(F32, 4100, 129), (F32, 4100, 516), (BF16, 4100, 129), (BF16, 4100, 1032)]

ADDLIN_SHAPES = [(1, 1, 1), (63, 65, 31), (64, 64, 32), (65, 63, 33), (130, 70, 200)]


def case_id(c):
    return c.name if isinstance(c, Case) else f"{'f32' if c[0] == F32 else 'bf16'}-{c[1]}x{c[2]}"


def vec_width(c):
    """The instance the shape selects (all pointers aligned)."""
    if c.dtype == F32:
        return 4 if c.H % 4 == 0 else 1
    return 8 if c.H % 8 == 0 else 1


def near_discontinuity(n, L):
    """Elements whose n lies within NEAR of 0 or of L + 1 without being exactly there."""
    return ((n.abs() < NEAR) & (n != 0)) | (((n - (L + 1.0)).abs() < NEAR) & (n != L + 1.0))


def forward(c, t):
    return R.gif_forward(t["h"], t["v0"], t["t0"], DECAY, c.L, c.alpha, THR0, gains=t["gains"], strength=STRENGTH,
                         prosody=c.kind == "prosody")


def backward(c, t, fwd):
    return R.gif_backward(fwd["save_a"], fwd["save_theta"], t["ws"], t["wv"], t["wt"], DECAY, c.L, c.alpha, THR0,
                          h=t["h"], gains=t["gains"], strength=STRENGTH, prosody=c.kind == "prosody")


def keep_distance(c, t):
    """Move the currents whose n falls within NEAR of a discontinuity toward zero, half a threshold at a time,
    until none does.  (At L = 1 the GIF's upper clamp bound 2 L theta lands on n = (L + 1) (1 - 1e-6): there
    the move takes the potential back under the bound, and the lower bound is the one that binds.)"""
    for _ in range(64):
        n = forward(c, t)["n"]
        near = near_discontinuity(n, c.L)
        if not bool(near.any()):
            return
        t["h"] = torch.where(near, (t["h"].float() - 0.5 * torch.sign(n)).to(c.dtype), t["h"])
    raise AssertionError(f"{c.name}: currents stay near a discontinuity")


def _build(c):
    g = torch.Generator().manual_seed(c.rows * 131 + c.T * 7 + c.H + 1000 * c.L)
    amp = float(max(3, c.L))
    t = dict(h=(torch.randn(c.rows, c.T, c.H, generator=g) * amp).to(c.dtype),
             v0=(0.4 * torch.randn(c.rows, c.H, generator=g)).to(c.dtype),
             t0=(1.0 + 0.3 * torch.rand(c.rows, c.H, generator=g)).to(c.dtype),
             gains=(0.2 + 3.0 * torch.rand(c.rows, c.T, generator=g)).to(c.dtype) if c.gains else None)
    for k, s in (("ws", (c.rows, c.T, c.H)), ("wv", (c.rows, c.H)), ("wt", (c.rows, c.H))):
        t[k] = torch.randn(s, generator=g).to(c.dtype)
    keep_distance(c, t)
    return t


@functools.lru_cache(maxsize=None)
def _small(c):
    t = _build(c)
    fwd = forward(c, t)
    return t, fwd, backward(c, t, fwd)


@functools.lru_cache(maxsize=1)
def _big(c):
    t = _build(c)
    fwd = forward(c, t)
    return t, fwd, backward(c, t, fwd)


def gif_case(c):
    """``(tensors, rule forward, rule backward)``, computed once per case and shared; treat as read-only."""
    return _big(c) if c.rows * c.H > 100000 else _small(c)


# ---- hand-made decision points ---------------------------------------------------------------------------------
DP_L = 4
DP_DECAY = 0.5
DP_ALPHA = 0.25
DP_STRENGTH = 0.5
# GIF: theta_0 = 1 - 2^-20, for which d = fl(theta_0 + 1e-6f) = 1 exactly and n = b
DP_GIF_THETA = 1.0 - 2.0 ** -20
# gains whose raw scale 1 - 0.5 (g - 1) is 1; 0.5 exactly, just below (dead), just above; 1.5 exactly, just above
# (dead), just below
DP_GAINS = [1.0, 2.0, 2.0 + 2.0 ** -22, 2.0 - 2.0 ** -23, 0.0, -2.0 ** -22, 2.0 ** -22]
# rows whose scale is 1 or 0.5: every operation exact.  (Dividing by te = 1.5 rounds, and so does a scale one ulp
# off: on those rows the decision is held by the bound, which a wrong side of the scale clamp misses by far.)
DP_EXACT_ROWS = [0, 1, 2]


def _nx(x, to):
    return float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(to, dtype=F32)))


def _points(te, L):
    """Pre-clamp potentials standing on every decision point for an effective threshold te (n = a / te)."""
    cl = float((torch.tensor(float(L), dtype=F32) * torch.tensor(te, dtype=F32)) * 2.0)
    top = float(torch.tensor(te, dtype=F32) * (L + 1.0))
    return [cl, _nx(cl, math.inf), -cl, _nx(-cl, -math.inf), 3.0 * te, 2.5 * te, 0.0, -0.0, top, _nx(top, math.inf)]


DP_NAMES = ["a=+cl", "a>+cl", "a=-cl", "a<-cl", "n=3", "n=2.5", "n=+0", "n=-0", "n=L+1", "n>L+1"]
_DYADIC = [1.0, -0.5, 2.0, 0.75, -1.5, 0.25, -2.0, 1.25, 0.5, -0.75]


@functools.lru_cache(maxsize=None)
def decision_case(kind, gains):
    """T = 1.  ``(tensors, cfg)`` with cfg = (decay, L, alpha, thr0, strength).  a_0 = v0 decay + h g is reached
    through v0 (h is a per-row constant), so that the same potentials stand under every gain."""
    H = len(DP_NAMES)
    if kind == "gif":
        a = torch.tensor([_gif_points()], dtype=F32)
        t = dict(h=a.view(1, 1, H).clone(), v0=torch.zeros(1, H), t0=torch.full((1, H), DP_GIF_THETA), gains=None)
        rows = 1
    elif not gains:
        a = torch.tensor([_points(1.0, DP_L)], dtype=F32)
        t = dict(h=a.view(1, 1, H).clone(), v0=torch.zeros(1, H), t0=torch.ones(1, H), gains=None)
        rows = 1
    else:
        rows = len(DP_GAINS)
        g = torch.tensor(DP_GAINS, dtype=F32)
        scale = torch.clamp(1.0 - DP_STRENGTH * (g - 1.0), 0.5, 1.5)
        hx = torch.tensor([1.0, 0.25, 0.0, 0.0, 1.0, 0.0, 0.0])
        a = torch.stack([torch.tensor(_points(float(s), DP_L), dtype=F32) for s in scale])
        v0 = ((a.double() - (hx * g).double().unsqueeze(1)) / DP_DECAY).float()
        t = dict(h=hx.view(rows, 1, 1).expand(rows, 1, H).contiguous(), v0=v0, t0=torch.ones(rows, H),
                 gains=g.view(rows, 1).clone())
    dy = torch.tensor(_DYADIC)
    if not gains:
        t["v0"][0, 7] = -0.0                    # (-0) decay + (-0) = -0: the only way to a_0 = -0
    t["ws"] = dy.view(1, 1, H).expand(rows, 1, H).contiguous()
    t["wv"] = dy.flip(0).view(1, H).expand(rows, H).contiguous()
    t["wt"] = (0.5 * dy.roll(3)).view(1, H).expand(rows, H).contiguous()
    if gains:                                   # odd gains: keep the theta chain out of the inexact products
        odd = [r for r in range(rows) if r not in DP_EXACT_ROWS]
        t["wt"][odd] = 0.0
    return t, (DP_DECAY, DP_L, DP_ALPHA, THR0, DP_STRENGTH)


def _gif_points():
    th = torch.tensor(DP_GIF_THETA, dtype=F32)
    cl = float((DP_L * th) * 2.0)
    return [cl, _nx(cl, math.inf), -cl, _nx(-cl, -math.inf), 3.0, 2.5, 0.0, -0.0, DP_L + 1.0, _nx(DP_L + 1.0, math.inf)]


def decision_rule(kind, gains):
    t, (decay, L, alpha, thr0, strength) = decision_case(kind, gains)
    pros = kind == "prosody"
    fwd = R.gif_forward(t["h"], t["v0"], t["t0"], decay, L, alpha, thr0, gains=t["gains"], strength=strength,
                        prosody=pros)
    bwd = R.gif_backward(fwd["save_a"], fwd["save_theta"], t["ws"], t["wv"], t["wt"], decay, L, alpha, thr0,
                         h=t["h"], gains=t["gains"], strength=strength, prosody=pros)
    return t, fwd, bwd


# ---- LIF ------------------------------------------------------------------------------------------------------

def _lif_build(dtype, B, C):
    g = torch.Generator().manual_seed(B * 17 + C)
    t = dict(x=torch.randn(B, C, generator=g).to(dtype), mem=(0.5 * torch.randn(B, C, generator=g)).to(dtype),
             beta=(0.5 + 0.49 * torch.rand(C, generator=g)).to(dtype), thr=(0.3 + torch.rand(C, generator=g)).to(dtype),
             slope=(2 + 6 * torch.rand(C, generator=g)).to(dtype), g_spk=torch.randn(B, C, generator=g).to(dtype),
             g_mem=torch.randn(B, C, generator=g).to(dtype))
    fwd = R.lif_forward(t["x"], t["mem"], t["beta"], t["thr"])
    return t, fwd, R.lif_backward(fwd["pre"], t["g_spk"], t["g_mem"], t["beta"], t["thr"], t["slope"])


_lif_small = functools.lru_cache(maxsize=None)(_lif_build)
_lif_big = functools.lru_cache(maxsize=1)(_lif_build)


def lif_case(dtype, B, C):
    return _lif_big(dtype, B, C) if B * C > 100000 else _lif_small(dtype, B, C)


@functools.lru_cache(maxsize=None)
def lif_decision_case():
    """pre = 0 (x = thr, mem = 0: sign 0), the fp32 neighbours of it on both sides, and +-1; dyadic throughout."""
    thr = torch.tensor([0.5, 0.5, 0.5, 0.75, 0.75, 0.5, 1.0, 0.25])
    x = thr.clone()
    x[1], x[2] = _nx(0.5, 1.0), _nx(0.5, 0.0)
    x[5], x[6] = 1.5, 0.0                                          # pre = 1, -1
    x = torch.stack([x, x])
    t = dict(x=x, mem=torch.zeros(2, 8), beta=torch.full((8,), 0.5), thr=thr, slope=torch.full((8,), 4.0),
             g_spk=torch.tensor(_DYADIC[:8]).expand(2, 8).contiguous(),
             g_mem=torch.tensor(_DYADIC[2:]).expand(2, 8).contiguous())
    fwd = R.lif_forward(t["x"], t["mem"], t["beta"], t["thr"])
    return t, fwd, R.lif_backward(fwd["pre"], t["g_spk"], t["g_mem"], t["beta"], t["thr"], t["slope"])


# ---- AdditionLinear -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def addition_linear_case(B, IN, OUT):
    """Random x, w, g with a block of exact ties (x == w), among them x = +0 against w = -0."""
    g = torch.Generator().manual_seed(B * 7 + IN * 3 + OUT)
    x = torch.randn(B, IN, generator=g) * 0.2
    w = torch.randn(OUT, IN, generator=g) * 0.2
    gout = torch.randn(B, OUT, generator=g)
    nb, no, ni = min(B, 3), min(OUT, 2), min(IN, 5)
    if B:
        x[:nb, :ni] = w[no - 1, :ni]                                # ties of rows 0..nb-1 with template no-1
        x[0, 0], w[:, 0] = 0.0, -0.0                                # +0 against -0: a tie for every template
        x[:nb, 0] = 0.0
    return x, w, gout
