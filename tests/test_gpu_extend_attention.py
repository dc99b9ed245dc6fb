"""``ops.attn_decode_extend`` on the GPU (csrc/aura_decode.hip) against ``m`` calls of ``ops.attn_decode_step`` on clones
of the same caches: the rule of ``include/aura_hip.h`` ("Decode attention: extend") is the step's rule per query, so the
comparison is for bits.  The step is not under test here: tests/test_gpu_decode_attention.py holds it to fp64, and
bit-equality inherits that bound.

Every cache position at or past a row's length holds NaN before the call, so a new position read back from the cache
(a race between the appending and the reading waves) shows in ``ctx``.  All comparisons are on integer views: NaN
compares.  Asserted per case, no element left out: ``ctx``, the scales, both caches and the lengths equal the ``m``
steps'; the cache positions ``L .. L + m - 1`` are the bits of ``k_new`` / ``v_new`` and every other cache element is
unchanged; inactive rows (retired, or ``L + m > cap``) are untouched with zero ``ctx`` and scale; a row's bits are the
same alone and in the batch, for ``cap`` and ``2 cap``, for the minimal and the default ``n_chunks`` and over two calls;
``advance=False`` leaves the lengths alone.

Shapes ``(H, dh, m, lengths)`` with ``B = len(lengths)``: dh = 4, 32, 48, 64, 128 (every lane-group width); m = 1, 2, 3,
5, 8, 9, 17, 32 (the query group is 8: one group, one more than a group, two groups and one, four groups); L = 0, 1, 3,
4, 5, 62, 63, 250, 254, 255, 256, 257, 508, 1000, so that ``L .. L + m - 1`` crosses a block-of-four edge, a slot edge
and a chunk edge (L = 250 with m = 9, 255 with 2, 254 with 32); a ragged batch with a retired row, a row that does not
fit and an active one.  Kinds as in the step's test: random, peaked (one score 200 above the rest, among the old and
among the new positions), flat (equal keys), saturated prosody (+-50), no prosody, no memory gate."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

CHUNK = 256
KINDS = ["random", "peaked", "flat", "saturated", "no_prosody", "no_memory"]
# (H, dh, m, lengths); -1 retires a row, "full" marks a row that is m - 1 short of fitting
SHAPES = [
    (1, 4, 1, (0,)),
    (3, 32, 2, (255, 0, 1)),
    (3, 32, 9, (250, 3, 4)),
    (3, 32, 32, (254, 5, 62)),
    (1, 32, 3, (63, 256, 257)),
    (3, 32, 5, (508, 1000, 255)),
    (1, 32, 8, (1000,)),
    (3, 32, 17, (250, 254, 1000)),
    (1, 4, 9, (3, 254, 508)),
    (3, 4, 32, (62,)),
    (1, 48, 17, (4, 255, 63)),
    (3, 48, 32, (250,)),
    (1, 64, 9, (255, 5, 257)),
    (3, 64, 32, (254, 0, 508)),
    (1, 128, 32, (254, 63, 1)),
    (3, 128, 5, (256,)),
    (3, 32, 9, (-1, "full", 250)),
    (1, 64, 32, (250, "full", -1)),
]
ALL_KINDS = {2, 3, 13, 16}                               # these shapes run every kind, the others random inputs only
CASES = [(i, k) for i in range(len(SHAPES)) for k in (KINDS if i in ALL_KINDS else KINDS[:1])]


def _id(case):
    i, kind = case
    H, dh, m, lengths = SHAPES[i]
    return f"H{H}-dh{dh}-m{m}-L{'_'.join(str(x) for x in lengths)}-{kind}"


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs of one case, computed once and never modified."""
    i, kind = case
    H, dh, m, lengths = SHAPES[i]
    rng = np.random.default_rng(1000 + 7 * i + KINDS.index(kind))
    B, D = len(lengths), H * dh
    cap = max(x for x in lengths if x != "full") + m + 3 if any(x != "full" and x >= 0 for x in lengths) else m + 3
    L = np.array([cap - m + 1 if x == "full" else x for x in lengths], np.int32)
    act = (L >= 0) & (L + m <= cap)
    draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    q, k, v, x = draw(B, m, D), draw(B, m, D), draw(B, m, D), draw(B, m, D)
    K, V = draw(B, H, cap, dh), draw(B, H, cap, dh)
    prosody = (1.5 * rng.standard_normal((B, m, 4))).astype(np.float32)
    Wp, bp = draw(H, 4), draw(H)
    wm, bm = (rng.standard_normal((1, D)) / np.sqrt(D)).astype(np.float32), draw(1)
    if kind == "saturated":
        prosody = np.where(rng.random((B, m, 4)) < 0.5, -50.0, 50.0).astype(np.float32)
    if kind == "no_prosody":
        prosody = None
    if kind == "no_memory":
        wm = bm = None
    if kind == "flat":
        K[:] = K[:, :, :1]
        k[:] = K[:, :, 0].reshape(B, 1, D)
    if kind == "peaked":                                 # the scale is at least 0.76: a score of at least 220 against ~0.05 |q|
        K *= np.float32(0.05)
        k *= np.float32(0.05)
        for b in np.nonzero(act)[0]:
            for h in range(H):
                hs = slice(h * dh, (h + 1) * dh)
                q0, ql = q[b, 0, hs].astype(np.float64), q[b, m - 1, hs].astype(np.float64)
                if L[b] > 0:                             # among the old positions, aligned with the first query
                    K[b, h, L[b] // 2] = (q0 * (290.0 * np.sqrt(dh) / (q0 @ q0))).astype(np.float32)
                k[b, m // 2, hs] = (ql * (290.0 * np.sqrt(dh) / (ql @ ql))).astype(np.float32)   # among the new ones
    for b in range(B):                                   # NaN wherever nothing may be read
        K[b, :, max(int(L[b]), 0):] = np.nan
        V[b, :, max(int(L[b]), 0):] = np.nan
    out = dict(B=B, H=H, dh=dh, D=D, m=m, cap=cap, L=L, act=act, q=q, k=k, v=v, x=x, K=K, V=V,
               gates=dict(prosody=prosody, Wp=Wp, bp=bp, wm=wm, bm=bm))
    for a in (q, k, v, x, K, V, L, act):
        a.setflags(write=False)
    return out


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _gates(c, dev, sel):
    g = c["gates"]
    return (None if g["prosody"] is None else _dev(g["prosody"][sel], dev), _dev(g["Wp"], dev), _dev(g["bp"], dev),
            _dev(g["wm"], dev), _dev(g["bm"], dev))


def _extend(ops, c, dev, K, V, L, rows=None, n_chunks=None, advance=True):
    """One extend on fresh device copies (rows: a sub-batch).  Returns ctx, scale, K, V, lengths."""
    sel = slice(None) if rows is None else rows
    t = {n: _dev(c[n][sel], dev) for n in ("q", "k", "v", "x")}
    prosody, Wp, bp, wm, bm = _gates(c, dev, sel)
    Kd, Vd, Ld = _dev(K[sel], dev), _dev(V[sel], dev), _dev(L[sel], dev)
    B, H, cap, dh = Kd.shape
    nc = ops.attn_decode_chunks(cap) if n_chunks is None else n_chunks
    ws = torch.full((ops.attn_decode_extend_workspace_floats(B, c["m"], H, dh, nc),), float("nan"), device=dev)
    keep = {n: a.clone() for n, a in t.items()}
    ctx, s = ops.attn_decode_extend(t["q"], t["k"], t["v"], t["x"], prosody, Wp, bp, wm, bm, Ld, Kd, Vd, ws,
                                    n_chunks=nc, advance=advance, return_scale=True)
    for n, a in keep.items():
        assert torch.equal(_bits(t[n]), _bits(a)), f"input {n} was written"
    return ctx, s, Kd, Vd, Ld


def _steps(ops, c, dev):
    """The reference: ``m`` calls of the step on fresh device copies of the same caches."""
    t = {n: _dev(c[n], dev) for n in ("q", "k", "v", "x")}
    prosody, Wp, bp, wm, bm = _gates(c, dev, slice(None))
    Kd, Vd, Ld = _dev(c["K"], dev), _dev(c["V"], dev), _dev(c["L"], dev)
    # a row that does not fit whole is inactive whole in the extend; the steps would fill it until it is full
    Ld[torch.from_numpy(~c["act"]).to(dev)] = -1
    B, H, cap, dh = Kd.shape
    nc = ops.attn_decode_chunks(cap)
    ws = torch.empty(ops.attn_decode_workspace_floats(B, H, dh, nc), device=dev)
    ctx, scale = [], []
    for j in range(c["m"]):
        o, s = ops.attn_decode_step(t["q"][:, j].contiguous(), t["k"][:, j].contiguous(), t["v"][:, j].contiguous(),
                                    t["x"][:, j].contiguous(), None if prosody is None else prosody[:, j].contiguous(),
                                    Wp, bp, wm, bm, Ld, Kd, Vd, ws, n_chunks=nc, return_scale=True)
        ctx.append(o)
        scale.append(s)
    Ld = torch.where(_dev(c["act"], dev), Ld, _dev(c["L"], dev))
    return torch.stack(ctx, dim=1), torch.stack(scale, dim=1), Kd, Vd, Ld


@functools.lru_cache(maxsize=None)
def _run(case, dev):
    """One extend and the ``m`` steps of one case on the device, once: shared by the tests that compare with them."""
    from aura_snn_rag_amd import ops
    c = _case(case)
    got = _extend(ops, c, dev, c["K"], c["V"], c["L"])
    want = _steps(ops, c, dev)
    torch.cuda.synchronize()
    return got, want


COUNTS = dict(cases=0, elements=0, mismatches=0)


def _same(name, got, want):
    """Bit equality, counted for the recorded profile."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{name}: shape {tuple(g.shape)} against {tuple(w.shape)}"
    bad = int((g != w).sum())
    COUNTS["elements"] += g.numel()
    COUNTS["mismatches"] += bad
    helpers.record_parity("extend attention: bits against m steps", COUNTS["elements"] - COUNTS["mismatches"],
                          COUNTS["elements"], cases=COUNTS["cases"], mismatches=COUNTS["mismatches"])
    assert bad == 0, f"{name}: {bad} of {g.numel()} elements differ from the m steps"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_one_extend_leaves_the_bits_of_m_steps(dev, case):
    c = _case(case)
    got, want = _run(case, dev)
    COUNTS["cases"] += 1
    for name, g, w in zip(("ctx", "scale", "K", "V", "lengths"), got, want):
        _same(f"{_id(case)} {name}", g, w)
    ctx, scale, K, V, Ln = got
    assert np.array_equal(Ln.cpu().numpy(), np.where(c["act"], c["L"] + c["m"], c["L"])), "lengths advance by m"
    assert bool(torch.isfinite(ctx).all()), "a NaN position was read"
    assert bool((ctx.cpu()[~c["act"]] == 0).all()) and bool((scale.cpu()[~c["act"]] == 0).all()), "inactive rows are 0"
    assert bool((scale.cpu()[np.array(c["act"])] > 0).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_caches_change_at_the_new_positions_only(dev, case):
    c = _case(case)
    (_, _, K, V, _), _ = _run(case, dev)
    B, H, dh, m, L, act = c["B"], c["H"], c["dh"], c["m"], c["L"], c["act"]
    K, V = _bits(K).numpy(), _bits(V).numpy()
    K0, V0 = c["K"].view(np.int32), c["V"].view(np.int32)
    for b in range(B):
        keep = np.ones(c["cap"], bool)
        if act[b]:
            keep[L[b]:L[b] + m] = False
            new_k = c["k"][b].reshape(m, H, dh).transpose(1, 0, 2).view(np.int32)
            new_v = c["v"][b].reshape(m, H, dh).transpose(1, 0, 2).view(np.int32)
            assert np.array_equal(K[b, :, L[b]:L[b] + m], new_k), f"row {b}: appended K"
            assert np.array_equal(V[b, :, L[b]:L[b] + m], new_v), f"row {b}: appended V"
        assert np.array_equal(K[b][:, keep], K0[b][:, keep]), f"row {b}: K written away from the new positions"
        assert np.array_equal(V[b][:, keep], V0[b][:, keep]), f"row {b}: V written away from the new positions"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_do_not_depend_on_batch_capacity_chunks_or_the_call(dev, case):
    from aura_snn_rag_amd import ops
    c = _case(case)
    (ctx, _, K, V, _), _ = _run(case, dev)
    B, m, L, act = c["B"], c["m"], c["L"], c["act"]
    want = _bits(ctx)
    again = _extend(ops, c, dev, c["K"], c["V"], L)
    assert torch.equal(_bits(again[0]), want), "two calls differ"
    assert torch.equal(_bits(again[2]), _bits(K)) and torch.equal(_bits(again[3]), _bits(V))
    still = _extend(ops, c, dev, c["K"], c["V"], L, advance=False)
    assert torch.equal(_bits(still[0]), want) and np.array_equal(still[4].cpu().numpy(), L), "advance=False"
    if act.any():
        minimal = (int(L[act].max()) + m - 1) // CHUNK + 1
        few = _extend(ops, c, dev, c["K"], c["V"], L, n_chunks=minimal)
        assert torch.equal(_bits(few[0]), want), f"n_chunks={minimal} differs from the default"
        assert torch.equal(_bits(few[2]), _bits(K))
    # twice the capacity (NaN beyond): a row that did not fit would fit there, so it is retired; the others keep their bits
    K2, V2 = (np.concatenate([a, np.full_like(a, np.nan)], axis=2) for a in (c["K"], c["V"]))
    wide = _extend(ops, c, dev, K2, V2, np.where(act, L, -1).astype(np.int32))
    assert torch.equal(_bits(wide[0]), want), "cap and 2 cap differ"
    for b in range(B):
        alone = _extend(ops, c, dev, c["K"], c["V"], L, rows=slice(b, b + 1))
        assert torch.equal(_bits(alone[0])[0], want[b]), f"row {b} alone differs from the batch"
    torch.cuda.synchronize()


def test_m_equal_one_is_the_step_and_the_limits_are_refused(dev):
    from aura_snn_rag_amd import ops
    f = lambda *s: torch.zeros(*s, device=dev)
    B, H, dh, cap = 2, 2, 8, 40
    args = lambda m: (f(B, m, 16), f(B, m, 16), f(B, m, 16), None, None, None, None, None, None,
                      torch.zeros(B, dtype=torch.int32, device=dev), f(B, H, cap, dh), f(B, H, cap, dh),
                      f(ops.attn_decode_extend_workspace_floats(B, max(m, 1), H, dh, 1)))
    with pytest.raises(ValueError, match="m=33"):
        ops.attn_decode_extend(*args(33))
    with pytest.raises(ValueError, match="m=0"):
        ops.attn_decode_extend(*args(0))
    a = args(32)
    out = ops.attn_decode_extend(*a)
    assert out.shape == (B, 32, 16) and a[9].tolist() == [32, 32]
    out = ops.attn_decode_extend(*a)                                    # 32 + 32 > 40: inactive whole, nothing advances
    assert a[9].tolist() == [32, 32] and bool((out == 0).all())
