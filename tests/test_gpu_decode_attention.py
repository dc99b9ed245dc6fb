"""``ops.attn_decode_step`` and the modules' ``prefill`` / ``step`` on the GPU (csrc/aura_decode.hip) against the rule of
``include/aura_hip.h`` ("Decode attention") as restated in tests/decode_attention_rule.py.

Every case runs the op once on caches whose positions ``>= L`` hold NaN in every row (a read past L shows in ``ctx``)
and asserts, with no element left out: the appended K/V are the bits of ``k_new`` / ``v_new``; every other cache
element, and every inactive row, is bit-unchanged; the lengths advanced by exactly one on active rows; ``ctx`` and the
scale ``s`` are within the rule file's derived bounds of fp64 on the same fp32 inputs; and every bit of ``ctx`` is the
same for a row alone and in the batch, for ``cap`` and ``2 cap``, for the minimal and the default ``n_chunks`` and for
two calls.  Three consecutive steps are compared with three steps of the rule.  A measured maximum above half its bound
is flagged in the recorded profile (``over_half_bound``).

Shapes ``(B, H, dh, cap, lengths)``: one element; dh = 4, 32, 48, 64, 128 (every lane-group width, 48 the one that is
no power of two); one batch with L = 0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 1000 (slot, block and chunk edges); a
ragged batch with a retired row and a full one at cap = 257; B H = 108 (more than a workgroup).  Kinds: random, peaked
(one score 200 above the rest), flat (equal keys), saturated prosody (+-50), no prosody, no memory gate.

Module level, D = 96 / H = 2 and D = 768 / H = 12: ``prefill(7)`` + 6 steps against ``forward(13)``.  Both are fp32
evaluations of one formula, so the tolerance is 8 x the error of the torch composition (``forward`` on the same GPU)
against the fp64 formula, computed here from the composition, not from the code under test; the margin is wide because
this test guards wiring."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import decode_attention_rule as R
from tests import helpers

pytestmark = pytest.mark.gpu

L_EDGES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 1000]
SHAPES = [(1, 1, 4, 1, (0,)),
          (2, 2, 4, 300, (100, 257)), (2, 2, 32, 300, (100, 257)), (2, 2, 48, 300, (100, 257)),
          (2, 2, 64, 300, (100, 257)), (2, 2, 128, 300, (100, 257)),
          (len(L_EDGES), 2, 32, 1001, tuple(L_EDGES)),
          (5, 2, 32, 257, (0, 255, 256, -1, 257)),
          (9, 12, 64, 300, (5, 299, 256, 0, 130, 64, 255, 17, 200))]
KINDS = ["random", "peaked", "flat", "saturated", "no_prosody", "no_memory"]
CASES = [(s, k) for s in SHAPES for k in KINDS]
STEPS = 3


def _id(case):
    (B, H, dh, cap, lengths), kind = case
    return f"B{B}-H{H}-dh{dh}-cap{cap}-{kind}"


def _draw(rng, B, D, s=1.0):
    return (s * rng.standard_normal((B, D))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs of one case and the fp64 rule on them, computed once and never modified."""
    (B, H, dh, cap, lengths), kind = case
    rng = np.random.default_rng(sum(map(ord, _id(case))))
    D = H * dh
    L = np.array(lengths, np.int32)
    act = R.active_rows(L, cap)
    steps = [dict(q=_draw(rng, B, D), k=_draw(rng, B, D), v=_draw(rng, B, D), x=_draw(rng, B, D)) for _ in range(STEPS)]
    K, V = (rng.standard_normal((B, H, cap, dh)).astype(np.float32) for _ in range(2))
    prosody = (1.5 * rng.standard_normal((B, 4))).astype(np.float32)
    Wp, bp = rng.standard_normal((H, 4)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    wm = (rng.standard_normal((1, D)) / np.sqrt(D)).astype(np.float32)
    bm = rng.standard_normal(1).astype(np.float32)
    if kind == "saturated":
        prosody = np.where(rng.random((B, 4)) < 0.5, -50.0, 50.0).astype(np.float32)
    if kind == "no_prosody":
        prosody = None
    if kind == "no_memory":
        wm = bm = None
    gates = dict(prosody=prosody, Wp=Wp, bp=bp, wm=wm, bm=bm)
    if kind == "flat":
        K[:] = K[:, :, :1]
        for st in steps:
            st["k"] = K[:, :, 0].reshape(B, D).copy()
    if kind == "peaked":                                # one position of every (b, h) scores 200 above the others
        s = R.scale64(B, H, x=steps[0]["x"], **gates)
        K *= np.float32(0.05)
        steps[0]["k"] *= np.float32(0.05)
        for b in np.nonzero(act)[0]:
            t = int(L[b]) // 2
            for h in range(H):
                qh = steps[0]["q"][b, h * dh:(h + 1) * dh].astype(np.float64)
                peak = (qh * (215.0 * np.sqrt(dh) / (s[b, h] * (qh @ qh)))).astype(np.float32)
                if t == L[b]:
                    steps[0]["k"][b, h * dh:(h + 1) * dh] = peak
                else:
                    K[b, h, t] = peak
    for b in range(B):                                  # NaN wherever nothing may be read
        K[b, :, max(int(L[b]), 0):] = np.nan
        V[b, :, max(int(L[b]), 0):] = np.nan
    # the rule, stepped STEPS times on its own copy of the caches
    rK, rV, rL, want = K.copy(), V.copy(), L.copy(), []
    for st in steps:
        want.append(R.step64(st["q"], st["k"], st["v"], rK, rV, rL, x=st["x"], with_bound=True, **gates))
        rL = want[-1]["lengths"]
        if len(want) == 1:
            K1, V1 = rK.copy(), rV.copy()
    out = dict(B=B, H=H, dh=dh, D=D, cap=cap, L=L, act=act, steps=steps, K=K, V=V, gates=gates, want=want, K1=K1,
               V1=V1)
    for a in (K, V, K1, V1, L, act):
        a.setflags(write=False)
    return out


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _call(ops, c, step, dev, K, V, L, rows=None, n_chunks=None, scale=False):
    """One op call on fresh device copies of the caches (rows: a sub-batch).  Returns ctx, scale, K, V, lengths."""
    sel = slice(None) if rows is None else rows
    g = c["gates"]
    t = {k: _dev(step[k][sel], dev) for k in ("q", "k", "v", "x")}
    prosody = None if g["prosody"] is None else _dev(g["prosody"][sel], dev)
    Kd, Vd, Ld = _dev(K[sel], dev), _dev(V[sel], dev), _dev(L[sel], dev)
    B, H, cap, dh = Kd.shape
    nc = ops.attn_decode_chunks(cap) if n_chunks is None else n_chunks
    ws = torch.full((ops.attn_decode_workspace_floats(B, H, dh, nc),), float("nan"), device=dev)
    keep = {k: v.clone() for k, v in t.items()}
    out = ops.attn_decode_step(t["q"], t["k"], t["v"], t["x"], prosody, _dev(g["Wp"], dev), _dev(g["bp"], dev),
                               _dev(g["wm"], dev), _dev(g["bm"], dev), Ld, Kd, Vd, ws, n_chunks=nc, advance=True,
                               return_scale=scale)
    for k, v in keep.items():
        assert torch.equal(_bits(t[k]), _bits(v)), f"input {k} was written"
    ctx, s = out if scale else (out, None)
    return ctx, s, Kd, Vd, Ld


@functools.lru_cache(maxsize=None)
def _run(case, dev):
    """The first step of one case on the device, once: shared by the tests that compare with it."""
    from aura_snn_rag_amd import ops
    c = _case(case)
    ctx, s, K, V, L = _call(ops, c, c["steps"][0], dev, c["K"], c["V"], c["L"], scale=True)
    torch.cuda.synchronize()
    return dict(ctx=ctx, scale=s, K=K, V=V, L=L)


WORST = {}                                              # one profile entry per shape and quantity, over the six kinds


def _record(case, what, ok, n, frac):
    (B, H, dh, cap, _), kind = case
    key = f"decode B{B}-H{H}-dh{dh}-cap{cap} {what}"
    w = WORST.setdefault(key, dict(ok=0, n=0, frac=-1.0, kind=None))
    w["ok"], w["n"] = w["ok"] + int(ok), w["n"] + int(n)
    if frac > w["frac"]:
        w["frac"], w["kind"] = float(frac), kind
    helpers.record_parity(key, w["ok"], w["n"], max_frac_of_bound=round(w["frac"], 4),
                          over_half_bound=bool(w["frac"] > 0.5), worst_kind=w["kind"])


def _within(case, what, got, want, bound):
    """Record and assert ``|got - want| <= bound`` elementwise; returns the largest fraction of the bound."""
    name = f"{_id(case)} {what}"
    got = np.asarray(got, np.float64)
    want, bound = np.broadcast_arrays(np.asarray(want, np.float64), np.asarray(bound, np.float64))
    assert got.shape == want.shape, f"{name}: shape {got.shape} against {want.shape}"
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), f"{name}: not finite"
    err = np.abs(got - want)
    ok = err <= bound
    frac = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"decode {name}: at {frac:.4f} of its bound")
    _record(case, what, ok.sum(), err.size, frac)
    assert bool(ok.all()), f"{name}: max fraction of the bound {frac}"
    return frac


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_caches_and_lengths(dev, case):
    c, r = _case(case), _run(case, dev)
    B, H, dh, L, act = c["B"], c["H"], c["dh"], c["L"], c["act"]
    K, V = _bits(r["K"]).numpy(), _bits(r["V"]).numpy()
    K0, V0 = c["K"].view(np.int32), c["V"].view(np.int32)
    st = c["steps"][0]
    for b in range(B):
        keep = np.ones(c["cap"], bool)
        if act[b]:
            keep[L[b]] = False
            assert np.array_equal(K[b, :, L[b]], st["k"][b].reshape(H, dh).view(np.int32)), f"row {b}: appended K"
            assert np.array_equal(V[b, :, L[b]], st["v"][b].reshape(H, dh).view(np.int32)), f"row {b}: appended V"
        assert np.array_equal(K[b][:, keep], K0[b][:, keep]), f"row {b}: K written away from position L"
        assert np.array_equal(V[b][:, keep], V0[b][:, keep]), f"row {b}: V written away from position L"
    assert np.array_equal(_np(r["L"]), np.where(act, L + 1, L)), "lengths advance by one on active rows only"
    assert np.array_equal(_np(r["L"]), c["want"][0]["lengths"])
    assert bool((_np(r["ctx"])[~act] == 0).all()) and bool((_np(r["scale"])[~act] == 0).all()), "inactive rows are 0"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ctx_and_scale_within_the_bounds(dev, case):
    c, r = _case(case), _run(case, dev)
    w = c["want"][0]
    _within(case, "scale", _np(r["scale"]), w["scale"], w["scale_bound"])
    _within(case, "ctx", _np(r["ctx"]), w["ctx"], w["bound"])
    if case[1] == "flat":                                # equal keys: the mean of the values
        for b in np.nonzero(c["act"])[0]:
            mean = c["V1"][b, :, :c["L"][b] + 1].astype(np.float64).mean(axis=1)
            assert np.max(np.abs(_np(r["ctx"])[b].reshape(c["H"], c["dh"]) - mean)) <= 2e-5


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_do_not_depend_on_batch_capacity_chunks_or_the_call(dev, case):
    from aura_snn_rag_amd import ops
    c, r = _case(case), _run(case, dev)
    B, cap, L, act, st = c["B"], c["cap"], c["L"], c["act"], c["steps"][0]
    want = _bits(r["ctx"])
    again = _call(ops, c, st, dev, c["K"], c["V"], L)
    assert torch.equal(_bits(again[0]), want), "two calls differ"
    assert torch.equal(_bits(again[2]), _bits(r["K"])) and torch.equal(_bits(again[3]), _bits(r["V"]))
    if act.any():
        minimal = int(L[act].max()) // R.CHUNK + 1
        few = _call(ops, c, st, dev, c["K"], c["V"], L, n_chunks=minimal)
        assert torch.equal(_bits(few[0]), want), f"n_chunks={minimal} differs from the default"
    # twice the capacity (NaN beyond): rows that were full at cap are retired there, the others must not move a bit
    K2, V2 = (np.concatenate([a, np.full_like(a, np.nan)], axis=2) for a in (c["K"], c["V"]))
    wide = _call(ops, c, st, dev, K2, V2, np.where(act, L, -1).astype(np.int32))
    assert torch.equal(_bits(wide[0]), want), "cap and 2 cap differ"
    for b in range(B):
        alone = _call(ops, c, st, dev, c["K"], c["V"], L, rows=slice(b, b + 1))
        assert torch.equal(_bits(alone[0])[0], want[b]), f"row {b} alone differs from the batch"
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_three_steps_follow_the_rule(dev, case):
    from aura_snn_rag_amd import ops
    c = _case(case)
    g = c["gates"]
    K, V, L = _dev(c["K"], dev), _dev(c["V"], dev), _dev(c["L"], dev)
    nc = ops.attn_decode_chunks(c["cap"])
    ws = torch.empty(ops.attn_decode_workspace_floats(c["B"], c["H"], c["dh"], nc), device=dev)
    gates = [None if g[k] is None else _dev(g[k], dev) for k in ("prosody", "Wp", "bp", "wm", "bm")]
    worst = 0.0
    for n, (st, w) in enumerate(zip(c["steps"], c["want"])):
        ctx = ops.attn_decode_step(_dev(st["q"], dev), _dev(st["k"], dev), _dev(st["v"], dev), _dev(st["x"], dev),
                                   *gates, L, K, V, ws, n_chunks=nc)
        got = _np(ctx)
        assert np.all(np.isfinite(got)), f"step {n}: not finite"
        err = np.abs(got - w["ctx"])
        assert bool((err <= w["bound"]).all()), f"step {n}: {float(np.max(err / np.maximum(w['bound'], 1e-300)))}"
        worst = max(worst, float(np.max(err / np.maximum(w["bound"], 1e-300))))
        assert np.array_equal(_np(L), w["lengths"]), f"step {n}: lengths"
    _record(case, "ctx over three steps", STEPS, STEPS, worst)


# ------------------------------------------------------------------------------------------------------- the modules
def _config(D, H):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D)


@pytest.mark.parametrize("D,H", [(96, 2), (768, 12)])
@pytest.mark.parametrize("which", ["attention", "layer"])
def test_prefill_and_steps_equal_forward(dev, D, H, which):
    from aura_snn_rag_amd import HippocampalProsodyAttention, HippocampalTransformerLayer
    torch.manual_seed(D + len(which))
    cls = HippocampalProsodyAttention if which == "attention" else HippocampalTransformerLayer
    mod = cls(_config(D, H), hippocampus=object()).to(dev).eval()
    B, S, P = 3, 13, 7
    hidden, prosody = torch.randn(B, S, D, device=dev), 1.5 * torch.randn(B, S, 4, device=dev)
    with torch.no_grad():
        full = mod(hidden, prosody=prosody)
        full = full[0] if which == "attention" else full
        ref64 = mod.double()(hidden.double(), prosody=prosody.double())
        ref64 = ref64[0] if which == "attention" else ref64
        mod.float()
        cache = mod.new_cache(B, 16)
        pre = mod.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=cache)
        pre = pre[0] if which == "attention" else pre
        rows = [pre] + [mod.step(hidden[:, t], prosody=prosody[:, t], cache=cache)[:, None] for t in range(P, S)]
    stepped = torch.cat(rows, dim=1)
    assert torch.equal(cache.lengths.cpu(), torch.full((B,), S, dtype=torch.int32)) and cache.max_length == S
    comp = float((full.double() - ref64).abs().max())           # the torch composition's own error
    err = float((stepped.double() - ref64).abs().max())
    ratio = err / max(comp, 1e-300)
    print(f"decode module {which} D={D}: stepped {err:.3e}, composition {comp:.3e}, ratio {ratio:.3f}")
    helpers.record_parity(f"decode module {which} D{D}", int(err <= 8 * comp), 1, error=err, composition_error=comp,
                          ratio_to_composition=round(ratio, 4))
    assert comp > 0 and err <= 8.0 * comp, (err, comp)
