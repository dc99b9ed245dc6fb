"""``ops.attn_decode_extend(.., counts=)`` on the GPU (csrc/aura_decode.hip) against ``counts[b]`` calls of
``ops.attn_decode_step`` per row on clones of the same caches: the rule of ``include/aura_hip.h`` ("Decode attention:
extend with per-row counts") is the step's rule per query, so the comparison is for bits, on integer views, no element
left out.  The step is not under test here: tests/test_gpu_decode_attention.py holds it to fp64.

Poisoned with NaN before every call: every cache position at or past a row's length, and every row ``j >= counts[b]``
of ``q``, ``k_new``, ``v_new``, ``x`` and ``prosody``.  Anything read that may not be read shows in ``ctx``, the scales
or the caches.

Shapes ``(H, dh, m, lengths, counts)``: the smallest (m = 1 with a count of 1 and of 0); a chunk edge crossed in one
row only (250 + 9); counts of one group of 8 queries, one more than a group and all four groups; dh = 4, 32, 48, 64,
128 (every lane-group width); a count of 0 next to full rows; and the policy row: a retired row, a row whose padded
``m`` does not fit but whose own count does (active), a row one position short of fitting its count (inactive), and the
counts -1 and m + 1 (inactive)."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

CHUNK = 256
POLICY_CAP = 300
# (H, dh, m, lengths, counts, cap or None: the largest length + m + 3)
SHAPES = [
    (1, 4, 1, (0,), (1,), None),
    (1, 4, 1, (0,), (0,), None),
    (3, 32, 9, (250, 3, 4), (9, 1, 0), None),
    (3, 32, 32, (254, 5, 62), (8, 9, 32), None),
    (1, 64, 17, (255, 256, 1000), (2, 17, 16), None),
    (3, 48, 32, (250, 0), (7, 25), None),
    (1, 128, 32, (63, 1), (31, 1), None),
    # retired; 295 + 9 > cap but 295 + 3 <= cap: active; 296 + 5 = cap + 1: inactive; counts -1 and m + 1: inactive
    (3, 32, 9, (-1, POLICY_CAP - 5, POLICY_CAP - 4, 10, 10), (5, 3, 5, -1, 10), POLICY_CAP),
]
POLICY = len(SHAPES) - 1
KINDS = ["random", "no_prosody", "no_memory"]
CASES = [(i, k) for i in range(len(SHAPES)) for k in (KINDS if i == 3 else KINDS[:1])]


def _id(case):
    i, kind = case
    H, dh, m, lengths, counts, _ = SHAPES[i]
    return f"H{H}-dh{dh}-m{m}-L{'_'.join(map(str, lengths))}-c{'_'.join(map(str, counts))}-{kind}"


def _active(L, n, m, cap):
    return (L >= 0) & (n >= 0) & (n <= m) & (L + n <= cap)


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs of one case, computed once and never modified.  ``clean`` holds the new rows without the poison."""
    i, kind = case
    H, dh, m, lengths, counts, cap = SHAPES[i]
    rng = np.random.default_rng(5000 + 7 * i + KINDS.index(kind))
    B, D = len(lengths), H * dh
    cap = max(lengths) + m + 3 if cap is None else cap
    L, n = np.array(lengths, np.int32), np.array(counts, np.int32)
    act = _active(L, n, m, cap)
    draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    clean = dict(q=draw(B, m, D), k=draw(B, m, D), v=draw(B, m, D), x=draw(B, m, D),
                 prosody=(1.5 * rng.standard_normal((B, m, 4))).astype(np.float32))
    K, V = draw(B, H, cap, dh), draw(B, H, cap, dh)
    Wp, bp = draw(H, 4), draw(H)
    wm, bm = (rng.standard_normal((1, D)) / np.sqrt(D)).astype(np.float32), draw(1)
    if kind == "no_memory":
        wm = bm = None
    for b in range(B):                                   # NaN wherever nothing may be read
        K[b, :, max(int(L[b]), 0):] = np.nan
        V[b, :, max(int(L[b]), 0):] = np.nan
    out = dict(B=B, H=H, dh=dh, D=D, m=m, cap=cap, L=L, n=n, act=act, K=K, V=V, clean=clean,
               no_prosody=kind == "no_prosody", gates=dict(Wp=Wp, bp=bp, wm=wm, bm=bm))
    out.update(_poisoned(clean, n))
    for a in (K, V, L, n, act, *clean.values(), *(out[k] for k in ("q", "k", "v", "x", "prosody"))):
        a.setflags(write=False)
    return out


def _poisoned(clean, n):
    """The new rows with NaN in every row ``j >= n[b]``."""
    out = {k: a.copy() for k, a in clean.items()}
    for a in out.values():
        for b in range(len(n)):
            a[b, max(int(n[b]), 0):] = np.nan
    return out


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _extend(ops, c, dev, K, V, L, counts, rows=None, n_chunks=None, advance=True, new=None):
    """One extend on fresh device copies (rows: a sub-batch; counts ``None``: the call without counts; new: other new
    rows than the case's poisoned ones).  Returns ctx, scale, K, V, lengths."""
    sel = slice(None) if rows is None else rows
    new = c if new is None else new
    t = {k: _dev(new[k][sel], dev) for k in ("q", "k", "v", "x")}
    prosody = None if c["no_prosody"] else _dev(new["prosody"][sel], dev)
    g = {k: _dev(a, dev) for k, a in c["gates"].items()}
    Kd, Vd, Ld = _dev(K[sel], dev), _dev(V[sel], dev), _dev(L[sel], dev)
    nd = None if counts is None else _dev(np.asarray(counts, np.int32)[sel], dev)
    B, H, cap, dh = Kd.shape
    nc = ops.attn_decode_chunks(cap) if n_chunks is None else n_chunks
    ws = torch.full((ops.attn_decode_extend_workspace_floats(B, c["m"], H, dh, nc),), float("nan"), device=dev)
    keep = {k: a.clone() for k, a in t.items()}
    kw = {} if nd is None else dict(counts=nd)
    ctx, s = ops.attn_decode_extend(t["q"], t["k"], t["v"], t["x"], prosody, g["Wp"], g["bp"], g["wm"], g["bm"], Ld, Kd,
                                    Vd, ws, n_chunks=nc, advance=advance, return_scale=True, **kw)
    for k, a in keep.items():
        assert torch.equal(_bits(t[k]), _bits(a)), f"input {k} was written"
    if nd is not None:
        assert nd.tolist() == np.asarray(counts, np.int32)[sel].tolist(), "counts were written"
    return ctx, s, Kd, Vd, Ld


def _steps(ops, c, dev):
    """The reference: per row ``n[b]`` calls of the step on fresh device copies of the same caches.  In step ``j`` the
    rows that have no token ``j`` (and the inactive ones) are retired, so the step reads none of their poisoned rows
    and returns the zeros the rule asks for."""
    t = {k: _dev(c[k], dev) for k in ("q", "k", "v", "x")}
    prosody = None if c["no_prosody"] else _dev(c["prosody"], dev)
    g = {k: _dev(a, dev) for k, a in c["gates"].items()}
    Kd, Vd = _dev(c["K"], dev), _dev(c["V"], dev)
    B, H, cap, dh = Kd.shape
    nc = ops.attn_decode_chunks(cap)
    ws = torch.empty(ops.attn_decode_workspace_floats(B, H, dh, nc), device=dev)
    ctx, scale = [], []
    for j in range(c["m"]):
        Ld = _dev(np.where(c["act"] & (j < c["n"]), c["L"] + j, -1).astype(np.int32), dev)
        o, s = ops.attn_decode_step(t["q"][:, j].contiguous(), t["k"][:, j].contiguous(), t["v"][:, j].contiguous(),
                                    t["x"][:, j].contiguous(), None if prosody is None else prosody[:, j].contiguous(),
                                    g["Wp"], g["bp"], g["wm"], g["bm"], Ld, Kd, Vd, ws, n_chunks=nc, return_scale=True)
        ctx.append(o)
        scale.append(s)
    Ln = _dev(np.where(c["act"], c["L"] + c["n"], c["L"]).astype(np.int32), dev)
    return torch.stack(ctx, dim=1), torch.stack(scale, dim=1), Kd, Vd, Ln


@functools.lru_cache(maxsize=None)
def _run(case, dev):
    """One ragged extend and the steps of one case on the device, once: shared by the tests that compare with them."""
    from aura_snn_rag_amd import ops
    c = _case(case)
    got = _extend(ops, c, dev, c["K"], c["V"], c["L"], c["n"])
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
    helpers.record_parity("ragged extend: bits against counts[b] steps per row", COUNTS["elements"] - COUNTS["mismatches"],
                          COUNTS["elements"], cases=COUNTS["cases"], mismatches=COUNTS["mismatches"])
    assert bad == 0, f"{name}: {bad} of {g.numel()} elements differ from the steps"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_ragged_extend_leaves_the_bits_of_each_rows_own_steps(dev, case):
    c = _case(case)
    got, want = _run(case, dev)
    COUNTS["cases"] += 1
    for name, g, w in zip(("ctx", "scale", "K", "V", "lengths"), got, want):
        _same(f"{_id(case)} {name}", g, w)
    ctx, scale, _, _, Ln = (t.cpu() for t in got)
    assert np.array_equal(Ln.numpy(), np.where(c["act"], c["L"] + c["n"], c["L"])), "lengths advance by the row's count"
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(scale).all()), "a poisoned place was read"
    for b in range(c["B"]):
        first_pad = int(c["n"][b]) if c["act"][b] else 0
        assert bool((ctx[b, first_pad:] == 0).all()) and bool((scale[b, first_pad:] == 0).all()), \
            f"row {b}: ctx and scale are 0 from query {first_pad} on"
        assert bool((scale[b, :first_pad] > 0).all()), f"row {b}: an active query has a scale"


def test_the_policy_row_is_active_by_its_own_count(dev):
    c = _case((POLICY, "random"))
    assert c["act"].tolist() == [False, True, False, False, False]
    assert c["L"][1] + c["m"] > c["cap"] >= c["L"][1] + c["n"][1] and c["L"][2] + c["n"][2] == c["cap"] + 1
    (ctx, _, _, _, Ln), _ = _run((POLICY, "random"), dev)
    assert Ln.tolist() == [-1, POLICY_CAP - 2, POLICY_CAP - 4, 10, 10]
    assert bool((ctx[1, :3] != 0).any()) and bool((ctx.cpu()[[0, 2, 3, 4]] == 0).all())


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_caches_change_at_a_rows_own_new_positions_only(dev, case):
    c = _case(case)
    (_, _, K, V, _), _ = _run(case, dev)
    H, dh, m, L, n, act = c["H"], c["dh"], c["m"], c["L"], c["n"], c["act"]
    K, V = _bits(K).numpy(), _bits(V).numpy()
    K0, V0 = c["K"].view(np.int32), c["V"].view(np.int32)
    for b in range(c["B"]):
        keep = np.ones(c["cap"], bool)
        if act[b]:
            keep[L[b]:L[b] + n[b]] = False
            new_k = c["k"][b, :n[b]].reshape(n[b], H, dh).transpose(1, 0, 2).view(np.int32)
            new_v = c["v"][b, :n[b]].reshape(n[b], H, dh).transpose(1, 0, 2).view(np.int32)
            assert np.array_equal(K[b, :, L[b]:L[b] + n[b]], new_k), f"row {b}: appended K"
            assert np.array_equal(V[b, :, L[b]:L[b] + n[b]], new_v), f"row {b}: appended V"
        assert np.array_equal(K[b][:, keep], K0[b][:, keep]), f"row {b}: K written away from its new positions"
        assert np.array_equal(V[b][:, keep], V0[b][:, keep]), f"row {b}: V written away from its new positions"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_rows_bits_do_not_depend_on_the_other_rows_or_the_call(dev, case):
    from aura_snn_rag_amd import ops
    c = _case(case)
    (ctx, scale, K, V, _), _ = _run(case, dev)
    B, m, L, n, act, cap = c["B"], c["m"], c["L"], c["n"], c["act"], c["cap"]
    want, want_s = _bits(ctx), _bits(scale)
    again = _extend(ops, c, dev, c["K"], c["V"], L, n)
    assert torch.equal(_bits(again[0]), want) and torch.equal(_bits(again[1]), want_s), "two calls differ"
    assert torch.equal(_bits(again[2]), _bits(K)) and torch.equal(_bits(again[3]), _bits(V))
    still = _extend(ops, c, dev, c["K"], c["V"], L, n, advance=False)
    assert torch.equal(_bits(still[0]), want) and np.array_equal(still[4].cpu().numpy(), L), "advance=False"
    assert torch.equal(_bits(still[2]), _bits(K)), "advance=False appends all the same"
    if act.any():
        minimal = int((L[act] + np.maximum(n[act], 1) - 1).max()) // CHUNK + 1
        few = _extend(ops, c, dev, c["K"], c["V"], L, n, n_chunks=minimal)
        assert torch.equal(_bits(few[0]), want), f"n_chunks={minimal} differs from the default"
        assert torch.equal(_bits(few[2]), _bits(K))
    # twice the capacity (NaN beyond): a row whose count did not fit would fit there, so it is retired
    K2, V2 = (np.concatenate([a, np.full_like(a, np.nan)], axis=2) for a in (c["K"], c["V"]))
    wide = _extend(ops, c, dev, K2, V2, np.where(act, L, -1).astype(np.int32), n)
    assert torch.equal(_bits(wide[0]), want), "cap and 2 cap differ"
    for b in range(B):
        alone = _extend(ops, c, dev, c["K"], c["V"], L, n, rows=slice(b, b + 1))
        assert torch.equal(_bits(alone[0])[0], want[b]), f"row {b} alone differs from the batch"
        assert torch.equal(_bits(alone[2])[0], _bits(K)[b]), f"row {b} alone leaves another cache"
        # the other rows bring other counts (and read their own poison, which is theirs to suffer)
        other = np.where(np.arange(B) == b, n, (n + 1 + np.arange(B)) % (m + 1)).astype(np.int32)
        mixed = _extend(ops, c, dev, c["K"], c["V"], L, other)
        assert torch.equal(_bits(mixed[0])[b], want[b]), f"row {b} differs when the other rows' counts change"
        assert torch.equal(_bits(mixed[2])[b], _bits(K)[b]) and int(mixed[4][b]) == (L[b] + n[b] if act[b] else L[b])
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [k for k in CASES if k[0] != POLICY], ids=_id)
def test_counts_all_equal_to_m_are_the_call_without_counts(dev, case):
    from aura_snn_rag_amd import ops
    c = _case(case)
    full = np.full(c["B"], c["m"], np.int32)
    plain = _extend(ops, c, dev, c["K"], c["V"], c["L"], None, new=c["clean"])
    ragged = _extend(ops, c, dev, c["K"], c["V"], c["L"], full, new=c["clean"])
    torch.cuda.synchronize()
    assert bool((plain[4].cpu() == torch.from_numpy(c["L"] + c["m"])).all()), "every row of these cases fits m"
    for name, g, w in zip(("ctx", "scale", "K", "V", "lengths"), ragged, plain):
        assert torch.equal(_bits(g), _bits(w)), f"{name}: counts == m differs from the call without counts"
