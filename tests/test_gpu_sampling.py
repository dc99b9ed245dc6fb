"""``ops.sample_next`` on the GPU against the rule of ``include/aura_hip.h`` ("Next token"), every decision checked from
the kernel's own inspection outputs (tests/sampling_rule.py restates the rule).

  selection   ``cand_ids`` / ``cand_z`` equal the fp32 rule bit for bit (penalty, temperature and ranking contain no
              transcendental); greedy tokens are exact.
  prefix sums with e64_j = exp(cand_z_j - cand_z_0) in fp64 from the kernel's own candidates and S64 their sum,
              ``|cand_cum_j - sum_{i<=j} e64_i| <= (k' + U_EXP) 2^-23 S64``.  Derivation: expf is within U_EXP = 1 ulp
              (ROCm's device-library (OCML) documentation gives expf 1 ulp; one ulp of a value <= its 2^-23 multiple),
              so term i is off by at most U_EXP 2^-23 e64_i, in all at most U_EXP 2^-23 S64.  In the blocked order c_j
              is reached through at most min(k', 16) additions inside its block, ceil(k' / 16) for the block bases and
              one more, of which those with a zero operand are exact: at most 2 k' inexact ones (none at k' = 1), each
              off by at most 2^-24 of a partial sum <= S64 (1 + o(1)): k' 2^-23 S64 in all.
  kept count  ``n_kept`` is exactly step 6 on the kernel's own ``cand_cum``; against fp64 it lies between the counts
              for top_p (1 - eps) and top_p (1 + eps), eps = b (1 + 1 / top_p) + 2^-24 with b = (k' + U_EXP) 2^-23: the
              kernel tests c_{j-1} <= fl(top_p S) where c_{j-1} and S are within b S64 of fp64 and the product rounds
              once, so c64_{j-1} <= top_p S64 (1 - eps) implies kept and c64_{j-1} > top_p S64 (1 + eps) implies not.
  uniforms    the Philox words are checked through d.  With g64 = -log(-log u) in fp64, u exactly from the NumPy
              Philox, the kernel's g = -logf(-logf(u)) is within t = 2^-23 (4 |g64| + 3) of g64: the bound
              tests/test_gpu_replay.py derives for its keys (3 ulp of logf twice and the roundings).  d = fl(z + g) adds
              one rounding, at most half an ulp of d (replay's keys of order 10 carry it inside t; here |z| reaches 10^4
              at temperature 10^-3), so ``max(0, |(d - z) - g64| - ulp(d) / 2) <= t``; the recorded share is of t.
  token       exactly the argmax of the kernel's own ``cand_d`` over the kept ranks, equal d -> the lower id; with
              ``top_k = 0`` the argmax over the returned [B, V] keys.
  row state   the whole ``seen`` mask gains the drawn token's byte and nothing else; a finished row writes the pad id
              and leaves its mask and its inspection outputs alone; ``finished`` is set exactly where EOS was drawn.
  invariance  a row's outputs are bit-equal alone (with its stream) and in the batch, over two calls, and with the
              logits as a strided view of a wider tensor.  The wrapper has no geometry knob.
The worst used share of each bound goes to the parity record (``profiles/sampling_parity_counts.json``)."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import sampling_rule as R
from tests.cpu_stub_replay import uniforms

pytestmark = pytest.mark.gpu

U_EXP = 1.0                     # expf: 1 ulp (ROCm device libraries, OCML documentation)
SEED, STEP = (1 << 32) + 5, (1 << 33) + 7
PAD = 123456789

# (V, top_k, B, kind, temperature, top_p, penalty, rule, strided)
CASES = [
    (1, 1, 1, "normal", 0.8, 0.9, 1.0, "divide", False), (1, 50, 3, "normal", 5.0, 1.0, 1.2, "divide", False),
    (2, 1, 1, "normal", 0.8, 0.5, 1.2, "signed", False), (2, 2, 3, "equal", 0.8, 0.9, 1.0, "divide", True),
    (63, 50, 3, "normal", 0.8, 0.9, 1.2, "divide", False), (63, 64, 1, "ties", 1e-3, 0.5, 1.2, "signed", True),
    (64, 64, 3, "normal", 0.8, 1.0, 1.0, "divide", False), (64, 65, 33, "special", 0.8, 0.9, 1.2, "divide", False),
    (65, 64, 3, "ties", 5.0, 0.9, 1.2, "signed", True), (65, 65, 1, "equal", 0.8, 0.5, 1.0, "divide", False),
    (65, 1024, 3, "normal", 0.8, 0.0, 1.2, "divide", False),
    (1000, 1, 3, "normal", 0.8, 0.9, 1.2, "divide", False), (1000, 2, 1, "peak", 0.8, 0.9, 1.2, "signed", True),
    (1000, 50, 33, "normal", 0.8, 0.9, 1.2, "divide", True), (1000, 64, 3, "ties", 0.8, 0.5, 1.2, "divide", False),
    (1000, 65, 3, "special", 1e-3, 0.9, 1.2, "signed", False), (1000, 1024, 3, "normal", 5.0, 1.0, 1.0, "divide", False),
    (1000, 1024, 1, "equal", 0.8, 0.9, 1.2, "divide", True),
    (4097, 50, 3, "normal", 0.8, 0.9, 1.2, "divide", False), (4097, 1024, 3, "ties", 0.8, 0.9, 1.2, "signed", True),
    (4097, 1024, 33, "normal", 5.0, 0.5, 1.2, "divide", False), (4097, 65, 1, "special", 0.8, 0.0, 1.2, "divide", False),
    (4097, 2, 3, "peak", 1e-3, 0.9, 1.0, "divide", False),
    (32000, 50, 3, "normal", 0.8, 0.9, 1.2, "divide", False), (32000, 1024, 3, "ties", 0.8, 0.9, 1.2, "divide", True),
    (32000, 64, 33, "special", 5.0, 1.0, 1.2, "signed", False), (32000, 1, 1, "equal", 0.8, 0.9, 1.2, "divide", False),
    (50257, 50, 3, "normal", 0.8, 0.9, 1.2, "divide", True), (50257, 1024, 1, "normal", 1e-3, 0.5, 1.2, "signed", False),
    (50257, 65, 3, "ties", 0.8, 0.9, 1.0, "divide", False), (50257, 2, 33, "peak", 5.0, 0.9, 1.2, "divide", False),
    (131072, 50, 3, "normal", 0.8, 0.9, 1.2, "divide", False), (131072, 1024, 3, "ties", 0.8, 0.9, 1.2, "signed", False),
    (131072, 64, 1, "special", 0.8, 0.5, 1.2, "divide", True), (131072, 1024, 33, "normal", 5.0, 1.0, 1.2, "divide", False),
    (131072, 1, 3, "equal", 0.8, 0.9, 1.0, "divide", False),
    # greedy
    (1, 50, 1, "normal", 0.0, 0.9, 1.2, "divide", False), (65, 50, 3, "ties", 0.0, 0.9, 1.2, "signed", True),
    (1000, 50, 3, "special", 0.0, 0.9, 1.2, "divide", False), (50257, 50, 33, "normal", 0.0, 0.9, 1.2, "signed", False),
    (131072, 50, 3, "equal", 0.0, 0.9, 1.2, "divide", False),
    # the whole vocabulary
    (1, 0, 1, "normal", 0.8, 1.0, 1.2, "divide", False), (65, 0, 3, "ties", 0.8, 1.0, 1.2, "signed", True),
    (4097, 0, 3, "special", 5.0, 2.0, 1.2, "divide", False), (50257, 0, 33, "normal", 0.8, 1.0, 1.2, "divide", False),
]
IDS = [f"V{c[0]}-k{c[1]}-B{c[2]}-{c[3]}-T{c[4]:g}-p{c[5]:g}-{c[7]}{'-view' if c[8] else ''}" for c in CASES]

_INPUTS = {}


def _inputs(V, B, kind):
    """``(logits fp32 [B, V], seen uint8 [B, V])`` on the host, built once per (V, B, kind) and left unchanged."""
    key = (V, B, kind)
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.default_rng(V * 131 + B * 7 + len(kind))
    z = (4 * rng.standard_normal((B, V))).astype(np.float32)
    if kind == "ties":                                      # a handful of values: the k-th is shared by hundreds
        z = np.round(z / 4).astype(np.float32)
    elif kind == "equal":
        z[:] = np.float32(-2.5)
    elif kind == "peak":
        z[np.arange(B), rng.integers(0, V, B)] += np.float32(200.0)
    elif kind == "special":
        for v in (-np.inf, np.nan, np.inf):
            z[rng.random((B, V)) < 0.05] = v
        if B > 1:
            z[0] = np.where(rng.random(V) < 0.5, -np.inf, np.nan)        # an empty row
    if V >= 8 and kind in ("normal", "special"):
        z[:, 1], z[:, 2], z[:, 3] = 0.0, -0.0, 0.0
    seen = (rng.random((B, V)) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 7, 255], dtype=np.uint8), (B, V))
    if V >= 8:
        seen[:, 1:3] = 1                                    # a seen zero of either sign; column 3 an unseen zero
        seen[:, 3] = 0
    _INPUTS[key] = (z, seen)
    return _INPUTS[key]


WORST = {}


def _share(case, what, frac):
    key = f"sampling V{case[0]}-k{case[1]}-B{case[2]} {what}"
    w = WORST.setdefault(key, dict(frac=-1.0, kind=None))
    if frac > w["frac"]:
        w["frac"], w["kind"] = float(frac), case[3]
    helpers.record_parity(key, 1, 1, max_frac_of_bound=round(w["frac"], 4), over_half_bound=bool(w["frac"] > 0.5),
                          worst_kind=w["kind"])


def _draw_error(d, z, g64):
    """``(t, what |(d - z) - g64| leaves after half an ulp of d)`` elementwise (see the module docstring)."""
    t = 2.0 ** -23 * (4 * np.abs(g64) + 3)
    with np.errstate(invalid="ignore", over="ignore"):
        half = 0.5 * np.spacing(np.abs(np.where(np.isfinite(d), d, np.float32(0)))).astype(np.float64)
        err = np.abs((d.astype(np.float64) - z.astype(np.float64)) - g64) - half
    return t, np.maximum(err, 0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _run(ops, dev, z, seen, fin, case, wide=None, streams=None, eos=None):
    """One call on fresh copies of the row state -> (tokens, candidates, seen, finished) on the host."""
    V, k, B, kind, T, top_p, pen, rule, _ = case
    if wide is None:
        lg = torch.from_numpy(z).to(dev)
    else:
        buf = torch.full((z.shape[0], V + 37), 9.0e9, dtype=torch.float32, device=dev)
        buf[:, 3:3 + V] = torch.from_numpy(z).to(dev)
        lg = buf[:, 3:3 + V]
    s = torch.from_numpy(seen).to(dev, copy=True)
    f = torch.from_numpy(fin).to(dev, copy=True)
    out = torch.full((z.shape[0], 3), -7, dtype=torch.int64, device=dev)
    tok, cand = ops.sample_next(lg, seen=s, finished=f, stream_ids=streams, penalty=pen, penalty_rule=rule, temperature=T,
                                top_k=k, top_p=top_p, seed=SEED, step=STEP, eos_id=eos, pad_id=PAD, out=out[:, 1],
                                return_candidates=True)
    assert tok.data_ptr() == out[:, 1].data_ptr()
    o = out.cpu().numpy()
    assert np.all(o[:, 0] == -7) and np.all(o[:, 2] == -7), "the neighbouring columns of out were written"
    return o[:, 1].copy(), {n: v.cpu().numpy() for n, v in cand.items()}, s.cpu().numpy(), f.cpu().numpy()


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    assert np.array_equal(a[0][rows_a], b[0][rows_b])
    assert a[1].keys() == b[1].keys()
    for n in a[1]:
        assert np.array_equal(_bits(a[1][n][rows_a]), _bits(b[1][n][rows_b])), n
    assert np.array_equal(a[2][rows_a], b[2][rows_b]) and np.array_equal(a[3][rows_a], b[3][rows_b])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sample_next_against_the_rule(dev, case):
    from aura_snn_rag_amd import ops
    V, k, B, kind, T, top_p, pen, rule, strided = case
    z, seen = _inputs(V, B, kind)
    fin = np.zeros(B, dtype=np.uint8)
    if B >= 3:
        fin[B - 1] = 1                                      # a row that enters finished
    live = fin == 0
    first = _run(ops, dev, z, seen, fin, case, wide=strided or None)
    tok, cand, seen_after, fin_after = first

    # ---- row state
    want_seen = seen.copy()
    for b in np.nonzero(live & (tok >= 0))[0]:
        want_seen[b, tok[b]] = 1
    assert np.array_equal(seen_after, want_seen), "the mask gains the drawn token's byte and nothing else"
    assert np.all(tok[~live] == PAD) and np.array_equal(fin_after, fin)
    assert np.all((tok[live] >= -1) & (tok[live] < V))

    zp = R.penalise(z, seen, pen, rule)
    streams = np.arange(B)
    if T == 0.0:
        assert cand == {}
        assert np.array_equal(tok[live], R.greedy(zp)[live])
    elif k == 0:
        zt = R.temper(zp, T)
        d = cand["d"]
        assert set(cand) == {"d"} and d.shape == (B, V)
        assert np.all(np.isneginf(d[~live]))
        ok = live[:, None] & (zt > -np.inf)
        assert np.array_equal(d > -np.inf, ok)
        ids = np.broadcast_to(np.arange(V), (B, V))
        g = R.gumbel64(uniforms(R.words(ids, streams, SEED, STEP))[0])
        tol, err = _draw_error(d, zt, g)
        if ok.any():
            frac = float(np.max(err[ok] / tol[ok]))
            print(f"{IDS[CASES.index(case)]}: d at {frac:.4f} of its bound")
            _share(case, "d", frac)
            assert frac <= 1.0
        assert np.array_equal(tok[live], R.argmax_kept(d, ids, ok)[live])
    else:
        kk = min(k, V)
        zt = R.temper(zp, T)
        ids_w, z_w = R.rank(zt, k)
        assert cand["ids"].shape == (B, kk) and cand["n_kept"].shape == (B,)
        # a finished row keeps the fill
        assert np.all(cand["ids"][~live] == -1) and np.all(cand["n_kept"][~live] == 0)
        assert all(np.all(np.isneginf(cand[n][~live])) for n in ("z", "cum", "d"))
        # ---- selection: exact
        assert np.array_equal(cand["ids"][live], ids_w[live])
        assert np.array_equal(_bits(cand["z"][live]), _bits(z_w[live]))
        cz, cc, cd = cand["z"][live], cand["cum"][live], cand["d"][live]
        empty = ~(cz[:, 0] > -np.inf)
        # ---- prefix sums
        c64 = R.cum64(cz)
        S64 = c64[:, -1:]
        b_rel = (kk + U_EXP) * 2.0 ** -23
        assert np.all(cc[empty] == 0)
        if (~empty).any():
            frac = float(np.max(np.abs(cc[~empty] - c64[~empty]) / (b_rel * S64[~empty])))
            print(f"{IDS[CASES.index(case)]}: cum at {frac:.4f} of its bound")
            _share(case, "cum", frac)
            assert frac <= 1.0
        assert np.all(np.diff(cc, axis=1) >= 0)
        # ---- kept count: exactly from the kernel's own sums, and bracketed by fp64
        kept = R.kept_from_cum(cc, top_p) & ~empty[:, None]
        assert np.array_equal(cand["n_kept"][live], kept.sum(axis=1))
        ne = ~empty
        if top_p >= 1.0:
            assert np.all(cand["n_kept"][live][ne] == kk)
        elif top_p == 0.0:
            assert np.all(cand["n_kept"][live][ne] == 1)
        else:
            eps = b_rel * (1.0 + 1.0 / top_p) + 2.0 ** -24
            lo, hi = R.kept_count64(cz[ne], top_p * (1 - eps)), R.kept_count64(cz[ne], top_p * (1 + eps))
            n = cand["n_kept"][live][ne]
            assert np.all((lo <= n) & (n <= hi))
        # ---- uniforms through d
        may_win = kept & (cz > -np.inf)
        assert np.array_equal(cd > -np.inf, may_win)
        g = R.gumbel64(uniforms(R.words(cand["ids"][live], streams[live], SEED, STEP))[0])
        tol, err = _draw_error(cd, cz, g)
        if may_win.any():
            frac = float(np.max(err[may_win] / tol[may_win]))
            print(f"{IDS[CASES.index(case)]}: d at {frac:.4f} of its bound")
            _share(case, "d", frac)
            assert frac <= 1.0
        # ---- the token: exactly the argmax of the kernel's own keys
        assert np.array_equal(tok[live], R.argmax_kept(cd, cand["ids"][live], may_win))
        assert np.all(tok[live][empty] == -1)

    # ---- invariance: two calls (the second with an EOS id), the other layout of the logits, a row alone
    eos = int(tok[0]) if tok[0] >= 0 and live[0] else 0
    second = _run(ops, dev, z, seen, fin, case, wide=strided or None, eos=eos)
    assert np.array_equal(second[3], fin | (live & (second[0] == eos)).astype(np.uint8)), "finished exactly where EOS"
    _same((first[0], first[1], first[2], fin), (second[0], second[1], second[2], fin))
    other = _run(ops, dev, z, seen, fin, case, wide=(not strided) or None)
    _same(first, other)
    r = min(1, B - 1)
    alone = _run(ops, dev, z[r:r + 1], seen[r:r + 1], fin[r:r + 1], case, wide=strided or None, streams=[r])
    _same(first, alone, slice(r, r + 1), slice(0, 1))
    if B > 1:
        dev_streams = torch.arange(B, dtype=torch.int64, device=dev)
        _same(first, _run(ops, dev, z, seen, fin, case, streams=dev_streams))


def test_steps_seeds_and_streams_change_the_draw_and_nothing_else(dev):
    from aura_snn_rag_amd import ops
    z, _ = _inputs(1000, 3, "normal")
    lg = torch.from_numpy(z).to(dev)
    kw = dict(top_k=50, top_p=1.0, temperature=1.0, return_candidates=True)
    base_t, base = ops.sample_next(lg, seed=1, step=0, **kw)
    for other in (dict(seed=2, step=0), dict(seed=1, step=1), dict(seed=1, step=0, stream_ids=[5, 6, 7]),
                  dict(seed=1 + (1 << 32), step=0), dict(seed=1, step=1 << 32)):
        t, c = ops.sample_next(lg, **dict(kw, **other))
        assert torch.equal(c["ids"], base["ids"]) and torch.equal(c["z"], base["z"]) and torch.equal(c["cum"], base["cum"])
        assert not torch.equal(c["d"], base["d"]), other
    # without out, a fresh int64 [B]
    assert base_t.dtype == torch.int64 and base_t.shape == (3,) and base_t.is_contiguous()
