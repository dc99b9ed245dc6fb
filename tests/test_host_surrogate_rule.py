"""tests/surrogate_rule.py anchored in the oracle before any kernel is judged by it, on exactly the tensors that
tests/test_gpu_surrogate.py feeds the kernels (tests/surrogate_cases.py):

* the rule's forward is bit-equal to ``O.gif_run_grad`` / ``O.prosody_gif_run_grad`` / ``O.lif_step_grad``;
* the oracle's autograd lies within the derived bound of the fp64 rule for every output of every case (fp32 with
  u = 2^-24; the bf16 graph rounds every node to bf16: the same K with u = 2^-8);
* on the hand-made decision points the rule equals the oracle's autograd bit for bit, and each case holds the
  points it claims;
* the random cases keep their distance from the surrogate window's two discontinuities."""
import pytest
import torch

from oracle import aura_oracle as O
from tests import surrogate_cases as C
from tests import surrogate_rule as R

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def _oracle_gif(kind, t, decay, L, alpha, thr0, strength):
    names = ["h", "v0", "t0"] + (["gains"] if t["gains"] is not None else [])
    leaves = {k: t[k].clone().requires_grad_(True) for k in names}
    if kind == "gif":
        s, v, th = O.gif_run_grad(leaves["h"], leaves["v0"], leaves["t0"], decay, L, alpha, thr0)
    else:
        s, v, th = O.prosody_gif_run_grad(leaves["h"], leaves["v0"], leaves["t0"], leaves.get("gains"), decay, L,
                                          alpha, thr0, strength)
    loss = (s * t["ws"]).sum() + (v * t["wv"]).sum() + (th * t["wt"]).sum()
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    out = dict(zip(("g_h", "g_v0", "g_theta0", "g_gains"), grads))
    return (s.detach(), v.detach(), th.detach()), out


def _within(got, rule, u, what):
    """max of err / bound over every element; asserts none above 1."""
    want, M, K = rule
    err = (got.to(F64) - want).abs()
    bnd = R.bound(K, M, u=u)
    ratio = torch.where(err > 0, err / bnd, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, f"{what}: err / bound = {worst:.3f} (max err {float(err.max()):.3e})"
    return worst


@pytest.mark.parametrize("c", C.SMALL_CASES + C.BIG_CASES, ids=C.case_id)
def test_gif_rule_against_the_oracle(c):
    t, fwd, bwd = C.gif_case(c)
    assert not bool(C.near_discontinuity(fwd["n"], c.L).any()), "a current within 1e-4 of a discontinuity"
    (s, v, th), grads = _oracle_gif(c.kind, t, C.DECAY, c.L, c.alpha, C.THR0, C.STRENGTH)
    assert s.dtype == c.dtype
    assert torch.equal(fwd["spikes"], s) and torch.equal(fwd["v"], v) and torch.equal(fwd["theta"], th)
    assert (s == 0).any() and (s == c.L).any(), "both spike extremes"
    u = R.U24 if c.dtype == F32 else R.U8
    worst = {k: _within(g, bwd[k], u, f"{c.name} {k}") for k, g in grads.items() if g is not None}
    assert (bwd["g_gains"] is not None) == (c.kind == "prosody" and c.gains)
    assert set(worst) == {k for k, v_ in bwd.items() if v_ is not None}
    print(f"\n[oracle vs rule {c.name}] " + " ".join(f"{k} {w:.3f}" for k, w in worst.items()))


def test_small_cases_bind_the_clamp_and_both_scale_sides():
    """Somewhere among the small cases of each kind and dtype the +-2 L te clamp binds on both sides, and with
    gains the scale clamp is live in some steps and dead in others."""
    seen = {}
    for c in C.SMALL_CASES:
        t, fwd, _ = C.gif_case(c)
        a, th = fwd["save_a"].float(), fwd["save_theta"].float()
        key = (c.kind, c.gains, c.dtype)
        lo = hi = 0
        if not c.gains:                                    # te = theta: the clamp bound is L theta 2
            cl = (c.L * th) * 2.0 if c.dtype == F32 else R.rb(R.rb(c.L * th) * 2.0)
            lo, hi = int((a < -cl).sum()), int((a > cl).sum())
        else:
            raw = 1.0 - C.STRENGTH * (t["gains"].float() - 1.0)
            seen.setdefault(key + ("live",), 0)
            seen.setdefault(key + ("dead",), 0)
            seen[key + ("live",)] += int(((raw > 0.5) & (raw < 1.5)).sum())
            seen[key + ("dead",)] += int(((raw < 0.5) | (raw > 1.5)).sum())
        seen[key + ("lo",)] = seen.get(key + ("lo",), 0) + lo
        seen[key + ("hi",)] = seen.get(key + ("hi",), 0) + hi
    for key, n in seen.items():
        if key[1] and key[3] in ("lo", "hi"):
            continue
        assert n > 0, key


# ---- decision points -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,gains", [("gif", False), ("prosody", False), ("prosody", True)])
def test_decision_points_bit_equal(kind, gains):
    t, fwd, bwd = C.decision_rule(kind, gains)
    decay, L, alpha, thr0, strength = C.decision_case(kind, gains)[1]
    rows = t["h"].shape[0]
    exact = C.DP_EXACT_ROWS if gains else [0]
    # each case holds the points it claims (on the rows whose scale is a short dyadic number)
    a, n, th = fwd["save_a"][:, 0], fwd["n"][:, 0], fwd["save_theta"][:, 0]
    if kind == "gif":
        assert torch.equal(th + 1e-6, torch.ones_like(th)), "d = theta + 1e-6 must be 1 exactly"
        te = th
    else:
        g = t["gains"] if gains else torch.ones(rows, 1)
        raw = 1.0 - strength * (g - 1.0)
        te = th * torch.clamp(raw, 0.5, 1.5)
        if gains:
            assert [float(x) for x in raw[:, 0]] == [1.0, 0.5, 0.5 - 2.0 ** -23, 0.5 + 2.0 ** -24, 1.5,
                                                      1.5 + 2.0 ** -23, 1.5 - 2.0 ** -23]
    cl = (L * te) * 2.0
    for r in exact:
        count = lambda m: int(m[r].sum())
        assert count(a == cl) == 1 and count(a > cl) == 1 and count(a == -cl) == 1 and count(a < -cl) == 1
        assert count(n == 3.0) == 1 and count(n == 2.5) == 1 and count(n == L + 1.0) == 1
        assert count(n == 0.0) == 2 and count((n == 0.0) & torch.signbit(n)) == (0 if gains else 1)
        assert count((n > L + 1.0) & (n < L + 1.0 + 1e-5)) == 1
    (s, v, thT), grads = _oracle_gif(kind, t, decay, L, alpha, thr0, strength)
    assert torch.equal(fwd["spikes"], s) and torch.equal(fwd["v"], v) and torch.equal(fwd["theta"], thT)
    for k, got in grads.items():
        if got is None:
            continue
        want, M, K = bwd[k]
        assert float(M.sum()) > 0
        assert torch.equal(want.float()[exact], got[exact]), \
            f"{k}: rule and autograd differ on the exact rows:\n{want.float()[exact]}\n{got[exact]}"
        _within(got, bwd[k], R.U24, f"{kind} {k}")            # the rows with an inexact scale: the bound
    # the gradient goes to the input at equality with the clamp bound and to theta just beyond it
    gh = bwd["g_h"][0][:, 0]
    for r in exact:
        assert float(gh[r, 1]) == 0.0 and float(gh[r, 3]) == 0.0
        if not (gains and float(t["gains"][r, 0]) == 0.0):
            assert float(gh[r, 0]) != 0.0 and float(gh[r, 2]) != 0.0


# ---- LIF -------------------------------------------------------------------------------------------------------

def _oracle_lif(t):
    x, mem, slope = (t[k].clone().requires_grad_(True) for k in ("x", "mem", "slope"))
    spk, mem_out = O.lif_step_grad(x, mem, t["beta"], t["thr"], slope)
    grads = torch.autograd.grad((spk * t["g_spk"]).sum() + (mem_out * t["g_mem"]).sum(), [x, mem, slope])
    return spk.detach(), mem_out.detach(), dict(zip(("g_x", "g_mem_prev", "slope_sum"), grads))


@pytest.mark.parametrize("case", C.LIF_CASES + C.LIF_BIG_CASES, ids=C.case_id)
def test_lif_rule_against_the_oracle(case):
    t, fwd, bwd = C.lif_case(*case)
    spk, mem_out, grads = _oracle_lif(t)
    assert torch.equal(fwd["spikes"], spk) and torch.equal(fwd["mem"], mem_out)
    assert spk.numel() < 50 or 0.05 < float(spk.float().mean()) < 0.95
    u = R.U24 if case[0] == F32 else R.U8
    for k, g in grads.items():
        _within(g, bwd[k], u, f"lif {k}")


def test_lif_decision_points_bit_equal():
    t, fwd, bwd = C.lif_decision_case()
    pre = fwd["pre"]
    assert int((pre == 0).sum()) == 2 * 4 and int((pre > 0).sum()) == 2 * 2 and int((pre < 0).sum()) == 2 * 2
    assert 0 < float(pre[0, 1]) < 1e-6 and -1e-6 < float(pre[0, 2]) < 0
    spk, mem_out, grads = _oracle_lif(t)
    assert torch.equal(fwd["spikes"], spk) and torch.equal(fwd["mem"], mem_out)
    assert torch.equal(bwd["raw_slope"][0][pre == 0], torch.zeros(8, dtype=F64))
    exact = pre.abs() != 1.0                          # at |pre| = 1 the denominator 25 makes the quotient inexact
    for k, got in grads.items():
        want = bwd[k][0].float()
        if k == "slope_sum":
            _within(got, bwd[k], R.U24, k)
            assert torch.equal(want[exact[0]], got[exact[0]])
        else:
            assert torch.equal(want[exact], got[exact]), k
            _within(got, bwd[k], R.U24, k)


# ---- AdditionLinear ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,IN,OUT", C.ADDLIN_SHAPES)
def test_addition_linear_rule_against_the_oracle(B, IN, OUT):
    x, w, g = C.addition_linear_case(B, IN, OUT)
    ties = x.unsqueeze(1) == w.unsqueeze(0)
    assert int(ties.sum()) >= OUT and bool(ties[0, :, 0].all())
    assert not torch.signbit(x[0, 0]) and bool(torch.signbit(w[:, 0]).all()), "+0 against -0"
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    gx, gw = torch.autograd.grad((O.addition_linear(xo, wo) * g).sum(), [xo, wo])
    rule = R.addition_linear_backward(x, w, g)
    for got, (want, bnd) in ((gx, rule["g_x"]), (gw, rule["g_w"])):
        assert bool(((got.double() - want).abs() <= bnd).all())
    # a tie contributes nothing: the tied column of row 0 has a zero input gradient
    assert float(rule["g_x"][0][0, 0]) == 0.0
