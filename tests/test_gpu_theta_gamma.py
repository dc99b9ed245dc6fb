"""GPU tests of the theta-gamma kernels (``aura_theta_gamma_table``, ``aura_theta_gamma_norm``,
``aura_theta_gamma_norm_backward`` and everything above them) against the rule restated in NumPy
(tests/theta_gamma_rule.py): phases in fp32 as the rule rounds them, the rest in fp64 on those fp32 numbers.

Tolerances (derived from the formats in the rule file's docstring, not from a run):
  pe, d_*  ``|amp| (1.75 E + 9u) + u |value|``, E = 2^-21, u = 2^-24; the committed reference output within the same.
  y        ``|w| (T_D + 8) u (A rstd + 2 |n|) + 2u |y|`` on the fp32 ``h = fl(x + pe_kernel)`` (the table's error is not
           counted twice); mean ``T_D u A``; rstd ``rstd ((T_D / 2 + 4) u + (T_D u A rstd)^2)``.
  g_x      ``rstd [(T_D + 10) u (|wg| + mean|wg| + |n| mean|wg n|) + dn |c2| + |n| mean(|wg| dn)] + 2u |g_x|``.
  sums     ``(T_N + 3) u S`` plus the propagated bounds of the factors (``R.token_sum``).
  Function against torch autograd of the composition on the device, whose phases are the rule's fp32 phases (torch on a
           GPU would multiply by a reciprocal where the rule divides) but whose sines are torch's: both tables are within
           the pe bound of the fp64 one, so the two ``h`` differ by at most ``dh = 2 max(pe bound) + 2u max|h|``, which
           widens ``dn`` by ``rstd (2 + |n|) dh``; with that, twice the bounds above, the token sums with
           ``T = max(T_N, N + 3)`` (torch's order is not ours).
A measured maximum above half its bound is flagged in the recorded profile (``over_half_bound``).

Shapes ``(B, S, D)``: one element, one unit per lane, ragged tails, the float and the float4 path, more than one
workgroup and more than one token per wave in the backward, the limit D = 2048.  Positions: ``start = 0``; a start past
``max_seq_len``; explicit shared positions that repeat, are unsorted and include 1e5; per-item [B, S]."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import helpers
from tests import theta_gamma_rule as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 64), (3, 5, 65), (2, 3, 100), (5, 129, 36), (2, 70, 768), (4, 16, 1024), (2, 3, 2047),
          (1, 2, 2048)]
POSITIONS = ["start0", "start700", "shared", "per_item"]
CASES = [(s, p, "random") for s in SHAPES for p in POSITIONS] + \
        [(s, POSITIONS[i % 4], "offset") for i, s in enumerate(SHAPES)]
MAX_SEQ_LEN, EPS = 512, 1e-5
RATIO = float(R.ratio(8.0, 40.0))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "theta_gamma.pt")


def _id(case):
    (B, S, D), pos, kind = case
    return f"B{B}-S{S}-D{D}-{pos}-{kind}"


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs of one case, computed once and never modified."""
    (B, S, D), pos, kind = case
    rng = np.random.default_rng(sum(map(ord, _id(case))))
    N = B * S
    th, ga = ((0.1 * rng.standard_normal(D)).astype(np.float32) for _ in range(2))
    amp = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    w = (1.0 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    b = (0.3 * rng.standard_normal(D)).astype(np.float32)
    x = rng.standard_normal((N, D)).astype(np.float32)
    if kind == "offset":                                # the row mean 1e3 spreads from zero
        x = (x + 1e3 * np.where(rng.random((N, 1)) < 0.5, -1.0, 1.0)).astype(np.float32)
    g_y = rng.standard_normal((N, D)).astype(np.float32)
    start, positions = 0, None
    if pos == "start700":
        start = 700
    elif pos == "shared":
        positions = rng.integers(0, 600, S).astype(np.float32)
        positions[0] = 1e5
        if S > 2:
            positions[-1] = positions[1]                # a repeat; the draw is unsorted already
    elif pos == "per_item":
        positions = rng.integers(0, 2000, N).astype(np.float32)
    used = positions if positions is not None else np.arange(start, start + S).astype(np.float32)
    out = dict(B=B, S=S, D=D, N=N, th=th, ga=ga, amp=amp, w=w, b=b, x=x, g_y=g_y, start=start, positions=positions,
               used=used, rows=np.arange(N) if pos == "per_item" else np.arange(N) % S,
               table=R.table(used, th, ga, amp, MAX_SEQ_LEN, RATIO))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _run(case, dev):
    """Every op of one case on the device, once: shared by the tests that compare with it."""
    from aura_snn_rag_amd import ops
    c = _case(case)
    t = {k: _dev(c[k], dev) for k in ("th", "ga", "amp", "w", "b", "x", "g_y", "positions")}
    keep = {k: v.clone() for k, v in t.items() if v is not None}
    geo = dict(positions=t["positions"], start=c["start"], rows=None if t["positions"] is not None else c["S"])
    pe, d_th, d_ga, d_amp = ops.theta_gamma_table(t["th"], t["ga"], t["amp"], MAX_SEQ_LEN, RATIO, derivatives=True, **geo)
    y, mean, rstd = ops.theta_gamma_norm(t["x"], pe, t["w"], t["b"], c["S"], EPS)
    g_x, grads = ops.theta_gamma_norm_backward(t["g_y"], t["x"], pe, (d_th, d_ga, d_amp), mean, rstd, t["w"], c["S"])
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(_bits(t[k]), _bits(v)), f"input {k} was written"
    return dict(t, pe=pe, d_theta=d_th, d_gamma=d_ga, d_amp=d_amp, y=y, mean=mean, rstd=rstd, g_x=g_x, grads=grads,
                geo=geo)


def _flag(frac):
    return dict(max_frac_of_bound=round(float(frac), 4), over_half_bound=bool(frac > 0.5))


def _within(name, got, want, bound):
    """Record and assert ``|got - want| <= bound`` elementwise; returns the largest fraction of the bound."""
    got = np.asarray(got, np.float64)
    want, bound = np.broadcast_arrays(np.asarray(want, np.float64), np.asarray(bound, np.float64))
    assert got.shape == want.shape, f"{name}: shape {got.shape} against {want.shape}"
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), f"{name}: not finite"
    err = np.abs(got - want)
    ok = err <= bound
    frac = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"theta {name}: at {frac:.4f} of its bound")
    helpers.record_parity(f"theta {name}", int(ok.sum()), err.size, **_flag(frac))
    assert bool(ok.all()), f"{name}: max fraction of the bound {frac}"
    return frac


TABLE_CASES = [c for c in CASES if c[2] == "random"]


@pytest.mark.parametrize("case", TABLE_CASES, ids=_id)
def test_table_and_derivatives_against_the_rule(dev, case):
    from aura_snn_rag_amd import ops
    c, r = _case(case), _run(case, dev)
    amp = c["amp"][None, :]
    for k in ("pe", "d_theta", "d_gamma", "d_amp"):
        assert r[k].shape == (len(c["used"]), c["D"])
        _within(f"{k} {_id(case)}", _np(r[k]), c["table"][k], R.pe_bound(1.0 if k == "d_amp" else amp, c["table"][k]))
    # the table alone, and without pe, has the same bits
    alone = ops.theta_gamma_table(r["th"], r["ga"], r["amp"], MAX_SEQ_LEN, RATIO, **r["geo"])
    assert torch.equal(_bits(alone), _bits(r["pe"]))
    none, *d = ops.theta_gamma_table(r["th"], r["ga"], r["amp"], MAX_SEQ_LEN, RATIO, derivatives=True, pe=False, **r["geo"])
    assert none is None and all(torch.equal(_bits(a), _bits(r[k])) for a, k in zip(d, ("d_theta", "d_gamma", "d_amp")))
    if c["positions"] is None:                          # start, start + 1, .. formed in the kernel == explicit positions
        explicit = ops.theta_gamma_table(r["th"], r["ga"], r["amp"], MAX_SEQ_LEN, RATIO, positions=_dev(c["used"], dev))
        assert torch.equal(_bits(explicit), _bits(r["pe"]))


def test_table_against_the_golden_reference_output(dev):
    from aura_snn_rag_amd import ops
    g = torch.load(GOLDEN)
    th, ga, amp, pos = (g[k].to(dev) for k in ("theta_phase_offsets", "gamma_phase_offsets", "amplitude_modulation",
                                               "positions"))
    ratio = ops.theta_gamma_ratio(g["theta_frequency"], g["gamma_frequency"])
    pe = ops.theta_gamma_table(th, ga, amp, g["max_seq_len"], ratio, positions=pos)
    a = g["amplitude_modulation"].numpy()
    t = R.table(g["positions"].numpy(), g["theta_phase_offsets"].numpy(), g["gamma_phase_offsets"].numpy(), a,
                g["max_seq_len"], ratio)
    bound = R.pe_bound(a[None, :], t["pe"])
    _within("pe golden vs rule", _np(pe), t["pe"], bound)
    _within("pe golden vs reference output", _np(pe), g["output"].numpy(), bound)


def _forward_rule(c, r):
    h = (c["x"] + _np(r["pe"])[c["rows"]]).astype(np.float32)          # fl(x + pe_kernel)
    return h, R.norm(h, c["w"], c["b"], EPS)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_against_the_rule(dev, case):
    c, r = _case(case), _run(case, dev)
    assert r["y"].shape == (c["N"], c["D"]) and r["mean"].shape == (c["N"],) and r["rstd"].shape == (c["N"],)
    h, f = _forward_rule(c, r)
    _within(f"y {_id(case)}", _np(r["y"]), f["y"], f["y_bound"])
    _within(f"mean {_id(case)}", _np(r["mean"]), f["mean"], f["mean_bound"])
    _within(f"rstd {_id(case)}", _np(r["rstd"]), f["rstd"], f["rstd_bound"])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_token_alone_has_the_bits_it_has_in_the_batch(dev, case):
    from aura_snn_rag_amd import ops
    c, r = _case(case), _run(case, dev)
    again = ops.theta_gamma_norm(r["x"], r["pe"], r["w"], r["b"], c["S"], EPS)
    for a, k in zip(again, ("y", "mean", "rstd")):
        assert torch.equal(_bits(a), _bits(r[k])), "the same call gave other bits"
    for n in sorted({0, c["N"] // 2, c["N"] - 1}):
        row = int(c["rows"][n])
        alone = ops.theta_gamma_norm(r["x"][n:n + 1].contiguous(), r["pe"][row:row + 1].contiguous(), r["w"], r["b"], 1, EPS)
        for a, k in zip(alone, ("y", "mean", "rstd")):
            assert torch.equal(_bits(a), _bits(r[k][n:n + 1])), f"token {n} alone differs from token {n} in the batch"
    if c["positions"] is None and c["B"] > 1:           # one sequence of the batch, the table shared
        one = ops.theta_gamma_norm(r["x"][c["S"]:2 * c["S"]].contiguous(), r["pe"], r["w"], r["b"], c["S"], EPS)
        assert torch.equal(_bits(one[0]), _bits(r["y"][c["S"]:2 * c["S"]]))


def _backward_rule(c, r, dh=0.0, T=None):
    """``{name: (value64, bound)}`` of g_x and the five column sums for the fp32 h the kernels formed."""
    h = (c["x"] + _np(r["pe"])[c["rows"]]).astype(np.float32)
    bw = R.norm_backward(h, c["w"], c["g_y"], EPS, dh)
    T = R.T_N(c["N"]) if T is None else T
    gy = c["g_y"].astype(np.float64)
    amp = c["amp"][None, :]
    out = {"g_x": (bw["g_x"], bw["g_x_bound"]), "g_w": R.token_sum(gy, 0.0, bw["n"], bw["dn"], T),
           "g_b": R.token_sum(gy, 0.0, np.ones_like(gy), 0.0, T)}
    for k, name in (("d_theta", "g_theta"), ("d_gamma", "g_gamma"), ("d_amp", "g_amp")):
        d = c["table"][k]
        db = R.pe_bound(1.0 if k == "d_amp" else amp, d)
        out[name] = R.token_sum(bw["g_x"], bw["g_x_bound"], d[c["rows"]], db[c["rows"]], T)
    return out


GRADS = ("g_w", "g_b", "g_theta", "g_gamma", "g_amp")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_against_the_rule(dev, case):
    from aura_snn_rag_amd import ops
    c, r = _case(case), _run(case, dev)
    assert r["g_x"].shape == (c["N"], c["D"]) and r["grads"].shape == (5, c["D"])
    want = _backward_rule(c, r)
    _within(f"g_x {_id(case)}", _np(r["g_x"]), *want["g_x"])
    for i, k in enumerate(GRADS):
        _within(f"{k} {_id(case)}", _np(r["grads"][i]), *want[k])
    derivs = (r["d_theta"], r["d_gamma"], r["d_amp"])
    g_x, grads = ops.theta_gamma_norm_backward(r["g_y"], r["x"], r["pe"], derivs, r["mean"], r["rstd"], r["w"], c["S"])
    assert torch.equal(_bits(g_x), _bits(r["g_x"])) and torch.equal(_bits(grads), _bits(r["grads"])), \
        "two backward calls differ"
    # fewer outputs, the same bits: without the derivative tables, and g_x alone in one launch
    g_x2, two = ops.theta_gamma_norm_backward(r["g_y"], r["x"], r["pe"], None, r["mean"], r["rstd"], r["w"], c["S"])
    assert two.shape == (2, c["D"]) and torch.equal(_bits(two), _bits(r["grads"][:2])) and torch.equal(_bits(g_x2), _bits(g_x))
    g_x1, none = ops.theta_gamma_norm_backward(r["g_y"], r["x"], r["pe"], None, r["mean"], r["rstd"], r["w"], c["S"],
                                               column_sums=False)
    assert none is None and torch.equal(_bits(g_x1), _bits(g_x))


# ------------------------------------------------------------------------------------- special rows
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-S%d-D%d" % s)
def test_zero_amplitude_and_constant_rows_give_the_bias(dev, shape):
    """amp = 0: pe = +-0 and h = x.  A row of one constant c whose multiples up to D c are fp32 numbers has mean c exactly
    (every partial sum is exact, D c / D is correctly rounded), so n = 0, var = 0, rstd = fl(1 / fl(sqrt(eps)))."""
    from aura_snn_rag_amd import ops
    B, S, D = shape
    c = _case((shape, "start700", "random"))
    th, ga, w, b = (_dev(c[k], dev) for k in ("th", "ga", "w", "b"))
    pe = ops.theta_gamma_table(th, ga, torch.zeros(D, device=dev), MAX_SEQ_LEN, RATIO, start=700, rows=S)
    assert bool((pe == 0).all())
    consts = torch.tensor([1.5, -3.0, 0.25, 96.0, -0.0, 7.0], device=dev)
    x = consts[torch.arange(B * S, device=dev) % 6][:, None].expand(B * S, D).contiguous()
    y, mean, rstd = ops.theta_gamma_norm(x, pe, w, b, S, EPS)
    assert torch.equal(_bits(y), _bits(b[None, :].expand(B * S, D))), "y is not the bias bit for bit"
    assert torch.equal(mean.cpu(), x[:, 0].cpu())
    want = np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(EPS))
    assert np.all(_np(rstd) == want), "rstd is not 1 / sqrt(eps)"


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] * s[1] >= 3], ids=lambda s: "B%d-S%d-D%d" % s)
def test_an_inf_and_a_nan_row_stay_in_their_rows(dev, shape):
    from aura_snn_rag_amd import ops
    case = (shape, "start0", "random")
    c, r = _case(case), _run(case, dev)
    N, D = c["N"], c["D"]
    x = r["x"].clone()
    x[0, D // 2] = float("inf")
    x[N - 1, D - 1] = float("nan")
    y, mean, rstd = ops.theta_gamma_norm(x, r["pe"], r["w"], r["b"], c["S"], EPS)
    assert bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[N - 1]).all()), "a poisoned row is not all NaN"
    assert torch.equal(_bits(y[1:N - 1]), _bits(r["y"][1:N - 1])), "another row changed"
    assert torch.equal(_bits(mean[1:N - 1]), _bits(r["mean"][1:N - 1]))
    assert torch.equal(_bits(rstd[1:N - 1]), _bits(r["rstd"][1:N - 1]))
    g_x, _ = ops.theta_gamma_norm_backward(r["g_y"], x, r["pe"], None, mean, rstd, r["w"], c["S"], column_sums=False)
    assert bool(torch.isnan(g_x[0]).all()) and bool(torch.isnan(g_x[N - 1]).all())
    assert torch.equal(_bits(g_x[1:N - 1]), _bits(r["g_x"][1:N - 1]))


# ------------------------------------------------------------------------------------- the Function and the module
class _Cfg:
    def __init__(self, D, vocab=40, P=100):
        self.embedding_dim, self.theta_frequency, self.gamma_frequency, self.max_seq_len = D, 8.0, 40.0, MAX_SEQ_LEN
        self.vocab_size, self.n_place_cells = vocab, P


def _module(c, dev):
    from aura_snn_rag_amd.core.language_zone.theta_gamma_encoding import ThetaGammaPositionalEncoding
    enc, norm = ThetaGammaPositionalEncoding(_Cfg(c["D"])).to(dev), nn.LayerNorm(c["D"], eps=EPS).to(dev)
    with torch.no_grad():
        for p, k in ((enc.theta_phase_offsets, "th"), (enc.gamma_phase_offsets, "ga"), (enc.amplitude_modulation, "amp"),
                     (norm.weight, "w"), (norm.bias, "b")):
            p.copy_(_dev(c[k], dev))
    return enc, norm


FUNCTION_CASES = [(s, POSITIONS[(i + 1) % 4], "random") for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("case", FUNCTION_CASES, ids=_id)
def test_function_against_torch_autograd_of_the_composition(dev, case):
    c, r = _case(case), _run(case, dev)
    B, S, D, N = c["B"], c["S"], c["D"], c["N"]
    enc, norm = _module(c, dev)
    params = [enc.theta_phase_offsets, enc.gamma_phase_offsets, enc.amplitude_modulation, norm.weight, norm.bias]
    hidden = r["x"].reshape(B, S, D).clone().requires_grad_()
    positions = None if c["positions"] is None else r["positions"].reshape((B, S) if case[1] == "per_item" else (S,))
    y = enc.encode_add_norm(hidden, norm, positions=positions, start=c["start"])
    assert torch.equal(_bits(y.reshape(N, D)), _bits(r["y"])), "the module's call differs from the ops'"
    (y * r["g_y"].reshape(B, S, D)).sum().backward()
    got = [hidden.grad.reshape(N, D).clone()] + [p.grad.clone() for p in params]
    assert torch.equal(_bits(got[0]), _bits(r["g_x"]))
    for g, i in zip(got[1:], (2, 3, 4, 0, 1)):
        assert torch.equal(_bits(g), _bits(r["grads"][i])), "the Function's gradients differ from the ops'"
    # forward(positions, S): bit-equal to the table the fused call used
    pos_t = torch.arange(c["start"], c["start"] + S, device=dev)[None] if positions is None else positions
    with torch.no_grad():
        assert torch.equal(_bits(enc(pos_t, S).reshape(-1, D)), _bits(r["pe"]))
    # the composition: the rule's fp32 phases, torch's sines, add, layer_norm, autograd
    for p in params:
        p.grad = None
    zero = np.zeros(D, np.float32)
    phi, phir = (_dev(v[:, :1].copy(), dev) for v in R.phases(c["used"], zero, zero, MAX_SEQ_LEN, RATIO))
    a, g = phi + params[0], phir + params[1]
    pe = (torch.sin(a) + 0.5 * (((torch.cos(a) + 1.0) * 0.5) * torch.sin(g))) * params[2]
    x2 = r["x"].clone().requires_grad_()
    y2 = F.layer_norm(x2 + pe[_dev(c["rows"], dev)], (D,), norm.weight, norm.bias, EPS)
    (y2 * r["g_y"]).sum().backward()
    h, _ = _forward_rule(c, r)
    dh = 2.0 * float(R.pe_bound(c["amp"][None, :], c["table"]["pe"]).max()) + 2.0 * R.U24 * float(np.abs(h).max())
    f = R.norm(h, c["w"], c["b"], EPS, dh)
    want = _backward_rule(c, r, dh, T=max(R.T_N(N), N + 3))
    name = _id(case)
    _within(f"function y {name}", _np(y).reshape(N, D), _np(y2), 2.0 * f["y_bound"])
    _within(f"function g_x {name}", _np(got[0]), _np(x2.grad), 2.0 * want["g_x"][1])
    for g_mine, p, k in zip(got[1:], params, ("g_theta", "g_gamma", "g_amp", "g_w", "g_b")):
        _within(f"function {k} {name}", _np(g_mine), _np(p.grad), 2.0 * want[k][1])


def test_only_the_wanted_gradients_are_computed(dev):
    case = ((2, 70, 768), "start0", "random")
    c, r = _case(case), _run(case, dev)
    enc, norm = _module(c, dev)
    for p in (*enc.parameters(), *norm.parameters()):
        p.requires_grad_(False)
    hidden = r["x"].reshape(2, 70, 768).clone().requires_grad_()
    (enc.encode_add_norm(hidden, norm) * r["g_y"].reshape(2, 70, 768)).sum().backward()
    assert torch.equal(_bits(hidden.grad.reshape(140, 768)), _bits(r["g_x"]))
    assert all(p.grad is None for p in (*enc.parameters(), *norm.parameters()))
    norm.bias.requires_grad_(True)
    (enc.encode_add_norm(hidden.detach(), norm) * r["g_y"].reshape(2, 70, 768)).sum().backward()
    assert torch.equal(_bits(norm.bias.grad), _bits(r["grads"][1])) and norm.weight.grad is None
    # under no_grad the range table is kept and follows the parameters
    with torch.no_grad():
        enc.encode_add_norm(hidden, norm)
        kept = enc._pe
        enc.encode_add_norm(hidden, norm)
        assert enc._pe is kept
        enc.amplitude_modulation.mul_(2.0)
        y = enc.encode_add_norm(hidden, norm)
        assert enc._pe is not kept and not torch.equal(y.reshape(140, 768), r["y"])


def test_embed_tokens_is_its_parts(dev):
    from aura_snn_rag_amd.core.language_zone.place_cell_encoder import PlaceCellSemanticEncoder
    from aura_snn_rag_amd.core.language_zone.theta_gamma_encoding import ThetaGammaPositionalEncoding, embed_tokens
    torch.manual_seed(41)
    cfg = _Cfg(36)
    sem, enc, norm = PlaceCellSemanticEncoder(cfg, None).to(dev), ThetaGammaPositionalEncoding(cfg).to(dev), \
        nn.LayerNorm(36).to(dev)
    ids = torch.randint(0, 40, (3, 7), generator=torch.Generator().manual_seed(42)).to(dev)
    with torch.no_grad():
        hidden, activity = embed_tokens(ids, sem, enc, norm, start=5)
        semantic, want_activity = sem(ids)
        pos = enc(torch.arange(5, 12, device=dev)[None], 7)
        assert torch.equal(_bits(activity), _bits(want_activity))
        assert torch.equal(_bits(hidden), _bits(enc.encode_add_norm(semantic, norm, start=5)))
        # against the three separate torch lines: the add rounds as the kernel's, LayerNorm within the y bound
        h = (semantic + pos).reshape(21, 36)
        f = R.norm(_np(h), _np(norm.weight), _np(norm.bias), norm.eps)
        _within("embed_tokens hidden", _np(hidden).reshape(21, 36), f["y"], f["y_bound"])
        sparse_hidden, code = embed_tokens(ids, sem, enc, norm, start=5, dense=False)
        assert torch.equal(_bits(sparse_hidden), _bits(hidden)) and torch.equal(_bits(code.to_dense()), _bits(activity))
    hidden, _ = embed_tokens(ids, sem, enc, norm)
    hidden.square().sum().backward()
    for n, p in (*sem.named_parameters(), *enc.named_parameters(), *norm.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
