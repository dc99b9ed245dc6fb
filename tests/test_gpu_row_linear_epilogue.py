"""The two epilogues of the row linear kernel on the GPU.  ``ops.row_linear_gif`` (below, "the GIF epilogue"): both
forms bit-equal to ``ops.gif_run`` applied to ``ops.row_linear``'s output, over T in {1, 4, 8}, 1 to 32 rows, K in {4, 96,
772}, N in {1, 5, 770}, L in {8, 16} and currents that leave neurons silent, spiking and saturated at L; the mix against
the NumPy rule.  ``ops.row_linear_gate`` against the fp64 rule (tests/row_linear_epilogue_rule.py): every element within
half its derived bound; a row's bits the same alone, in the batch and over two calls; a NaN row leaves the others alone;
the strided weight (the left half of a [N, 2K] parameter, read in place) gives the bits of the contiguous copy.

The cases are the product of R in {1, 3, 32} (one lane, a padded row tile, the limit), K in {4, 96, 772, 3072} (772 is
not a multiple of the 256-column tile), N in {1, 5, 770} and a row stride of K and 2K.  The gate's pre-activation ``a``
is steered to +-30, +-100 and 0 at five of every seven elements (u is chosen against the fp64 dot product) and is
random at the others; every third row of c is of magnitude 1e3.  The worst used share of the bound goes to the parity
record (``profiles/row_linear_epilogue_parity_counts.json``)."""
import itertools

import numpy as np
import pytest
import torch

from tests import helpers
from tests import row_linear_epilogue_rule as EPI
from tests import row_linear_rule as RULE

pytestmark = pytest.mark.gpu

CASES = list(itertools.product((1, 3, 32), (4, 96, 772, 3072), (1, 5, 770), (1, 2)))
IDS = [f"R{r}-K{k}-N{n}-ldw{m}K" for r, k, n, m in CASES]
TARGETS = np.array([30.0, -30.0, 100.0, -100.0, 0.0])
_INPUTS = {}


def _inputs(case):
    """The case's inputs, made once and left unchanged.  ``Wfull`` [N, mult K] is the parameter, ``W`` its left K
    columns (a view)."""
    if case in _INPUTS:
        return _INPUTS[case]
    R, K, N, mult = case
    seed = CASES.index(case)
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x = f(R, K)
    Wfull = (f(N, mult * K) / np.sqrt(K)).astype(np.float32)
    W = Wfull[:, :K]
    b = f(N) if seed % 2 == 0 else None
    t64 = RULE.linear64(x, [W], [b])["y"][0]
    u = (2.0 * f(R, N)).astype(np.float32)
    flat = (np.arange(R * N).reshape(R, N) + seed) % 7
    steer = flat < len(TARGETS)
    u[steer] = (TARGETS[flat[steer]] - t64[steer]).astype(np.float32)
    c = f(R, N)
    c[1::3] *= np.float32(1e3)
    _INPUTS[case] = dict(x=x, Wfull=Wfull, W=W, b=b, u=u, c=c, res=f(R, N), steer=steer, flat=flat)
    return _INPUTS[case]


def _call(dev, i, rows=None, x=None, contiguous_weight=False, **kw):
    from aura_snn_rag_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sel = slice(None) if rows is None else rows
    K = i["x"].shape[1]
    W = t(i["W"]) if contiguous_weight else t(i["Wfull"])[:, :K]
    return ops.row_linear_gate(t((i["x"] if x is None else x)[sel]), W, t(i["b"]), t(i["u"][sel]), t(i["c"][sel]),
                               t(i["res"][sel]), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_the_steered_elements_reach_their_targets():
    i = _inputs((32, 96, 770, 2))
    a = EPI.gate64(i["x"], i["W"], i["b"], i["u"], i["c"], i["res"])["a"]
    for j, target in enumerate(TARGETS):
        hit = a[i["flat"] == j]
        assert hit.size > 0 and np.all(np.abs(hit - target) <= 1e-4), target


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_element_is_within_half_its_bound(dev, case):
    R, K, N, mult = case
    i = _inputs(case)
    want = EPI.gate64(i["x"], i["W"], i["b"], i["u"], i["c"], i["res"])
    y = _call(dev, i)
    assert y.shape == (R, N) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    share = np.abs(y.cpu().numpy().astype(np.float64) - want["y"]) / want["bound"]
    name = IDS[CASES.index(case)]
    steered = float(np.max(share[i["steer"]], initial=0.0))
    print(f"row_linear_gate {name}: worst share of the bound {share.max():.4f}, at the steered elements "
          f"{steered:.4f}, largest bound {want['bound'].max():.3e}, largest |y| "
          f"{np.abs(want['y']).max():.3e}")
    helpers.record_parity(f"row_linear_gate {name}", R * N, R * N, worst_share=float(share.max()),
                          worst_share_steered=steered)
    assert share.max() <= 0.5


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_row_has_the_same_bits_alone_in_the_batch_and_over_two_calls(dev, case):
    R, K, N, mult = case
    i = _inputs(case)
    y = _call(dev, i)
    assert torch.equal(_bits(_call(dev, i)), _bits(y)), "two calls"
    assert torch.equal(_bits(_call(dev, i, contiguous_weight=True)), _bits(y)), "the row stride is not part of the result"
    out = torch.full((R, N), 7.0, device=dev)
    assert _call(dev, i, out=out) is out and torch.equal(_bits(out), _bits(y)), "out= is honoured"
    for r in sorted({0, R // 2, R - 1}):
        alone = _call(dev, i, rows=slice(r, r + 1))
        assert torch.equal(_bits(alone[0]), _bits(y[r])), f"row {r} alone"
        copies = _call(dev, i, rows=[r] * 32)
        assert torch.equal(_bits(copies), _bits(y[r:r + 1].expand(32, -1))), f"row {r} in 32 copies"


@pytest.mark.parametrize("case", [c for c in CASES if c[0] >= 3], ids=[n for c, n in zip(CASES, IDS) if c[0] >= 3])
def test_a_nan_row_leaves_the_others_alone(dev, case):
    R, K, N, mult = case
    i = _inputs(case)
    y = _call(dev, i)
    x = i["x"].copy()
    x[1] = np.nan
    got = _call(dev, i, x=x)
    keep = [r for r in range(R) if r != 1]
    assert torch.equal(_bits(got[keep]), _bits(y[keep])) and bool(torch.isnan(got[1]).all())


def test_the_known_answers_on_the_device(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 8, generator=g).to(dev)
    zero = torch.zeros(6, 8, device=dev)
    res, c = torch.randn(4, 6, generator=g).to(dev), torch.randn(4, 6, generator=g).to(dev)
    u = torch.zeros(4, 6, device=dev)
    assert torch.equal(ops.row_linear_gate(x, zero, None, u, c, res), res + 0.5 * c), "sigmoid(0) is one half"
    far = torch.full((4, 6), 100.0, device=dev)
    assert torch.equal(ops.row_linear_gate(x, zero, None, far, c, res), res + c), "an open gate adds c"
    assert torch.equal(ops.row_linear_gate(x, zero, None, -far, c, res), res), "a closed gate adds nothing"
    # the layer's formula: sigmoid(W_g [h; ctx] + b_g) with the context half folded into u
    D = 96
    gate = torch.nn.Linear(2 * D, D).to(dev)
    h, ctx = torch.randn(3, D, generator=g).to(dev), torch.randn(3, D, generator=g).to(dev)
    with torch.no_grad():
        want = h + torch.sigmoid(gate(torch.cat([h, ctx], dim=-1))) * ctx
        fold = torch.nn.functional.linear(ctx, gate.weight[:, D:], gate.bias).contiguous()
        got = ops.row_linear_gate(h, gate.weight[:, :D], None, fold, ctx, h)
    assert float((got - want).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ the GIF epilogue
# (tokens, T): tokens * T covers 1, 4, 24 and 32 rows with T in {1, 4, 8}.  Time-major: R = tokens * T input rows;
# time-invariant: R = tokens rows that run T steps each.
GIF_ROWS = [(1, 1), (4, 1), (24, 1), (32, 1), (1, 4), (6, 4), (8, 4), (3, 8), (4, 8)]
GIF_CASES = list(itertools.product(GIF_ROWS, (4, 96, 772), (1, 5, 770), (8, 16)))
GIF_IDS = [f"tok{tok}-T{T}-K{k}-N{n}-L{L}" for (tok, T), k, n, L in GIF_CASES]
GIF_KW = dict(decay=float(np.exp(-1.0 / 10.0)), alpha=0.01, threshold=1.0)
REGIMES = (0.01, 1.0, 100.0)                                               # silent, spiking, saturated at L
_GIF_INPUTS = {}


def _gif_inputs(case, rows):
    """Inputs of ``rows`` rows for the case: the columns' currents cycle through the three regimes (the weights' rows are
    scaled; a single column takes the regime of the case's number)."""
    key = case + (rows,)
    if key not in _GIF_INPUTS:
        (tok, T), K, N, L = case
        seed = 1000 + GIF_CASES.index(case)
        rng = np.random.default_rng(seed)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        scale = np.array([REGIMES[(n + seed) % 3] for n in range(N)], dtype=np.float32)
        W = (f(N, K) / np.sqrt(K) * scale[:, None]).astype(np.float32)
        _GIF_INPUTS[key] = dict(x=f(rows, K), W=W, b=(0.1 * f(N) * scale).astype(np.float32) if seed % 2 else None)
    return _GIF_INPUTS[key]


def _reference(dev, i, T, L, time_major):
    """``ops.gif_run`` applied to ``ops.row_linear``'s output, from fresh state."""
    from aura_snn_rag_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    c = ops.row_linear(t(i["x"]), t(i["W"]), t(i["b"]))
    R, N = c.shape
    rows = R // T if time_major else R
    v = torch.zeros(rows, N, device=dev)
    theta = torch.full((rows, N), GIF_KW["threshold"], device=dev)
    out = torch.empty((rows, N) if time_major else (rows, T, N), device=dev)
    ops.gif_run(c.view(rows, T, N) if time_major else c, out, v, theta, GIF_KW["decay"], L, GIF_KW["alpha"],
                GIF_KW["threshold"], T, time_invariant=not time_major, mean_out=time_major)
    return out


@pytest.mark.parametrize("case", GIF_CASES, ids=GIF_IDS)
def test_both_gif_forms_are_gif_run_on_row_linear_bit_for_bit(dev, case):
    from aura_snn_rag_amd import ops
    (tok, T), K, N, L = case
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    ti = _gif_inputs(case, tok)
    spikes = ops.row_linear_gif(t(ti["x"]), t(ti["W"]), t(ti["b"]), T=T, L=L, **GIF_KW)
    assert spikes.shape == (tok, T, N) and torch.equal(_bits(spikes), _bits(_reference(dev, ti, T, L, False)))
    assert torch.equal(_bits(ops.row_linear_gif(t(ti["x"]), t(ti["W"]), t(ti["b"]), T=T, L=L, **GIF_KW)), _bits(spikes))
    tm = _gif_inputs(case, tok * T)
    mean = ops.row_linear_gif(t(tm["x"]), t(tm["W"]), t(tm["b"]), T=T, L=L, time_major=True, **GIF_KW)
    assert mean.shape == (tok, N) and torch.equal(_bits(mean), _bits(_reference(dev, tm, T, L, True)))
    # a token alone gives its bits, and out= is honoured
    for k in sorted({0, tok - 1}):
        alone = ops.row_linear_gif(t(tm["x"][k * T:(k + 1) * T]), t(tm["W"]), t(tm["b"]), T=T, L=L, time_major=True,
                                   **GIF_KW)
        assert torch.equal(_bits(alone[0]), _bits(mean[k])), f"token {k} alone"
        assert torch.equal(_bits(ops.row_linear_gif(t(ti["x"][k:k + 1]), t(ti["W"]), t(ti["b"]), T=T, L=L, **GIF_KW)[0]),
                           _bits(spikes[k])), f"row {k} alone"
    out = torch.full((tok, N), 7.0, device=dev)
    assert ops.row_linear_gif(t(tm["x"]), t(tm["W"]), t(tm["b"]), T=T, L=L, time_major=True, out=out, **GIF_KW) is out
    assert torch.equal(_bits(out), _bits(mean))


@pytest.mark.parametrize("case", GIF_CASES, ids=GIF_IDS)
def test_the_mix_and_residual_form_follows_the_rule(dev, case):
    """``y = fl(res + fl(fl(fl(1 - g) m) + fl(g mean)))`` with the mean of the plain form.  The device's g comes from its
    expf, NumPy's from its own: each is within ``4 * 2^-24 g`` of the exact sigmoid (exp within 1 ulp, two roundings), so
    g and 1 - g differ by at most ``8 * 2^-24`` between the sides, and each side rounds three more times: the outputs
    differ by at most ``16 * 2^-24 (|res| + |m| + |mean|)``."""
    from aura_snn_rag_amd import ops
    (tok, T), K, N, L = case
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    tm = _gif_inputs(case, tok * T)
    rng = np.random.default_rng(5000 + GIF_CASES.index(case))
    res, m = rng.standard_normal((tok, N)).astype(np.float32), rng.standard_normal((tok, N)).astype(np.float32)
    worst = 0.0
    for gate in (0.5, -3.0, 12.0):
        mean = ops.row_linear_gif(t(tm["x"]), t(tm["W"]), t(tm["b"]), T=T, L=L, time_major=True, **GIF_KW).cpu().numpy()
        y = ops.row_linear_gif(t(tm["x"]), t(tm["W"]), t(tm["b"]), T=T, L=L, time_major=True,
                               mix=(t(res), t(m), torch.tensor(gate, device=dev)), **GIF_KW).cpu().numpy()
        want = EPI.hybrid_mix32(res, m, mean, gate)
        tol = 16.0 * 2.0 ** -24 * (np.abs(res) + np.abs(m) + np.abs(mean))
        worst = max(worst, float((np.abs(y.astype(np.float64) - want.astype(np.float64)) / np.maximum(tol, 1e-30)).max()))
        assert np.all(np.abs(y.astype(np.float64) - want.astype(np.float64)) <= tol), gate
    helpers.record_parity(f"row_linear_gif mix {GIF_IDS[GIF_CASES.index(case)]}", tok * N, tok * N, worst_share=worst)


def test_the_three_regimes_are_present(dev):
    from aura_snn_rag_amd import ops
    case = ((32, 1), 96, 770, 8)
    i = _gif_inputs(case, 32)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    spikes = ops.row_linear_gif(t(i["x"]), t(i["W"]), t(i["b"]), T=4, L=8, **GIF_KW)
    seed = 1000 + GIF_CASES.index(case)
    regime = torch.tensor([(n + seed) % 3 for n in range(770)], device=dev)
    assert bool((spikes[:, :, regime == 0] == 0).all()), "currents of 0.01 never reach the threshold"
    mid = spikes[:, :, regime == 1]
    assert bool(((mid > 0) & (mid < 8)).any()) and bool((mid == 0).any())
    assert bool((spikes[:, :, regime == 2] == 8).any()), "currents of 100 saturate at L"
    assert bool((spikes == spikes.floor()).all()) and float(spikes.min()) == 0.0 and float(spikes.max()) == 8.0
