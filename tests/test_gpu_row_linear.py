"""``ops.row_linear`` on the GPU against the fp64 rule (tests/row_linear_rule.py): every element within half its derived
bound; a row's bits the same alone, in the batch, in a batch of 32 copies and over two calls; a NaN / inf row leaves
the finite rows' bits alone; ``out=`` is honoured; the three-matrix form is bit-equal to three single calls.

The shapes (R, K, N): the K edges of the lane pattern (4: below one lane's quad run; 96, 100, 260: no multiple of 256;
768, 2048, 8192: whole runs, the prologue's limit and the op's), N that no workgroup geometry divides (1, 5, 33, 257),
every row-count path of the kernel (1, 2, 3 -> 4, 8, 9 and 13 -> 16, 32), its three columns-per-wave paths (below 2048
columns, from 2048, from 8192, at up to 4 / 8 rows) and its two workgroup sizes (sixteen waves from 9 rows and 2048
columns up), and every combination of prologue / GELU / residual.  The rows of a case mix the input
kinds: random, mean 1e3 with spread 1, constant.  The worst used share of each bound goes to the parity record
(``profiles/row_linear_parity_counts.json``)."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import row_linear_rule as RULE

pytestmark = pytest.mark.gpu

#        R   K     N                norm   gelu   res    normed
CASES = [
    (1, 4, (1,), False, False, False, False),
    (3, 96, (5,), True, False, False, True),
    (3, 100, (257,), True, True, False, False),
    (32, 260, (96,), False, True, True, False),
    (8, 768, (768, 768, 768), True, False, False, True),
    (32, 2048, (64,), True, True, True, True),
    (2, 8192, (33,), False, False, True, False),
    (13, 520, (3, 130), False, True, False, False),
    (4, 256, (7,), True, False, True, True),
    (3, 12, (2049,), False, False, False, False),
    (2, 8, (8200,), False, True, False, False),
    (32, 264, (2050,), True, True, False, False),
    (9, 128, (1030, 1030), True, False, False, True),
]
IDS = [f"R{c[0]}-K{c[1]}-N{'+'.join(map(str, c[2]))}" + ("-ln" if c[3] else "") + ("-gelu" if c[4] else "")
       + ("-res" if c[5] else "") + ("-xh" if c[6] else "") for c in CASES]


def test_the_cases_cover_every_combination():
    assert {(c[3], c[4], c[5]) for c in CASES} == {(a, b, c) for a in (False, True) for b in (False, True)
                                                   for c in (False, True)}
    assert {c[6] for c in CASES if c[3]} == {False, True}


def _inputs(case, seed):
    R, K, Ns, norm, gelu, res, normed = case
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x = f(R, K)
    for r in range(R):
        if r % 3 == 1:
            x[r] += np.float32(1e3)                                    # mean 1e3, spread 1
        elif r % 3 == 2 and norm:
            x[r] = np.float32(rng.standard_normal() * 3.0)             # a constant row: the prologue returns beta
    return dict(x=x, W=[(f(n, K) / np.sqrt(K)).astype(np.float32) for n in Ns],
                b=[f(n) if (j + seed) % 2 == 0 or len(Ns) == 1 else None for j, n in enumerate(Ns)],
                norm=(1.0 + 0.3 * f(K), 0.3 * f(K)) if norm else None, res=f(R, Ns[0]) if res else None)


def _call(dev, i, case, rows=None, x=None, **kw):
    """The op on the device for the rows ``rows`` (default: all) of the case's inputs."""
    from aura_snn_rag_amd import ops
    R, K, Ns, norm, gelu, res, normed = case
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sel = slice(None) if rows is None else rows
    xs = (i["x"] if x is None else x)[sel]
    single = len(Ns) == 1
    W = t(i["W"][0]) if single else tuple(t(w) for w in i["W"])
    b = t(i["b"][0]) if single else tuple(t(v) for v in i["b"])
    out = ops.row_linear(t(xs), W, b, norm=None if not norm else (t(i["norm"][0]), t(i["norm"][1])), eps=1e-5,
                         activation="gelu" if gelu else None, residual=None if not res else t(i["res"][sel]),
                         return_normed=normed, **kw)
    y, xh = out if normed else (out, None)
    return ([y] if single else list(y)), xh


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_element_is_within_half_its_bound(dev, case):
    R, K, Ns, norm, gelu, res, normed = case
    i = _inputs(case, seed=CASES.index(case))
    want = RULE.linear64(i["x"], i["W"], i["b"], norm=i["norm"], eps=1e-5, gelu=gelu, residual=i["res"])
    ys, xh = _call(dev, i, case)
    worst = 0.0
    for j, y in enumerate(ys):
        assert y.shape == (R, Ns[j]) and y.dtype == torch.float32
        share = np.abs(y.cpu().numpy().astype(np.float64) - want["y"][j]) / want["bound"][j]
        print(f"{IDS[CASES.index(case)]} y{j}: worst share of the bound {share.max():.4f}, largest bound "
              f"{want['bound'][j].max():.3e}, largest |y| {np.abs(want['y'][j]).max():.3e}")
        worst = max(worst, float(share.max()))
    extra = {}
    if normed:
        assert xh.shape == (R, K)
        s = np.abs(xh.cpu().numpy().astype(np.float64) - want["xh"]) / want["xh_bound"]
        print(f"{IDS[CASES.index(case)]} xh: worst share of the bound {s.max():.4f}")
        extra["worst_share_xh"] = float(s.max())
        worst = max(worst, float(s.max()))
    helpers.record_parity(f"row_linear {IDS[CASES.index(case)]}", R * sum(Ns), R * sum(Ns), worst_share=worst, **extra)
    assert worst <= 0.5


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_row_has_the_same_bits_alone_in_any_batch_and_over_two_calls(dev, case):
    R, K, Ns, norm, gelu, res, normed = case
    i = _inputs(case, seed=100 + CASES.index(case))
    ys, xh = _call(dev, i, case)
    again, xh2 = _call(dev, i, case)
    for a, b in zip(ys, again):
        assert torch.equal(_bits(a), _bits(b)), "two calls"
    if normed:
        assert torch.equal(_bits(xh), _bits(xh2))
    for r in sorted({0, R // 2, R - 1}):
        alone, xh1 = _call(dev, i, case, rows=slice(r, r + 1))
        copies, xhc = _call(dev, i, case, rows=[r] * 32)
        for y, a, c in zip(ys, alone, copies):
            assert torch.equal(_bits(a[0]), _bits(y[r])), f"row {r} alone"
            assert torch.equal(_bits(c), _bits(y[r:r + 1].expand(32, -1))), f"row {r} in 32 copies"
        if normed:
            assert torch.equal(_bits(xh1[0]), _bits(xh[r])) and torch.equal(_bits(xhc[31]), _bits(xh[r]))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] >= 3], ids=[n for c, n in zip(CASES, IDS) if c[0] >= 3])
def test_a_nan_or_inf_row_leaves_the_finite_rows_alone(dev, case):
    R, K, Ns, norm, gelu, res, normed = case
    i = _inputs(case, seed=200 + CASES.index(case))
    ys, xh = _call(dev, i, case)
    for bad in (np.nan, np.inf):
        x = i["x"].copy()
        x[1] = bad if bad is np.nan else np.where(np.arange(K) % 2 == 0, np.inf, x[1])
        got, xh_b = _call(dev, i, case, x=x)
        keep = [r for r in range(R) if r != 1]
        for y, g in zip(ys, got):
            assert torch.equal(_bits(g[keep]), _bits(y[keep]))
            assert not bool(torch.isfinite(g[1]).all())
        if normed:
            assert torch.equal(_bits(xh_b[keep]), _bits(xh[keep]))


def test_out_is_honoured_and_three_matrices_equal_three_calls(dev):
    from aura_snn_rag_amd import ops
    case = CASES[4]
    R, K, Ns, *_ = case
    i = _inputs(case, seed=300)
    (q, k, v), xh = _call(dev, i, case)
    t = lambda a: torch.from_numpy(a).to(dev)
    norm = (t(i["norm"][0]), t(i["norm"][1]))
    outs = tuple(torch.full((R, n), 7.0, device=dev) for n in Ns)
    (ys, xh2) = ops.row_linear(t(i["x"]), tuple(t(w) for w in i["W"]), tuple(None if b is None else t(b) for b in i["b"]),
                               norm=norm, return_normed=True, out=outs)
    assert all(a is b for a, b in zip(ys, outs)), "out= returns the tensors it was given"
    for j, (want, o) in enumerate(zip((q, k, v), outs)):
        assert torch.equal(_bits(o), _bits(want))
        single = ops.row_linear(t(i["x"]), t(i["W"][j]), None if i["b"][j] is None else t(i["b"][j]), norm=norm)
        assert torch.equal(_bits(single), _bits(want)), f"matrix {j} on its own"
        two = ops.row_linear(t(i["x"]), (t(i["W"][j]), t(i["W"][0])), None, norm=norm)[0]
        plain = ops.row_linear(t(i["x"]), t(i["W"][j]), norm=norm)
        assert torch.equal(_bits(two), _bits(plain)), "two matrices without biases against one"
    o1 = torch.empty(R, Ns[0], device=dev)
    y1 = ops.row_linear(t(i["x"]), t(i["W"][0]), out=o1, activation="gelu", residual=q)
    assert y1 is o1 and torch.equal(_bits(o1), _bits(ops.row_linear(t(i["x"]), t(i["W"][0]), activation="gelu",
                                                                    residual=q)))
    # the weights' cache policy is not part of the result
    try:
        ops.ROW_LINEAR_NONTEMPORAL = not ops.ROW_LINEAR_NONTEMPORAL
        other, _ = _call(dev, i, case)
    finally:
        ops.ROW_LINEAR_NONTEMPORAL = not ops.ROW_LINEAR_NONTEMPORAL
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(other, (q, k, v)))


def test_a_zero_variance_row_and_the_known_answers_on_the_device(dev):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(4)
    gamma, beta = torch.randn(256, generator=g).to(dev), torch.randn(256, generator=g).to(dev)
    eye = torch.eye(256, device=dev)
    y, xh = ops.row_linear(torch.full((2, 256), 0.75, device=dev), eye, norm=(gamma, beta), return_normed=True)
    assert torch.equal(y, beta.expand(2, -1)) and torch.equal(xh, y), "a constant row gives beta; identity is exact"
    res = torch.randn(5, 7, generator=g).to(dev)
    zero = ops.row_linear(torch.randn(5, 12, generator=g).to(dev), torch.zeros(7, 12, device=dev), residual=res)
    assert torch.equal(zero, res)
    t = torch.tensor([[0.0, 1.0, -1.0, 6.0, -6.0, 0.5, -0.5, 3.0]], device=dev)
    got = ops.row_linear(t, torch.eye(8, device=dev), activation="gelu")[0].cpu().double()
    want = torch.from_numpy(RULE.gelu64(t.cpu().numpy()))[0]
    assert float(got[0]) == 0.0 and float((got - want).abs().max()) <= 6.0 * 0.5 * 2.0 ** -19
