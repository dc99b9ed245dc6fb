"""``ops.memory_attend`` on the GPU against the fp64 rule (tests/memory_attend_rule.py): every element within half its
derived bound; the known answers bit for bit; a row's bits the same alone, in the batch, over two calls and through
``out=``; a NaN row leaves the others alone; the host refusals raise without a launch.

Shapes ``(R, D, H, M)``: (1, 4, 1, 1): p = 1, so ``y = fl(x + fl(bo + U))`` exactly; (3, 96, 4, 5) the small layer;
(3, 100, 5, 3) D no multiple of 64; (32, 768, 12, 5) the workload's width at full R; (2, 768, 7, 3) H M = 21, odd against
any wave count; (2, 2048, 16, 32) both limits; (1, 64, 32, 32) H M = 1024.  Kinds of input: ``random``; ``uniform``
(G = 0 and equal s0 within a head: p is uniform, and exactly 1/M where M is a power of two, so the output equals the
rule's fp32 sum with that p bit for bit); ``onehot`` (G = 0, one score of each head 200 above the rest: p is one-hot
exactly, checked the same way); ``offset`` (rows of mean 1e3 and unit spread); ``nobias``.  The worst used share of the
bound goes to the parity record (``profiles/memory_attend_parity_counts.json``)."""
import itertools

import numpy as np
import pytest
import torch

from tests import helpers
from tests import memory_attend_rule as RULE

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 1, 1), (3, 96, 4, 5), (3, 100, 5, 3), (32, 768, 12, 5), (2, 768, 7, 3), (2, 2048, 16, 32),
          (1, 64, 32, 32)]
KINDS = ("random", "uniform", "onehot", "offset", "nobias")
CASES = list(itertools.product(SHAPES, KINDS))
IDS = ["R{}-D{}-H{}-M{}-{}".format(*s, k) for s, k in CASES]
SHAPE_IDS = ["R{}-D{}-H{}-M{}".format(*s) for s in SHAPES]
EPS = 1e-5
_INPUTS, _WANT = {}, {}


def _inputs(shape, kind):
    """The case's inputs, made once and left unchanged."""
    key = (shape, kind)
    if key in _INPUTS:
        return _INPUTS[key]
    R, D, H, M = shape
    rng = np.random.default_rng(1000 * SHAPES.index(shape) + KINDS.index(kind))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    i = dict(x=f(R, D), gamma=(1.0 + 0.3 * f(D)).astype(np.float32), beta=(0.3 * f(D)).astype(np.float32),
             G=(f(R, H, M, D) / np.sqrt(D)).astype(np.float32), s0=f(R, H, M), U=f(R, H, M, D), bo=f(D), p=None)
    if kind == "uniform":
        i["G"][:] = 0.0
        i["s0"][:] = f(R, H, 1)
        i["p"] = np.full((R, H, M), 1.0 / M)                          # fp64: exact in fp32 where M is a power of two
    elif kind == "onehot":
        i["G"][:] = 0.0
        i["s0"] = rng.uniform(-1.0, 1.0, (R, H, M)).astype(np.float32)
        star = rng.integers(0, M, (R, H))
        hot = np.zeros((R, H, M), dtype=bool)
        np.put_along_axis(hot, star[..., None], True, axis=2)
        i["s0"][hot] = np.float32(201.0)
        i["p"] = hot.astype(np.float64)
    elif kind == "offset":
        i["x"] = (np.float32(1e3) + i["x"]).astype(np.float32)
    elif kind == "nobias":
        i["bo"] = None
    _INPUTS[key] = i
    return i


def _want(shape, kind):
    key = (shape, kind)
    if key not in _WANT:
        i = _inputs(shape, kind)
        _WANT[key] = RULE.attend64(i["x"], i["gamma"], i["beta"], i["G"], i["s0"], i["U"], i["bo"], EPS)
    return _WANT[key]


def _call(dev, i, rows=None, x=None, **kw):
    from aura_snn_rag_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sel = slice(None) if rows is None else rows
    return ops.memory_attend(t((i["x"] if x is None else x)[sel]), (t(i["gamma"]), t(i["beta"])), t(i["G"][sel]),
                             t(i["s0"][sel]), t(i["U"][sel]), t(i["bo"]), eps=EPS, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_every_element_is_within_half_its_bound(dev, shape, kind):
    R, D, H, M = shape
    i = _inputs(shape, kind)
    want = _want(shape, kind)
    y = _call(dev, i)
    assert y.shape == (R, D) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    got = y.cpu().numpy()
    share = np.abs(got.astype(np.float64) - want["y"]) / want["bound"]
    name = IDS[CASES.index((shape, kind))]
    print(f"memory_attend {name}: worst share of the bound {share.max():.4f}, largest bound {want['bound'].max():.3e}, "
          f"largest |y| {np.abs(want['y']).max():.3e}, largest score bound {want['ds'].max():.3e}")
    helpers.record_parity(f"memory_attend {name}", R * D, R * D, worst_share=float(share.max()),
                          largest_bound=float(want["bound"].max()))
    assert share.max() <= 0.5
    if i["p"] is not None:
        exact = kind == "onehot" or M & (M - 1) == 0
        assert np.allclose(want["p"], i["p"], rtol=0.0, atol=1e-12), "the fp64 weights are the intended ones"
        if exact:
            known = RULE.finish32(i["p"], i["U"], i["x"], i["bo"])
            assert np.array_equal(got.view(np.int32), known.view(np.int32)), "p is exact, so the sum is the rule's bits"


def test_a_single_memory_adds_its_row_exactly(dev):
    i = _inputs((1, 4, 1, 1), "random")
    y = _call(dev, i).cpu().numpy()
    known = (i["x"] + (i["bo"][None, :] + i["U"][:, 0, 0, :]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(y.view(np.int32), known.view(np.int32))
    i = _inputs((1, 4, 1, 1), "nobias")
    y = _call(dev, i).cpu().numpy()
    assert np.array_equal(y.view(np.int32), (i["x"] + i["U"][:, 0, 0, :]).astype(np.float32).view(np.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_row_has_the_same_bits_alone_in_the_batch_over_two_calls_and_through_out(dev, shape):
    R, D, H, M = shape
    i = _inputs(shape, "random")
    y = _call(dev, i)
    assert torch.equal(_bits(_call(dev, i)), _bits(y)), "two calls"
    out = torch.full((R, D), 7.0, device=dev)
    assert _call(dev, i, out=out) is out and torch.equal(_bits(out), _bits(y)), "out= is honoured"
    for r in sorted({0, R // 2, R - 1}):
        alone = _call(dev, i, rows=slice(r, r + 1))
        assert torch.equal(_bits(alone[0]), _bits(y[r])), f"row {r} alone"
        if H * M * D <= 2 ** 16:
            copies = _call(dev, i, rows=[r] * 32)
            assert torch.equal(_bits(copies), _bits(y[r:r + 1].expand(32, -1))), f"row {r} in 32 copies"


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2], ids=[n for s, n in zip(SHAPES, SHAPE_IDS) if s[0] >= 2])
def test_a_nan_row_leaves_the_others_alone(dev, shape):
    R, D, H, M = shape
    i = _inputs(shape, "random")
    y = _call(dev, i)
    x = i["x"].copy()
    x[1, D // 2] = np.nan
    got = _call(dev, i, x=x)
    keep = [r for r in range(R) if r != 1]
    assert torch.equal(_bits(got[keep]), _bits(y[keep])) and bool(torch.isnan(got[1]).all())


def test_the_layers_formula_on_the_device(dev):
    """``fold_memory`` and one launch against ``inject_cross_attention`` in fp64, D = 96 / H = 4 and D = 768 / H = 12."""
    import types
    from aura_snn_rag_amd import MemoryAugmentedLayer, MemoryContext, ops
    for D, H in ((96, 4), (768, 12)):
        torch.manual_seed(D)
        cfg = types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D)
        layer = MemoryAugmentedLayer(cfg, None, memory_injection="cross_attention").eval().to(dev)
        ctx = MemoryContext(torch.randn(3, 5, D, device=dev), torch.rand(3, 5, device=dev), None)
        cache = layer.new_cache(3, 4)
        layer._pin(cache, ctx)
        fold = layer.fold_memory(cache)
        h = torch.randn(3, D, device=dev)
        mn, att = layer.memory_norm, layer.memory_attention
        with torch.no_grad():
            got = ops.memory_attend(h, (mn.weight, mn.bias), fold.G, fold.s0, fold.U, att.out_proj.bias, eps=mn.eps)
            layer.double()
            want = layer.inject_memories(h.double()[:, None], ctx.features.double(), ctx.scores.double())[:, 0]
        err = float((got.double() - want).abs().max())
        print(f"memory_attend against the module in fp64, D {D}: {err:.3e} at magnitude {float(want.abs().max()):.2f}")
        assert err <= 2e-5 * max(1.0, float(want.abs().max()))


def test_each_host_refusal_raises_without_a_launch(dev, monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "lib", no_lib)
    z = lambda *s: torch.zeros(*s, device=dev)
    good = dict(x=z(3, 16), norm=(z(16), z(16)), G=z(3, 2, 5, 16), s0=z(3, 2, 5), U=z(3, 2, 5, 16), bias=z(16), out=None)
    bad = [
        (dict(x=z(33, 16), G=z(33, 2, 5, 16), s0=z(33, 2, 5), U=z(33, 2, 5, 16)), ValueError),
        (dict(x=z(3, 18), norm=(z(18), z(18)), G=z(3, 2, 5, 18), U=z(3, 2, 5, 18), bias=z(18)), ValueError),
        (dict(x=z(3, 16).half()), TypeError),
        (dict(G=z(3, 2, 33, 16), s0=z(3, 2, 33), U=z(3, 2, 33, 16)), ValueError),
        (dict(G=z(3, 33, 32, 16), s0=z(3, 33, 32), U=z(3, 33, 32, 16)), ValueError),
        (dict(G=z(3, 2, 5, 32)[..., ::2]), ValueError),
        (dict(U=z(3, 2, 5, 16).bfloat16()), TypeError),
        (dict(s0=z(3, 2, 4)), ValueError),
        (dict(norm=(z(16), None)), ValueError),
        (dict(bias=z(12)), ValueError),
        (dict(out=z(3, 12)), ValueError),
        (dict(G=z(3 * 2 * 5 * 16 + 1)[1:].view(3, 2, 5, 16)), ValueError),
        (dict(U=torch.zeros(3, 2, 5, 16)), ops.AuraDeviceError),
    ]
    for change, exc in bad:
        a = dict(good)
        a.update(change)
        with pytest.raises(exc):
            ops.memory_attend(a["x"], a["norm"], a["G"], a["s0"], a["U"], a["bias"], out=a["out"])
