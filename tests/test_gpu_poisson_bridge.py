"""``ops.poisson_rate`` on the GPU against the rule of tests/poisson_bridge_rule.py (``include/aura_hip.h``, "Poisson
bridge").

Every case asks for all three outputs and checks, from the kernel's own intermediate result:
  a  ``q`` within HALF its derived bound of the fp64 probability, in every element;
  b  ``spikes`` equal to the rule's decision ``u < q`` on the kernel's own ``q``, in every element;
  c  ``rate`` bit-equal to ``spikes.mean(dim=1)`` from torch, and to the rule's ``count / T``.
Shapes: the full product of N in {1, 31, 32, 33, 97} (the 32-row tile), K in {4, 64, 100, 256} (the chain's blocks of
eight, the limit), H in {1, 4, 36, 64, 516} (the wave's 32 channels, the workgroup's 128) and T in {1, 3, 4, 5, 10, 64}
(the four words of a draw).  The uniforms of a smaller case are a corner of the largest one's, so the rule's generator runs
once.  Inputs: random; ``z`` forced to +-100 (q exactly 1 / 0); a NaN row and a +-inf row among normal rows; zero
weights (q = 0.5 exactly).  Then the bits of every output alone and in the batch, over (S, start) splits, with a device
``start``, over two calls, through ``out=`` and with or without the optional outputs.  The worst share of the bound
goes to the parity record (``profiles/poisson_bridge_parity_counts.json``)."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import poisson_bridge_rule as RULE

pytestmark = pytest.mark.gpu

NS, KS, HS, TS = (1, 31, 32, 33, 97), (4, 64, 100, 256), (1, 4, 36, 64, 516), (1, 3, 4, 5, 10, 64)
SEED = 0x5eed0123456789ab


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def uniforms():
    """u [97, 64, 516] of the default addressing (stream n, position 0) under SEED; never written."""
    s, p = RULE.row_addresses(max(NS))
    u = RULE.uniforms(max(HS), max(TS), s, p, SEED)
    u.setflags(write=False)
    return u


def _inputs(K, seed=0):
    g = torch.Generator().manual_seed(seed + K)
    return (torch.randn(max(NS), K, generator=g), torch.randn(max(HS), K, generator=g) * (2.0 / K ** 0.5),
            torch.randn(max(HS), generator=g))


def _check(out, x, W, b, T, u, q64=None, bound=None):
    """a, b and c on one call's ``(rate, q, spikes)``; returns the worst share of the bound among the finite rows."""
    rate, q, spikes = out
    qh = q.cpu().numpy()
    if q64 is None:
        q64, bound = RULE.probability64(x.numpy(), W.numpy(), None if b is None else b.numpy())
    finite = np.isfinite(q64) & np.isfinite(bound)
    share = float((np.abs(qh.astype(np.float64) - q64)[finite] / bound[finite]).max()) if finite.any() else 0.0
    want = RULE.spikes_of(qh, u)
    assert np.array_equal(spikes.cpu().numpy(), want), "a spike differs from the rule on the kernel's own q"
    mean = spikes.mean(dim=1)
    differ = int((_bits(rate) != _bits(mean)).sum())
    print(f"N={x.shape[0]} K={x.shape[1]} H={W.shape[0]} T={T}: worst q share {share:.4f}, rate != torch mean in {differ}")
    assert np.array_equal(rate.cpu().numpy().view(np.int32), RULE.rate_of(want).view(np.int32))
    assert differ == 0, "rate is not the bits of spikes.mean(dim=1)"
    assert share <= 0.5
    return share


@pytest.mark.parametrize("K", KS)
def test_every_tile_and_word_edge_against_the_rule(dev, K, uniforms):
    from aura_snn_rag_amd import ops
    x, W, b = _inputs(K)
    q64, bound = RULE.probability64(x.numpy(), W.numpy(), b.numpy())
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    worst, cases = 0.0, 0
    for N in NS:
        for H in HS:
            Wh, bh = Wd[:H].contiguous(), bd[:H].contiguous()
            for T in TS:
                out = ops.poisson_rate(xd[:N], Wh, bh, T=T, seed=SEED, return_probs=True, return_spikes=True)
                assert out[0].shape == (N, H) and out[1].shape == (N, H) and out[2].shape == (N, T, H)
                worst = max(worst, _check(out, x[:N], W[:H], b[:H], T, uniforms[:N, :T, :H], q64[:N, :H], bound[:N, :H]))
                cases += 1
    assert cases == len(NS) * len(HS) * len(TS)
    helpers.record_parity(f"poisson_bridge K={K}", cases, cases, worst_q_share=worst)


def test_forced_and_special_inputs(dev, uniforms):
    from aura_snn_rag_amd import ops
    N, K, H, T = 33, 64, 36, 10
    x, W, b = _inputs(K, seed=1)
    x, W, b = x[:N].clone(), W[:H].clone(), b[:H].clone()
    u = uniforms[:N, :T, :H]
    run = lambda x_, W_, b_: ops.poisson_rate(x_.to(dev), W_.to(dev), None if b_ is None else b_.to(dev), T=T,
                                              seed=SEED, return_probs=True, return_spikes=True)
    # z = +-100 through the bias over zero weights: q exactly 1 / 0, all / no spikes
    forced = torch.where(torch.arange(H) % 2 == 0, 100.0, -100.0)
    rate, q, spikes = run(x, torch.zeros(H, K), forced)
    assert torch.equal(q.cpu(), (forced > 0).float().expand(N, H)) and torch.equal(rate.cpu(), q.cpu())
    assert torch.equal(spikes.cpu(), q.cpu()[:, None, :].expand(N, T, H))
    # zero weights without a bias: q = 0.5 exactly, the spikes are u < 0.5
    out = run(x, torch.zeros(H, K), None)
    assert (out[1] == 0.5).all()
    _check(out, x, torch.zeros(H, K), None, T, u)
    # without a bias on random weights
    _check(run(x, W, None), x, W, None, T, u)
    # a NaN row and a +-inf row among normal rows: the NaN row never spikes, the others keep their bits
    clean = run(x, W, b)
    dirty_x = x.clone()
    dirty_x[5] = float("nan")
    dirty_x[17, ::2] = float("inf")
    dirty_x[17, 1::2] = float("-inf")
    dirty_x[20, 3] = float("inf")
    dirty = run(dirty_x, W, b)
    assert (dirty[0][5] == 0).all() and (dirty[2][5] == 0).all() and torch.isnan(dirty[1][5]).all()
    keep = [n for n in range(N) if n not in (5, 17, 20)]
    for a, c in zip(clean, dirty):
        assert _same(a[keep], c[keep])
    # the inf rows: wherever q is a number the decision is still the rule's on it, and q is 0 or 1 on an infinite z
    qh = dirty[1].cpu().numpy()
    assert np.array_equal(dirty[2].cpu().numpy(), RULE.spikes_of(qh, u))
    z20 = dirty_x[20, 3] * W[:, 3]
    assert np.array_equal(qh[20], (z20 > 0).float().numpy())
    assert np.isnan(qh[17]).all() or set(np.unique(qh[17][~np.isnan(qh[17])])) <= {0.0, 1.0}
    _check(clean, x, W, b, T, u)


def test_the_bits_do_not_depend_on_the_batch_the_split_or_the_call(dev):
    from aura_snn_rag_amd import ops
    N, K, H, T = 97, 100, 516, 10
    B, S = 1, 97
    x, W, b = _inputs(K, seed=2)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    kw = dict(T=T, seed=SEED, return_probs=True, return_spikes=True)
    # one stream of 97 consecutive positions from 1000
    whole = ops.poisson_rate(xd, Wd, bd, streams=[7], rows_per_stream=S, start=1000, **kw)
    s, p = RULE.row_addresses(N, [7], S, 1000)
    assert np.array_equal(whole[2].cpu().numpy(), RULE.spikes_of(whole[1].cpu().numpy(), RULE.uniforms(H, T, s, p, SEED)))
    # over two calls
    for a, c in zip(whole, ops.poisson_rate(xd, Wd, bd, streams=[7], rows_per_stream=S, start=1000, **kw)):
        assert _same(a, c)
    # (S, start) = (N, 1000) against (1, start[b] = 1000 + n) over renumbered streams, the start on the device
    per_row = torch.arange(1000, 1000 + N, dtype=torch.int32, device=dev)
    sevens = torch.full((N,), 7, dtype=torch.int32, device=dev)
    split = ops.poisson_rate(xd, Wd, bd, streams=sevens, rows_per_stream=1, start=per_row, **kw)
    for a, c in zip(whole, split):
        assert _same(a, c)
    # a device start against a host one, int64 streams against int32 ones
    host = ops.poisson_rate(xd, Wd, bd, streams=[7], rows_per_stream=S, start=torch.tensor([1000], dtype=torch.int32,
                                                                                           device=dev), **kw)
    wide = ops.poisson_rate(xd, Wd, bd, streams=torch.tensor([7 + (1 << 32)], device=dev), rows_per_stream=S,
                            start=1000, **kw)
    for a, c, d in zip(whole, host, wide):
        assert _same(a, c) and _same(a, d)
    # two streams of different starts in one call
    two = ops.poisson_rate(xd[:96], Wd, bd, streams=[7, 7], rows_per_stream=48,
                           start=torch.tensor([1000, 1048], dtype=torch.int32, device=dev), **kw)
    for a, c in zip(whole, two):
        assert _same(a[:96], c)
    # a row alone, at three places of its tile, and a slice of the batch
    for n in (0, 31, 32, 96):
        alone = ops.poisson_rate(xd[n:n + 1], Wd, bd, streams=[7], rows_per_stream=1, start=1000 + n, **kw)
        for a, c in zip(whole, alone):
            assert _same(a[n:n + 1], c), n
    part = ops.poisson_rate(xd[40:73], Wd, bd, streams=[7], rows_per_stream=33, start=1040, **kw)
    for a, c in zip(whole, part):
        assert _same(a[40:73], c)
    # through out=, and with or without the optional outputs
    out = torch.full((N, H), -1.0, device=dev)
    got = ops.poisson_rate(xd, Wd, bd, T=T, seed=SEED, streams=[7], rows_per_stream=S, start=1000, out=out)
    assert got is out and _same(out, whole[0])
    only_q = ops.poisson_rate(xd, Wd, bd, T=T, seed=SEED, streams=[7], rows_per_stream=S, start=1000, return_probs=True)
    only_s = ops.poisson_rate(xd, Wd, bd, T=T, seed=SEED, streams=[7], rows_per_stream=S, start=1000, return_spikes=True)
    assert len(only_q) == 2 and len(only_s) == 2
    assert _same(only_q[0], whole[0]) and _same(only_q[1], whole[1])
    assert _same(only_s[0], whole[0]) and _same(only_s[1], whole[2])
    # another seed, stream or position draws something else; the default is stream n at position 0
    for other in (dict(seed=SEED + 1), dict(streams=[8]), dict(start=1001)):
        args = dict(dict(T=T, seed=SEED, streams=[7], rows_per_stream=S, start=1000), **other)
        assert not _same(ops.poisson_rate(xd, Wd, bd, **args), whole[0])
    default = ops.poisson_rate(xd, Wd, bd, T=T, seed=SEED)
    named = ops.poisson_rate(xd, Wd, bd, T=T, seed=SEED, streams=list(range(N)), rows_per_stream=1)
    assert _same(default, named)
    # the last position below 2^31
    edge = ops.poisson_rate(xd[:2], Wd[:4].contiguous(), bd[:4].contiguous(), streams=[3], rows_per_stream=2,
                            start=(1 << 31) - 2, **kw)
    s, p = RULE.row_addresses(2, [3], 2, (1 << 31) - 2)
    assert np.array_equal(edge[2].cpu().numpy(), RULE.spikes_of(edge[1].cpu().numpy(), RULE.uniforms(4, T, s, p, SEED)))
    assert ops.poisson_rate(xd[:0], Wd, bd, T=T, seed=SEED).shape == (0, H)


def test_the_bridge_module_on_the_device(dev):
    from aura_snn_rag_amd.core.language_zone.spike_bridge import ContinuousToSpikeBridge
    torch.manual_seed(0)
    bridge = ContinuousToSpikeBridge(64, 100).to(dev)
    x = torch.randn(12, 64, device=dev, requires_grad=True)
    kw = dict(seed=5, streams=[1, 2, 3], rows_per_stream=4, start=2)
    train = bridge(x, **kw)
    rate = bridge.rate_code(x, **kw)
    assert train.shape == (12, 10, 100) and not rate.requires_grad and not train.requires_grad
    assert _same(rate, train.mean(dim=1))
    torch.manual_seed(3)
    old = bridge(x)
    torch.manual_seed(3)
    draw = torch.rand(12, 10, 100, device=dev)
    assert torch.equal(old, (draw < torch.sigmoid(bridge.proj(x)).unsqueeze(1)).float())
