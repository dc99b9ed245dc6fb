"""GPU tests of timestep STDP (``aura_stdp_update`` and everything above it) against the rule restated in NumPy
(tests/stdp_rule.py): traces in fp32 exactly as written, ``dW`` in fp64 from those traces, and the magnitude sum ``S``.

Tolerances (from the formats, not from a run): ``|dW_dev - dW_64| <= (2 B T + 8) 2^-24 S`` -- any summation order of the
``2 B T`` terms plus the operand and output scalings -- with ``dW_dev == 0`` exactly where ``S == 0``, and
``|W'_dev - W'_64| <= lr * that + 2^-23 max(|W|, |W'|)`` (the clamp is 1-Lipschitz: no element is excluded).  Final traces
are compared on the bits.

Shapes ``(B, T, I, O)``: (3, 5, 36, 68), (2, 1, 8, 8), (5, 16, 132, 264), (7, 64, 40, 72), (16, 16, 256, 192) -- ragged
tile edges both ways, T = 1, more than one 128-tile each way, a long T, and splits over the batch rows (asserted from
``aura_stdp_workspace_bytes``) -- each in fp32 and bf16 with levels 0..8 at densities 0.3 (pre) / 0.2 (post), decays
drawn from [0.5, 0.99], non-zero incoming traces; and (5, 16, 132, 264) with a time-invariant Gaussian ``pre``.  The
apply tests use lr = 0.5 (halved, by the rule's fp64 weights alone, while more than a tenth would end on a bound),
a = 0.01 / 0.012, W ~ N(0, 0.5) and bounds +-1, and assert that 2 % to 10 % of the fp64 weights end on a bound.  The known answers use B = 4 (the division is exact) so that two roundings of the trace and one of the
product remain: 2 ulp."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers
from tests import stdp_rule as R

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 36, 68), (2, 1, 8, 8), (5, 16, 132, 264), (7, 64, 40, 72), (16, 16, 256, 192)]
SPLITTING = (16, 16, 256, 192)
A_PLUS, A_MINUS, LR, W_MIN, W_MAX = 0.01, 0.012, 0.5, -1.0, 1.0
CASES = [(s, dt, False) for s in SHAPES for dt in ("f32", "bf16")] + [((5, 16, 132, 264), "f32", True),
                                                                      ((5, 16, 132, 264), "bf16", True)]


def _id(case):
    (B, T, I, O), dt, inv = case
    return f"B{B}-T{T}-I{I}-O{O}-{dt}" + ("-invariant" if inv else "")


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs and the rule's answers for one case, computed once and never modified."""
    (B, T, I, O), dt, inv = case
    rng = np.random.default_rng(sum(map(ord, _id(case))))               # a seed of the case's own, stable across runs
    if inv:
        pre = rng.standard_normal((B, I)).astype(np.float32)
        if dt == "bf16":
            pre = R.to_bf16_exact(pre)
        pre_full = R.expand_pre(pre, T)
    else:
        pre = pre_full = R.spikes(rng, (B, T, I), 0.3)
    post = R.spikes(rng, (B, T, O), 0.2)
    lam_pre, lam_post = (float(v) for v in rng.uniform(0.5, 0.99, 2))
    x0 = rng.random((B, I)).astype(np.float32)
    y0 = rng.random((B, O)).astype(np.float32)
    w = (0.5 * rng.standard_normal((O, I))).astype(np.float32)
    dw, s, xf, yf = R.rule(pre_full, post, lam_pre, lam_post, A_PLUS, A_MINUS, x0, y0)
    # lr: 0.5, halved until at most a tenth of the fp64 weights end on a bound (decided by the rule alone)
    lr = LR
    while True:
        w_new = R.apply(w, dw, lr, W_MIN, W_MAX)
        if np.mean((w_new == W_MIN) | (w_new == W_MAX)) <= 0.10 or lr < 1e-3:
            break
        lr = lr / 2
    for a in (pre, post, x0, y0, w, dw, s, xf, yf, w_new):
        a.setflags(write=False)
    return dict(B=B, T=T, I=I, O=O, inv=inv, pre=pre, post=post, x0=x0, y0=y0, w=w, dw=dw, s=s, xf=xf, yf=yf,
                w_new=w_new, lr=lr, kw=dict(lambda_pre=lam_pre, lambda_post=lam_post, a_plus=A_PLUS, a_minus=A_MINUS,
                                            lr=lr, w_min=W_MIN, w_max=W_MAX, pre_time_invariant=inv))


def _dev(a, dev, dt="f32"):
    t = torch.from_numpy(np.array(a)).to(dev)
    return t.bfloat16() if dt == "bf16" else t


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inputs(case, dev):
    c = _case(case)
    dt = case[1]
    return c, _dev(c["pre"], dev, dt), _dev(c["post"], dev, dt), _dev(c["x0"], dev), _dev(c["y0"], dev)


@functools.lru_cache(maxsize=None)
def _dw_only(case, dev):
    """The NO_APPLY call of a case: ``(dW, x, y)`` on the device, shared by the tests that compare with it."""
    from aura_snn_rag_amd import ops
    c, pre, post, x0, y0 = _inputs(case, dev)
    keep = pre.clone(), post.clone(), x0.clone(), y0.clone()
    dw = torch.full((c["O"], c["I"]), float("nan"), device=dev)
    x, y = ops.stdp_update(pre, post, x0, y0, None, dw, **c["kw"])
    torch.cuda.synchronize()
    for a, b in zip((pre, post, x0, y0), keep):
        assert torch.equal(a, b), "an input was written"
    return dw, x, y


def test_one_of_the_shapes_splits_over_batch_rows():
    from aura_snn_rag_amd import ops
    B, T, I, O = SPLITTING
    one = (O * I * 4 + 255) // 256 * 256
    got = {s: int(ops.lib().aura_stdp_workspace_bytes(*s)) for s in SHAPES}
    assert got[SPLITTING] >= 2 * O * I * 4 > one, got
    assert all(v >= s[2] * s[3] * 4 for s, v in got.items())
    assert int(ops.lib().aura_stdp_workspace_bytes(0, 1, 8, 8)) < 0


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dw_stays_within_the_bound_and_traces_are_exact(dev, case):
    c = _case(case)
    dw, x, y = _dw_only(case, dev)
    got = dw.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - c["dw"]), R.dw_bound(c["B"], c["T"], c["s"])
    zero = c["s"] == 0
    assert np.all(got[zero] == 0.0), "dW is not exactly zero where no term exists"
    frac = float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0
    print(f"{_id(case)}: max |dW - dW_64| / bound = {frac:.4f}; worst abs {err.max():.3e}")
    helpers.record_parity(f"stdp dW {_id(case)}", int((err <= bound).sum()), err.size, max_frac_of_bound=round(frac, 4))
    assert np.all(err <= bound), f"max fraction of the bound: {frac}"
    assert torch.equal(_bits(x), _bits(torch.from_numpy(np.array(c["xf"])))), "x trace bits"
    assert torch.equal(_bits(y), _bits(torch.from_numpy(np.array(c["yf"])))), "y trace bits"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_apply_stays_within_its_bound(dev, case):
    from aura_snn_rag_amd import ops
    c, pre, post, x0, y0 = _inputs(case, dev)
    on_bound = float(np.mean((c["w_new"] == W_MIN) | (c["w_new"] == W_MAX)))
    print(f"{_id(case)}: lr = {c['lr']}, {100 * on_bound:.2f} % of the fp64 weights end on a bound")
    assert 0.02 <= on_bound <= 0.10
    keep = pre.clone(), post.clone()
    w = _dev(c["w"], dev)
    dw = torch.full_like(w, float("nan"))
    x, y = ops.stdp_update(pre, post, x0, y0, w, dw, **c["kw"])
    got = w.cpu().numpy().astype(np.float64)
    err = np.abs(got - c["w_new"])
    bound = R.w_bound(c["B"], c["T"], c["s"], c["lr"], c["w"], c["w_new"])
    frac = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{_id(case)}: max |W' - W'_64| / bound = {frac:.4f}")
    assert np.all(err <= bound), f"max fraction of the bound: {frac}"
    assert got.min() >= W_MIN and got.max() <= W_MAX
    ref_dw, ref_x, ref_y = _dw_only(case, dev)
    assert torch.equal(_bits(dw), _bits(ref_dw)), "dw_out of an applying call differs from the NO_APPLY call"
    assert torch.equal(_bits(x), _bits(ref_x)) and torch.equal(_bits(y), _bits(ref_y))
    assert torch.equal(pre, keep[0]) and torch.equal(post, keep[1])
    # W alone (no dw_out) ends on the same bits
    w2 = _dev(c["w"], dev)
    ops.stdp_update(pre, post, x0, y0, w2, None, **c["kw"])
    assert torch.equal(_bits(w2), _bits(w))


@pytest.mark.parametrize("case", [((3, 5, 36, 68), "f32", False), ((7, 64, 40, 72), "bf16", False),
                                  ((5, 16, 132, 264), "f32", True)], ids=_id)
def test_T_runs_of_one_step_end_in_the_same_trace_bits(dev, case):
    from aura_snn_rag_amd import ops
    c, pre, post, x0, y0 = _inputs(case, dev)
    _, x_all, y_all = _dw_only(case, dev)
    x, y = x0, y0
    dw = torch.empty(c["O"], c["I"], device=dev)
    total = torch.zeros(c["O"], c["I"], device=dev, dtype=torch.float64)
    for t in range(c["T"]):
        p = pre if c["inv"] else pre[:, t:t + 1].contiguous()
        x, y = ops.stdp_update(p, post[:, t:t + 1].contiguous(), x, y, None, dw, **c["kw"])
        total += dw.double()
    assert torch.equal(_bits(x), _bits(x_all)) and torch.equal(_bits(y), _bits(y_all))
    # and the T one-step updates add up to the T-step update, each within its own bound (S adds up over the steps)
    err = np.abs(total.cpu().numpy() - c["dw"])
    assert np.all(err <= (2 * c["B"] * c["T"] + 8 * c["T"]) * R.U24 * c["s"] + 1e-300)
    # from zero traces too: None and explicit zeros are the same call
    a = ops.stdp_update(pre, post, None, None, None, dw, **c["kw"])
    first = dw.clone()
    b = ops.stdp_update(pre, post, torch.zeros_like(x0), torch.zeros_like(y0), None, dw, **c["kw"])
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert torch.equal(_bits(first), _bits(dw))


@pytest.mark.parametrize("t_pre,t_post,which", [(2, 5, "ltp"), (5, 2, "ltd"), (4, 4, "same")])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_known_answers(dev, t_pre, t_post, which, dt):
    from aura_snn_rag_amd import ops
    B, T, I, O, i, o = 4, 8, 8, 8, 3, 5
    lp, lq, ap, am = 0.9, 0.8, 0.75, 0.6
    pre = np.zeros((B, T, I), np.float32)
    post = np.zeros((B, T, O), np.float32)
    pre[1, t_pre, i] = 1.0
    post[1, t_post, o] = 1.0
    dw = torch.full((O, I), float("nan"), device=dev)
    ops.stdp_update(_dev(pre, dev, dt), _dev(post, dev, dt), None, None, None, dw, lambda_pre=lp, lambda_post=lq,
                    a_plus=ap, a_minus=am, lr=0.0, w_min=0.0, w_max=0.0)
    got = dw.cpu().numpy()
    f = lambda v: float(np.float32(v))
    want = {"ltp": f(ap) * f(lp) ** 3 / B, "ltd": -f(am) * f(lq) ** 3 / B, "same": f(ap) / B}[which]
    assert np.count_nonzero(got) == 1, got
    ulp = float(np.spacing(np.float32(abs(want))))
    print(f"{which} {dt}: got {got[o, i]!r}, want {want!r}, {abs(float(got[o, i]) - want) / ulp:.2f} ulp")
    assert abs(float(got[o, i]) - want) <= 2 * ulp
    if which == "same":
        assert float(got[o, i]) == want                               # a_plus / 4 exactly: no depression


def test_the_same_call_gives_the_same_bits(dev):
    from aura_snn_rag_amd import ops
    case = (SPLITTING, "f32", False)
    c, pre, post, x0, y0 = _inputs(case, dev)
    outs = []
    for _ in range(2):
        w = _dev(c["w"], dev)
        dw = torch.empty_like(w)
        x, y = ops.stdp_update(pre, post, x0, y0, w, dw, **c["kw"])
        outs.append((w, dw, x, y))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------- modules
def test_synapsis_leaves_the_weight_bits_of_the_direct_call(dev):
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.language_zone.synapsis import StdpState, Synapsis
    case = ((3, 5, 36, 68), "f32", False)
    c, pre, post, x0, y0 = _inputs(case, dev)
    torch.manual_seed(0)
    syn = Synapsis(c["I"], c["O"], enable_plasticity=True, stdp_lr=0.05, trace_decay=0.9, stdp_a_plus=0.5,
                   stdp_a_minus=0.6, stdp_bounds=(-0.4, 0.4)).to(dev)
    kw = dict(lambda_pre=0.9, lambda_post=0.9, a_plus=0.5, a_minus=0.6, lr=0.05, w_min=-0.4, w_max=0.4)
    w = syn.weight.detach().clone()
    dw = torch.empty_like(w)
    x, y = ops.stdp_update(pre, post, x0, y0, w, dw, **kw)
    version = syn.weight._version
    state, got_dw = syn.stdp_update(pre, post, StdpState(x0, y0), return_dw=True)
    assert isinstance(state, StdpState) and syn.weight._version > version and syn.weight.requires_grad
    assert torch.equal(_bits(syn.weight), _bits(w)) and torch.equal(_bits(got_dw), _bits(dw))
    assert torch.equal(_bits(state.x), _bits(x)) and torch.equal(_bits(state.y), _bits(y))
    assert not got_dw.requires_grad and float(syn.weight.detach().abs().max()) <= float(np.float32(0.4))
    # apply=False hands back the raw dW and leaves the weight alone
    before, version = syn.weight.detach().clone(), syn.weight._version
    _, raw = syn.stdp_update(pre, post, StdpState(x0, y0), apply=False, return_dw=True)
    assert torch.equal(syn.weight, before) and syn.weight._version == version and torch.equal(_bits(raw), _bits(dw))
    assert syn.stdp_update(pre, post)[1] is None
    with pytest.raises(ValueError):
        syn.stdp_update(pre, post, apply=False)


def test_snnffn_stdp_step_is_two_direct_calls_on_its_spikes(dev):
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.language_zone.gif_neuron import run_gif_loop
    from aura_snn_rag_amd.core.language_zone.snn_ffn import SNNFFN
    F = torch.nn.functional
    torch.manual_seed(3)
    plain = SNNFFN(32, 64, num_timesteps=4, L=8).to(dev).eval()
    torch.manual_seed(3)
    ffn = SNNFFN(32, 64, num_timesteps=4, L=8, plasticity=True).to(dev).eval()
    assert list(plain.state_dict()) == list(ffn.state_dict())
    for a, b in zip(plain.state_dict().values(), ffn.state_dict().values()):
        assert torch.equal(a, b)
    x = 3.0 * torch.randn(2, 3, 32, device=dev)
    with torch.no_grad():
        assert torch.equal(ffn(x), plain(x)), "forward changed with plasticity on"
        # the spikes of both layers, from the module's own pieces and the weights as they are now
        n1, n2 = ffn.neuron1, ffn.neuron2
        x1 = x.reshape(6, 32).contiguous()
        c1 = n1.currents(F.linear(x1, ffn.syn1.weight, ffn.syn1.bias))
        s1, _ = run_gif_loop(c1, None, decay=n1.decay, L=n1.L, alpha=n1.alpha, threshold=n1.threshold, T=4,
                             time_invariant=True)
        c2 = n2.currents(F.linear(s1.reshape(24, 64), ffn.syn2.weight, ffn.syn2.bias)).reshape(6, 4, 32)
        s2, _ = run_gif_loop(c2, None, decay=n2.decay, L=n2.L, alpha=n2.alpha, threshold=n2.threshold, T=4)
    assert float(s1.sum()) > 0 and float(s2.sum()) > 0, "the input drives no spikes: the test would check nothing"
    w1, w2 = ffn.syn1.weight.detach().clone(), ffn.syn2.weight.detach().clone()
    kw = dict(lambda_pre=0.95, lambda_post=0.95, a_plus=1.0, a_minus=1.05, lr=0.001, w_min=-10.0, w_max=10.0)
    st2 = ops.stdp_update(s1, s2, None, None, w2, **kw)
    st1 = ops.stdp_update(x1, s1, None, None, w1, pre_time_invariant=True, **kw)
    out, (state1, state2) = ffn.stdp_step(x)
    assert out.shape == (2, 3, 32) and torch.equal(out, s2.mean(dim=1).reshape(2, 3, 32))
    assert torch.equal(_bits(ffn.syn1.weight), _bits(w1)) and torch.equal(_bits(ffn.syn2.weight), _bits(w2))
    assert not torch.equal(ffn.syn1.weight, plain.syn1.weight) and not torch.equal(ffn.syn2.weight, plain.syn2.weight)
    assert torch.equal(_bits(state1.x), _bits(st1[0])) and torch.equal(_bits(state1.y), _bits(st1[1]))
    assert torch.equal(_bits(state2.x), _bits(st2[0])) and torch.equal(_bits(state2.y), _bits(st2[1]))
    assert state1.x.shape == (6, 32) and state1.y.shape == (6, 64) and state2.y.shape == (6, 32)
    # a second step carries the traces; the keys of the checkpoint stay what they were
    out2, (n1s, n2s) = ffn.stdp_step(x, (state1, state2))
    assert not torch.equal(n1s.x, state1.x) and list(plain.state_dict()) == list(ffn.state_dict())
    with pytest.raises(RuntimeError):
        plain.stdp_step(x)
