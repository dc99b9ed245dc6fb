"""The surrogate-gradient training kernels of csrc/aura_train.hip and ``aura_addition_linear_backward``, op by op
through ``aura_snn_rag_amd.ops``, against tests/surrogate_rule.py (anchored in the oracle on the same tensors by
tests/test_host_surrogate_rule.py).

Forward: spikes, state, ``save_a``, ``save_theta`` and ``pre`` are bit-equal to the rule's forward.  Backward:
EVERY element lies within the bound derived in the rule's docstring, ``gamma_K M`` (plus one rounding for a bf16
output); nothing is left out.  Output buffers are pre-filled with NaN; ``g_gains`` once with zeros and once with a
known pattern (the kernel accumulates into it).  On the hand-made decision points the device equals the rule bit
for bit.  The measured maximum of err / bound of every case is recorded through ``helpers.record_parity``
(``over_half_bound`` flags a maximum above 0.5) and kept in profiles/surrogate_parity.json.

DESIGN.md ("Neuron loops: which test reaches which instance") names the case that reaches each instantiation."""
import pytest
import torch

from tests import helpers
from tests import surrogate_cases as C
from tests import surrogate_rule as R
from tests.test_gpu_neuron_paths import _alignment_case

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _ratio(got, rule, out_dtype):
    """max over every element of err / bound (NaN counts as infinite)."""
    return R.worst_ratio(got, rule, out_dtype=out_dtype)


def _record_and_assert(name, worst):
    """worst: {output: max err / bound}.  Recorded first, so that a failing run leaves its figures behind."""
    top = max(worst.values()) if worst else 0.0
    helpers.record_parity(f"surrogate {name}", int(top <= 1.0), 1, max_frac_of_bound=round(top, 4),
                          over_half_bound=bool(top > 0.5), **{k: round(v, 4) for k, v in worst.items()})
    print(f"\n[surrogate {name}] " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"{name}: {k}: err / bound = {v:.3f}"


def _opt(t, dev):
    return None if t is None else t.to(dev)


def _gif_forward(kind, t, cfg, dev):
    """cfg = (decay, L, alpha, thr0, strength).  Returns dict(spikes, v, theta, save_a, save_theta) on the device."""
    from aura_snn_rag_amd import ops
    decay, L, alpha, thr0, strength = cfg
    h = t["h"].to(dev)
    out = dict(spikes=_nan(h.shape, h.dtype, dev), save_a=_nan(h.shape, h.dtype, dev),
               save_theta=_nan(h.shape, h.dtype, dev), v=t["v0"].to(dev).clone(), theta=t["t0"].to(dev).clone())
    if kind == "gif":
        ops.gif_train_forward(h, out["spikes"], out["v"], out["theta"], out["save_a"], out["save_theta"], decay, L,
                              alpha, thr0)
    else:
        ops.gif_prosody_train_forward(h, _opt(t["gains"], dev), out["spikes"], out["v"], out["theta"], out["save_a"],
                                      out["save_theta"], decay, L, alpha, thr0, strength)
    return out


def _gif_backward(kind, t, cfg, save_a, save_theta, dev, g_gains=None):
    from aura_snn_rag_amd import ops
    decay, L, alpha, thr0, strength = cfg
    out = dict(g_h=_nan(save_a.shape, save_a.dtype, dev), g_v0=t["wv"].to(dev).clone(),
               g_theta0=t["wt"].to(dev).clone())
    if kind == "gif":
        ops.gif_backward(save_a, save_theta, t["ws"].to(dev), out["g_h"], out["g_v0"], out["g_theta0"], decay, L,
                         alpha, thr0)
    else:
        gains = _opt(t["gains"], dev)
        if gains is not None:
            out["g_gains"] = torch.zeros(gains.shape, device=dev) if g_gains is None else g_gains.to(dev).clone()
        ops.gif_prosody_backward(save_a, save_theta, t["h"].to(dev), gains, t["ws"].to(dev), out["g_h"],
                                 out.get("g_gains"), out["g_v0"], out["g_theta0"], decay, L, alpha, thr0, strength)
    return out


def _assert_forward(got, fwd, what):
    for k in ("spikes", "v", "theta", "save_a", "save_theta"):
        g, w = got[k].cpu(), fwd[k]
        assert torch.equal(g[-1:], w[-1:]), f"{what}: {k}: last row differs"
        assert torch.equal(g, w), f"{what}: {k} differs in {int((g != w).sum())} cells"


def _cfg(c):
    return (C.DECAY, c.L, c.alpha, C.THR0, C.STRENGTH)


def _out_dtype(k, dtype):
    return F32 if k == "g_gains" else dtype


# ---------------------------------------------------------------------------------------------------------
# A. every entry point x dtype x vector width; T = 1, alpha = 0, L = 1 / 2 / 16 / 256; second grid pass
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.SMALL_CASES + C.BIG_CASES, ids=C.case_id)
def test_gif_train_forward_and_backward(dev, c):
    """{GIF, prosody GIF with gains, without} x {fp32, bf16}: H 24 is the vector instance, H 13 the scalar one,
    H 20 the vector one in fp32 and the scalar one in bf16; 4100 rows x H 129 / 516 / 1032 at T = 1 are more
    work items than one grid pass (2048 blocks of 256) for the scalar, VEC 4 and VEC 8 instance."""
    if c in C.BIG_CASES:
        assert c.rows * (c.H // C.vec_width(c)) > C.ONE_GRID_PASS
    t, fwd, bwd = C.gif_case(c)
    got = _gif_forward(c.kind, t, _cfg(c), dev)
    _assert_forward(got, fwd, c.name)
    out = _gif_backward(c.kind, t, _cfg(c), got["save_a"], got["save_theta"], dev)
    assert set(out) == {k for k, v in bwd.items() if v is not None}
    worst = {k: _ratio(out[k], bwd[k], _out_dtype(k, c.dtype)) for k in out}
    if "g_gains" in out and c in C.SMALL_CASES:
        # the kernel accumulates into g_gains: a known pattern in the buffer is added to, not overwritten
        pattern = 0.5 + torch.arange(c.rows * c.T, dtype=F32).view(c.rows, c.T)
        out2 = _gif_backward(c.kind, t, _cfg(c), got["save_a"], got["save_theta"], dev, g_gains=pattern)
        want, M, K = bwd["g_gains"]
        worst["g_gains_accumulated"] = _ratio(out2["g_gains"], (want + pattern.double(), M + pattern.double().abs(), K), F32)
        for k in ("g_h", "g_v0", "g_theta0"):
            assert torch.equal(out2[k], out[k]), f"{k} depends on what g_gains held"
    _record_and_assert(c.name, worst)


# ---------------------------------------------------------------------------------------------------------
# B. decision points
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,gains", [("gif", False), ("prosody", False), ("prosody", True)])
def test_decision_points_bit_equal_on_the_device(dev, kind, gains):
    """a == +-cl and just beyond, n == 0 / -0 / 3 / 2.5 / L + 1 and just above, the scale clamp at raw == 0.5 and
    1.5 and their neighbours, T == 1 (test_host_surrogate_rule.py counts the points and shows the oracle's
    autograd bit-equal to the rule on them).  On the rows whose effective threshold is a power of two every
    operation is exact: the device equals the rule bit for bit.  The other rows are held to the bound."""
    t, fwd, bwd = C.decision_rule(kind, gains)
    cfg = C.decision_case(kind, gains)[1]
    got = _gif_forward(kind, t, cfg, dev)
    _assert_forward(got, fwd, f"decision {kind}")
    out = _gif_backward(kind, t, cfg, got["save_a"], got["save_theta"], dev)
    exact = C.DP_EXACT_ROWS if gains else [0]
    worst = {}
    for k in out:
        want = bwd[k][0].float()
        g = out[k].cpu()
        assert torch.equal(g[exact], want[exact]), f"{k}: device and rule differ on the exact rows:\n{g[exact]}\n{want[exact]}"
        worst[k] = _ratio(out[k], bwd[k], F32)
    _record_and_assert(f"decision-{kind}{'-gains' if gains else ''}", worst)


# ---------------------------------------------------------------------------------------------------------
# C. 16-byte misalignment: the scalar fall-back at a vector shape
# ---------------------------------------------------------------------------------------------------------
ALIGN_CASES = [c for c in C.INSTANCE_CASES if c.H == 24]


@pytest.mark.parametrize("c", ALIGN_CASES, ids=C.case_id)
def test_alignment_fallback_training(dev, c):
    """Each pointer argument shifted off 16 bytes alone, then all of them: bit-equal to the aligned run (and the
    forward to the rule); ``g_gains``, filled by float atomics in no fixed order, within its bound."""
    from aura_snn_rag_amd import ops
    assert C.vec_width(c) > 1
    t, fwd, bwd = C.gif_case(c)
    decay, L, alpha, thr0, strength = _cfg(c)
    mod = t["gains"] is not None
    blank = torch.zeros_like(t["h"])

    if c.kind == "gif":
        call = lambda h, spikes, v, theta, save_a, save_theta: ops.gif_train_forward(
            h, spikes, v, theta, save_a, save_theta, decay, L, alpha, thr0)
    else:
        call = lambda h, spikes, v, theta, save_a, save_theta, gains=None: ops.gif_prosody_train_forward(
            h, gains, spikes, v, theta, save_a, save_theta, decay, L, alpha, thr0, strength)
    tensors = dict(h=t["h"], spikes=blank, v=t["v0"], theta=t["t0"], save_a=blank, save_theta=blank)
    if mod:
        tensors["gains"] = t["gains"]
    _alignment_case(dev, call, tensors, tuple(tensors), {k: fwd[k] for k in ("spikes", "v", "theta", "save_a", "save_theta")})

    def check(res, shift):
        for k in ("g_h", "g_v", "g_theta") + (("g_gains",) if mod else ()):
            name = {"g_v": "g_v0", "g_theta": "g_theta0"}.get(k, k)
            r = _ratio(res[k], bwd[name], _out_dtype(k, c.dtype))
            assert r <= 1.0, f"shifted {shift}: {k}: err / bound = {r:.3f}"

    if c.kind == "gif":
        call = lambda save_a, save_theta, g_spikes, g_h, g_v, g_theta: ops.gif_backward(
            save_a, save_theta, g_spikes, g_h, g_v, g_theta, decay, L, alpha, thr0)
        tensors = dict(save_a=fwd["save_a"], save_theta=fwd["save_theta"], g_spikes=t["ws"], g_h=blank, g_v=t["wv"],
                       g_theta=t["wt"])
    else:
        call = lambda save_a, save_theta, h, g_spikes, g_h, g_v, g_theta, gains=None, g_gains=None: \
            ops.gif_prosody_backward(save_a, save_theta, h, gains, g_spikes, g_h, g_gains, g_v, g_theta, decay, L,
                                     alpha, thr0, strength)
        tensors = dict(save_a=fwd["save_a"], save_theta=fwd["save_theta"], h=t["h"], g_spikes=t["ws"], g_h=blank,
                       g_v=t["wv"], g_theta=t["wt"])
        if mod:
            tensors.update(gains=t["gains"], g_gains=torch.zeros(c.rows, c.T))
    _alignment_case(dev, call, tensors, tuple(tensors), {}, order_free=("g_gains",), check=check)


# ---------------------------------------------------------------------------------------------------------
# D. limits
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gif", "prosody"])
def test_bf16_refuses_L_above_256(dev, kind):
    """Spike counts up to 256 are exact in bf16: L = 256 runs (section A), L = 257 is AURA_E_INVAL."""
    from aura_snn_rag_amd._lib import AuraHipError
    c = [x for x in C.EDGE_CASES if x.L == 256 and x.kind == kind][0]
    t, fwd, _ = C.gif_case(c)
    cfg = (C.DECAY, 257, c.alpha, C.THR0, C.STRENGTH)
    with pytest.raises(AuraHipError, match="AURA_E_INVAL"):
        _gif_forward(kind, t, cfg, dev)
    with pytest.raises(AuraHipError, match="AURA_E_INVAL"):
        _gif_backward(kind, t, cfg, fwd["save_a"].to(dev), fwd["save_theta"].to(dev), dev)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,H", [(0, 8), (3, 0)])
def test_empty_shapes_touch_nothing(dev, dtype, rows, H):
    from aura_snn_rag_amd import ops
    T = 2
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)
    gains, g_gains = torch.full((rows, T), 1.5, dtype=dtype, device=dev), torch.full((rows, T), 7.0, device=dev)
    ops.gif_train_forward(z(rows, T, H), z(rows, T, H), z(rows, H), z(rows, H), z(rows, T, H), z(rows, T, H),
                          C.DECAY, 8, 0.05, 1.0)
    ops.gif_backward(z(rows, T, H), z(rows, T, H), z(rows, T, H), z(rows, T, H), z(rows, H), z(rows, H), C.DECAY, 8,
                     0.05, 1.0)
    ops.gif_prosody_train_forward(z(rows, T, H), gains, z(rows, T, H), z(rows, H), z(rows, H), z(rows, T, H),
                                  z(rows, T, H), C.DECAY, 8, 0.05, 1.0, 0.3)
    ops.gif_prosody_backward(z(rows, T, H), z(rows, T, H), z(rows, T, H), gains, z(rows, T, H), z(rows, T, H), g_gains,
                             z(rows, H), z(rows, H), C.DECAY, 8, 0.05, 1.0, 0.3)
    assert bool((g_gains == 7.0).all()), "g_gains touched"
    ops.lif_train_forward(z(rows, H), z(rows, H), z(H), z(H), z(rows, H), z(rows, H), z(rows, H))
    ops.lif_backward(z(rows, H), z(rows, H), z(rows, H), z(H), z(H), z(H), z(rows, H), z(rows, H),
                     torch.zeros(rows, H, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# E. LIF step
# ---------------------------------------------------------------------------------------------------------
def _lif_ops(t, dev):
    from aura_snn_rag_amd import ops
    d = {k: v.to(dev) for k, v in t.items()}
    dt, shape = t["x"].dtype, t["x"].shape
    fwd = dict(spikes=_nan(shape, dt, dev), mem=_nan(shape, dt, dev), pre=_nan(shape, dt, dev))
    ops.lif_train_forward(d["x"], d["mem"], d["beta"], d["thr"], fwd["spikes"], fwd["mem"], fwd["pre"])
    bwd = dict(g_x=_nan(shape, dt, dev), g_mem_prev=_nan(shape, dt, dev), raw_slope=_nan(shape, F32, dev))
    ops.lif_backward(fwd["pre"], d["g_spk"], d["g_mem"], d["beta"], d["thr"], d["slope"], bwd["g_x"],
                     bwd["g_mem_prev"], bwd["raw_slope"])
    return fwd, bwd


@pytest.mark.parametrize("case", C.LIF_CASES + C.LIF_BIG_CASES, ids=C.case_id)
def test_lif_train_forward_and_backward(dev, case):
    """{fp32, bf16} x sizes 24 (vector), 13 (scalar), 20 (vector in fp32, scalar in bf16), 4; B 4100 x 129 / 516 /
    1032 past one grid pass."""
    dtype, B, size = case
    t, fwd, bwd = C.lif_case(*case)
    got, out = _lif_ops(t, dev)
    for k in ("spikes", "mem", "pre"):
        assert torch.equal(got[k].cpu(), fwd[k]), f"{k} differs in {int((got[k].cpu() != fwd[k]).sum())} cells"
    worst = {k: _ratio(out[k], bwd[k], F32 if k == "raw_slope" else dtype) for k in out}
    _record_and_assert(f"lif-{C.case_id(case)}", worst)


def test_lif_decision_points_bit_equal_on_the_device(dev):
    """pre == 0 (sign 0: no slope gradient), one ulp on either side of it, and +-1."""
    t, fwd, bwd = C.lif_decision_case()
    got, out = _lif_ops(t, dev)
    for k in ("spikes", "mem", "pre"):
        assert torch.equal(got[k].cpu(), fwd[k]), k
    exact = fwd["pre"].abs() != 1.0
    for k in out:
        assert torch.equal(out[k].cpu()[exact], bwd[k][0].float()[exact]), k
    assert bool((out["raw_slope"].cpu()[fwd["pre"] == 0] == 0).all())
    _record_and_assert("lif-decision", {k: _ratio(out[k], bwd[k], F32) for k in out})


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_alignment_fallback_lif_training(dev, dtype):
    from aura_snn_rag_amd import ops
    t, fwd, bwd = C.lif_case(dtype, 5, 24)
    blank = torch.zeros_like(t["x"])
    _alignment_case(dev, lambda x, mem_in, beta, threshold, spikes, mem_out, pre: ops.lif_train_forward(
                        x, mem_in, beta, threshold, spikes, mem_out, pre),
                    dict(x=t["x"], mem_in=t["mem"], beta=t["beta"], threshold=t["thr"], spikes=blank, mem_out=blank,
                         pre=blank),
                    ("x", "mem_in", "beta", "threshold", "spikes", "mem_out", "pre"),
                    dict(spikes=fwd["spikes"], mem_out=fwd["mem"], pre=fwd["pre"]))

    def check(res, shift):
        for k in ("g_x", "g_mem_prev", "raw_slope"):
            r = _ratio(res[k], bwd[k], F32 if k == "raw_slope" else dtype)
            assert r <= 1.0, f"shifted {shift}: {k}: err / bound = {r:.3f}"

    _alignment_case(dev, lambda pre, g_spikes, g_mem, beta, threshold, slope, g_x, g_mem_prev, raw_slope:
                    ops.lif_backward(pre, g_spikes, g_mem, beta, threshold, slope, g_x, g_mem_prev, raw_slope),
                    dict(pre=fwd["pre"], g_spikes=t["g_spk"], g_mem=t["g_mem"], beta=t["beta"], threshold=t["thr"],
                         slope=t["slope"], g_x=blank, g_mem_prev=blank, raw_slope=torch.zeros(5, 24)),
                    ("pre", "g_spikes", "g_mem", "beta", "threshold", "slope", "g_x", "g_mem_prev", "raw_slope"),
                    {}, check=check)


# ---------------------------------------------------------------------------------------------------------
# F. AdditionLinear backward
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,IN,OUT", C.ADDLIN_SHAPES)
def test_addition_linear_backward(dev, B, IN, OUT):
    """Shapes around the 64 x 64 x 32 tiling; ``need_x`` / ``need_w`` alone and together (both roles of
    ``addition_linear_bwd_kernel``); a block of exact ties with x = +0 against w = -0; bound
    ``(T + 2) 2^-24 sum|g|`` over the reduction length T on every element."""
    from aura_snn_rag_amd import ops
    x, w, g = C.addition_linear_case(B, IN, OUT)
    rule = R.addition_linear_backward(x, w, g)
    xd, wd, gd = x.to(dev), w.to(dev), g.to(dev)
    gx, gw = ops.addition_linear_backward(xd, wd, gd)
    gx1, none_w = ops.addition_linear_backward(xd, wd, gd, need_x=True, need_w=False)
    none_x, gw1 = ops.addition_linear_backward(xd, wd, gd, need_x=False, need_w=True)
    assert none_w is None and none_x is None
    assert torch.equal(gx1, gx) and torch.equal(gw1, gw), "one role alone differs from both together"
    worst = {}
    for k, got in (("g_x", gx), ("g_w", gw)):
        want, bnd = rule[k]
        err = (got.cpu().double() - want).abs()
        worst[k] = float(torch.where(err > 0, err / bnd, torch.zeros_like(err)).max())
    ties = x.unsqueeze(1) == w.unsqueeze(0)
    assert float(gx.cpu()[0, 0]) == 0.0 and bool(ties[0, :, 0].all()), "+0 against -0 is a tie for every template"
    _record_and_assert(f"addition-linear-{B}x{IN}x{OUT}", worst)


def test_addition_linear_backward_empty_batch(dev):
    """B = 0: no input gradient to compute, and a g_w of zeros."""
    from aura_snn_rag_amd import ops
    w = torch.randn(5, 7, device=dev)
    gx, gw = ops.addition_linear_backward(torch.empty(0, 7, device=dev), w, torch.empty(0, 5, device=dev))
    assert gx.shape == (0, 7) and torch.equal(gw, torch.zeros_like(w))


# ---------------------------------------------------------------------------------------------------------
# G. the autograd Functions hand the ops what they document
# ---------------------------------------------------------------------------------------------------------
def _hook_currents(linear):
    """Keep the linear layer's output (the device's own currents) and its gradient."""
    kept = {}

    def hook(_, __, out):
        out.retain_grad()
        kept["h"] = out
    return kept, linear.register_forward_hook(hook)


def test_gif_module_hands_the_op_contiguous_gradients(dev):
    """``v.sum()`` hands ``GifLoopFunction.backward`` an expanded (stride 0) gradient: g_h of the module equals the
    rule fed the device's own currents."""
    from aura_snn_rag_amd.core.language_zone.gif_neuron import GIFNeuron
    torch.manual_seed(3)
    B, T, I, H, L, alpha = 4, 6, 16, 20, 8, 0.05
    n = GIFNeuron(I, H, L=L, alpha=alpha).to(dev)
    kept, handle = _hook_currents(n.linear)
    x = torch.randn(B, T, I, device=dev) * 3
    ws, wt = torch.randn(B, T, H), torch.randn(B, H)
    s, (v, th) = n(x)
    handle.remove()
    ((s * ws.to(dev)).sum() + v.sum() + (th * wt.to(dev)).sum()).backward()
    h = kept["h"].detach().cpu()
    fwd = R.gif_forward(h, torch.zeros(B, H), torch.full((B, H), float(n.threshold)), n.decay, L, alpha, n.threshold)
    assert torch.equal(s.detach().cpu(), fwd["spikes"]) and torch.equal(v.detach().cpu(), fwd["v"])
    bwd = R.gif_backward(fwd["save_a"], fwd["save_theta"], ws, torch.ones(B, H), wt, n.decay, L, alpha, n.threshold)
    _record_and_assert("module-gif", {"g_h": _ratio(kept["h"].grad, bwd["g_h"], F32)})


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_prosody_module_zeroes_and_casts_g_gains(dev, dtype):
    """Two backward passes through ``ProsodyGifFunction`` give the same ``gains.grad`` contribution each (the fp32
    buffer is zeroed per call), in the gains' dtype; every gradient equals the rule fed the device's currents."""
    from aura_snn_rag_amd.core.language_zone.prosody_gif import ProsodyModulatedGIF
    torch.manual_seed(4)
    B, T, I, H, L, alpha, strength = 4, 6, 16, 24, 8, 0.05, 0.3
    pg = ProsodyModulatedGIF(I, H, L=L, alpha=alpha, attention_modulation_strength=strength).to(dev).to(dtype)
    kept, handle = _hook_currents(pg.linear)
    x = (torch.randn(B, T, I) * 3).to(dtype).to(dev)
    t = dict(gains=(0.2 + 3.0 * torch.rand(B, T)).to(dtype), v0=(0.4 * torch.randn(B, H)).to(dtype),
             t0=(1.0 + 0.3 * torch.rand(B, H)).to(dtype), ws=torch.randn(B, T, H).to(dtype), wt=torch.randn(B, H).to(dtype))
    leaves = {k: t[k].to(dev).requires_grad_(True) for k in ("gains", "v0", "t0")}
    first = None
    for _ in range(2):
        s, (v, th) = pg(x, state=(leaves["v0"], leaves["t0"]), attention_gains=leaves["gains"])
        ((s * t["ws"].to(dev)).sum() + v.sum() + (th * t["wt"].to(dev)).sum()).backward()
        if first is None:
            first = leaves["gains"].grad.clone()
            g_h = kept["h"].grad.clone()
    handle.remove()
    assert leaves["gains"].grad.dtype == dtype
    if dtype == F32:
        # the second pass added its own contribution: the same one but for the order of the float atomics
        second = leaves["gains"].grad - first
    h = kept["h"].detach().cpu()
    fwd = R.gif_forward(h, t["v0"], t["t0"], pg.decay, L, alpha, pg.threshold, gains=t["gains"], strength=strength,
                        prosody=True)
    assert torch.equal(s.detach().cpu(), fwd["spikes"]) and torch.equal(th.detach().cpu(), fwd["theta"])
    bwd = R.gif_backward(fwd["save_a"], fwd["save_theta"], t["ws"], torch.ones(B, H, dtype=dtype), t["wt"], pg.decay,
                         L, alpha, pg.threshold, h=h, gains=t["gains"], strength=strength, prosody=True)
    worst = {"g_h": _ratio(g_h, bwd["g_h"], dtype), "g_gains": _ratio(first, bwd["g_gains"], dtype)}
    if dtype == F32:
        want, M, K = bwd["g_gains"]
        # (first + second) - first rounds twice more, relative to the doubled magnitude
        worst["g_gains_second_pass"] = _ratio(second, (want, 3 * M, K + 2), F32)
    _record_and_assert(f"module-prosody-{'f32' if dtype == F32 else 'bf16'}", worst)


def test_lif_module_slope_gradient_is_the_batch_sum(dev):
    from aura_snn_rag_amd.base.neuron import VectorizedLIFNeuron
    dtype, B, size = F32, 7, 13
    t, fwd, bwd = C.lif_case(dtype, B, size)
    lif = VectorizedLIFNeuron(size).to(dev)
    with torch.no_grad():
        lif.beta.copy_(t["beta"]); lif.threshold.copy_(t["thr"]); lif.slope.copy_(t["slope"])
    lif.mem = t["mem"].to(dev).requires_grad_(True)
    x = t["x"].to(dev).requires_grad_(True)
    spk, mem = lif(x)
    assert torch.equal(spk.detach().cpu(), fwd["spikes"]) and torch.equal(mem.detach().cpu(), fwd["mem"])
    gx, gs = torch.autograd.grad((spk * t["g_spk"].to(dev)).sum() + (mem * t["g_mem"].to(dev)).sum(), [x, lif.slope])
    _record_and_assert("module-lif", {"g_x": _ratio(gx, bwd["g_x"], F32), "slope_sum": _ratio(gs, bwd["slope_sum"], F32)})
