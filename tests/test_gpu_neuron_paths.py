"""GPU parity for every kernel instance that the inference entry points of csrc/aura_neuron.hip select (and the
grid-stride trip of the training kernels in csrc/aura_train.hip), against the CPU oracle.

tests/test_gpu_neurons.py has one parameter point per model; this file walks the dispatch instead: dtype, H % 4,
H % 8, L a power of two or not, the two GIF flags, 16-byte alignment, T % 4, T % 32, T > 128, partial tiles, more
work items than one grid pass, and the three AURA_NT_* switches.  DESIGN.md ("Neuron loops: which test reaches
which instance") lists the case that reaches each instance.

Every comparison is bit-exact (``torch.equal``) except AdEx's V and w, which keep the two bars of
``test_gpu_neurons.py::test_adex_nt``, and the BPTT gradients, which keep the bound of
``test_gpu_training.py::test_gif_bptt_matches_oracle`` and, beside it, the derived bound of the fp64 rule.

The mean over T is ``RNE_dtype(fp32 sum / T)``: what ``spikes.mean(dim=1)`` computes on the CPU
(tests/test_host_neuron_rules.py).  Section A drives row sums past 256, where a sum rounded to bf16 before the
division gives another result.
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import aura_oracle as O
from tests import neuron_path_cases as C
from tests import surrogate_rule as R
from tests.test_gpu_training import _close

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
GD = O.gif_decay()
IZH = (0.02, 0.2, -65.0, 8.0, 0.2)


def _gif(h, state, L, alpha, thr, decay, T, **flags):
    from aura_snn_rag_amd.core.language_zone.gif_neuron import run_gif_loop
    return run_gif_loop(h, state, decay=decay, L=L, alpha=alpha, threshold=thr, T=T, **flags)


# ---------------------------------------------------------------------------------------------------------
# A. fused mean past 256
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MEAN_CASES, ids=C.mean_case_id)
def test_fused_mean_past_256(dev, case):
    """``seq_rtc_kernel<.., MEAN_OUT>``: the fused T-mean is ``spikes.mean(dim=1)`` of the oracle, and of the
    kernel's own full-spike output, where row sums exceed 256 (the share of such cells is asserted on the CPU,
    test_host_neuron_rules.py::test_mean_cases_saturate).

    At the parent of this change the kernel rounded the sum to bf16 before dividing.  On an MI355X all eight
    bf16 cases failed there, in 20 to 49 cells each, and all eight fp32 cases passed."""
    dtype, ti, (rows, T, H, L), _ = case
    h, _, spikes = C.mean_case(case)
    args = (L, C.MEAN_ALPHA, C.MEAN_THRESHOLD, C.MEAN_DECAY, T)
    mean, _ = _gif(h.to(dev), None, *args, time_invariant=ti, mean_out=True)
    full, _ = _gif(h.to(dev), None, *args, time_invariant=ti)
    assert torch.equal(full.cpu(), spikes), "full-spike output differs from the oracle"
    want = spikes.mean(dim=1)
    bad = int((mean.cpu() != want).sum())
    print(f"\n[mean {C.mean_case_id(case)}] cells differing from spikes.mean(dim=1): {bad} of {want.numel()}")
    assert torch.equal(mean.cpu(), want), f"fused mean differs from the oracle's mean in {bad} cells"
    assert torch.equal(mean.cpu(), full.cpu().mean(dim=1)), "fused mean differs from the mean of the kernel's spikes"


# ---------------------------------------------------------------------------------------------------------
# B. GIF parameter points
# ---------------------------------------------------------------------------------------------------------
# instance: dtype and H pick the vector width (H 24: VEC 4 / 8, H 13: scalar); in bf16 at VEC 8, L picks POW2L.
# (dtype, H, L, alpha, threshold, decay, time_invariant, mean_out)
GIF_POINTS = [
    # <f32, 4>
    (F32, 24, 1, 0.0, 0.5, 1.0, False, False),
    (F32, 24, 3, 0.05, 1.0, 0.5, True, False),
    (F32, 24, 12, 0.05, 2.0, GD, False, True),
    (F32, 24, 16, 0.0, 1.0, 0.5, True, True),
    # <f32, 1>
    (F32, 13, 5, 0.05, 2.0, 1.0, False, False),
    (F32, 13, 16, 0.0, 1.0, GD, True, False),
    (F32, 13, 3, 0.05, 1.0, 0.5, False, True),
    (F32, 13, 12, 0.0, 0.5, GD, True, True),
    # <bf16, 8, POW2L>
    (BF16, 24, 1, 0.05, 2.0, 0.5, False, False),
    (BF16, 24, 1, 0.0, 1.0, GD, True, False),
    (BF16, 24, 16, 0.05, 1.0, 1.0, False, True),
    (BF16, 24, 16, 0.0, 0.5, GD, True, True),
    # <bf16, 8, !POW2L>
    (BF16, 24, 5, 0.05, 0.5, GD, False, False),
    (BF16, 24, 12, 0.0, 2.0, 1.0, True, False),
    (BF16, 24, 3, 0.05, 1.0, 0.5, False, True),
    (BF16, 24, 12, 0.05, 0.5, GD, True, True),
    # <bf16, 1> (always the !POW2L model)
    (BF16, 13, 12, 0.05, 1.0, GD, False, False),
    (BF16, 13, 5, 0.05, 0.5, 0.5, True, False),
    (BF16, 13, 3, 0.05, 0.5, 1.0, False, True),
    (BF16, 13, 16, 0.0, 2.0, 0.5, True, True),
]


def _gif_point_id(p):
    dtype, H, L, alpha, thr, decay, ti, mo = p
    return (f"{'f32' if dtype == F32 else 'bf16'}-H{H}-L{L}-a{alpha}-thr{thr}-d{decay:.3f}"
            f"{'-ti' if ti else ''}{'-mean' if mo else ''}")


def test_gif_points_cover_every_listed_value():
    pts = GIF_POINTS
    assert {p[2] for p in pts} == {1, 3, 5, 12, 16}
    assert {p[3] for p in pts} == {0.0, 0.05} and {p[4] for p in pts} == {0.5, 1.0, 2.0}
    assert {p[5] for p in pts} == {1.0, 0.5, GD}
    pow2 = lambda L: L & (L - 1) == 0
    inst = lambda p: (p[0], p[1] == 24, p[0] == BF16 and p[1] == 24 and pow2(p[2]))
    for want in ((F32, True, False), (F32, False, False), (BF16, True, True), (BF16, True, False),
                 (BF16, False, False)):
        flags = {(p[6], p[7]) for p in pts if inst(p) == want}
        assert flags == {(a, b) for a in (False, True) for b in (False, True)}, (want, flags)


@pytest.mark.parametrize("point", GIF_POINTS, ids=_gif_point_id)
def test_gif_parameter_points(dev, point):
    """rows 5, T 9 (two unrolled groups and a tail of one); random initial (v, theta); currents of 30 randn so
    that spikes of 0 and of L both occur and the +-2 L theta clamp binds; then a second call on the returned
    state."""
    dtype, H, L, alpha, thr, decay, ti, mo = point
    rows, T = 5, 9
    g = torch.Generator().manual_seed(H * 100 + L)
    h = (30 * torch.randn((rows, H) if ti else (rows, T, H), generator=g)).to(dtype)
    v0 = torch.randn(rows, H, generator=g).to(dtype)
    t0 = (0.5 + 1.5 * torch.rand(rows, H, generator=g)).to(dtype)
    full = h.unsqueeze(1).expand(rows, T, H).contiguous() if ti else h
    state_o, state_d = (v0, t0), (v0.to(dev), t0.to(dev))
    for call in range(2):
        rs, rv, rt = O.gif_run(full, *state_o, decay, L, alpha, thr)
        assert (rs == 0).any() and (rs == L).any(), "the input must produce both spike extremes"
        out, (v, th) = _gif(h.to(dev), state_d, L, alpha, thr, decay, T, time_invariant=ti, mean_out=mo)
        want = rs.mean(dim=1) if mo else rs
        assert torch.equal(out.cpu(), want), f"call {call}: output differs in {int((out.cpu() != want).sum())} cells"
        assert torch.equal(v.cpu(), rv), f"call {call}: v differs"
        assert torch.equal(th.cpu(), rt), f"call {call}: theta differs"
        state_o, state_d = (rv, rt), (v, th)


# ---------------------------------------------------------------------------------------------------------
# C. LIF per-channel constants
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("size", C.LIF_SIZES)
def test_lif_per_channel_constants(dev, dtype, size):
    """Every channel has its own beta and threshold (tests/test_host_neuron_rules.py shows that a wrong channel
    index changes the spikes of exactly these inputs): ``ops.lif_run``, the module's ``forward_sequence``, and
    its single-step ``forward`` with and without autograd recording."""
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.base.neuron import VectorizedLIFNeuron
    x, beta, thr = C.lif_case(size, dtype)
    B, T = C.LIF_B, C.LIF_T
    rs, rm = O.lif_run(x, torch.zeros(B, size, dtype=dtype), beta, thr)
    assert 0.05 < rs.float().mean().item() < 0.95

    xd, bd, td = x.to(dev), beta.to(dev), thr.to(dev)
    spikes, mem = torch.empty_like(xd), torch.zeros(B, size, device=dev, dtype=dtype)
    ops.lif_run(xd, spikes, mem, bd, td)
    assert torch.equal(spikes.cpu(), rs) and torch.equal(mem.cpu(), rm), "ops.lif_run"

    def module():
        lif = VectorizedLIFNeuron(size).to(dev).to(dtype)
        with torch.no_grad():
            lif.beta.copy_(bd)
            lif.threshold.copy_(td)
        return lif

    lif = module()
    s = lif.forward_sequence(xd)
    assert torch.equal(s.cpu(), rs) and torch.equal(lif.mem.cpu(), rm), "forward_sequence"
    for recording in (False, True):
        lif = module()
        mem_o = torch.zeros(B, size, dtype=dtype)
        for t in range(4):
            with torch.set_grad_enabled(recording):
                spk, m = lif(xd[:, t])
            assert spk.requires_grad == recording
            so, mem_o = O.lif_step(x[:, t], mem_o, beta, thr)
            assert torch.equal(spk.detach().cpu(), so) and torch.equal(m.detach().cpu(), mem_o), \
                f"forward, step {t}, recording={recording}"


# ---------------------------------------------------------------------------------------------------------
# D. second grid pass
# ---------------------------------------------------------------------------------------------------------
ONE_GRID_PASS = 2048 * 256      # rtc_grid / grid_for: at most 2048 blocks of 256 threads; the rest is grid-strided


def _tail_equal(got, want, what):
    """Last row and last channel first, so that a failure names the tail."""
    got = got.cpu()
    assert torch.equal(got[-1], want[-1]), f"{what}: last row differs"
    assert torch.equal(got[..., -1], want[..., -1]), f"{what}: last channel differs"
    assert torch.equal(got, want), f"{what}: differs in {int((got != want).sum())} cells"


@pytest.mark.parametrize("dtype,rows,H,vec", [(F32, 4100, 516, 4), (F32, 4099, 129, 1), (BF16, 4100, 1032, 8),
                                              (BF16, 4099, 129, 1)])
def test_second_grid_pass_gif(dev, dtype, rows, H, vec):
    T = 2
    assert rows * (H // vec) > ONE_GRID_PASS
    h = (3 * torch.randn(rows, T, H, generator=torch.Generator().manual_seed(H))).to(dtype)
    v0, t0 = O.gif_initial_state(rows, H, 1.0, dtype)
    rs, rv, rt = O.gif_run(h, v0, t0, GD, 8, 0.01, 1.0)
    assert rs[-1].sum() > 0
    out, (v, th) = _gif(h.to(dev), None, 8, 0.01, 1.0, GD, T)
    _tail_equal(out, rs, "spikes")
    _tail_equal(v, rv, "v")
    _tail_equal(th, rt, "theta")


def test_second_grid_pass_lif(dev):
    from aura_snn_rag_amd import ops
    B, T, size = 4099, 2, 129
    assert B * size > ONE_GRID_PASS
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, size, generator=g)
    beta = torch.linspace(0.5, 0.99, size)[torch.randperm(size, generator=g)]
    thr = torch.linspace(0.2, 1.5, size)[torch.randperm(size, generator=g)]
    rs, rm = O.lif_run(x, torch.zeros(B, size), beta, thr)
    assert rs[-1].sum() > 0
    spikes, mem = torch.empty(B, T, size, device=dev), torch.zeros(B, size, device=dev)
    ops.lif_run(x.to(dev), spikes, mem, beta.to(dev), thr.to(dev))
    _tail_equal(spikes, rs, "spikes")
    _tail_equal(mem, rm, "mem")


def test_second_grid_pass_izhikevich_btd(dev):
    from aura_snn_rag_amd import ops
    B, T, D = 4099, 2, 129
    assert B * D > ONE_GRID_PASS
    I = 20 * torch.rand(B, T, D, generator=torch.Generator().manual_seed(6))
    # one call from rest cannot spike in two steps: start near threshold instead
    v0 = -65.0 + 90.0 * torch.rand(B * D, generator=torch.Generator().manual_seed(7))
    u0 = 0.2 * v0
    flat, btd = O.flatten_seq(I)
    rs, rv, ru = O.izh_run(flat, v0, u0, *IZH)
    rs = O.unflatten_spikes(rs, btd)
    assert rs[-1].sum() > 0
    spikes, v, u = torch.empty(B, T, D, device=dev), v0.to(dev), u0.to(dev)
    ops.izh_run_btd(I.to(dev), spikes, v, u, *IZH)
    _tail_equal(spikes, rs, "spikes")
    _tail_equal(v.view(B, D), rv.view(B, D), "v")
    _tail_equal(u.view(B, D), ru.view(B, D), "u")


def test_second_grid_pass_gif_training(dev):
    """``gif_fwd_kernel<F32, 1>`` and ``gif_bwd_kernel<F32, 1>`` past one grid pass; gradients held to the bound of
    ``test_gif_bptt_matches_oracle`` (its ``_close``)."""
    from aura_snn_rag_amd.core.language_zone.gif_neuron import run_gif_loop_grad
    rows, T, H, L, alpha = 4099, 2, 129, 8, 0.01
    assert rows * H > ONE_GRID_PASS
    g = torch.Generator().manual_seed(8)
    h = torch.randn(rows, T, H, generator=g) * 3
    v0 = 0.4 * torch.randn(rows, H, generator=g)
    t0 = 1.0 + 0.3 * torch.rand(rows, H, generator=g)
    ws, wv, wt = (torch.randn(s, generator=g) for s in ((rows, T, H), (rows, H), (rows, H)))
    ho, vo, to = (x.clone().requires_grad_(True) for x in (h, v0, t0))
    s, v, th = O.gif_run_grad(ho, vo, to, GD, L, alpha, 1.0)
    ref = torch.autograd.grad((s * ws).sum() + (v * wv).sum() + (th * wt).sum(), [ho, vo, to])
    hd, vd, td = (x.to(dev).requires_grad_(True) for x in (h, v0, t0))
    sd, (vT, tT) = run_gif_loop_grad(hd, (vd, td), decay=GD, L=L, alpha=alpha, threshold=1.0)
    _tail_equal(sd.detach(), s.detach(), "spikes")
    _tail_equal(vT.detach(), v.detach(), "v")
    _tail_equal(tT.detach(), th.detach(), "theta")
    got = torch.autograd.grad((sd * ws.to(dev)).sum() + (vT * wv.to(dev)).sum() + (tT * wt.to(dev)).sum(),
                              [hd, vd, td])
    for a, b, name in zip(got, ref, ("g_h", "g_v0", "g_theta0")):
        assert b[-1].abs().sum() > 0
        assert _close(a[-1], b[-1]), f"{name}: last row: max err {(a[-1].cpu() - b[-1]).abs().max().item():.3e}"
        assert _close(a[..., -1], b[..., -1]), f"{name}: last channel"
        assert _close(a, b), f"{name}: max err {(a.cpu() - b).abs().max().item():.3e}"
    # beside ``_close``: every element within the derived bound of the fp64 rule (tests/surrogate_rule.py)
    fwd = R.gif_forward(h, v0, t0, GD, L, alpha, 1.0)
    bwd = R.gif_backward(fwd["save_a"], fwd["save_theta"], ws, wv, wt, GD, L, alpha, 1.0)
    for a, name in zip(got, ("g_h", "g_v0", "g_theta0")):
        worst = R.worst_ratio(a, bwd[name])
        assert worst <= 1.0, f"{name}: err / bound = {worst:.3f}"


# ---------------------------------------------------------------------------------------------------------
# E. alignment fallback
# ---------------------------------------------------------------------------------------------------------
def _shifted(t):
    """The same values in a contiguous view one element into a fresh buffer: never 16-byte aligned."""
    flat = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _alignment_case(dev, call, tensors, pointer_args, oracle, oracle_skips=(), order_free=(), check=None):
    """``call(**tensors)`` updates its tensors in place.  Run it on aligned tensors, then with each pointer
    argument shifted alone and with all of them shifted: every tensor afterwards is bit-equal to the aligned run,
    and (but for ``oracle_skips``) to the oracle.  ``order_free`` names tensors that float atomics fill (equal
    only within a bound): they are left out of the bit comparison and ``check(results, shift)`` judges them."""
    def run(shift):
        args = {k: t.to(dev).clone() for k, t in tensors.items()}
        for k in args:
            assert args[k].data_ptr() % 16 == 0
        for k in shift:
            args[k] = _shifted(args[k])
        call(**args)
        out = {k: t.cpu() for k, t in args.items()}
        if check is not None:
            check(out, shift)
        return out

    base = run(())
    for k, want in oracle.items():
        if k not in oracle_skips:
            assert torch.equal(base[k], want), f"aligned run: {k} differs from the oracle"
    for shift in [(k,) for k in pointer_args] + [tuple(pointer_args)]:
        got = run(shift)
        for k in tensors:
            if k in order_free:
                continue
            assert torch.equal(got[k], base[k]), f"shifted {shift}: {k} differs from the aligned run"
        for k, want in oracle.items():
            if k not in oracle_skips:
                assert torch.equal(got[k], want), f"shifted {shift}: {k} differs from the oracle"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_alignment_fallback_gif(dev, dtype):
    from aura_snn_rag_amd import ops
    rows, T, H, L = 5, 9, 24, 8
    g = torch.Generator().manual_seed(21)
    h = (3 * torch.randn(rows, T, H, generator=g)).to(dtype)
    v0 = torch.randn(rows, H, generator=g).to(dtype)
    t0 = (0.5 + 1.5 * torch.rand(rows, H, generator=g)).to(dtype)
    rs, rv, rt = O.gif_run(h, v0, t0, GD, L, 0.01, 1.0)
    assert rs.sum() > 0
    _alignment_case(dev, lambda h, out, v, theta: ops.gif_run(h, out, v, theta, GD, L, 0.01, 1.0, T),
                    dict(h=h, out=torch.zeros_like(h), v=v0, theta=t0), ("h", "out", "v", "theta"),
                    dict(out=rs, v=rv, theta=rt))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_alignment_fallback_lif(dev, dtype):
    from aura_snn_rag_amd import ops
    x, beta, thr = C.lif_case(96, dtype)
    mem0 = torch.zeros(C.LIF_B, 96, dtype=dtype)
    rs, rm = O.lif_run(x, mem0, beta, thr)
    _alignment_case(dev, lambda x, spikes, mem, beta, threshold: ops.lif_run(x, spikes, mem, beta, threshold),
                    dict(x=x, spikes=torch.zeros_like(x), mem=mem0, beta=beta, threshold=thr),
                    ("x", "spikes", "mem") + (("beta", "threshold") if dtype == BF16 else ()),
                    dict(spikes=rs, mem=rm))


def test_alignment_fallback_izhikevich_btd(dev):
    from aura_snn_rag_amd import ops
    B, T, D = 3, 50, 64
    I = 20 * torch.rand(B, T, D, generator=torch.Generator().manual_seed(22))
    v0, u0 = O.izh_initial_state(B * D, 0.2)
    flat, btd = O.flatten_seq(I)
    rs, rv, ru = O.izh_run(flat, v0, u0, *IZH)
    assert rs.sum() > 0
    _alignment_case(dev, lambda I, spikes, v, u: ops.izh_run_btd(I, spikes, v, u, *IZH),
                    dict(I=I, spikes=torch.zeros_like(I), v=v0, u=u0), ("I", "spikes", "v", "u"),
                    dict(spikes=O.unflatten_spikes(rs, btd).contiguous(), v=rv, u=ru))


def test_alignment_fallback_time_contiguous(dev):
    """(130, 100): aligned, the wave-tile form with LDS-DMA; shifted, ``seq_nt_kernel<., 1>``."""
    from aura_snn_rag_amd import ops
    N, T = 130, 100
    I = 20 * torch.rand(N, T, generator=torch.Generator().manual_seed(23))
    v0, u0 = O.izh_initial_state(N, 0.2)
    rs, rv, ru = O.izh_run(I, v0, u0, *IZH)
    assert rs.sum() > 0
    _alignment_case(dev, lambda I, spikes, v, u: ops.izh_run_nt(I, spikes, v, u, *IZH),
                    dict(I=I, spikes=torch.zeros_like(I), v=v0, u=u0), ("I", "spikes"),
                    dict(spikes=rs, v=rv, u=ru))
    p = O.adex_params(a=2.0, b=60.0)
    I = 600 * torch.rand(N, T, generator=torch.Generator().manual_seed(24))
    V0, w0 = torch.full((N,), float(p[1])), torch.zeros(N)
    rs, rV, rw = O.adex_run(I, V0, w0, p)
    assert rs.sum() > 0
    _alignment_case(dev, lambda I, spikes, V, w: ops.adex_run_nt(I, spikes, V, w, p.tolist()),
                    dict(I=I, spikes=torch.zeros_like(I), V=V0, w=w0), ("I", "spikes"),
                    dict(spikes=rs, V=rV, w=rw), oracle_skips=("V", "w"))


# ---------------------------------------------------------------------------------------------------------
# F. time-contiguous shapes
# ---------------------------------------------------------------------------------------------------------
# wave-tile form (T % 4 == 0, T % 32 != 0): T 4 and 12 are one and three float4 per row; 4, 12, 20 and 124 keep
# the row stride at T (LDS-DMA on whole tiles), 8, 40 and 72 pad it; 132 and 260 are 128-step chunks and a 4-step
# tail.  N 1 / 63 / 65 / 130 leave a partial tile, alone or after whole ones.
NTW_SHAPES = [(N, T) for T in (4, 8, 12, 20, 40, 72, 124, 132, 260) for N in (1, 63, 64, 65, 130)]
NT4_SHAPES = [(N, T) for T in (32, 96, 160) for N in (255, 257)]          # seq_nt_kernel<., 4>: T % 32 == 0
NT1_SHAPES = [(N, T) for T in (2, 3, 31, 35, 67) for N in (65, 257)]      # seq_nt_kernel<., 1>: T % 4 != 0


@pytest.mark.parametrize("N,T", NTW_SHAPES + NT4_SHAPES + NT1_SHAPES)
def test_izhikevich_time_contiguous_shapes(dev, N, T):
    from aura_snn_rag_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + T)
    I = 20 * torch.rand(N, T, generator=g)
    # short runs cannot reach the threshold from rest: start between rest and threshold
    state_o = (-65.0 + 90.0 * torch.rand(N, generator=g), -13.0 + 4.0 * torch.rand(N, generator=g))
    v, u = (s.to(dev) for s in state_o)
    Id, spikes = I.to(dev), torch.empty(N, T, device=dev)
    assert Id.data_ptr() % 16 == 0 and spikes.data_ptr() % 16 == 0
    total = 0
    for call in range(2):
        rs, rv, ru = O.izh_run(I, *state_o, *IZH)
        ops.izh_run_nt(Id, spikes, v, u, *IZH)
        got = spikes.cpu()
        assert torch.equal(got, rs), f"call {call}: spikes differ in {int((got != rs).sum())} cells; " \
                                     f"first at {tuple((got != rs).nonzero()[0].tolist())}"
        assert torch.equal(v.cpu(), rv) and torch.equal(u.cpu(), ru), f"call {call}: state differs"
        state_o = (rv, ru)
        total += int(rs.sum())
    assert total > 0 or N * T < 64


ADEX_SHAPES = [(130, 72), (65, 132), (257, 96), (63, 35)]


def test_adex_time_contiguous_shapes(dev):
    """Spike trains identical; V and w held to the two bars of ``test_adex_nt`` over the four cases pooled (one
    neuron caught mid-spike would decide a 63-neuron case alone)."""
    from aura_snn_rag_amd import ops
    p = O.adex_params(a=2.0, b=60.0)
    c5, c4 = [], []
    for N, T in ADEX_SHAPES:
        I = 600 * torch.rand(N, T, generator=torch.Generator().manual_seed(N + T))
        rs, rV, rw = O.adex_run(I, torch.full((N,), float(p[1])), torch.zeros(N), p)
        assert rs.sum() > 0
        spikes = torch.empty(N, T, device=dev)
        V, w = torch.full((N,), float(p[1]), device=dev), torch.zeros(N, device=dev)
        ops.adex_run_nt(I.to(dev), spikes, V, w, p.tolist())
        assert torch.equal(spikes.cpu(), rs), f"({N}, {T}): spike mismatch fraction " \
                                              f"{(spikes.cpu() != rs).float().mean().item()}"
        V, w = V.cpu(), w.cpu()
        c5.append(torch.isclose(V, rV, rtol=1e-5, atol=1e-5) & torch.isclose(w, rw, rtol=1e-5, atol=1e-5))
        c4.append(torch.isclose(V, rV, rtol=1e-4, atol=1e-4) & torch.isclose(w, rw, rtol=1e-4, atol=1e-3))
    s5, s4 = torch.cat(c5).float().mean().item(), torch.cat(c4).float().mean().item()
    print(f"\n[adex, {len(ADEX_SHAPES)} shapes pooled] within 1e-5: {s5:.4f}, within 1e-4: {s4:.4f}")
    assert s5 >= 0.995
    assert s4 >= 0.998


# ---------------------------------------------------------------------------------------------------------
# G. environment switches
# ---------------------------------------------------------------------------------------------------------
def test_time_contiguous_environment_switches(dev):
    """AURA_NT_LEGACY (the 32-step tiling at every T), AURA_NT_NO_DMA (register-staged loads) and
    AURA_NT_STORE_NT (non-temporal spike stores) are read once per process, so each runs in a fresh child, one
    at a time; the child compares with the oracle itself."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "neuron_env_child.py")
    for switch in ("AURA_NT_LEGACY", "AURA_NT_NO_DMA", "AURA_NT_STORE_NT"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("AURA_NT_")}
        env[switch] = "1"
        r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"{switch} OK" in r.stdout, \
            f"{switch}: exit {r.returncode}\n{r.stdout[-1500:]}{r.stderr[-1500:]}"
