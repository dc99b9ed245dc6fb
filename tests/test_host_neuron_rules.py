"""CPU controls for tests/test_gpu_neuron_paths.py: the rule the fused T-mean is held to, and proof that the
device tests' inputs can expose the faults they look for.

* The mean rule.  ``spikes.mean(dim=1)`` on the CPU (torch 2.10) is ``RNE_dtype(fp32 sum / T)`` and nothing else:
  the sum is NOT rounded to bf16 before the division, and the division is not a multiplication by ``1/T``.  Both
  rejected rules agree with torch while the spike total stays at or below 256 and T is a power of two -- which is
  all the older mean tests ever ran.  An older torch may have reduced differently; the rule is pinned here so that
  a change shows up on the CPU first.
* LIF control: rolling ``beta`` or ``threshold`` by one channel, or giving every channel the constants of channel
  0, changes the spikes of the LIF cases, so a kernel that indexes the constants wrongly cannot pass them.
* Saturation control: the GIF mean cases drive at least a tenth of their cells past a spike total of 256 that
  bf16 cannot hold, and in every bf16 case the rounded-sum rule gives another mean somewhere.
"""
import numpy as np
import pytest
import torch

from oracle import aura_oracle as O
from tests import neuron_path_cases as C

MEAN_T = (3, 7, 12, 33, 100)
MEAN_L = 8


def _spike_rows(total: int, T: int, H: int, L: int, dtype) -> torch.Tensor:
    """[1, T, H] integer spikes in 0..L whose sum over T is ``total`` in every channel; each channel puts its
    larger counts at other timesteps."""
    q, r = divmod(total, T)
    col = torch.full((T,), float(q))
    col[:r] += 1.0
    assert col.max() <= L and col.sum() == total
    return torch.stack([col.roll(c) for c in range(H)], dim=1).unsqueeze(0).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mean_over_time_is_one_rounding_of_the_fp32_quotient(dtype):
    cases = rejected_differs = 0
    for T in MEAN_T:
        totals = np.arange(T * MEAN_L + 1)
        for H in (1, 24):
            got = np.stack([C.bits(_spike_rows(int(n), T, H, MEAN_L, dtype).mean(dim=1))[0] for n in totals])
            want = C.mean_rule(totals, T, dtype)
            assert got.shape == (len(totals), H)
            wrong = np.nonzero((got != want[:, None]).any(axis=1))[0]
            assert wrong.size == 0, f"T={T} H={H}: torch's mean is not RNE(fp32 sum / T) at totals {wrong[:8]}"
            rejected = C.mean_rule_rounded_sum(totals, T) if dtype == torch.bfloat16 else \
                C.mean_rule_reciprocal(totals, T)
            differs = (got != rejected[:, None]).any(axis=1)
            if dtype == torch.bfloat16:
                assert not differs[totals <= 256].any(), "rounding the sum cannot matter while it is exact"
            rejected_differs += int(differs.sum())
            cases += len(totals)
    assert cases == 2 * 1245                            # every total 0..T*L, for H = 1 and H = 24
    # why the two other rules were rejected: each disagrees with torch somewhere in this set
    assert rejected_differs > 0
    print(f"\n[{dtype}] {cases} cases; the rejected rule differs from torch in {rejected_differs}")


def test_rejected_rule_example():
    """Total 301 over T = 100 in bf16: 3.01 rounds to 3.015625; 301 rounded to bf16 first is 300, giving 3.0."""
    got = _spike_rows(301, 100, 1, MEAN_L, torch.bfloat16).mean(dim=1)
    assert got.item() == 3.015625
    assert C.mean_rule(301, 100, torch.bfloat16) == C.bits(got).item()
    assert C.mean_rule_rounded_sum(301, 100) == C.bits(torch.tensor(3.0, dtype=torch.bfloat16)).item()


def test_reference_readout_on_a_saturated_bf16_case():
    """The reference's own readout line (``SNNFFN.forward``: ``spikes2.mean(dim=1)``) on spike totals past 256."""
    from oracle import _ref_loader
    if not _ref_loader.available():
        pytest.skip("reference checkout not present")
    ref = _ref_loader.load("core.language_zone.snn_ffn")
    T, D = 100, 24
    torch.manual_seed(0)
    ffn = ref.SNNFFN(D, 32, num_timesteps=T, L=8).eval()
    with torch.no_grad():
        ffn.neuron2.linear.bias.fill_(12.0)         # the drive of the device tests: currents around 12
    ffn = ffn.to(torch.bfloat16)
    seen = {}
    ffn.neuron2.register_forward_hook(lambda mod, args, out: seen.update(spikes=out[0]))
    with torch.no_grad():
        out = ffn(torch.randn(1, 8, D).to(torch.bfloat16))
    sums = C.cell_sums(seen["spikes"])
    assert ((sums > 256) & ~C.bf16_exact(sums)).any(), "the case must saturate"
    assert np.array_equal(C.bits(out.reshape(8, D)), C.mean_rule(sums, T, torch.bfloat16))
    assert not np.array_equal(C.bits(out.reshape(8, D)), C.mean_rule_rounded_sum(sums, T))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("size", C.LIF_SIZES)
def test_lif_cases_expose_a_wrong_channel_index(size, dtype):
    x, beta, thr = C.lif_case(size, dtype)
    assert beta.unique().numel() > size // 2 and thr.unique().numel() > size // 2
    mem0 = torch.zeros(C.LIF_B, size, dtype=dtype)
    true, _ = O.lif_run(x, mem0, beta, thr)
    for name, b, t in (("beta rolled", beta.roll(1), thr),
                       ("threshold rolled", beta, thr.roll(1)),
                       ("beta of channel 0", beta[:1].expand(size).contiguous(), thr),
                       ("threshold of channel 0", beta, thr[:1].expand(size).contiguous())):
        other, _ = O.lif_run(x, mem0, b, t)
        changed = (other != true).any(dim=0).any(dim=0)        # per channel
        print(f"\n[lif {size} {dtype}] {name}: spikes change in {int(changed.sum())} of {size} channels")
        assert changed.any(), f"{name}: the spikes do not change"


@pytest.mark.parametrize("case", C.MEAN_CASES, ids=C.mean_case_id)
def test_mean_cases_saturate(case):
    dtype, _, (rows, T, H, L), _ = case
    _, _, spikes = C.mean_case(case)
    sums = C.cell_sums(spikes)
    assert sums.shape == (rows, H) and sums.max() <= T * L
    saturated = (sums > 256) & ~C.bf16_exact(sums)
    assert saturated.mean() >= 0.10, f"only {saturated.mean():.1%} of the cells pass 256 with an inexact sum"
    assert np.array_equal(C.bits(spikes.mean(dim=1)), C.mean_rule(sums, T, dtype)), "the oracle's mean is the rule"
    if dtype == torch.bfloat16:
        differs = C.mean_rule_rounded_sum(sums, T) != C.bits(spikes.mean(dim=1))
        assert differs.any(), "the rounded-sum rule must give another mean in at least one cell"
