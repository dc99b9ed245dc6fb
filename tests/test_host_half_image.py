"""The half image's conversion rule on the CPU (tests/half_image_rule.py, the host model the GPU tests compare the
kernels' bits with): ties to even, everything below 2^-14 stored as +0, no subnormal pattern, 65504 out of reach, and
the residual bound the two-stage recall relies on."""
import numpy as np
import pytest
import torch

from tests import half_image_rule as R


def _f32(*v):
    return np.array(v, dtype=np.float32)


def test_ties_go_to_even_in_both_directions():
    ulp = 2.0 ** -13                                          # spacing of half in [0.125, 0.25)
    lo = 0.125
    x = _f32(lo + 0.5 * ulp,                                  # tie between an even (0x3000) and an odd fraction: down
             lo + 1.5 * ulp,                                  # tie between odd and even: up
             lo + 0.5 * ulp + 2.0 ** -24, lo + 0.5 * ulp - 2.0 ** -24,      # just beside the tie: nearest
             -(lo + 0.5 * ulp), -(lo + 1.5 * ulp))
    assert R.half_bits(x).tolist() == [0x3000, 0x3002, 0x3001, 0x3000, 0xB000, 0xB002]
    # a fraction that rounds up to 2.0 carries into the exponent
    assert R.half_bits(_f32(0.25 - 2.0 ** -15)).tolist() == [0x3400]


def test_below_two_to_minus_fourteen_is_stored_as_plus_zero():
    m = 2.0 ** -14
    x = _f32(m, -m, np.nextafter(np.float32(m), np.float32(0)), -np.nextafter(np.float32(m), np.float32(0)),
             m * 0.75, 2.0 ** -20, 1e-30, 1e-40, 0.0, -0.0)
    assert R.half_bits(x).tolist() == [0x0400, 0x8400] + [0] * 8
    # the value just below 2^-14 would ROUND to 2^-14; the rule is on x, so it is flushed all the same
    assert np.float32(x[2]).astype(np.float16) == np.float16(m)


def test_no_subnormal_pattern_and_agreement_with_ieee_rounding_on_normals():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-1, 1, 200_000), rng.uniform(-1, 1, 100_000) * 2.0 ** rng.integers(-30, 0, 100_000),
                        [1.0, -1.0, 1.0 - 2.0 ** -25]]).astype(np.float32)
    b = R.half_bits(x)
    exp, frac = (b >> 10) & 0x1F, b & 0x3FF
    assert not ((exp == 0) & (frac != 0)).any(), "a subnormal bit pattern"
    assert not (b == 0x8000).any(), "a negative zero"
    assert int((b & 0x7FFF).max()) == 0x3C00, "|x| <= 1 never rounds above 1.0: 65504 (0x7BFF) is out of reach"
    normal = np.abs(x) >= R.MIN_NORMAL
    assert np.array_equal(b[normal], x[normal].astype(np.float16).view(np.uint16)), "not IEEE round-to-nearest-even"
    assert np.array_equal(b[normal], torch.from_numpy(x[normal]).to(torch.float16).numpy().view(np.uint16))
    assert not b[~normal].any()


@pytest.mark.parametrize("D", [8, 64, 768])
def test_residual_obeys_the_worst_case_bound(D):
    """||half(x) - x|| <= 2^-11 ||x|| + sqrt(n_flushed) 2^-14: relative half an ulp on what stays normal, the element
    itself (< 2^-14) on what is stored as 0 -- the derivation behind coarse_eq_worst_f16 (csrc/aura_rowc.inl)."""
    rng = np.random.default_rng(D)
    x = rng.standard_normal((4000, D))
    x[::3] *= 2.0 ** rng.integers(-12, 1, (x[::3].shape[0], D))         # rows with many tiny elements
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    e = np.linalg.norm(R.half_values(x).astype(np.float64) - x.astype(np.float64), axis=1)
    flushed = (np.abs(x) < R.MIN_NORMAL).sum(axis=1)
    assert flushed.max() > 0
    bound = 2.0 ** -11 * np.linalg.norm(x.astype(np.float64), axis=1) + np.sqrt(flushed) * 2.0 ** -14
    assert (e <= bound).all()
    assert (R.rho16(x, D) <= 1.001 * (2.0 ** -11 * 1.00001 + np.sqrt(D) * 2.0 ** -14) + (0.5 * D + 3) * 2.0 ** -24).all()
