"""Host model of the half image's conversion rule (csrc/aura_row.inl, aura_half_flush + the hardware's
round-to-nearest-even): integer arithmetic on the fp32 bit patterns, no float16 arithmetic of numpy's involved.

    half(x), |x| <= 1:   |x| < 2^-14  ->  +0     (no subnormal is ever stored; the rule is on x, not on the rounded value)
                         otherwise    ->  x rounded to 11 significand bits, ties to even (a carry may raise the exponent)

Inputs are finite fp32 values in [-1, 1] (normalised rows and queries), so the largest result is 1.0 = 0x3C00 and 65504
(0x7BFF) is never reached."""
import numpy as np

MIN_NORMAL = np.float32(2.0 ** -14)


def half_bits(x) -> np.ndarray:
    """uint16 bit patterns of the stored half values of fp32 ``x`` (any shape, |x| <= 1)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    sign = ((u >> 31) & 1).astype(np.uint64)
    mag = u & 0x7FFFFFFF
    # round the 23-bit fraction to 10 bits, ties to even, on the magnitude's bits: exponent and fraction are adjacent,
    # so a fraction that rounds up to 2.0 carries into the exponent by itself
    r = (mag + 0xFFF + ((mag >> 13) & 1)) >> 13              # (8-bit exponent, 10-bit fraction)
    r = r - ((127 - 15) << 10)                               # re-bias the exponent 127 -> 15
    bits = (sign << 15) | (r & 0x7FFF)
    flushed = np.abs(x) < MIN_NORMAL                          # includes +-0 and fp32 subnormals
    bits = np.where(flushed, 0, bits)
    return bits.astype(np.uint16)


def half_values(x) -> np.ndarray:
    """The stored values as fp32 (exact: every half is an fp32)."""
    return half_bits(x).view(np.float16).astype(np.float32)


def rho16(x_hat, D: int) -> np.ndarray:
    """Per-row residual norm of the half image of normalised rows ``x_hat`` [n, D] with the kernels' formula
    (aura_rho_from_e2), evaluated in float64: 1.001 ||half(x) - x|| + (D/2 + 3) 2^-24."""
    e = half_values(x_hat).astype(np.float64) - np.asarray(x_hat, dtype=np.float32).astype(np.float64)
    return 1.001 * np.sqrt((e * e).sum(axis=-1)) + (0.5 * D + 3) * 2.0 ** -24
