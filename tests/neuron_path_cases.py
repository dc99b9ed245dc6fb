"""Seeded inputs shared by tests/test_host_neuron_rules.py (CPU controls) and tests/test_gpu_neuron_paths.py
(device parity), so the controls are asserted on exactly the tensors the device tests run.

Nothing here touches a GPU.  The rounding helpers are written with numpy on the raw bits, independent of torch's
own conversions, because they state the rule that torch's results are held to.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import aura_oracle as O

# ---------------------------------------------------------------------------------------------------------
# rounding rules on raw bits
# ---------------------------------------------------------------------------------------------------------


def rne_bf16(x) -> np.ndarray:
    """float32 -> the float32 value of its round-to-nearest-even bfloat16 (finite inputs)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def bits(t: torch.Tensor) -> np.ndarray:
    """Raw bits of an fp32 / bf16 tensor, as integers."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def as_dtype_bits(x_f32: np.ndarray, dtype) -> np.ndarray:
    """Bits of the fp32 values ``x_f32`` once stored as ``dtype`` (RNE for bf16)."""
    x_f32 = np.asarray(x_f32, dtype=np.float32)
    if dtype == torch.float32:
        return x_f32.view(np.int32)
    return (rne_bf16(x_f32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def mean_rule(total, T: int, dtype) -> np.ndarray:
    """THE rule of ``spikes.mean(dim=1)``: the fp32 sum divided by T in fp32, rounded once to the dtype."""
    return as_dtype_bits(np.asarray(total, dtype=np.float32) / np.float32(T), dtype)


def mean_rule_rounded_sum(total, T: int) -> np.ndarray:
    """Rejected (bf16): the sum rounded to bf16 before the division."""
    return as_dtype_bits(rne_bf16(np.asarray(total, dtype=np.float32)) / np.float32(T), torch.bfloat16)


def mean_rule_reciprocal(total, T: int) -> np.ndarray:
    """Rejected (fp32): the sum multiplied by the rounded reciprocal of T."""
    return as_dtype_bits(np.asarray(total, dtype=np.float32) * (np.float32(1.0) / np.float32(T)), torch.float32)


def bf16_exact(total) -> np.ndarray:
    total = np.asarray(total, dtype=np.float32)
    return rne_bf16(total) == total


# ---------------------------------------------------------------------------------------------------------
# A. fused mean past 256
# ---------------------------------------------------------------------------------------------------------
MEAN_DECAY, MEAN_ALPHA, MEAN_THRESHOLD = O.gif_decay(), 0.01, 1.0
MEAN_SHAPES = [(8, 100, 24, 8), (8, 72, 24, 16), (8, 100, 24, 5), (8, 100, 13, 8)]     # rows, T, H, L
MEAN_CASES = [(dtype, ti, shape, seed)
              for dtype in (torch.float32, torch.bfloat16)
              for ti in (False, True)
              for seed, shape in enumerate(MEAN_SHAPES)]


def mean_case_id(case) -> str:
    dtype, ti, (rows, T, H, L), _ = case
    return f"{'f32' if dtype == torch.float32 else 'bf16'}-{'ti' if ti else 'seq'}-{rows}x{T}x{H}-L{L}"


@functools.lru_cache(maxsize=None)
def mean_case(case):
    """``(h, full, spikes)``: the kernel's input ([rows, H] if time-invariant), the same currents as
    [rows, T, H], and the oracle's spikes from the initial state.  Computed once, never modified."""
    dtype, ti, (rows, T, H, L), seed = case
    g = torch.Generator().manual_seed(seed)
    if ti:
        h = (6 * torch.randn(rows, H, generator=g) + 12).to(dtype)
        full = h.unsqueeze(1).expand(rows, T, H).contiguous()
    else:
        h = full = (6 * torch.randn(rows, T, H, generator=g) + 12).to(dtype)
    v0, t0 = O.gif_initial_state(rows, H, MEAN_THRESHOLD, dtype)
    spikes, _, _ = O.gif_run(full, v0, t0, MEAN_DECAY, L, MEAN_ALPHA, MEAN_THRESHOLD)
    return h, full, spikes


def cell_sums(spikes: torch.Tensor) -> np.ndarray:
    """Exact per-cell spike totals over T (integers, summed in fp64)."""
    return spikes.double().sum(dim=1).numpy()


# ---------------------------------------------------------------------------------------------------------
# C. LIF per-channel constants
# ---------------------------------------------------------------------------------------------------------
LIF_SIZES = (96, 13, 130)
LIF_B, LIF_T = 5, 23


@functools.lru_cache(maxsize=None)
def lif_case(size: int, dtype):
    """``(x, beta, threshold)``: every channel has its own beta and threshold, in shuffled order.  For bf16 the
    constants are cast first, so the oracle and the kernel are handed the same tensors."""
    g = torch.Generator().manual_seed(1000 + size)
    beta = torch.linspace(0.5, 0.99, size)[torch.randperm(size, generator=g)]
    thr = torch.linspace(0.2, 1.5, size)[torch.randperm(size, generator=g)]
    x = torch.randn(LIF_B, LIF_T, size, generator=g)
    return x.to(dtype), beta.to(dtype).contiguous(), thr.to(dtype).contiguous()
