"""``bank_compact`` in torch on the CPU, on top of ``tests/cpu_stub_consolidate.py`` -- TEST INFRASTRUCTURE ONLY.

The move (``include/aura_hip.h``, ``aura_bank_compact``): row ``src[i]`` of every array goes to row ``dst0 + i``, as if
every source were read before any destination is written; ``src`` ascends strictly, ``dst0 + i <= src[i] < rows``."""
import numpy as np
import torch

from tests.cpu_stub_consolidate import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_consolidate import (CALLS, LAST, FIND_SIZES, KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE,  # noqa: F401
                                        AuraDeviceError, CONSOLIDATE_MAX_BATCH, CONSOLIDATE_MAX_IMAGE_DIM, tolerance)

CALLS["compact"] = 0
MOVES = []                                         # (n, dst0, rows that change place) of every stub bank_compact call


def compact_reference(arrays, src, dst0):
    """The move on torch tensors (any device), in place: gather everything first, then store."""
    src = torch.as_tensor(np.asarray(src, dtype=np.int64), device=arrays[0].device)
    n = src.numel()
    staged = [a.index_select(0, src) for a in arrays]
    for a, t in zip(arrays, staged):
        a[dst0:dst0 + n] = t


def bank_compact(bank, loc, meta, inv_norm, src, dst0=0, shadow=None, rho=None):
    CALLS["compact"] += 1
    s = np.asarray(src).reshape(-1).astype(np.int64)
    rows, n = bank.shape[0], s.size
    assert (shadow is None) == (rho is None)
    assert loc.shape[0] == rows and meta.shape == (rows, 4) and inv_norm.numel() == rows
    assert 0 <= dst0 and dst0 + n <= rows
    assert n == 0 or (s[-1] < rows and bool((np.diff(s) > 0).all()) and bool((s >= dst0 + np.arange(n)).all())), \
        "src must ascend strictly with dst0 + i <= src[i] < rows"
    arrays = [bank, loc, meta, inv_norm] + ([shadow, rho] if shadow is not None else [])
    compact_reference(arrays, s, dst0)
    moved = int((s != dst0 + np.arange(n)).sum())
    MOVES.append((n, dst0, moved))
    return moved
