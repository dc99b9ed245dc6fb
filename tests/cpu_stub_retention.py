"""CPU stand-ins for the retention ops (``bank_retention_keys``, ``bank_select_weakest``,
``bank_reinforce``) on top of ``tests/cpu_stub_ops.py`` -- TEST INFRASTRUCTURE ONLY.

They restate the rule literally with torch on the CPU:
  key(r)   = strength(r) * exp(-(now32 - timestamp(r)) / 3600)                (fp32)
  eviction = rows ordered by (key, (r - cursor) mod count) ascending, a NaN key first
  reinforce: s < cap -> min(s + amount, cap), once per distinct valid row."""
import numpy as np
import torch

from tests.cpu_stub_ops import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_ops import KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError  # noqa: F401

CALLS = {"select": 0, "reinforce": 0, "keys": 0}


def ordered_bits(keys: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 in [0, 2^32) that ascends with the key: NaN lowest, -0 == +0."""
    k = keys.detach().cpu().to(torch.float32)
    u = k.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    o = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    o = torch.where(k == 0, torch.full_like(o, 0x80000000), o)
    return torch.where(torch.isnan(k), torch.zeros_like(o), o)


def eviction_order(keys: torch.Tensor, cursor: int) -> torch.Tensor:
    """All rows of ``keys`` ([count]) in eviction order (int64 [count])."""
    count = keys.numel()
    rot = (torch.arange(count, dtype=torch.int64) - int(cursor) % count) % count
    o = ordered_bits(keys)
    # (o << 32 | rot) needs 64 unsigned bits: order by the two components instead, same order
    idx = torch.argsort(rot, stable=True)
    return idx[torch.argsort(o[idx], stable=True)]


def bank_retention_keys(meta, count, now):
    CALLS["keys"] += 1
    now32 = torch.tensor(float(np.float32(now)), dtype=torch.float32)
    return meta[:count, 0] * torch.exp(-(now32 - meta[:count, 1]) / 3600.0)


def bank_select_weakest(meta, count, now, cursor, n):
    CALLS["select"] += 1
    assert 1 <= n <= count and cursor >= 0
    keys = bank_retention_keys(meta, count, now)
    CALLS["keys"] -= 1
    rows = eviction_order(keys, cursor)[:n]
    return rows, keys[rows]


def reinforce_reference(meta, count, rows, amount, cap=1.0):
    """The rule on a copy of the metadata (used by the GPU tests as the expected result)."""
    out = meta.clone()
    r = torch.unique(rows.reshape(-1).to(torch.int64))
    r = r[(r >= 0) & (r < count)]
    s = out[r, 0]
    capt = torch.tensor(cap, dtype=torch.float32)
    out[r, 0] = torch.where(s < capt, torch.minimum(s + torch.tensor(amount, dtype=torch.float32), capt), s)
    return out


def bank_reinforce(meta, count, rows, amount, cap=1.0):
    CALLS["reinforce"] += 1
    assert rows.dtype == torch.int32 and amount >= 0
    meta.copy_(reinforce_reference(meta, count, rows, amount, cap))
