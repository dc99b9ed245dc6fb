"""Consolidation within tags in torch fp64 on the CPU: ``find_repeats_scoped`` on top of ``tests/cpu_stub_scoped.py``
(which brings ``find_repeats``, ``bank_compact``, ``bank_set_tags`` and every other stand-in) -- TEST INFRASTRUCTURE ONLY.

The rule (``include/aura_hip.h``, ``aura_bank_find_repeats`` by tag) is the rule of ``tests/cpu_stub_consolidate.py``
applied to masked cosines: ``cs[i, r] = -inf`` where the held row's tag differs from ``tags[i]``, ``cb[i, j] = -inf``
where ``tags[i] != tags[j]``.  A held row's tag is ``int(meta[r, 3])`` when that lies in (-1, 2^24), else no tag at all; a
batch tag outside [0, 2^24) matches nothing, not even the same value on another batch row.  ``rule``, ``undecided`` and
``replay_check`` are used unchanged on the masked matrices."""
import torch

from tests.cpu_stub_scoped import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_scoped import (CALLS, LAST, FIND_SIZES, MOVES, STAMPS, KNN_FLAG_NO_CANDIDATES,  # noqa: F401
                                   KNN_FLAG_LISTS_STALE, AuraDeviceError, CONSOLIDATE_MAX_BATCH,
                                   CONSOLIDATE_MAX_IMAGE_DIM, TAG_LIMIT, tolerance, compact_reference)
from tests.cpu_stub_consolidate import cosines, rule, undecided, replay_check, degenerate  # noqa: F401

CALLS["find_repeats_scoped"] = 0
SCOPED_FINDS = []                                  # (count, tags as a list) of every stub find_repeats_scoped call
INF = float("inf")


def held_tags(meta, count):
    """int64 [count]: the tag of every held row as the kernels read column 3; -2 where it holds no tag."""
    t = meta[:count, 3].detach().cpu().float()
    ok = (t > -1.0) & (t < float(TAG_LIMIT))
    return torch.where(ok, torch.where(ok, t, torch.zeros_like(t)).to(torch.int64), torch.full(t.shape, -2, dtype=torch.int64))


def batch_tags(tags):
    """int64 [n]: the batch tags, -1 where a tag lies outside [0, 2^24)."""
    t = tags.detach().cpu().to(torch.int64).reshape(-1)
    return torch.where((t >= 0) & (t < TAG_LIMIT), t, torch.full_like(t, -1))


def mask_cosines(cs, cb, bank_tag, tag):
    """The cosine matrices with every ineligible pair at -inf (``bank_tag`` [count], ``tag`` [n]: as the two above)."""
    ok_s = (bank_tag[None, :] == tag[:, None]) & (tag[:, None] >= 0)
    ok_b = (tag[None, :] == tag[:, None]) & (tag[:, None] >= 0)
    return (torch.where(ok_s, cs, torch.full_like(cs, -INF)), torch.where(ok_b, cb, torch.full_like(cb, -INF)))


def scoped_cosines(bank, inv_norm, meta, count, feats, tags):
    cs, cb = cosines(bank, inv_norm, count, feats)
    return mask_cosines(cs, cb, held_tags(meta, count), batch_tags(tags))


def find_repeats_scoped_reference(bank, inv_norm, meta, count, feats, tags, tau):
    return rule(*scoped_cosines(bank, inv_norm, meta, count, feats, tags), float(tau))


def find_repeats_scoped(bank, inv_norm, meta, count, feats, tags, tau, image=None, image_rows=None, n_image=None,
                        rho=None, lists_flag=None):
    CALLS["find_repeats_scoped"] += 1
    n = feats.shape[0]
    assert feats.dtype == torch.float32 and n <= CONSOLIDATE_MAX_BATCH and 0.0 < tau <= 1.0
    assert isinstance(tags, torch.Tensor) and tags.dtype == torch.int32 and tags.shape == (n,) and tags.is_contiguous()
    assert meta.dtype == torch.float32 and meta.shape == (bank.shape[0], 4)
    SCOPED_FINDS.append((count, tags.tolist()))
    stored, leader, cos = find_repeats_scoped_reference(bank, inv_norm, meta, count, feats, tags, tau)
    packed = torch.zeros(3 * n + 2, dtype=torch.int32)
    packed[:n], packed[n:2 * n] = stored.to(torch.int32), leader.to(torch.int32)
    packed[2 * n:3 * n] = cos.to(torch.float32).view(torch.int32)
    if lists_flag is not None:
        packed[3 * n + 1] = int(lists_flag.reshape(-1)[0])
    return packed[:n], packed[n:2 * n], packed[2 * n:3 * n].view(torch.float32), packed
