"""``tests/cpu_stub_retention.py`` with a ``bank_write`` that holds the caller to the kernel's contract -- TEST
INFRASTRUCTURE ONLY.

The product's parallel write kernel (one wave per row, no ordering between rows) serves a call without
centroids, and phase 0 of the online kernel a call with ``distinct_slots`` (unless ``serial``).  Two rows of
one such call that name the same slot race on the GPU; the Python loop of the plain stand-in writes them in
order and cannot see it.  Here such a call raises ``AssertionError`` before anything is written."""
import torch

from tests import cpu_stub_retention as _base
from tests.cpu_stub_retention import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_retention import (KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError,  # noqa: F401
                                      CALLS, eviction_order, ordered_bits, reinforce_reference)

WRITES = {"calls": 0, "rows": 0}


def repeated_slots(slots) -> list:
    """The slots (ascending) that ``slots`` names more than once."""
    s = torch.as_tensor(slots).detach().cpu().reshape(-1).to(torch.int64)
    u, c = torch.unique(s, return_counts=True)
    return u[c > 1].tolist()


def runs_parallel_kernel(centroids, distinct_slots: bool, serial: bool) -> bool:
    return centroids is None or (bool(distinct_slots) and not serial)


def check_write_contract(slots, centroids, distinct_slots, serial) -> None:
    if runs_parallel_kernel(centroids, distinct_slots, serial):
        rep = repeated_slots(slots)
        assert not rep, (f"bank_write: slots {rep[:16]}{' ...' if len(rep) > 16 else ''} ({len(rep)} in all) are named "
                         f"more than once in a call of {int(torch.as_tensor(slots).numel())} rows that runs the parallel "
                         f"kernel (centroids {'off' if centroids is None else 'on'}, distinct_slots={bool(distinct_slots)}, "
                         f"serial={bool(serial)})")


def bank_write(bank, loc, meta, inv_norm, feats, slots, cur_loc, now, centroids=None,
               centroid_counts=None, eff_k=0, distinct_slots=False, serial=False):
    check_write_contract(slots, centroids, distinct_slots, serial)
    WRITES["calls"] += 1
    WRITES["rows"] += int(slots.numel())
    _base.bank_write(bank, loc, meta, inv_norm, feats, slots, cur_loc, now, centroids=centroids,
                     centroid_counts=centroid_counts, eff_k=eff_k, distinct_slots=distinct_slots, serial=serial)
