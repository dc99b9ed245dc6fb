"""Blending merges in torch fp32 on the CPU: the rule of ``include/aura_hip.h`` ("Blending merges") and a stand-in
``bank_blend`` on top of ``tests/cpu_stub_replay.py`` (which brings every other stand-in) -- TEST INFRASTRUCTURE ONLY.

The rule, restated literally.  Group key of batch row i: ``stored_target[i] = r >= 0`` -> held row r; else
``batch_leader[i] = j >= 0`` -> batch row j; else none.  For a key, ``g`` starts as the key's row and takes its members
in ascending i: ``g = g + beta * (f_i - g)`` -- ``torch.sub``, ``torch.mul``, ``torch.add`` on fp32 tensors, one rounding
each, which is what the kernel computes (three unfused fp32 operations per component): the two are bit-equal by
definition.  Members are read unblended; a held key's result replaces ``bank[r]``, a batch key's replaces row j of the
batch as it will be stored.  Entries out of range are ignored exactly as the kernel ignores them."""
import numpy as np
import torch

from tests.cpu_stub_replay import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_replay import (CALLS, LAST, FIND_SIZES, MOVES, STAMPS, SCOPED_FINDS,  # noqa: F401
                                   KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError,
                                   CONSOLIDATE_MAX_BATCH, CONSOLIDATE_MAX_IMAGE_DIM, TAG_LIMIT, QUOTA_MAX_SCOPES)

CALLS["blend"] = 0
BLENDS = []                                        # (count, n, beta, feats_row0, keys moved) of every stub bank_blend call


def blend_step(g, f, beta):
    """``g + beta * (f - g)`` in fp32: three roundings, never fused."""
    assert g.dtype == torch.float32 and f.dtype == torch.float32
    return torch.add(g, torch.mul(torch.tensor(float(beta), dtype=torch.float32), torch.sub(f, g)))


def group_keys(stored, leader, count):
    """One key per batch row: ``r >= 0`` (held row r), ``-2 - j`` (batch row j) or -1 (a member of nothing), with the
    kernel's checks: a stored target outside ``[0, count)`` is ignored, so is a leader outside ``[0, i)`` or one that is
    not itself a kept row."""
    st = np.asarray(stored, dtype=np.int64).reshape(-1)
    ld = np.asarray(leader, dtype=np.int64).reshape(-1)
    keys = np.full(st.size, -1, dtype=np.int64)
    for i in range(st.size):
        if st[i] >= 0:
            keys[i] = st[i] if st[i] < count else -1
        elif 0 <= ld[i] < i and st[ld[i]] < 0 and ld[ld[i]] < 0:
            keys[i] = -2 - ld[i]
    return keys


def blend_reference(bank, feats, stored, leader, beta, count):
    """``({held row r: its blended row}, {batch row j: its blended row})`` (fp32 CPU tensors) by the rule."""
    bank, feats = bank.detach().cpu(), feats.detach().cpu()
    keys = group_keys(stored, leader, count)
    held, batch = {}, {}
    for i in range(keys.size):                     # ascending i: the chain's order
        k = int(keys[i])
        if k >= 0:
            held[k] = blend_step(held.get(k, bank[k]), feats[i], beta)
        elif k <= -2:
            batch[-2 - k] = blend_step(batch.get(-2 - k, feats[-2 - k]), feats[i], beta)
    return held, batch


def bank_blend(bank, inv_norm, count, stored_target, batch_leader, beta, feats=None, out=None, feats_row0=-1,
               shadow=None, rho=None, shadow_upto=0, sorted_bf16=None, sorted_rows=None, pos_of_row=None, n_sorted=None):
    CALLS["blend"] += 1
    n = stored_target.numel()
    assert stored_target.dtype == torch.int32 and batch_leader.dtype == torch.int32 and batch_leader.numel() == n
    assert 0.0 < float(beta) <= 1.0 and n <= CONSOLIDATE_MAX_BATCH and 0 <= count <= bank.shape[0]
    assert shadow is None and rho is None and sorted_bf16 is None, "the CPU banks keep no bf16 image"
    if feats_row0 < 0:
        assert feats.shape == out.shape == (n, bank.shape[1]) and out.data_ptr() != feats.data_ptr()
        batch_rows = feats
    else:
        assert feats is None and out is None and count <= feats_row0 and feats_row0 + n <= bank.shape[0]
        batch_rows = bank[feats_row0:feats_row0 + n]
    held, batch = blend_reference(bank, batch_rows, stored_target.numpy(), batch_leader.numpy(), beta, count)
    for r, g in held.items():
        bank[r] = g
        inv_norm[r] = 1.0 / g.norm().clamp_min(1e-12)
    for j, g in batch.items():
        if feats_row0 < 0:
            out[j] = g
        else:
            bank[feats_row0 + j] = g
            inv_norm[feats_row0 + j] = 1.0 / g.norm().clamp_min(1e-12)
    BLENDS.append((count, n, float(beta), int(feats_row0), len(held) + len(batch)))


# ----------------------------------------------------------------------------------------------------- the bank model
INF = float("inf")


class BlendedBank:
    """A bank of blended consolidating writes by the rule alone: decisions by the fp64 rule of
    tests/cpu_stub_consolidate.py on fp64 cosines of the model's CURRENT (blended) fp32 rows, the blend by
    ``blend_reference``.  Rows are held in write order (nothing overflows).  The fp64 products run on ``device`` (a GPU
    does them in a moment); the rows themselves, and every blend, stay fp32 on the CPU.

    What the device may be judged by is asserted from the model before: ``min_margin`` is the smallest distance of any
    decision -- a row's best held cosine, and for a row without a stored target its best cosine to an earlier kept row
    of its chunk -- from tau; ``near_ties`` counts rows whose best two candidates, where they can matter, lie within
    ``tol`` of each other."""

    def __init__(self, D, capacity, device="cpu", tol=0.0):
        self.D, self.device, self.tol = D, torch.device(device), tol
        self.feats = torch.zeros(capacity, D)
        self.unit = torch.zeros(capacity, D, dtype=torch.float64, device=self.device)
        self.tag = np.zeros(capacity, dtype=np.int64)
        self.origin = []                                # for every held row: what the caller named it
        self.count = 0
        self.min_margin, self.near_ties, self.moved, self.merged = INF, 0, 0, 0

    def _units(self, f):
        f = f.detach().to(self.device).double()
        return f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)

    def _set(self, rows, f):
        if len(rows):
            r = torch.as_tensor(rows, dtype=torch.int64)
            self.feats[r] = f
            self.unit[r.to(self.device)] = self._units(f)

    def _margins(self, cs, cb, st, ld, tau):
        def close(x, rows):
            if x.shape[1] == 0 or not bool(rows.any()):
                return
            best = x.max(1).values
            second = torch.where(x == best[:, None], torch.full_like(x, -INF), x).max(1).values
            live = rows & torch.isfinite(best)
            if bool(live.any()):
                self.min_margin = min(self.min_margin, float((best[live] - tau).abs().min()))
                self.near_ties += int((live & (best >= tau - self.tol) & (best - second < self.tol)).sum())
        n = cs.shape[0]
        kept = (st < 0) & (ld < 0)
        close(cs, torch.ones(n, dtype=torch.bool))
        lower = torch.tril(torch.ones(n, n, dtype=torch.bool), -1) & kept[None, :]
        close(torch.where(lower, cb, torch.full_like(cb, -INF)), st < 0)

    def chunk(self, f, names, tau, beta, tags=None):
        """One chunk (at most 1024 rows) of a blended consolidating write; ``beta`` None: a plain consolidating one.
        Returns the fp64 rule's ``(stored_target, batch_leader)`` (int64 tensors)."""
        f = f.detach().cpu().float()
        n, c = f.shape[0], self.count
        fn = self._units(f)
        cs, cb = (fn @ self.unit[:c].t()).cpu(), (fn @ fn.t()).cpu()
        if tags is not None:
            t = torch.as_tensor(np.asarray(tags), dtype=torch.int64)
            cs = torch.where(t[:, None] == torch.from_numpy(self.tag[:c])[None, :], cs, torch.full_like(cs, -INF))
            cb = torch.where(t[:, None] == t[None, :], cb, torch.full_like(cb, -INF))
        st, ld, _ = rule(cs, cb, float(tau))
        self._margins(cs, cb, st, ld, float(tau))
        f = f.clone()
        if beta is not None:
            held, batch = blend_reference(self.feats, f, st.numpy(), ld.numpy(), beta, c)
            self.moved += len(held) + len(batch)
            if held:
                self._set(list(held), torch.stack(list(held.values())))
            for j, g in batch.items():
                f[j] = g
        kept = torch.nonzero((st < 0) & (ld < 0)).flatten()
        k = kept.numel()
        self._set(list(range(c, c + k)), f[kept])
        if tags is not None:
            self.tag[c:c + k] = np.asarray(tags)[kept.numpy()]
        self.origin += [names[i] for i in kept.tolist()]
        self.count = c + k
        self.merged += n - k
        return st, ld

    def write(self, f, names, tau, beta, tags=None, step=CONSOLIDATE_MAX_BATCH):
        for lo in range(0, f.shape[0], step):
            self.chunk(f[lo:lo + step], names[lo:lo + step], tau, beta, None if tags is None else tags[lo:lo + step])

    def bulk(self, f, names, tags=None):
        c, k = self.count, f.shape[0]
        self._set(list(range(c, c + k)), f.detach().cpu().float())
        self.tag[c:c + k] = 0 if tags is None else np.asarray(tags)
        self.origin += list(names)
        self.count = c + k

    def forget(self, kill):
        keep = np.ones(self.count, dtype=bool)
        keep[np.asarray(kill, dtype=np.int64)] = False
        rows = np.nonzero(keep)[0]
        f, t, names = self.feats[torch.from_numpy(rows)].clone(), self.tag[rows].copy(), [self.origin[r] for r in rows]
        self.count, self.origin = 0, []
        self.bulk(f, names, t)

    def consolidate(self, tau, beta, within=False):
        """The held rows, oldest first, through blended consolidating writes in chunks of 1024 into an empty bank."""
        n = self.count
        f, t, names = self.feats[:n].clone(), self.tag[:n].copy(), list(self.origin)
        self.count, self.origin = 0, []
        self.write(f, names, tau, beta, t if within else None)
        if not within:                                  # a kept row keeps its own tag
            where = {name: i for i, name in enumerate(names)}
            self.tag[:self.count] = t[[where[name] for name in self.origin]]
