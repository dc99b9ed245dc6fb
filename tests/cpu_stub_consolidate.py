"""The consolidating-write rule in torch fp64 on the CPU, a replay check of a device's decisions against it, and CPU
``find_repeats`` / ``bank_touch`` for the host tests, on top of ``tests/cpu_stub_diverse.py`` -- TEST INFRASTRUCTURE
ONLY.

The rule (``include/aura_hip.h``): cos(x, y) = dot product of the two rows, each scaled by 1 / max(||.||, 1e-12) (bank
rows: the stored fp32 ``inv_norm``); ``stored_target[i]`` = the held row of largest cos(f_i, r) if >= tau (equal ->
the lowest r) else -1; walking i = 0..n-1, a row with a stored target is a repeat and never a leader, another row
repeats the KEPT earlier row of largest cosine >= tau (equal -> the lowest j) or is kept; ``cos_out`` = the cosine to
what the row repeats, -inf for a kept row; rows with a NaN / Inf component or of norm 0 are kept and nobody's target."""
import torch

from tests.cpu_stub_diverse import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_diverse import CALLS, LAST, KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError  # noqa: F401
from tests.cpu_stub_diverse import tolerance  # noqa: F401  (2 (D + 8) 2^-24: the rule's ``tol``)

CONSOLIDATE_MAX_BATCH = 1024
CONSOLIDATE_MAX_IMAGE_DIM = 768
CALLS["find_repeats"] = 0
CALLS["touch"] = 0
FIND_SIZES = []                                    # batch rows of every stub find_repeats call

INF = float("inf")


def degenerate(feats):
    """bool [n]: rows with a NaN / Inf component or of norm 0."""
    f = feats.detach().cpu().double()
    return ~torch.isfinite(f).all(1) | (f.norm(dim=1) == 0)


def cosines(bank, inv_norm, count, feats):
    """fp64 ``(stored [n, count], batch [n, n])``; NaN and the cosines of degenerate rows are -inf (never >= tau)."""
    f = feats.detach().cpu().double()
    bad = degenerate(feats)
    f = torch.where(bad[:, None], torch.zeros_like(f), f)
    fn = f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)
    b = bank[:count].detach().cpu().double() * inv_norm[:count].detach().cpu().double()[:, None]
    cs = fn @ b.t()
    cb = fn @ fn.t()
    cs = torch.where(torch.isnan(cs) | bad[:, None], torch.full_like(cs, -INF), cs)
    cb = torch.where(torch.isnan(cb) | bad[:, None] | bad[None, :], torch.full_like(cb, -INF), cb)
    return cs, cb


def _first_argmax(x):
    """(max, the LOWEST index that attains it) along dim 1; (-inf, 0) for an empty row."""
    if x.shape[1] == 0:
        return torch.full((x.shape[0],), -INF, dtype=x.dtype), torch.zeros(x.shape[0], dtype=torch.int64)
    best = x.max(1).values
    return best, (x == best[:, None]).to(torch.int8).argmax(1)


def rule(cs, cb, tau):
    """The rule on fp64 cosines: ``(stored_target, batch_leader int64 [n], cos fp64 [n])``."""
    n = cs.shape[0]
    best, arg = _first_argmax(cs)
    stored = torch.where(best >= tau, arg, torch.full_like(arg, -1))
    cos = torch.where(stored >= 0, best, torch.full_like(best, -INF))
    leader = torch.full((n,), -1, dtype=torch.int64)
    kept = torch.zeros(n, dtype=torch.bool)
    for i in range(n):
        if stored[i] >= 0:
            continue
        c = torch.where(kept[:i], cb[i, :i], torch.full((i,), -INF, dtype=cb.dtype))
        if i and float(c.max()) >= tau:
            j = int((c == c.max()).to(torch.int8).argmax())
            leader[i], cos[i] = j, c[j]
        else:
            kept[i] = True
    return stored, leader, cos


def find_repeats_reference(bank, inv_norm, count, feats, tau):
    cs, cb = cosines(bank, inv_norm, count, feats)
    return rule(cs, cb, float(tau))


def undecided(cs, cb, tau, tol):
    """bool [n]: rows the rule decides by less than ``tol`` -- the stored maximum within tol of tau, its runner-up
    (among different cosines: bit-identical rows tie by rule) within tol of it while it can matter, or the same for
    the in-batch maximum over the reference's kept rows."""
    n = cs.shape[0]
    stored, leader, _ = rule(cs, cb, tau)
    kept = (stored < 0) & (leader < 0)

    def close(x):
        best = x.max(1).values if x.shape[1] else torch.full((x.shape[0],), -INF, dtype=x.dtype)
        second = torch.where(x == best[:, None], torch.full_like(x, -INF), x)
        second = second.max(1).values if x.shape[1] else best
        return ((best - tau).abs() < tol) | ((best >= tau - tol) & (best - second < tol))
    und = close(cs)
    lower = torch.tril(torch.ones(n, n, dtype=torch.bool), -1) & kept[None, :]
    und |= (stored < 0) & close(torch.where(lower, cb, torch.full_like(cb, -INF)))
    return und


def replay_check(cs, cb, tau, tol, stored, leader, cos, bad=None):
    """Every row, given the result's OWN earlier decisions: a row whose best stored cosine is >= tau + tol reports a
    target within tol of the best, one below tau - tol reports none, a reported target reaches tau - tol and the best
    - tol; a row with a stored target has no leader; among the others the same holds for the leader over the rows the
    RESULT kept before it; ``cos`` is within tol of the fp64 cosine of what is reported, -inf for a kept row."""
    stored, leader, cos = stored.cpu().long(), leader.cpu().long(), cos.cpu().double()
    n, N = cs.shape
    ar = torch.arange(n)
    assert stored.shape == (n,) and leader.shape == (n,) and cos.shape == (n,)
    assert bool(((stored >= -1) & (stored < N)).all()), "a stored target outside the bank"
    best = cs.max(1).values if N else torch.full((n,), -INF, dtype=cs.dtype)
    has = stored >= 0
    got = torch.where(has, cs[ar, stored.clamp(min=0)] if N else best, torch.full_like(best, -INF))
    assert not bool(((best >= tau + tol) & ~has).any()), "a clear stored repeat was missed"
    assert not bool(((best < tau - tol) & has).any()), "a stored target below the threshold"
    assert bool((got[has] >= tau - tol).all()) and bool((got[has] >= best[has] - tol).all()), "not the best target"
    assert bool(((cos[has] - got[has]).abs() <= tol).all()), "cos_out of a stored repeat"
    assert bool((leader[has] == -1).all()), "a row with a stored target names a leader"
    kept = ~has & (leader < 0)
    assert bool((leader < ar).all()), "a leader is not an earlier row"
    lead = ~has & (leader >= 0)
    assert bool(kept[leader[lead]].all()), "a leader is not a kept row"
    lower = torch.tril(torch.ones(n, n, dtype=torch.bool), -1) & kept[None, :]
    cbk = torch.where(lower, cb, torch.full_like(cb, -INF))
    bb = cbk.max(1).values if n else torch.zeros(0, dtype=cb.dtype)
    gotb = torch.where(lead, cb[ar, leader.clamp(min=0)], torch.full_like(bb, -INF))
    assert not bool((~has & (bb >= tau + tol) & ~lead).any()), "a clear in-batch repeat was missed"
    assert not bool(((bb < tau - tol) & lead).any()), "an in-batch leader below the threshold"
    assert bool((gotb[lead] >= tau - tol).all()) and bool((gotb[lead] >= bb[lead] - tol).all()), "not the best leader"
    assert bool(((cos[lead] - gotb[lead]).abs() <= tol).all()), "cos_out of an in-batch repeat"
    assert bool((cos[kept] == -INF).all()), "cos_out of a kept row"
    if bad is not None:
        assert bool(kept[bad].all()), "a degenerate row was not kept"


def find_repeats(bank, inv_norm, count, feats, tau, image=None, image_rows=None, n_image=None, rho=None,
                 lists_flag=None):
    CALLS["find_repeats"] += 1
    n = feats.shape[0]
    FIND_SIZES.append(n)
    assert feats.dtype == torch.float32 and n <= CONSOLIDATE_MAX_BATCH and 0.0 < tau <= 1.0
    stored, leader, cos = find_repeats_reference(bank, inv_norm, count, feats, tau)
    packed = torch.zeros(3 * n + 2, dtype=torch.int32)
    packed[:n], packed[n:2 * n] = stored.to(torch.int32), leader.to(torch.int32)
    packed[2 * n:3 * n] = cos.to(torch.float32).view(torch.int32)
    if lists_flag is not None:
        packed[3 * n + 1] = int(lists_flag.reshape(-1)[0])
    return packed[:n], packed[n:2 * n], packed[2 * n:3 * n].view(torch.float32), packed


def bank_touch(meta, count, rows, now):
    CALLS["touch"] += 1
    assert rows.dtype == torch.int32
    r = rows.reshape(-1).long()
    r = r[(r >= 0) & (r < count)]
    meta[r, 1] = now
