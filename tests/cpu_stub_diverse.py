"""The diverse-recall rule in torch fp64 on the CPU, a replay check of a device's picks against it, and a CPU
``diverse_select`` for the host tests, on top of ``tests/cpu_stub_retention.py`` -- TEST INFRASTRUCTURE ONLY.

The rule (``include/aura_hip.h``): candidates j = 0..F-1 in rank order, valid if 0 <= row < count and the score is
not NaN; cos(i, j) = dot product of bank[row_i] * inv_norm[row_i] and bank[row_j] * inv_norm[row_j]; S = picks so
far, m(c) = max cos(c, S); eligible = valid, unpicked and (S empty or m(c) < tau); value = (1 - d) score[c] while S
is empty, else (1 - d) score[c] - d m(c); the largest value wins, equal values go to the smallest j; k picks at most;
output = the picks' rows and score bits in pick order, then -1 / -inf."""
import torch

from tests.cpu_stub_retention import *          # noqa: F401,F403  (the stand-ins of every other op)
from tests.cpu_stub_retention import CALLS, KNN_FLAG_NO_CANDIDATES, KNN_FLAG_LISTS_STALE, AuraDeviceError  # noqa: F401

DIVERSE_MAX_CANDIDATES = 128
CALLS["diverse"] = 0
LAST = {}                                         # arguments of the most recent stub diverse_select

INF = float("inf")


def tolerance(D: int) -> float:
    """Two fp32 cosines of unit rows are compared: each is within (D + 8) 2^-24 of the exact one (dot-product bound
    plus the two inv_norm roundings)."""
    return 2.0 * (D + 8) * 2.0 ** -24


def valid_mask(cand_rows, cand_scores, count):
    r = cand_rows.long()
    return (r >= 0) & (r < count) & ~torch.isnan(cand_scores)


def cosines(bank, inv_norm, cand_rows, count, dtype=torch.float64, chunk=50):
    """[nq, F, F] cosines of the candidates' rows (zero rows and columns for candidates outside [0, count))."""
    rows = cand_rows.cpu().long()
    ok = (rows >= 0) & (rows < count)
    b, inv = bank.cpu(), inv_norm.cpu()
    nq, F = rows.shape
    out = torch.zeros(nq, F, F, dtype=dtype)
    for lo in range(0, nq, chunk):
        r = rows[lo:lo + chunk].clamp(0, max(count - 1, 0))
        x = b[r].to(dtype) * inv[r].to(dtype).unsqueeze(-1) * ok[lo:lo + chunk].unsqueeze(-1)
        out[lo:lo + chunk] = x @ x.transpose(1, 2)
    return out


def _values(sc, m, d, first):
    return (1.0 - d) * sc if first else (1.0 - d) * sc - d * m


def select_reference(cand_rows, cand_scores, cos, count, k, d, tau=None):
    """The rule, every query at once: ``(picks [nq, k] candidate numbers or -1, margin [nq])`` -- margin = the
    smallest gap, over the steps taken, between the best and the runner-up value and between any unpicked valid
    candidate's m and tau (a query whose margin is at least the tolerance is DECIDED: rounding cannot change it)."""
    sc = cand_scores.cpu().to(cos.dtype)
    valid = valid_mask(cand_rows.cpu(), cand_scores.cpu(), count)
    nq, F = valid.shape
    tau = INF if tau is None else float(tau)
    ar = torch.arange(nq)
    picked = torch.zeros(nq, F, dtype=torch.bool)
    m = torch.full((nq, F), -INF, dtype=cos.dtype)
    picks = torch.full((nq, k), -1, dtype=torch.int64)
    margin = torch.full((nq,), INF, dtype=cos.dtype)
    alive = torch.ones(nq, dtype=torch.bool)
    for s in range(k):
        elig = valid & ~picked & ((m < tau) if s else torch.ones_like(valid))
        val = torch.where(elig, _values(sc, m, d, s == 0), torch.full_like(sc, -INF))
        go = alive & elig.any(1)
        best = val.argmax(1)                      # the first of equal maxima: the smallest j
        second = val.clone()
        second[ar, best] = -INF
        gap = val[ar, best] - second.max(1).values
        gap = torch.where(torch.isnan(gap), torch.full_like(gap, INF), gap)
        if s and tau < INF:
            near = torch.where(valid & ~picked, (m - tau).abs(), torch.full_like(m, INF)).min(1).values
            gap = torch.minimum(gap, near)
        margin = torch.where(go, torch.minimum(margin, gap), margin)
        picks[go, s] = best[go]
        alive = go
        picked[ar[go], best[go]] = True
        m[go] = torch.maximum(m[go], cos[ar[go], best[go]])
    return picks, margin


def output_of(picks, cand_rows, cand_scores):
    """(scores, rows) the library returns for these picks."""
    p = picks.clamp(min=0)
    rows = torch.where(picks >= 0, cand_rows.gather(1, p), torch.full_like(p, -1, dtype=cand_rows.dtype))
    scores = torch.where(picks >= 0, cand_scores.gather(1, p), torch.full(p.shape, -INF, dtype=cand_scores.dtype))
    return scores, rows


def picks_of(out_rows, cand_rows, cand_scores, count):
    """Candidate numbers of a result's rows ([nq, k], -1 for padding); every returned row must be exactly one valid
    candidate of its query."""
    rows, out = cand_rows.cpu().long(), out_rows.cpu().long()
    valid = valid_mask(cand_rows.cpu(), cand_scores.cpu(), count)
    filled = out >= 0
    match = (rows[:, None, :] == out[:, :, None]) & valid[:, None, :]
    assert bool((match.sum(2)[filled] == 1).all()), "a returned row is not (exactly one) valid candidate of its query"
    pj = match.to(torch.int8).argmax(2)
    pj[~filled] = -1
    return pj


def replay_check(cand_rows, cand_scores, cos, count, k, d, tau, out_scores, out_rows, tol):
    """Check 1 of the feature's tests, every query: given the result's OWN earlier picks, each pick is valid, unpicked,
    has m < tau + tol and a value no less than the best value among candidates with m < tau - tol, minus tol; a result
    that stops early leaves no candidate with m < tau - tol; rows come from the candidate list, none twice; scores are
    the candidates' bits; padding is -1 / -inf to the end.  Returns the picks as candidate numbers."""
    cand_rows, cand_scores = cand_rows.cpu(), cand_scores.cpu()
    out_scores, out_rows = out_scores.cpu(), out_rows.cpu()
    nq, F = cand_rows.shape
    assert out_rows.shape == (nq, k) and out_scores.shape == (nq, k)
    assert out_rows.dtype == torch.int32 and out_scores.dtype == torch.float32
    pj = picks_of(out_rows, cand_rows, cand_scores, count)
    filled = pj >= 0
    assert bool((filled[:, 1:] <= filled[:, :-1]).all()), "padding before a pick"
    want_s, want_r = output_of(pj, cand_rows, cand_scores)
    assert torch.equal(out_rows, want_r)
    assert torch.equal(out_scores.view(torch.int32), want_s.view(torch.int32)), "scores are not the candidates' bits"
    sc = cand_scores.to(cos.dtype)
    valid = valid_mask(cand_rows, cand_scores, count)
    tau = INF if tau is None else float(tau)
    ar = torch.arange(nq)
    picked = torch.zeros(nq, F, dtype=torch.bool)
    m = torch.full((nq, F), -INF, dtype=cos.dtype)
    for s in range(k):
        f = filled[:, s]
        p = pj[:, s].clamp(min=0)
        clearly = valid & ~picked & ((m < tau - tol) if s else torch.ones_like(valid))
        val = _values(sc, m, d, s == 0)
        best = torch.where(clearly, val, torch.full_like(val, -INF)).max(1).values
        assert not bool((clearly.any(1) & ~f).any()), f"step {s}: a result stopped while a candidate was eligible"
        assert bool(valid[ar, p][f].all()), f"step {s}: an invalid candidate was picked"
        assert not bool(picked[ar, p][f].any()), f"step {s}: a candidate was picked twice"
        if s:
            assert bool((m[ar, p] < tau + tol)[f].all()), f"step {s}: a pick is too similar to an earlier one"
        short = (val[ar, p] < best - tol) & f
        assert not bool(short.any()), (f"step {s}: {int(short.sum())} picks fall short of the best value by more than "
                                       f"tol, worst {float((best - val[ar, p])[short].max()):.3e}")
        picked[ar[f], p[f]] = True
        m[f] = torch.maximum(m[f], cos[ar[f], p[f]])
    return pj


def diverse_select(bank, inv_norm, count, cand_rows, cand_scores, k, diversity=0.0, max_similarity=None):
    CALLS["diverse"] += 1
    assert cand_rows.dtype == torch.int32 and cand_scores.dtype == torch.float32 and cand_rows.shape == cand_scores.shape
    assert 1 <= k <= cand_rows.shape[1] <= DIVERSE_MAX_CANDIDATES and 0.0 <= diversity <= 1.0
    LAST.update(F=cand_rows.shape[1], k=k, diversity=diversity, max_similarity=max_similarity, count=count,
                cand_rows=cand_rows.clone(), cand_scores=cand_scores.clone())
    cos = cosines(bank, inv_norm, cand_rows, count)
    picks, _ = select_reference(cand_rows, cand_scores, cos, count, k, diversity, max_similarity)
    return output_of(picks, cand_rows, cand_scores)
