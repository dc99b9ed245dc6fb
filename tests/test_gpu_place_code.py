"""GPU tests of the place code (``aura_place_code``, ``aura_place_code_backward`` and everything above them) against
the rule restated in NumPy (tests/place_code_rule.py): winners by a stable sort, the rest in fp64 on the fp32 inputs.

Tolerances (from the formats, not from a run):
  idx      equal to the rule's in every row, no exclusion: selecting from given fp32 numbers has one right answer.
  act      ``|act - act_64| <= 2^-22``: expf within 1 ulp, one add, one divide, act <= 1.
  dense    bit-equal to ``act`` at the winners and +0.0 elsewhere.
  out      ``|out - out_64| <= 0.1 (k + 2) 2^-24 mag + 2^-23 |out_64|``, mag = sum_j |act_j W2t_j| + |b2|.
  g_z      ``<= (D + 3) 2^-24 * 0.1 * sum_d |g_out W2t_j| * 0.25 + 2^-23 |g_z64|`` at the winners (with a ``g_dense`` term
           one more rounding of that add, R.g_z_bound), exact zeros elsewhere.
  module   parameter gradients against the same formula from torch autograd ops in fp32 on the device with the kernel's
           winners.  Both sides are fp32 evaluations of the same sums in some order, each within ``T 2^-24 S`` of the
           exact value (T terms and roundings on the longest chain, S the sum of the terms' absolute values, computed
           here in fp64), so they differ by at most ``2 T 2^-24 S``; on top, torch's sigmoid and the kernel's may differ
           by 2^-22, which enters the sums through ``act`` and through ``act (1 - act)`` (|d| <= 2^-22 as well).
A measured maximum above half its bound is flagged in the recorded profile (``over_half_bound``).

Shapes ``(N, P, D, k)``: one element per lane, ragged tails, the limits (P = 8192, k = 256, k = P) and the reference's
three configurations.  Input kinds: random logits; logits rounded to multiples of 0.25 (the k-th value is tied in nearly
every row); all-equal rows (one of them a mix of -0.0 and +0.0); rows with +-0, +-inf and, in every other row, one NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers
from tests import place_code_rule as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 4, 1), (3, 100, 100, 3), (257, 500, 100, 15), (64, 1000, 768, 30), (64, 2000, 768, 60),
          (5, 4099, 36, 122), (2, 8192, 8, 256), (7, 64, 4, 64)]
KINDS = ["random", "quarter", "equal", "special"]
CASES = [(s, kind) for s in SHAPES for kind in KINDS]


def _id(case):
    (N, P, D, k), kind = case
    return f"N{N}-P{P}-D{D}-k{k}-{kind}"


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs and the rule's answers for one case, computed once and never modified."""
    (N, P, D, k), kind = case
    rng = np.random.default_rng(sum(map(ord, _id(case))))
    z = (2.0 * rng.standard_normal((N, P))).astype(np.float32)
    if kind == "quarter":
        z = (np.round(z * 4.0) / 4.0).astype(np.float32)
    elif kind == "equal":
        z[:] = rng.standard_normal((N, 1)).astype(np.float32)
        if N > 1:
            z[1] = np.where(rng.random(P) < 0.5, np.float32(-0.0), np.float32(0.0))
    elif kind == "special":
        for n in range(N):
            cells = rng.permutation(P)[:9]
            z[n, cells[:8]] = np.array([0.0, -0.0, 0.0, -0.0, np.inf, np.inf, -np.inf, -np.inf], np.float32)
            if n % 2 == 0:
                z[n, cells[8]] = np.float32(np.nan) if n % 4 == 0 else -np.float32(np.nan)
    e = rng.standard_normal((N, D)).astype(np.float32)
    w2t = (rng.standard_normal((P, D)) / np.sqrt(k)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(D)).astype(np.float32)
    r = R.rule(z, e, w2t, b2, k)
    if kind == "quarter" and P >= 500:
        srt = -np.sort(-z, axis=1)
        assert np.mean(srt[:, k - 1] == srt[:, k]) > 0.5, "the rounded logits hardly tie at the k-th value"
    for a in (z, e, w2t, b2, *r.values()):
        a.setflags(write=False)
    return dict(N=N, P=P, D=D, k=k, z=z, e=e, w2t=w2t, b2=b2, **r)


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inputs(case, dev):
    c = _case(case)
    return c, _dev(c["z"], dev), _dev(c["e"], dev), _dev(c["w2t"], dev), _dev(c["b2"], dev)


@functools.lru_cache(maxsize=None)
def _forward(case, dev):
    """The dense call of a case on the device, shared by the tests that compare with it."""
    from aura_snn_rag_amd import ops
    c, z, e, w, b = _inputs(case, dev)
    keep = z.clone(), e.clone(), w.clone(), b.clone()
    out, idx, act, dense = ops.place_code(z, e, w, b, c["k"])
    torch.cuda.synchronize()
    for a, b_ in zip((z, e, w, b), keep):
        assert torch.equal(_bits(a), _bits(b_)), "an input was written"
    return out, idx, act, dense


def _flag(frac):
    return dict(max_frac_of_bound=round(float(frac), 4), over_half_bound=bool(frac > 0.5))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_against_the_rule(dev, case):
    c = _case(case)
    out, idx, act, dense = _forward(case, dev)
    N, P, D, k = c["N"], c["P"], c["D"], c["k"]
    assert idx.dtype == torch.int32 and idx.shape == (N, k) and act.shape == (N, k)
    assert out.shape == (N, D) and dense.shape == (N, P)
    # winners: every row, exactly
    got_idx = idx.cpu().numpy()
    rows_equal = int(np.all(got_idx == c["idx"], axis=1).sum())
    helpers.record_parity(f"place idx {_id(case)}", rows_equal, N)
    assert rows_equal == N, f"{N - rows_equal} of {N} rows select other cells than the rule"
    # activations
    got_act = act.cpu().numpy().astype(np.float64)
    nan = np.isnan(c["act"])
    assert np.array_equal(np.isnan(got_act), nan)
    act_err = float(np.max(np.abs(got_act - c["act"])[~nan])) if (~nan).any() else 0.0
    # the dense code: the bits of act at the winners, +0.0 elsewhere
    want_dense = torch.zeros(N, P).scatter_(1, idx.cpu().long(), act.cpu())
    assert torch.equal(_bits(dense), _bits(want_dense)), "dense code bits"
    # out
    got = out.cpu().numpy().astype(np.float64)
    bad = np.isnan(c["out"])
    assert np.array_equal(np.isnan(got), bad)
    bound = R.out_bound(k, c["mag"], c["out"])
    err = np.abs(got - c["out"])
    frac = float(np.max(err[~bad] / bound[~bad])) if (~bad).any() else 0.0
    print(f"{_id(case)}: act error {act_err:.3e} ({act_err / R.U22:.3f} of 2^-22); out at {frac:.4f} of its bound")
    helpers.record_parity(f"place act {_id(case)}", int((np.abs(got_act - c["act"])[~nan] <= R.U22).sum()),
                          int((~nan).sum()), **_flag(act_err / R.U22))
    helpers.record_parity(f"place out {_id(case)}", int((err[~bad] <= bound[~bad]).sum()), int((~bad).sum()),
                          **_flag(frac))
    assert act_err <= R.U22
    assert np.all(err[~bad] <= bound[~bad]), f"max fraction of the bound: {frac}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_same_bits_again_without_the_dense_code_and_row_by_row(dev, case):
    from aura_snn_rag_amd import ops
    c, z, e, w, b = _inputs(case, dev)
    first = _forward(case, dev)
    again = ops.place_code(z, e, w, b, c["k"])
    for a, b_ in zip(first, again):
        assert torch.equal(_bits(a), _bits(b_)), "the same call gave other bits"
    out, idx, act, none = ops.place_code(z, e, w, b, c["k"], dense=False)
    assert none is None
    for a, b_ in zip(first[:3], (out, idx, act)):
        assert torch.equal(_bits(a), _bits(b_)), "dense=None changed another output"
    for n in sorted({0, c["N"] // 2, c["N"] - 1}):
        alone = ops.place_code(z[n:n + 1].contiguous(), e[n:n + 1].contiguous(), w, b, c["k"])
        for a, b_ in zip(first, alone):
            assert torch.equal(_bits(a[n:n + 1]), _bits(b_)), f"row {n} alone differs from row {n} in the batch"


BACKWARD = [(s, kind, gd) for s in SHAPES for kind, gd in (("random", False), ("random", True), ("quarter", True))]


@pytest.mark.parametrize("case", BACKWARD, ids=lambda c: _id(c[:2]) + ("-gdense" if c[2] else ""))
def test_backward_against_the_rule(dev, case):
    from aura_snn_rag_amd import ops
    fwd, with_dense = case[:2], case[2]
    c, z, e, w, b = _inputs(fwd, dev)
    _, idx, act, _ = _forward(fwd, dev)
    N, P, D, k = c["N"], c["P"], c["D"], c["k"]
    rng = np.random.default_rng(7 + sum(map(ord, _id(fwd))))
    g_out = rng.standard_normal((N, D)).astype(np.float32)
    g_dense = rng.standard_normal((N, P)).astype(np.float32) if with_dense else None
    g_z64, absdot = R.backward(g_out, g_dense, c["idx"], act.cpu().numpy(), c["w2t"])
    g_out_d, g_dense_d = _dev(g_out, dev), (_dev(g_dense, dev) if with_dense else None)
    keep = g_out_d.clone(), idx.clone(), act.clone(), w.clone()
    g_z = ops.place_code_backward(g_out_d, g_dense_d, idx, act, w)
    again = ops.place_code_backward(g_out_d, g_dense_d, idx, act, w)
    assert torch.equal(_bits(g_z), _bits(again)), "the same call gave other bits"
    for a, b_ in zip((g_out_d, idx, act, w), keep):
        assert torch.equal(_bits(a), _bits(b_)), "an input was written"
    got = g_z.cpu()
    win = torch.zeros(N, P, dtype=torch.bool).scatter_(1, idx.cpu().long(), True)
    assert bool((_bits(got)[~win] == 0).all()), "a cell that did not win has a gradient that is not +0.0"
    ii = c["idx"].astype(np.int64)
    at = np.take_along_axis(got.numpy().astype(np.float64), ii, axis=1)
    want = np.take_along_axis(g_z64, ii, axis=1)
    gd_at = np.take_along_axis(g_dense.astype(np.float64), ii, axis=1) if with_dense else None
    bound = R.g_z_bound(D, absdot, want, gd_at)
    err = np.abs(at - want)
    frac = float(np.max(err / np.maximum(bound, 1e-300)))
    name = _id(fwd) + ("-gdense" if with_dense else "")
    print(f"{name}: g_z at {frac:.4f} of its bound")
    helpers.record_parity(f"place g_z {name}", int((err <= bound).sum()), err.size, **_flag(frac))
    assert np.all(err <= bound), f"max fraction of the bound: {frac}"
    # a row alone gives the bits it has in the batch
    n = N // 2
    alone = ops.place_code_backward(g_out_d[n:n + 1].contiguous(), None if g_dense_d is None else
                                    g_dense_d[n:n + 1].contiguous(), idx[n:n + 1].contiguous(),
                                    act[n:n + 1].contiguous(), w)
    assert torch.equal(_bits(alone), _bits(g_z[n:n + 1]))


# ------------------------------------------------------------------------------------- the module
class _Cfg:
    def __init__(self, vocab, D, P):
        self.vocab_size, self.embedding_dim, self.n_place_cells = vocab, D, P


ACT = 2.0 ** -22


def _gradient_bounds(enc, ids, idx, act):
    """``{parameter name: bound}`` for ``loss = out.sum() + dense.mean()`` (the docstring's reasoning), in fp64."""
    N, k = idx.shape
    P, D = enc.config.n_place_cells, enc.config.embedding_dim
    d64 = lambda t: t.detach().double()
    e = d64(enc.token_embedding.weight)[ids.reshape(-1)]
    W1, W2 = d64(enc.semantic_projection.weight).abs(), d64(enc.place_to_semantic.weight).abs()
    act, ii = act.double(), idx.long()
    a_act = 0.1 * W2.t()[ii].sum(-1) + 1.0 / (N * P)                    # sum of |terms| of g_act, [N, k]
    counts = torch.bincount(ids.reshape(-1), minlength=enc.config.vocab_size).double()

    def sums(sp, code, ones):
        """S of every gradient, with act (1 - act) = sp, the code = code and the constant terms scaled by ones."""
        a_z = torch.zeros(N, P, dtype=torch.float64, device=idx.device).scatter_(1, ii, a_act * sp)
        dense = torch.zeros(N, P, dtype=torch.float64, device=idx.device).scatter_(1, ii, code)
        g_e = ones + a_z @ W1
        emb = torch.zeros_like(d64(enc.token_embedding.weight)).index_add_(0, ids.reshape(-1), g_e)
        return {"semantic_projection.weight": a_z.t() @ e.abs(), "semantic_projection.bias": a_z.sum(0),
                "place_to_semantic.weight": (0.1 * dense.sum(0)).expand(D, P),
                "place_to_semantic.bias": torch.full((D,), 0.1 * N * ones, dtype=torch.float64, device=idx.device),
                "token_embedding.weight": emb}

    S = sums(act * (1.0 - act), act, 1.0)
    delta = sums(torch.full_like(act, ACT), torch.full_like(act, ACT), 0.0)
    cmax = float(counts.max())
    T = {"semantic_projection.weight": D + N + 3, "semantic_projection.bias": D + N + 3,
         "place_to_semantic.weight": N + 2, "place_to_semantic.bias": N + 1, "token_embedding.weight": k + D + 4 + cmax}
    return {n: 2.0 * T[n] * R.U24 * S[n] + delta[n] for n in S}


@pytest.mark.parametrize("vocab,D,P,B,S", [(40, 36, 100, 3, 4), (64, 768, 2000, 2, 8)], ids=["P100-D36", "P2000-D768"])
def test_module_gradients_against_torch_autograd_with_the_kernels_winners(dev, vocab, D, P, B, S):
    from aura_snn_rag_amd.core.language_zone.place_cell_encoder import PlaceCellSemanticEncoder
    torch.manual_seed(21)
    enc = PlaceCellSemanticEncoder(_Cfg(vocab, D, P), None).to(dev)
    with torch.no_grad():
        enc.token_embedding.weight.mul_(50.0)                     # std 1: logits that spread
    ids = torch.randint(0, vocab, (B, S), generator=torch.Generator().manual_seed(22)).to(dev)
    ids[0, 1] = ids[0, 0]                                             # a token that occurs twice
    sem, dense = enc(ids)
    assert sem.shape == (B, S, D) and dense.shape == (B, S, P) and int((dense != 0).sum()) == B * S * enc.k
    (sem.sum() + dense.mean()).backward()
    got = {n: p.grad.detach().clone() for n, p in enc.named_parameters()}
    enc.zero_grad()
    # the sparse path: the same embedding bits, no dense tensor, the same gradients from the values
    sem_s, code = enc.forward_sparse(ids)
    assert torch.equal(_bits(sem_s), _bits(sem)) and torch.equal(_bits(code.to_dense()), _bits(dense))
    (sem_s.sum() + code.values.sum() / dense.numel()).backward()
    sparse = {n: p.grad.detach().clone() for n, p in enc.named_parameters()}
    enc.zero_grad()
    # the reference's formula from torch autograd ops, the winners given
    idx = code.indices.reshape(B * S, enc.k)
    e = enc.token_embedding(ids)
    z = enc.semantic_projection(e)
    ii = code.indices.long()
    ref_code = torch.zeros_like(z).scatter(-1, ii, torch.sigmoid(torch.gather(z, -1, ii)))
    ref_sem = e + 0.1 * enc.place_to_semantic(ref_code)
    (ref_sem.sum() + ref_code.mean()).backward()
    bounds = _gradient_bounds(enc, ids, idx, code.values.detach().reshape(B * S, enc.k))
    for n, p in enc.named_parameters():
        for label, g in (("dense", got[n]), ("sparse", sparse[n])):
            err = (g.double() - p.grad.double()).abs()
            frac = float((err / bounds[n].clamp_min(1e-300)).max())
            print(f"P{P}-D{D} {label} grad {n}: at {frac:.4f} of its bound")
            helpers.record_parity(f"place grad P{P}-D{D} {label} {n}", int((err <= bounds[n]).sum()), err.numel(),
                                  **_flag(frac))
            assert bool((err <= bounds[n]).all()), f"{n} ({label}): max fraction of the bound {frac}"
    # the table follows an optimizer step
    before = enc._table()
    torch.optim.SGD(enc.parameters(), lr=0.1).step()
    assert enc._table() is not before and torch.equal(enc._table(), enc.place_to_semantic.weight.detach().t())
