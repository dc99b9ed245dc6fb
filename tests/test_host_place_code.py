"""The place code without a GPU: the NumPy restatement of the rule (tests/place_code_rule.py) against answers known by
hand and against the reference module, the host-side argument checks of ``ops.place_code`` / ``place_code_backward``
(every one raised before the library is touched), and the module's plumbing on a CPU stand-in of the two ops
(tests/cpu_stub_place_code.py)."""
import types

import numpy as np
import pytest
import torch

from tests import cpu_stub_place_code as STUB
from tests import place_code_rule as R


def _config(vocab=50, D=100, P=500):
    return types.SimpleNamespace(vocab_size=vocab, embedding_dim=D, n_place_cells=P)


# ------------------------------------------------------------------------------------- the rule's own known answers
def test_all_equal_values_go_to_the_lowest_cells():
    z = np.full((2, 37), 1.25, np.float32)
    assert np.array_equal(R.winners(z, 5), np.tile(np.arange(5, dtype=np.int32), (2, 1)))


def test_the_two_zeros_tie_and_the_lower_cell_wins():
    assert R.winners(np.array([[-0.0, 0.0]], np.float32), 1).tolist() == [[0]]
    assert R.winners(np.array([[0.0, -0.0]], np.float32), 1).tolist() == [[0]]
    assert R.winners(np.array([[-1.0, -0.0, 0.0, -0.0]], np.float32), 2).tolist() == [[1, 2]]


def test_nan_ranks_first_then_inf():
    z = np.array([[1.0, np.inf, -np.inf, np.nan, 3.0, -np.nan]], np.float32)
    assert R.winners(z, 1).tolist() == [[3]]                   # the NaNs are equal: the lower cell
    assert R.winners(z, 2).tolist() == [[3, 5]]
    assert R.winners(z, 3).tolist() == [[1, 3, 5]]
    assert R.winners(z, 4).tolist() == [[1, 3, 4, 5]]


def test_k_equal_to_P_returns_every_cell_and_a_plain_sigmoid():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((3, 9)).astype(np.float32)
    e = rng.standard_normal((3, 4)).astype(np.float32)
    w = rng.standard_normal((9, 4)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    r = R.rule(z, e, w, b, 9)
    assert np.array_equal(r["idx"], np.tile(np.arange(9, dtype=np.int32), (3, 1)))
    s = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    assert np.array_equal(r["dense"], s) and np.array_equal(r["act"], s)
    want = e.astype(np.float64) + R.TENTH * (s @ w.astype(np.float64) + b.astype(np.float64))
    assert np.max(np.abs(r["out"] - want)) <= 1e-15
    assert np.all(r["mag"] >= np.abs(s @ w.astype(np.float64) + b) - 1e-15)


def test_winners_are_the_top_k_in_ascending_cell_order():
    z = np.array([[0.5, 2.0, -1.0, 2.0, 0.75, 2.0]], np.float32)
    assert R.winners(z, 2).tolist() == [[1, 3]]                # of three equal values the two lowest cells
    assert R.winners(z, 4).tolist() == [[1, 3, 4, 5]]
    r = R.rule(z, np.zeros((1, 2), np.float32), np.ones((6, 2), np.float32), np.zeros(2, np.float32), 2)
    assert np.count_nonzero(r["dense"]) == 2 and r["dense"][0, 1] == r["dense"][0, 3] == 1.0 / (1.0 + np.exp(-2.0))


def test_backward_rule_is_the_derivative_of_the_forward_rule():
    rng = np.random.default_rng(1)
    z = rng.standard_normal((2, 12)).astype(np.float32)
    e = rng.standard_normal((2, 3)).astype(np.float32)
    w = rng.standard_normal((12, 3)).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    g_out = rng.standard_normal((2, 3)).astype(np.float32)
    g_dense = rng.standard_normal((2, 12)).astype(np.float32)
    r = R.rule(z, e, w, b, 4)
    g_z, absdot = R.backward(g_out, g_dense, r["idx"], r["act"].astype(np.float32), w)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    idx = torch.from_numpy(r["idx"]).long()
    code = torch.zeros(2, 12, dtype=torch.float64).scatter(1, idx, torch.sigmoid(torch.gather(zt, 1, idx)))
    out = torch.tensor(e, dtype=torch.float64) + R.TENTH * (code @ torch.tensor(w, dtype=torch.float64)
                                                             + torch.tensor(b, dtype=torch.float64))
    ((out * torch.tensor(g_out, dtype=torch.float64)).sum()
     + (code * torch.tensor(g_dense, dtype=torch.float64)).sum()).backward()
    assert np.max(np.abs(zt.grad.numpy() - g_z)) <= 1e-7      # act enters the backward rule as its fp32 value
    assert np.all(absdot >= 0) and absdot.shape == (2, 4)


# ------------------------------------------------------------------------------------- the rule against the reference
def test_the_rule_matches_the_reference_module():
    from oracle import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    ref_mod = _ref_loader.load("core.language_zone.place_cell_encoder")
    cfg = _config()
    torch.manual_seed(11)
    ref = ref_mod.PlaceCellSemanticEncoder(cfg, None)
    ids = torch.randint(0, cfg.vocab_size, (3, 7), generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        sem, dense = ref(ids)
        e = ref.token_embedding(ids).reshape(21, -1)
        z = ref.semantic_projection(e)
    k = ref.k
    assert k == 15
    srt = np.sort(z.numpy().astype(np.float64), axis=1)[:, ::-1]
    assert np.all(srt[:, k - 1] > srt[:, k]), "the seeded logits tie at the k-th value: the comparison needs none"
    r = R.rule(z.numpy(), e.numpy(), ref.place_to_semantic.weight.detach().t().contiguous().numpy(),
               ref.place_to_semantic.bias.detach().numpy(), k)
    dense = dense.reshape(21, -1).numpy()
    for n in range(21):
        assert np.array_equal(np.nonzero(dense[n])[0], r["idx"][n]), f"winner set of token {n}"
    code_err = float(np.max(np.abs(dense.astype(np.float64) - r["dense"])))
    err = np.abs(sem.reshape(21, -1).numpy().astype(np.float64) - r["out"])
    frac = float(np.max(err / R.out_bound(k, r["mag"], r["out"])))
    print(f"reference vs rule: code error {code_err:.2e} (bound {R.U22:.2e}), output at {frac:.3f} of its bound")
    assert code_err <= R.U22
    assert frac <= 1.0


# ------------------------------------------------------------------------------------- ops: argument checks
def _args(N=4, P=64, D=8):
    return torch.zeros(N, P), torch.zeros(N, D), torch.zeros(P, D), torch.zeros(D)


def test_ops_refuse_cpu_tensors():
    from aura_snn_rag_amd import ops
    z, e, w, b = _args()
    with pytest.raises(ops.AuraDeviceError):
        ops.place_code(z, e, w, b, 3)
    with pytest.raises(ops.AuraDeviceError):
        ops.place_code_backward(e, None, torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3), w)


def test_ops_raise_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    z, e, w, b = _args()
    bad = [
        (dict(k=0), ValueError, "k < 1"),
        (dict(k=65), ValueError, "k > P"),
        (dict(z=torch.zeros(4, 600), w=torch.zeros(600, 8), k=257), ValueError, "k > 256"),
        (dict(z=torch.zeros(4, 8193), w=torch.zeros(8193, 8)), ValueError, "P > 8192"),
        (dict(e=torch.zeros(4, 0), w=torch.zeros(64, 0), b=torch.zeros(0)), ValueError, "D < 1"),
        (dict(z=torch.zeros(64)), ValueError, "rank"),
        (dict(e=torch.zeros(5, 8)), ValueError, "N"),
        (dict(w=torch.zeros(8, 64)), ValueError, "w2t is [P, D]"),
        (dict(b=torch.zeros(7)), ValueError, "b2"),
        (dict(z=torch.zeros(4, 128)[:, ::2]), ValueError, "non-contiguous z"),
        (dict(w=torch.zeros(8, 64).t()), ValueError, "non-contiguous w2t"),
        (dict(z=z.bfloat16()), TypeError, "bf16 logits"),
        (dict(e=e.half()), TypeError, "fp16 embeddings"),
        (dict(w=w.double()), TypeError, "fp64 table"),
        (dict(k=3.0), TypeError, "float k"),
    ]
    for change, exc, why in bad:
        a = dict(z=z, e=e, w=w, b=b, k=3)
        a.update(change)
        with pytest.raises(exc):
            ops.place_code(a["z"], a["e"], a["w"], a["b"], a["k"])
            pytest.fail(f"accepted: {why}")
    for t in (z.bfloat16(), z.half()):
        with pytest.raises(TypeError, match="fp32"):
            ops.place_code(t, e, w, b, 3)
    idx, act = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3)
    bad = [
        (dict(idx=idx.long()), TypeError, "int64 idx"),
        (dict(act=torch.zeros(4, 2)), ValueError, "act shape"),
        (dict(g_dense=torch.zeros(4, 63)), ValueError, "g_dense shape"),
        (dict(g_out=torch.zeros(4, 7)), ValueError, "D"),
        (dict(g_out=e.bfloat16()), TypeError, "bf16 gradient"),
        (dict(idx=torch.zeros(4, 65, dtype=torch.int32), act=torch.zeros(4, 65)), ValueError, "k > P"),
    ]
    for change, exc, why in bad:
        a = dict(g_out=e, g_dense=None, idx=idx, act=act, w=w)
        a.update(change)
        with pytest.raises(exc):
            ops.place_code_backward(a["g_out"], a["g_dense"], a["idx"], a["act"], a["w"])
            pytest.fail(f"accepted: {why}")
    # valid calls get as far as the device check, still without the library
    with pytest.raises(ops.AuraDeviceError):
        ops.place_code(z, e, w, b, 64)
    with pytest.raises(ops.AuraDeviceError):
        ops.place_code_backward(e, torch.zeros(4, 64), idx, act, w)


# ------------------------------------------------------------------------------------- the module on the CPU stand-in
def _encoder(seed=0, **kw):
    from aura_snn_rag_amd.core.language_zone.place_cell_encoder import PlaceCellSemanticEncoder
    torch.manual_seed(seed)
    return PlaceCellSemanticEncoder(_config(**kw), hippocampus="the formation")


def test_the_module_keeps_the_reference_surface():
    import aura_snn_rag_amd
    from aura_snn_rag_amd.core.language_zone import place_cell_encoder as M
    assert aura_snn_rag_amd.PlaceCellSemanticEncoder is M.PlaceCellSemanticEncoder
    assert aura_snn_rag_amd.PlaceCode is M.PlaceCode
    enc = _encoder()
    assert list(enc.state_dict()) == ["token_embedding.weight", "semantic_projection.weight",
                                      "semantic_projection.bias", "place_to_semantic.weight", "place_to_semantic.bias"]
    assert enc.sparsity == 0.03 and enc.k == 15 and enc.hippocampus == "the formation"
    assert "n_place_cells=500" in repr(enc) and "sparsity=3.0% (k=15)" in repr(enc)
    assert M.PlaceCode._fields == ("indices", "values", "n_cells")
    with pytest.raises(ValueError):
        _encoder(P=20)                                          # k = int(0.6) = 0
    big = _encoder(vocab=8, D=4, P=2000)
    assert big.k == 60


def test_the_module_refuses_the_cpu_and_half_precision():
    from aura_snn_rag_amd import ops
    enc = _encoder()
    ids = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ops.AuraDeviceError):
        enc(ids)
    with pytest.raises(ops.AuraDeviceError):
        enc.forward_sparse(ids)
    for half in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="fp32"):
            _encoder().to(half)(ids)


def test_forward_reshapes_and_returns_the_dense_code(monkeypatch):
    STUB.install(monkeypatch)
    enc = _encoder()
    ids = torch.randint(0, 50, (2, 5), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        sem, dense = enc(ids)
        sem_s, code = enc.forward_sparse(ids)
    assert STUB.CALLS["forward"] == 2 and STUB.LAST["shapes"] == (10, 500, 100, 15) and STUB.LAST["dense"] is False
    assert sem.shape == (2, 5, 100) and dense.shape == (2, 5, 500)
    assert code.indices.shape == (2, 5, 15) and code.indices.dtype == torch.int32 and code.n_cells == 500
    assert code.values.shape == (2, 5, 15)
    assert torch.equal(sem, sem_s) and torch.equal(code.to_dense(), dense)
    assert int((dense != 0).sum()) == 10 * 15
    # against the reference's own op sequence on the same parameters (no ties in seeded Gaussian logits)
    with torch.no_grad():
        e = enc.token_embedding(ids)
        z = enc.semantic_projection(e)
        v, i = torch.topk(z, enc.k, dim=-1)
        want_dense = torch.zeros_like(z).scatter(-1, i, torch.sigmoid(v))
        want = e + 0.1 * enc.place_to_semantic(want_dense)
    assert torch.equal(dense, want_dense)
    assert torch.allclose(sem, want, rtol=0, atol=1e-6)
    # one token's pattern is its row of the dense code (torch's Linear before it is not batch-invariant to the bit)
    with torch.no_grad():
        one = enc.get_place_cell_pattern(int(ids[1, 2]))
    assert one.shape == (500,) and torch.equal(one != 0, dense[1, 2] != 0)
    assert torch.allclose(one, dense[1, 2], rtol=0, atol=1e-6)
    # encode_logits: any leading shape, and a shape that disagrees is refused
    with torch.no_grad():
        out3, code3, dense3 = enc.encode_logits(z[0, :3], e[0, :3])
    assert torch.equal(out3, sem[0, :3]) and torch.equal(dense3, dense[0, :3]) and code3.indices.shape == (3, 15)
    with pytest.raises(ValueError):
        enc.encode_logits(z, e[:, :4])


def test_the_transposed_table_follows_the_weight(monkeypatch):
    STUB.install(monkeypatch)
    enc = _encoder()
    ids = torch.zeros(1, 2, dtype=torch.long)
    with torch.no_grad():
        a, _ = enc(ids)
        first = STUB.LAST["w2t"]
        assert first.shape == (500, 100) and first.is_contiguous() and not first.requires_grad
        assert torch.equal(first, enc.place_to_semantic.weight.detach().t())
        enc(ids)
        assert STUB.LAST["w2t"] is first, "the table was rebuilt although the weight did not change"
        enc.place_to_semantic.weight.mul_(2.0)                       # in place: the version counter moves
        b, _ = enc(ids)
        assert STUB.LAST["w2t"] is not first
        assert torch.equal(STUB.LAST["w2t"], enc.place_to_semantic.weight.detach().t())
        assert not torch.equal(a, b)
        second = STUB.LAST["w2t"]
        enc.place_to_semantic.weight.data = enc.place_to_semantic.weight.data.clone()   # a new allocation
        enc(ids)
        assert STUB.LAST["w2t"] is not second
    # an optimizer step writes in place too
    opt = torch.optim.SGD(enc.parameters(), lr=0.5)
    sem, dense = enc(ids)
    (sem.sum() + dense.mean()).backward()
    before = STUB.LAST["w2t"]
    opt.step()
    with torch.no_grad():
        enc(ids)
    assert STUB.LAST["w2t"] is not before and torch.equal(STUB.LAST["w2t"], enc.place_to_semantic.weight.detach().t())


def test_gradients_reach_every_parameter(monkeypatch):
    STUB.install(monkeypatch)
    enc = _encoder(seed=4)
    ids = torch.randint(0, 50, (2, 5), generator=torch.Generator().manual_seed(5))
    sem, dense = enc(ids)
    (sem.sum() + dense.mean()).backward()
    assert STUB.CALLS["backward"] == 1
    got = {n: p.grad.clone() for n, p in enc.named_parameters()}
    assert set(got) == set(dict(enc.named_parameters())) and all(g is not None for g in got.values())
    # the same loss from torch autograd ops with the same winners
    enc.zero_grad()
    e = enc.token_embedding(ids)
    z = enc.semantic_projection(e)
    idx = enc.forward_sparse(ids)[1].indices.long()
    code = torch.zeros_like(z).scatter(-1, idx, torch.sigmoid(torch.gather(z, -1, idx)))
    sem2 = e + 0.1 * enc.place_to_semantic(code)
    (sem2.sum() + code.mean()).backward()
    for n, p in enc.named_parameters():
        assert torch.allclose(got[n], p.grad, rtol=1e-4, atol=1e-6), n
    # forward_sparse is differentiable as well: values carry the gradient of the code
    enc.zero_grad()
    sem3, sparse = enc.forward_sparse(ids)
    (sem3.sum() + sparse.values.sum() / dense.numel()).backward()
    for n, p in enc.named_parameters():
        assert torch.allclose(got[n], p.grad, rtol=1e-4, atol=1e-6), n
