"""Theta-gamma positions without a GPU: the NumPy restatement of the rule (tests/theta_gamma_rule.py) against answers
known by hand, against fp64 autograd and against the reference module; the committed fixture
``tests/golden/theta_gamma.pt`` against the reference that wrote it; the host-side argument checks of the three ops
(every one raised before the library is touched); and the module's plumbing on a CPU stand-in of the ops
(tests/cpu_stub_theta_gamma.py)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import cpu_stub_theta_gamma as STUB
from tests import theta_gamma_rule as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "theta_gamma.pt")
GOLDEN_POSITIONS = list(range(30)) + [511, 512, 1000, 4095, 100000, 7, 7, 3, 65536, 99999]


def _config(D=100, max_seq_len=512, theta=8.0, gamma=40.0):
    return types.SimpleNamespace(embedding_dim=D, theta_frequency=theta, gamma_frequency=gamma, max_seq_len=max_seq_len)


def _params(D, seed=0):
    rng = np.random.default_rng(seed)
    return ((0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32),
            (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32))


# ------------------------------------------------------------------------------------- the rule's own known answers
def test_zero_amplitude_gives_exactly_zero():
    th, ga, _ = _params(9)
    t = R.table(np.arange(5, dtype=np.float32), th, ga, np.zeros(9, np.float32), 512, R.ratio(8, 40))
    assert np.all(t["pe"] == 0.0) and np.all(t["d_theta"] == 0.0) and np.all(t["d_gamma"] == 0.0)
    assert np.all(np.abs(t["d_amp"]) > 0.0)


def test_max_seq_len_one_divides_by_one_and_position_zero_leaves_the_offsets():
    th, ga, amp = _params(7)
    a, g = R.phases(np.array([0.0, 1.0, 3.0], np.float32), th, ga, 1, R.ratio(8, 40))
    assert np.array_equal(a[0], th) and np.array_equal(g[0], ga)          # position 0: a = theta_off
    assert np.array_equal(a[1], (R.TWO_PI + th).astype(np.float32))        # denom = max(0, 1) = 1
    assert np.array_equal(a[2], ((np.float32(3.0) * R.TWO_PI).astype(np.float32) + th).astype(np.float32))
    a2, _ = R.phases(np.array([1.0], np.float32), th, ga, 2, R.ratio(8, 40))
    assert np.array_equal(a2, a[1:2])                                      # max_seq_len = 2 also divides by 1
    assert float(R.ratio(8.0, 40.0)) == 5.0


def test_derivatives_match_fp64_autograd_of_the_forward_rule():
    th, ga, amp = _params(11, seed=3)
    pos = np.array([0, 1, 5, 40, 700], np.float32)
    r = R.ratio(8.0, 40.0)
    t = R.table(pos, th, ga, amp, 512, r)
    # the phases as functions of the offsets: a = phi + th, g = phi r + ga; differentiate the fp64 rule at the fp32 phases
    dth, dga, m = (torch.zeros(5, 11, dtype=torch.float64, requires_grad=True) for _ in range(3))
    a = torch.from_numpy(t["a"].astype(np.float64)) + dth
    g = torch.from_numpy(t["g"].astype(np.float64)) + dga
    q = torch.sin(a) + 0.5 * (((torch.cos(a) + 1.0) * 0.5) * torch.sin(g))
    pe = q * (torch.from_numpy(amp.astype(np.float64)) + m)
    assert np.max(np.abs(pe.detach().numpy() - t["pe"])) <= 1e-15
    pe.sum().backward()
    for name, got in (("d_theta", dth.grad), ("d_gamma", dga.grad), ("d_amp", m.grad)):
        assert np.max(np.abs(got.numpy() - t[name])) <= 1e-14, name


def test_chain_lengths_follow_the_kernel_geometry():
    # D % 4 == 0: float4 units, four elements per unit and lane; else one float per unit
    assert [R.elements_per_lane(D) for D in (1, 63, 64, 65, 100, 36, 768, 1024, 2047, 2048)] == \
        [1, 1, 4, 2, 4, 4, 12, 16, 32, 32]
    assert R.T_D(768) == 19 and R.groups(1) == 1 and R.groups(4096) == 256 and R.groups(10 ** 6) == 1024
    assert R.T_N(4096) == 4 + 3 + 32 + 8 and R.T_N(1) == 1 + 3 + 1 + 8
    # the library, the wrapper that sizes the workspace and the rule agree on G
    from aura_snn_rag_amd import _lib, ops
    for N in (0, 1, 15, 16, 17, 645, 4096, 16383, 16384, 16385, 10 ** 6, 2 ** 31 - 1):
        assert _lib.load().aura_theta_gamma_groups(N) == ops.theta_gamma_groups(N) == R.groups(N), N


def test_norm_rule_is_layer_norm_and_its_backward():
    rng = np.random.default_rng(5)
    h = (3.0 + rng.standard_normal((4, 37))).astype(np.float32)
    w, b = rng.standard_normal(37).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    g_y = rng.standard_normal((4, 37)).astype(np.float32)
    f = R.norm(h, w, b, 1e-5)
    ht = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(ht, (37,), torch.tensor(w, dtype=torch.float64), torch.tensor(b, dtype=torch.float64), 1e-5)
    assert np.max(np.abs(y.detach().numpy() - f["y"])) <= 1e-13
    (y * torch.tensor(g_y, dtype=torch.float64)).sum().backward()
    bw = R.norm_backward(h, w, g_y, 1e-5)
    assert np.max(np.abs(ht.grad.numpy() - bw["g_x"])) <= 1e-12
    assert np.all(bw["g_x_bound"] > 0) and np.all(f["y_bound"] > 0)


# ------------------------------------------------------------------------------------- the rule against the reference
def _reference():
    from oracle import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    return _ref_loader.load("core.language_zone.theta_gamma_encoding")


def _golden_from_reference(ref_mod):
    torch.manual_seed(31)
    ref = ref_mod.ThetaGammaPositionalEncoding(_config())
    with torch.no_grad():
        ref.amplitude_modulation.add_(0.2 * torch.randn(100))
        positions = torch.tensor(GOLDEN_POSITIONS, dtype=torch.float32)
        out = ref(positions[None], 40)
    return dict(theta_phase_offsets=ref.theta_phase_offsets.detach().clone(),
                gamma_phase_offsets=ref.gamma_phase_offsets.detach().clone(),
                amplitude_modulation=ref.amplitude_modulation.detach().clone(), positions=positions, output=out[0].clone(),
                max_seq_len=512, theta_frequency=8.0, gamma_frequency=40.0)


@pytest.mark.parametrize("D,scale", [(768, 1), (100, 1), (768, 200), (100, 200)])
def test_the_rule_matches_the_reference_module(D, scale):
    ref_mod = _reference()
    torch.manual_seed(D + scale)
    ref = ref_mod.ThetaGammaPositionalEncoding(_config(D=D))
    with torch.no_grad():
        ref.amplitude_modulation.add_(0.2 * torch.randn(D))
    positions = torch.arange(0, 512 * scale, 7 * scale)
    with torch.no_grad():
        out = ref(positions[None], positions.numel())[0].numpy().astype(np.float64)
    th, ga, amp = (p.detach().numpy() for p in (ref.theta_phase_offsets, ref.gamma_phase_offsets,
                                                 ref.amplitude_modulation))
    t = R.table(positions.numpy().astype(np.float32), th, ga, amp, ref.max_seq_len, R.ratio(ref.theta_freq, ref.gamma_freq))
    frac = float(np.max(np.abs(out - t["pe"]) / R.pe_bound(amp[None, :], t["pe"])))
    print(f"reference vs rule, D={D}, positions up to {int(positions[-1])}: {frac:.3f} of the pe bound")
    assert frac <= 1.0


def test_the_golden_fixture_is_what_the_reference_computes():
    want = _golden_from_reference(_reference())
    have = torch.load(GOLDEN)
    assert set(have) == set(want)
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(have[k], v), k
        else:
            assert have[k] == v, k


def test_the_golden_fixture_is_within_the_pe_bound_of_the_rule():
    g = torch.load(GOLDEN)
    assert g["output"].shape == (40, 100) and os.path.getsize(GOLDEN) < 64 * 1024
    amp = g["amplitude_modulation"].numpy()
    t = R.table(g["positions"].numpy(), g["theta_phase_offsets"].numpy(), g["gamma_phase_offsets"].numpy(), amp,
                g["max_seq_len"], R.ratio(g["theta_frequency"], g["gamma_frequency"]))
    err = np.abs(g["output"].numpy().astype(np.float64) - t["pe"])
    assert np.all(err <= R.pe_bound(amp[None, :], t["pe"]))


# ------------------------------------------------------------------------------------- ops: argument checks
def _vectors(D=8):
    return torch.zeros(D), torch.zeros(D), torch.ones(D)


def test_ops_refuse_cpu_tensors():
    from aura_snn_rag_amd import ops
    th, ga, amp = _vectors()
    x, tab = torch.zeros(6, 8), torch.zeros(3, 8)
    with pytest.raises(ops.AuraDeviceError):
        ops.theta_gamma_table(th, ga, amp, 512, 5.0, rows=3)
    with pytest.raises(ops.AuraDeviceError):
        ops.theta_gamma_norm(x, tab, amp, th, 3)
    with pytest.raises(ops.AuraDeviceError):
        ops.theta_gamma_norm_backward(x, x, tab, None, torch.zeros(6), torch.ones(6), amp, 3)


def test_ops_raise_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    assert ops.THETA_MAX_D == 2048
    th, ga, amp = _vectors()
    big = torch.zeros(2049)
    bad = [
        (dict(), ValueError, "neither positions nor rows"),
        (dict(rows=-1), ValueError, "negative rows"),
        (dict(rows=3.0), TypeError, "float rows"),
        (dict(rows=3, start=1.5), TypeError, "float start"),
        (dict(rows=3, positions=torch.zeros(3)), ValueError, "positions and rows"),
        (dict(positions=torch.zeros(3), start=2), ValueError, "positions and start"),
        (dict(positions=torch.zeros(2, 3)), ValueError, "positions rank"),
        (dict(positions=torch.zeros(3, dtype=torch.int64)), TypeError, "integer positions"),
        (dict(positions=torch.zeros(6)[::2]), ValueError, "non-contiguous positions"),
        (dict(rows=3, ga=torch.zeros(7)), ValueError, "gamma_off length"),
        (dict(rows=3, th=torch.zeros(2, 4), ga=torch.zeros(2, 4), amp=torch.zeros(2, 4)), ValueError, "rank"),
        (dict(rows=3, th=big, ga=big, amp=big), ValueError, "D > 2048"),
        (dict(rows=3, th=big[:0], ga=big[:0], amp=big[:0]), ValueError, "D < 1"),
        (dict(rows=3, max_seq_len=0), ValueError, "max_seq_len < 1"),
        (dict(rows=3, max_seq_len=512.0), ValueError, "float max_seq_len"),
        (dict(rows=2 ** 31), ValueError, "R > 2^31 - 1"),
        (dict(rows=3, amp=amp.half()), TypeError, "fp16 amplitude"),
        (dict(rows=3, th=th.bfloat16()), TypeError, "bf16 offsets"),
        (dict(rows=3, ga=None), ValueError, "missing gamma_off"),
        (dict(rows=3, pe=False), ValueError, "nothing to compute"),
    ]
    for change, exc, why in bad:
        a = dict(th=th, ga=ga, amp=amp, max_seq_len=512, positions=None, start=0, rows=None, pe=True)
        a.update(change)
        with pytest.raises(exc):
            ops.theta_gamma_table(a["th"], a["ga"], a["amp"], a["max_seq_len"], 5.0, positions=a["positions"],
                                  start=a["start"], rows=a["rows"], pe=a["pe"])
            pytest.fail(f"accepted: {why}")
    with pytest.raises(ValueError):
        ops.theta_gamma_ratio(0.0, 40.0)
    assert ops.theta_gamma_ratio(8.0, 40.0) == 5.0

    x, tab, w, b = torch.zeros(6, 8), torch.zeros(3, 8), torch.ones(8), torch.zeros(8)
    bad = [
        (dict(seq_len=4), ValueError, "a table of 3 rows for sequences of 4"),
        (dict(tab=torch.zeros(4, 8), seq_len=4), ValueError, "N no multiple of seq_len"),
        (dict(seq_len=0), ValueError, "seq_len < 1"),
        (dict(seq_len=3.0), ValueError, "float seq_len"),
        (dict(tab=torch.zeros(3, 7)), ValueError, "table D"),
        (dict(w=torch.ones(7)), ValueError, "w length"),
        (dict(b=torch.zeros(9)), ValueError, "b length"),
        (dict(x=torch.zeros(6)), ValueError, "x rank"),
        (dict(x=torch.zeros(6, 2049), tab=torch.zeros(3, 2049), w=big, b=big), ValueError, "D > 2048"),
        (dict(x=torch.zeros(6, 16)[:, ::2]), ValueError, "non-contiguous x"),
        (dict(x=x.bfloat16()), TypeError, "bf16 x"),
        (dict(tab=tab.half()), TypeError, "fp16 table"),
        (dict(w=w.double()), TypeError, "fp64 weight"),
        (dict(b=None), ValueError, "missing bias"),
        (dict(eps=-1.0), ValueError, "negative eps"),
        (dict(eps=1), ValueError, "integer eps"),
    ]
    for change, exc, why in bad:
        a = dict(x=x, tab=tab, w=w, b=b, seq_len=3, eps=1e-5)
        a.update(change)
        with pytest.raises(exc):
            ops.theta_gamma_norm(a["x"], a["tab"], a["w"], a["b"], a["seq_len"], a["eps"])
            pytest.fail(f"accepted: {why}")
    for t in (x.bfloat16(), x.half()):
        with pytest.raises(TypeError, match="fp32"):
            ops.theta_gamma_norm(t, tab, w, b, 3)

    mean, rstd, d = torch.zeros(6), torch.ones(6), (tab, tab, tab)
    bad = [
        (dict(g_y=torch.zeros(6, 7)), ValueError, "g_y shape"),
        (dict(g_y=x.half()), TypeError, "fp16 gradient"),
        (dict(mean=torch.zeros(5)), ValueError, "mean length"),
        (dict(rstd=torch.ones(6, 1)), ValueError, "rstd rank"),
        (dict(rstd=None), ValueError, "missing rstd"),
        (dict(d=(tab, tab)), ValueError, "two derivative tables"),
        (dict(d=(tab, tab, torch.zeros(6, 8))), ValueError, "a derivative table of another shape"),
        (dict(d=(tab, tab, tab.double())), TypeError, "fp64 derivative table"),
        (dict(d=(tab, None, tab)), ValueError, "a missing derivative table"),
        (dict(column_sums=False), ValueError, "derivatives without column sums"),
        (dict(seq_len=4), ValueError, "table rows"),
    ]
    for change, exc, why in bad:
        a = dict(g_y=x, x=x, tab=tab, d=d, mean=mean, rstd=rstd, w=w, seq_len=3, column_sums=True)
        a.update(change)
        with pytest.raises(exc):
            ops.theta_gamma_norm_backward(a["g_y"], a["x"], a["tab"], a["d"], a["mean"], a["rstd"], a["w"],
                                          a["seq_len"], column_sums=a["column_sums"])
            pytest.fail(f"accepted: {why}")
    # valid calls get as far as the device check, still without the library
    with pytest.raises(ops.AuraDeviceError):
        ops.theta_gamma_table(th, ga, amp, 512, 5.0, positions=torch.zeros(3))
    with pytest.raises(ops.AuraDeviceError):
        ops.theta_gamma_norm(x, torch.zeros(6, 8), w, b, 3)              # one table row per token
    with pytest.raises(ops.AuraDeviceError):
        ops.theta_gamma_norm_backward(x, x, tab, d, mean, rstd, w, 3)


# ------------------------------------------------------------------------------------- the module on the CPU stand-in
def _encoder(seed=0, **kw):
    from aura_snn_rag_amd.core.language_zone.theta_gamma_encoding import ThetaGammaPositionalEncoding
    torch.manual_seed(seed)
    return ThetaGammaPositionalEncoding(_config(**kw))


def _compose(enc, norm, hidden, positions):
    """The reference's op sequence in torch autograd ops: the formula, the add, LayerNorm."""
    denom = float(max(enc.max_seq_len - 1, 1))
    phi = ((positions.float() / denom) * (2.0 * np.pi)).unsqueeze(-1)
    a = phi + enc.theta_phase_offsets
    g = phi * (enc.gamma_freq / enc.theta_freq) + enc.gamma_phase_offsets
    pe = (torch.sin(a) + 0.5 * ((torch.cos(a) + 1.0) * 0.5 * torch.sin(g))) * enc.amplitude_modulation
    return norm(hidden + pe), pe


def test_the_module_keeps_the_reference_surface():
    import aura_snn_rag_amd
    from aura_snn_rag_amd.core.language_zone import theta_gamma_encoding as M
    assert aura_snn_rag_amd.ThetaGammaPositionalEncoding is M.ThetaGammaPositionalEncoding
    assert aura_snn_rag_amd.embed_tokens is M.embed_tokens
    enc = _encoder()
    assert list(enc.state_dict()) == ["theta_phase_offsets", "gamma_phase_offsets", "amplitude_modulation"]
    assert (enc.embedding_dim, enc.theta_freq, enc.gamma_freq, enc.max_seq_len) == (100, 8.0, 40.0, 512)
    assert repr(enc) == "ThetaGammaPositionalEncoding(embedding_dim=100, theta_freq=8.0Hz, gamma_freq=40.0Hz)"
    assert torch.equal(enc.amplitude_modulation, torch.ones(100))
    cfg = _config()
    del cfg.max_seq_len
    assert M.ThetaGammaPositionalEncoding(cfg).max_seq_len == 512
    with pytest.raises(ValueError):
        _encoder(D=2049)
    try:
        ref_mod = _reference()
    except pytest.skip.Exception:
        return
    torch.manual_seed(0)
    ref = ref_mod.ThetaGammaPositionalEncoding(_config())
    for (k, v), (k2, v2) in zip(enc.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), "the same seed must give the reference's initialisation"


def test_the_module_refuses_the_cpu_half_precision_and_other_norms():
    from aura_snn_rag_amd import ops
    enc = _encoder()
    hidden, norm = torch.zeros(2, 3, 100), nn.LayerNorm(100)
    with pytest.raises(ops.AuraDeviceError):
        enc(torch.arange(3)[None], 3)
    with pytest.raises(ops.AuraDeviceError):
        enc.encode_add_norm(hidden, norm)
    for half in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="fp32"):
            _encoder().to(half).encode_add_norm(hidden.to(half), nn.LayerNorm(100).to(half))
    for other in (nn.LayerNorm(100, elementwise_affine=False), nn.LayerNorm(99), nn.LayerNorm((3, 100)), nn.Identity(),
                  nn.LayerNorm(100, bias=False)):
        with pytest.raises(TypeError):
            enc.encode_add_norm(hidden, other)
    with pytest.raises(ValueError):
        enc.encode_add_norm(torch.zeros(2, 3, 99), norm)
    with pytest.raises(ValueError):
        enc.encode_add_norm(hidden, norm, positions=torch.zeros(2, 4))
    with pytest.raises(ValueError):
        enc.encode_add_norm(hidden, norm, positions=torch.zeros(3), start=1)


def test_shapes_for_the_three_kinds_of_positions(monkeypatch):
    STUB.install(monkeypatch)
    enc, norm = _encoder(seed=1), nn.LayerNorm(100)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn(100))
        norm.bias.add_(0.1 * torch.randn(100))
        enc.amplitude_modulation.add_(0.1 * torch.randn(100))
    hidden = torch.randn(2, 5, 100, generator=torch.Generator().manual_seed(2))
    cases = [(None, torch.arange(5)[None], 5), (torch.tensor([4, 4, 0, 900, 2]), None, 5),
             (torch.tensor([[4.0, 4.0, 0.5, 1e5, 2.0]]), None, 5), (torch.tensor([[0, 1, 2, 3, 4], [9, 8, 7, 600, 5]]), None, 10)]
    with torch.no_grad():
        for positions, implied, rows in cases:
            y = enc.encode_add_norm(hidden, norm, positions=positions)
            want, _ = _compose(enc, norm, hidden, implied if positions is None else positions)
            assert y.shape == (2, 5, 100) and STUB.LAST["shapes"] == (10, 5, rows, 100)
            assert torch.allclose(y, want, rtol=0, atol=2e-4), positions
        y7 = enc.encode_add_norm(hidden, norm, start=7)
        want, pe = _compose(enc, norm, hidden, torch.arange(7, 12)[None])
        assert torch.allclose(y7, want, rtol=0, atol=1e-5)
        # forward: any shape of positions, seq_length ignored
        for positions in (torch.arange(7, 12)[None], torch.arange(7, 12), torch.arange(12).reshape(2, 3, 2)):
            out = enc(positions, 123)
            assert out.shape == (*positions.shape, 100)
            assert torch.allclose(out, _compose(enc, norm, torch.zeros(1), positions)[1], rtol=0, atol=1e-5)


def test_the_table_cache_follows_the_parameters(monkeypatch):
    STUB.install(monkeypatch)
    enc, norm = _encoder(seed=2), nn.LayerNorm(100)
    hidden = torch.randn(2, 5, 100, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        a = enc.encode_add_norm(hidden, norm)
        first = STUB.LAST["used_table"]
        assert STUB.CALLS["table"] == 1 and first.shape == (5, 100) and not first.requires_grad
        enc.encode_add_norm(hidden, norm)
        assert STUB.CALLS["table"] == 1 and STUB.LAST["used_table"] is first, "the table was rebuilt without a change"
        enc.encode_add_norm(hidden, norm, start=3)
        assert STUB.CALLS["table"] == 2, "another start is another table"
        enc.encode_add_norm(hidden[:, :4].contiguous(), norm)
        assert STUB.CALLS["table"] == 3, "another length is another table"
        enc.encode_add_norm(hidden, norm)
        built = STUB.CALLS["table"]
        for p in (enc.theta_phase_offsets, enc.gamma_phase_offsets, enc.amplitude_modulation):
            p.mul_(1.5)                                              # in place: the version counter moves
            b = enc.encode_add_norm(hidden, norm)
            built += 1
            assert STUB.CALLS["table"] == built and not torch.equal(a, b)
            a = b
        enc.gamma_phase_offsets.data = enc.gamma_phase_offsets.data.clone()      # a new allocation
        enc.encode_add_norm(hidden, norm)
        assert STUB.CALLS["table"] == built + 1
        # explicit positions are never cached
        enc.encode_add_norm(hidden, norm, positions=torch.arange(5))
        enc.encode_add_norm(hidden, norm, positions=torch.arange(5))
        assert STUB.CALLS["table"] == built + 3
    # an optimizer step writes in place too; with gradients on, nothing is kept
    opt = torch.optim.SGD(list(enc.parameters()) + list(norm.parameters()), lr=0.5)
    enc.encode_add_norm(hidden, norm).square().sum().backward()
    with torch.no_grad():
        before = enc.encode_add_norm(hidden, norm)
        kept = STUB.LAST["used_table"]
    opt.step()
    with torch.no_grad():
        after = enc.encode_add_norm(hidden, norm)
    assert STUB.LAST["used_table"] is not kept and not torch.equal(before, after)


@pytest.mark.parametrize("kind", ["range", "shared", "per_item"])
def test_gradients_reach_hidden_and_all_five_parameters(monkeypatch, kind):
    STUB.install(monkeypatch)
    enc, norm = _encoder(seed=4), nn.LayerNorm(100)
    hidden = torch.randn(2, 5, 100, generator=torch.Generator().manual_seed(5)).requires_grad_()
    positions = {"range": None, "shared": torch.tensor([3, 3, 0, 700, 1]),
                 "per_item": torch.tensor([[0, 1, 2, 3, 4], [9, 8, 7, 600, 5]])}[kind]
    weights = torch.randn(2, 5, 100, generator=torch.Generator().manual_seed(6))
    params = dict(enc.named_parameters(), **{"norm." + k: v for k, v in norm.named_parameters()})
    (enc.encode_add_norm(hidden, norm, positions=positions) * weights).sum().backward()
    assert STUB.CALLS == dict(table=1, derivatives=1, forward=1, backward=1) and STUB.LAST["column_sums"]
    got = {k: p.grad.clone() for k, p in params.items()}
    got["hidden"] = hidden.grad.clone()
    assert len(got) == 6 and all(g is not None for g in got.values())
    for p in (*params.values(), hidden):
        p.grad = None
    want, _ = _compose(enc, norm, hidden, torch.arange(5)[None] if positions is None else positions)
    (want * weights).sum().backward()
    for k, p in dict(params, hidden=hidden).items():
        assert torch.allclose(got[k], p.grad, rtol=1e-3, atol=2e-4), k
    # only hidden wants a gradient: one launch, no derivative tables, no column sums
    for p in params.values():
        p.requires_grad_(False)
        p.grad = None
    hidden.grad = None
    STUB.install(monkeypatch)
    (enc.encode_add_norm(hidden, norm, positions=positions) * weights).sum().backward()
    assert STUB.CALLS["derivatives"] == 0 and STUB.LAST["column_sums"] is False and STUB.LAST["derivatives"] is False
    assert torch.allclose(hidden.grad, got["hidden"], rtol=0, atol=1e-6)
    # only the norm's parameters: column sums without derivative tables
    norm.weight.requires_grad_(True)
    STUB.install(monkeypatch)
    (enc.encode_add_norm(hidden.detach(), norm, positions=positions) * weights).sum().backward()
    assert STUB.CALLS["derivatives"] == 0 and STUB.LAST["column_sums"] is True and norm.bias.grad is None
    assert torch.allclose(norm.weight.grad, got["norm.weight"], rtol=0, atol=1e-5)
    # forward() is differentiable in the three parameters
    for p in enc.parameters():
        p.requires_grad_(True)
    pos = torch.tensor([[0, 3, 3, 800]])
    (enc(pos, 4) * weights[:1, :4]).sum().backward()
    mine = [p.grad.clone() for p in enc.parameters()]
    for p in enc.parameters():
        p.grad = None
    (_compose(enc, norm, torch.zeros(1), pos)[1] * weights[:1, :4]).sum().backward()
    for g, p in zip(mine, enc.parameters()):
        assert torch.allclose(g, p.grad, rtol=1e-3, atol=2e-4)


def test_embed_tokens_is_its_three_parts(monkeypatch):
    from tests import cpu_stub_place_code as PLACE
    from aura_snn_rag_amd.core.language_zone.place_cell_encoder import PlaceCellSemanticEncoder
    from aura_snn_rag_amd.core.language_zone.theta_gamma_encoding import embed_tokens
    PLACE.install(monkeypatch)
    STUB.install(monkeypatch)
    torch.manual_seed(8)
    sem = PlaceCellSemanticEncoder(types.SimpleNamespace(vocab_size=50, embedding_dim=100, n_place_cells=500), None)
    enc, norm = _encoder(seed=9), nn.LayerNorm(100)
    ids = torch.randint(0, 50, (2, 6), generator=torch.Generator().manual_seed(10))
    with torch.no_grad():
        hidden, activity = embed_tokens(ids, sem, enc, norm)
        semantic, want_activity = sem(ids)
        pos = enc(torch.arange(6)[None], seq_length=6)
        want = norm(semantic + pos)
        assert hidden.shape == (2, 6, 100) and torch.equal(activity, want_activity)
        assert torch.allclose(hidden, want, rtol=0, atol=1e-5)
        later, code = embed_tokens(ids, sem, enc, norm, start=40, dense=False)
        assert torch.equal(code.to_dense(), want_activity)
        assert torch.allclose(later, norm(semantic + enc(torch.arange(40, 46)[None], 6)), rtol=0, atol=1e-5)
    # differentiable end to end
    hidden, _ = embed_tokens(ids, sem, enc, norm)
    hidden.square().sum().backward()
    for n, p in (*sem.named_parameters(), *enc.named_parameters(), *norm.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
