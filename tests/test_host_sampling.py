"""Next-token sampling and ``HippocampalTransformer.generate`` without a GPU: the NumPy rule (tests/sampling_rule.py)
against answers known by hand, its kept set against the published top-k / top-p filter composed from torch ops, the
distribution of the draw against the exact softmax over the kept set, the host-side refusals of ``ops.sample_next``
(every one raised before a library is loaded), and the model's ``generate`` on the CPU stand-ins of its kernels."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import cpu_stub_decode_attention as DECODE
from tests import cpu_stub_place_code as PLACE
from tests import cpu_stub_sampling as STUB
from tests import cpu_stub_theta_gamma as THETA
from tests import sampling_rule as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hippocampal_transformer_keys.json")
INF = float("inf")


def chi2_sf(x: float, df: int) -> float:
    """P(chi2_df > x), closed forms for integer df."""
    h = 0.5 * x
    if df % 2 == 0:
        return math.exp(-h) * sum(h ** i / math.factorial(i) for i in range(df // 2))
    return math.erfc(math.sqrt(h)) + math.exp(-h) * sum(h ** (i - 0.5) / math.gamma(i + 0.5)
                                                         for i in range(1, (df - 1) // 2 + 1))


def test_the_chi_square_tail_is_the_tabulated_one():
    for df, x in ((1, 15.137), (2, 18.421), (5, 25.745), (10, 35.564), (15, 44.263)):
        assert abs(chi2_sf(x, df) / 1e-4 - 1.0) < 2e-3


# ------------------------------------------------------------------------------------------------- known answers
def test_an_all_equal_row_takes_the_lowest_ids():
    z = np.full((2, 37), 1.5, dtype=np.float32)
    r = R.sample(z, top_k=5, top_p=1.0, seed=3, step=1)
    assert r["ids"].tolist() == [[0, 1, 2, 3, 4]] * 2 and np.all(r["z"] == np.float32(1.5))
    assert r["n_kept"].tolist() == [5, 5] and np.all(np.isin(r["token"], np.arange(5)))
    assert R.sample(z, temperature=0.0)["token"].tolist() == [0, 0]
    # five equal terms: the prefix sums are 1 .. 5 exactly, so top_p = 0.6 keeps the ranks with c_{j-1} <= 3
    assert R.sample(z, top_k=5, top_p=0.6)["kept"].tolist() == [[True, True, True, True, False]] * 2


def test_top_p_zero_keeps_rank_zero_only():
    rng = np.random.default_rng(0)
    z = (4 * rng.standard_normal((6, 50))).astype(np.float32)
    for step in range(4):
        r = R.sample(z, top_k=10, top_p=0.0, seed=9, step=step)
        assert r["n_kept"].tolist() == [1] * 6
        assert r["token"].tolist() == np.argmax(z, axis=1).tolist()
        assert np.all(np.isneginf(r["d"][:, 1:])) and np.all(np.isfinite(r["d"][:, 0]))


def test_k_at_least_v_ranks_the_whole_row():
    z = np.array([[0.5, -1.0, 2.0, 2.0, -0.0, 0.0]], dtype=np.float32)
    for k in (6, 7, 1024):
        r = R.sample(z, top_k=k, top_p=1.0)
        assert r["ids"].tolist() == [[2, 3, 0, 4, 5, 1]] and r["n_kept"].tolist() == [6]
        assert not np.signbit(r["z"]).any() or r["z"][0, -1] < 0           # -0 is returned as +0


def test_a_row_of_minus_inf_and_nan_returns_minus_one():
    z = np.array([[-INF, np.nan, -INF, np.nan], [-INF, np.nan, 1.0, INF]], dtype=np.float32)
    for kw in (dict(top_k=3, top_p=0.9), dict(top_k=0, top_p=1.0), dict(temperature=0.0)):
        r = R.sample(z, **kw)
        assert r["token"][0] == -1 and r["token"][1] in (2, 3), kw
    r = R.sample(z, top_k=3, top_p=0.9)
    assert r["n_kept"][0] == 0 and r["z"][1, 0] == R.FLT_MAX and r["ids"][1].tolist() == [3, 2, 0]
    assert R.sample(z, temperature=0.0)["token"][1] == 3


def test_the_two_penalty_rules_on_a_positive_a_negative_and_a_zero_logit():
    z = np.array([[3.0, -3.0, 0.0, 3.0, -3.0, -0.0]], dtype=np.float32)
    seen = np.array([[1, 1, 1, 0, 0, 7]], dtype=np.uint8)
    p = np.float32(1.2)
    div = R.penalise(z, seen, 1.2, "divide")[0]
    sig = R.penalise(z, seen, 1.2, "signed")[0]
    assert div.tolist() == [np.float32(3.0) / p, np.float32(-3.0) / p, 0.0, 3.0, -3.0, 0.0]
    assert sig.tolist() == [np.float32(3.0) / p, np.float32(-3.0) * p, 0.0, 3.0, -3.0, 0.0]
    assert div[1] > z[0, 1] > sig[1]                   # 'divide' raises a seen negative logit, 'signed' lowers it
    assert np.array_equal(R.penalise(z, seen, 1.0, "signed"), R.clean(z))
    assert np.array_equal(R.penalise(z, None, 1.2), R.clean(z))
    # an overflowing quotient is FLT_MAX again, -inf stays
    big = np.array([[R.FLT_MAX, -INF]], dtype=np.float32)
    assert R.penalise(big, np.ones((1, 2), np.uint8), 0.5)[0].tolist() == [float(R.FLT_MAX), -INF]
    assert R.temper(big, 1e-3)[0].tolist() == [float(R.FLT_MAX), -INF]


def test_the_blocked_prefix_sum_is_monotone_and_close_to_fp64():
    rng = np.random.default_rng(5)
    e = np.sort(rng.random((8, 1000)).astype(np.float32), axis=1)[:, ::-1]
    c = R.prefix_sums32(e)
    assert np.all(np.diff(c, axis=1) >= 0)
    c64 = np.cumsum(e.astype(np.float64), axis=1)
    assert np.max(np.abs(c - c64) / c64[:, -1:]) < 1000 * 2.0 ** -24


# ------------------------------------------------------------------ the kept set against an independent composition
def _published_filter(logits: torch.Tensor, top_k: int, top_p: float) -> torch.Tensor:
    """The top-k then top-p logit filter as commonly published, from torch ops: the set left finite [N, V]."""
    z = logits.clone()
    kth = torch.topk(z, top_k, dim=-1).values[..., -1:]
    z = z.masked_fill(z < kth, -INF)
    sorted_z, order = torch.sort(z, dim=-1, descending=True)
    cum = torch.cumsum(torch.softmax(sorted_z, dim=-1), dim=-1)
    drop = cum > top_p
    drop = torch.cat([torch.zeros_like(drop[..., :1]), drop[..., :-1]], dim=-1)       # the crossing token stays
    z = z.masked_fill(torch.zeros_like(drop).scatter(-1, order, drop), -INF)
    return torch.isfinite(z), cum


KEPT_SEED = 2024


def test_kept_set_equals_the_published_filter_on_1000_rows():
    N, V, k, top_p = 1000, 300, 40, 0.9
    z = (4 * np.random.default_rng(KEPT_SEED).standard_normal((N, V))).astype(np.float32)
    assert all(np.unique(row).size == V for row in z), "distinct values"
    r = R.sample(z, top_k=k, top_p=top_p)
    mine = np.zeros((N, V), dtype=bool)
    np.put_along_axis(mine, r["ids"].astype(np.int64), r["kept"], axis=1)
    theirs, cum = _published_filter(torch.from_numpy(z), k, top_p)
    near = (np.abs(cum.numpy()[:, :k].astype(np.float64) - top_p) < 1e-6).any(axis=1)
    print(f"rows left out near the boundary: {int(near.sum())} of {N}")
    assert near.sum() <= N // 100
    assert np.array_equal(mine[~near], theirs.numpy()[~near])
    assert np.all(r["n_kept"] >= 1) and np.all(r["n_kept"] <= k)


# ------------------------------------------------------------------------------------------------- the distribution
DIST_SEED = 11


def test_draws_follow_the_softmax_over_the_kept_set():
    V, k, top_p, T, DRAWS = 64, 16, 0.9, 0.7, 20000
    row = (2 * np.random.default_rng(1).standard_normal(V)).astype(np.float32)
    one = R.sample(row[None], top_k=k, top_p=top_p, temperature=T, seed=DIST_SEED, step=0)
    kept_ids = one["ids"][0][one["kept"][0]]
    assert 3 <= kept_ids.size < k, "the nucleus must cut inside the candidates for the test to mean something"
    tokens = STUB.draws(row, np.arange(DRAWS), stream=0, top_k=k, top_p=top_p, temperature=T, seed=DIST_SEED)
    assert np.all(np.isin(tokens, kept_ids)), "a token outside the kept set was drawn"
    p = R.softmax64(one["z"], one["kept"])[0][one["kept"][0]]
    counts = np.array([(tokens == i).sum() for i in kept_ids])
    chi2 = float(np.sum((counts - DRAWS * p) ** 2 / (DRAWS * p)))
    pv = chi2_sf(chi2, kept_ids.size - 1)
    print(f"kept {kept_ids.size}, chi2 = {chi2:.2f}, p = {pv:.4f}")
    assert pv > 1e-4
    # the stub itself, one call per step, draws the same tokens
    lg = torch.from_numpy(row[None].copy())
    for step in (0, 1, 7, 19999):
        assert int(STUB.sample_next(lg, top_k=k, top_p=top_p, temperature=T, seed=DIST_SEED, step=step)[0]) == tokens[step]


# ------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_comes_before_any_library_is_loaded(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_library)
    lg = torch.zeros(3, 10)
    ok = dict(top_k=5, top_p=0.9)
    bad = [
        (TypeError, dict(logits=[[0.0]])), (TypeError, dict(logits=lg.double())), (TypeError, dict(logits=lg.bfloat16())),
        (ValueError, dict(logits=lg[0])), (ValueError, dict(logits=torch.zeros(0, 10))),
        (ValueError, dict(logits=torch.zeros(3, 0))), (ValueError, dict(logits=torch.zeros(10, 3).t())),
        (ValueError, dict(logits=torch.zeros(1, 10).expand(3, 10))),
        (ValueError, dict(top_k=-1)), (ValueError, dict(top_k=1025)), (TypeError, dict(top_k=5.0)),
        (TypeError, dict(top_k=True)), (ValueError, dict(top_k=0, top_p=0.9)),
        (ValueError, dict(temperature=-0.5)), (ValueError, dict(temperature=INF)), (ValueError, dict(temperature=math.nan)),
        (ValueError, dict(temperature=1e39)), (TypeError, dict(temperature="1")),
        (ValueError, dict(penalty=0.0)), (ValueError, dict(penalty=-1.0)), (ValueError, dict(penalty=INF)),
        (ValueError, dict(penalty=math.nan)),
        (ValueError, dict(top_p=-0.1)), (ValueError, dict(top_p=math.nan)),
        (ValueError, dict(penalty_rule="multiply")),
        (ValueError, dict(seed=-1)), (ValueError, dict(seed=1 << 64)), (ValueError, dict(step=-1)), (TypeError, dict(step=1.5)),
        (ValueError, dict(eos_id=-2)), (TypeError, dict(pad_id=None)),
        (TypeError, dict(seen=torch.zeros(3, 10, dtype=torch.bool))), (ValueError, dict(seen=torch.zeros(3, 9, dtype=torch.uint8))),
        (TypeError, dict(finished=torch.zeros(3, dtype=torch.int32))), (ValueError, dict(finished=torch.zeros(4, dtype=torch.uint8))),
        (ValueError, dict(stream_ids=[0, 1])), (ValueError, dict(stream_ids=[0, 1, -1])),
        (ValueError, dict(stream_ids=torch.zeros(3, dtype=torch.int32))),
        (TypeError, dict(out=torch.zeros(3, dtype=torch.int32))), (ValueError, dict(out=torch.zeros(4, dtype=torch.int64))),
    ]
    for exc, kw in bad:
        args = dict(ok, **kw)
        logits = args.pop("logits", lg)
        with pytest.raises(exc):
            ops.sample_next(logits, **args)
    with pytest.raises(ValueError, match="1024"):                       # the cap is named
        ops.sample_next(lg, top_k=0, top_p=0.5)
    # a good call on CPU tensors passes every check and is refused for the device, still without the library
    for kw in (ok, dict(top_k=0, top_p=1.0), dict(temperature=0.0), dict(ok, out=torch.zeros(3, 4, dtype=torch.int64)[:, 2]),
               dict(ok, seen=torch.zeros(3, 10, dtype=torch.uint8), finished=torch.zeros(3, dtype=torch.uint8), eos_id=2,
                    stream_ids=[4, 5, 6])):
        with pytest.raises(ops.AuraDeviceError):
            ops.sample_next(lg, **kw)
    with pytest.raises(ops.AuraDeviceError):
        ops.sample_next(torch.zeros(5, 30)[:, :10], **ok)               # rows as a strided view are fine


def test_the_library_refuses_what_the_header_says():
    import ctypes
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    assert lib.aura_sample_workspace_bytes(3, 1000, 50, 0.8) == (3 * 1000 * 4 + 255) // 256 * 256
    assert lib.aura_sample_workspace_bytes(3, 1000, 0, 0.8) == 0 and lib.aura_sample_workspace_bytes(3, 1000, 50, 0.0) == 0
    for args in ((0, 10, 5, 1.0), (1, 0, 5, 1.0), (1, 131073, 5, 1.0), (1, 10, 1025, 1.0), (1, 10, -1, 1.0),
                 (1, 10, 5, -1.0), (1, 10, 5, INF)):
        assert lib.aura_sample_workspace_bytes(*args) == -1, args
    buf = (ctypes.c_float * 64)()
    tok = (ctypes.c_int64 * 4)()
    ws = ctypes.create_string_buffer(1024 + 256)
    base = (ctypes.addressof(ws) + 255) // 256 * 256
    lg, tk = ctypes.addressof(buf), ctypes.addressof(tok)

    def call(logits=lg, stride=16, B=2, V=16, penalty=1.0, rule=0, temperature=1.0, top_k=4, top_p=0.9, tokens=tk,
             tstride=1, workspace=base, wbytes=1024):
        return lib.aura_sample_next(logits, stride, B, V, None, None, None, penalty, rule, temperature, top_k, top_p, 0, 0,
                                    -1, 0, tokens, tstride, None, None, None, None, None, workspace, wbytes, None)
    inval = [dict(top_k=-1), dict(top_k=1025), dict(top_k=0, top_p=0.5), dict(temperature=-1.0), dict(temperature=INF),
             dict(temperature=math.nan), dict(penalty=0.0), dict(penalty=-2.0), dict(penalty=INF), dict(top_p=-0.5),
             dict(top_p=math.nan), dict(rule=2), dict(logits=None), dict(tokens=None), dict(stride=15), dict(tstride=0),
             dict(B=0), dict(V=0), dict(V=131073, stride=131073), dict(workspace=None), dict(wbytes=255)]
    for kw in inval:
        assert call(**kw) == -1, kw                                     # AURA_E_INVAL, nothing launched
    for kw in (dict(logits=lg + 2), dict(tokens=tk + 4), dict(workspace=base + 16)):
        assert call(**kw) == -3, kw                                     # AURA_E_ALIGN


# ------------------------------------------------------------------------------------------------- generate on the stubs
def _config(V=61, D=96, H=2, **kw):
    return types.SimpleNamespace(vocab_size=V, embedding_dim=D, num_heads=H, num_layers=2, intermediate_size=2 * D,
                                 n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                 gamma_frequency=40.0, **kw)


@pytest.fixture()
def model(monkeypatch):
    for stub in (PLACE, THETA, DECODE, STUB):
        stub.install(monkeypatch)
    from aura_snn_rag_amd import HippocampalTransformer
    torch.manual_seed(0)
    m = HippocampalTransformer(_config(), None).eval()
    with torch.no_grad():
        m.semantic_encoder.token_embedding.weight.mul_(3.0)              # logits of order 1: decisive argmaxes
    return m


def _prompts(B=3, S=5, V=61, seed=1):
    return torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(seed))


def _recompute_greedy(m, ids, n):
    out = ids.clone()
    gaps = []
    with torch.no_grad():
        for _ in range(n):
            lg = m(out, use_memory=False)[0][:, -1]
            top2 = torch.topk(lg, 2, dim=-1).values
            gaps.append(float((top2[:, 0] - top2[:, 1]).min()))
            out = torch.cat([out, lg.argmax(-1, keepdim=True)], dim=1)
    return out, min(gaps)


def test_greedy_generate_equals_the_recompute_loop(model):
    ids = _prompts()
    want, gap = _recompute_greedy(model, ids, 9)
    assert gap > 1e-4, "the fixed seed must leave no argmax open"
    got = model.generate(ids, max_new_tokens=9, temperature=0.0, repetition_penalty=1.0, use_memory=False)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert DECODE.CALLS["step"] == 2 * 8 and STUB.CALLS["sample"] == 9


def test_the_same_seed_gives_the_same_tokens_and_torch_manual_seed_governs_none(model):
    ids = _prompts()
    kw = dict(max_new_tokens=8, temperature=0.9, top_k=20, top_p=0.95, use_memory=False)
    a, b, c = model.generate(ids, seed=7, **kw), model.generate(ids, seed=7, **kw), model.generate(ids, seed=8, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c) and a.shape == (3, 13)
    torch.manual_seed(123)
    d = model.generate(ids, **kw)
    torch.manual_seed(123)
    e = model.generate(ids, **kw)
    f = model.generate(ids, **kw)
    assert torch.equal(d, e) and not torch.equal(d, f)


def test_a_row_alone_with_its_stream_equals_the_row_in_the_batch(model):
    ids = _prompts()
    kw = dict(max_new_tokens=8, temperature=0.9, top_k=20, top_p=0.95, use_memory=False, seed=5)
    batch = model.generate(ids, **kw)
    for b in (0, 1, 2):
        assert torch.equal(model.generate(ids[b:b + 1], stream_ids=[b], **kw)[0], batch[b])
    assert not torch.equal(model.generate(ids[1:2], **kw)[0], batch[1])  # (stream 0 draws differently)


def test_eos_pads_the_finished_row_trims_and_retires_its_cache_rows(model, monkeypatch):
    ids = _prompts()
    S, n = ids.shape[1], 9
    kw = dict(max_new_tokens=n, temperature=0.0, repetition_penalty=1.3, use_memory=False)
    free = model.generate(ids, **kw)
    eos = int(free[1, S + 2])
    first = [(free[b, S:] == eos).nonzero()[0, 0].item() if (free[b, S:] == eos).any() else None for b in range(3)]
    assert first[1] is not None and first[1] <= 2
    states = []
    new_state = model.new_state
    monkeypatch.setattr(model, "new_state", lambda *a, **k: states.append(new_state(*a, **k)) or states[-1])
    got = model.generate(ids, eos_token_id=eos, pad_token_id=60, sync_every=2, **kw)
    keep = n if None in first else max(first) + 1
    want = free[:, :S + keep].clone()
    for b, f in enumerate(first):
        if f is not None:
            want[b, S + f + 1:] = 60
    assert torch.equal(got, want)
    assert any(f is None for f in (first[0], first[2])), "the seed must leave a row that never finishes"
    lengths = states[0].lengths
    assert all(c.lengths is lengths for c in states[0].caches)
    assert lengths[1].item() == -1 and states[0].finished.tolist() == [int(f is not None) for f in first]
    assert all(lengths[b].item() == S + n - 1 for b in range(3) if first[b] is None)
    # the config's EOS id is the default, and its default padding is the EOS id; every row finished: trimmed
    model.config.eos_token_id = eos
    alone = model.generate(ids[1:2], stream_ids=[1], sync_every=1, **kw)
    assert torch.equal(alone[0], free[1, :S + first[1] + 1]) and alone.shape[1] < S + n
    assert torch.equal(model.generate(ids[1:2], eos_token_id=None, **kw)[0], free[1])


def test_state_dict_matches_the_reference_and_the_tying_survives_a_round_trip(model):
    from aura_snn_rag_amd import HippocampalTransformer
    golden = json.load(open(GOLDEN))
    ref = HippocampalTransformer(types.SimpleNamespace(**golden["config"]), None)
    assert [[k, list(v.shape)] for k, v in ref.state_dict().items()] == golden["keys"]
    assert ref.output_head.weight is ref.semantic_encoder.token_embedding.weight
    other = HippocampalTransformer(_config(), None)
    other.load_state_dict(model.state_dict())
    assert other.output_head.weight is other.semantic_encoder.token_embedding.weight
    assert torch.equal(other.output_head.weight, model.semantic_encoder.token_embedding.weight)
    ids = _prompts()
    with torch.no_grad():
        assert torch.equal(other.eval()(ids, use_memory=False)[0], model(ids, use_memory=False)[0])


def test_forward_stores_the_pooled_batch_in_one_call_and_checkpoints(model):
    calls = []
    model.hippocampus = types.SimpleNamespace(create_episodic_memories=lambda ids, feats: calls.append((ids, feats)))
    ids = _prompts()
    logits, code = model(ids, use_memory=False, store_memory=True, memory_ids=["a", "b"])
    assert logits.shape == (3, 5, 61) and code.shape == (3, 5, 200)
    assert len(calls) == 1 and calls[0][0][:2] == ["a", "b"] and len(calls[0][0]) == 3 and calls[0][1].shape == (3, 96)
    model.hippocampus = None
    model.set_gradient_checkpointing(True)
    assert model.use_gradient_checkpointing
    model.train()
    out = model(ids, use_memory=False)[0]
    out.sum().backward()
    assert model.semantic_encoder.token_embedding.weight.grad is not None
    assert model.layers[1].ffn[0].weight.grad is not None
