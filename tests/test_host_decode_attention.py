"""Cached decoding without a GPU: the NumPy rule (tests/decode_attention_rule.py) against answers known by hand and
against the committed fixture ``tests/golden/hippocampal_attention.pt`` (the reference module's recorded outputs); the
host-side refusals of ``ops.attn_decode_step``, of the library's entry point and of the cache (every one raised before a
device is touched); the ``state_dict`` surface; and the modules' ``prefill`` / ``step`` on a CPU stand-in of the op
(tests/cpu_stub_decode_attention.py): stepping equals ``forward`` at every position, with right-padded prompts too, and
a retired row returns zeros and keeps its cache."""
import os
import types

import numpy as np
import pytest
import torch

from tests import cpu_stub_decode_attention as STUB
from tests import decode_attention_rule as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hippocampal_attention.pt")
GOLDEN_SHAPES = [(3, 13, 96, 2), (2, 9, 128, 4)]
KEYS = sorted(f"{m}.{p}" for m in ("q_proj", "k_proj", "v_proj", "o_proj", "prosody_gate", "memory_gate")
              for p in ("weight", "bias"))


def _config(D=96, H=2):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D)


def _inputs(B, H, dh, cap, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    D = H * dh
    return dict(q=f(B, D), k=f(B, D), v=f(B, D), x=f(B, D), K=f(B, H, cap, dh), V=f(B, H, cap, dh),
                gates=dict(prosody=f(B, 4), Wp=f(H, 4), bp=f(H), wm=(f(1, D) / np.sqrt(D)).astype(np.float32), bm=f(1)))


STEPS = [R.step64, R.step32]


# ------------------------------------------------------------------------------------- the rule's own known answers
@pytest.mark.parametrize("step", STEPS, ids=["fp64", "fp32"])
def test_an_empty_cache_returns_the_new_value_bit_for_bit(step):
    i = _inputs(3, 2, 8, 5)
    out = step(i["q"], i["k"], i["v"], i["K"], i["V"], [0, 0, 0], x=i["x"], **i["gates"])
    assert np.array_equal(out["ctx"].astype(np.float32).view(np.int32), i["v"].view(np.int32))
    assert np.array_equal(i["K"][:, :, 0].reshape(3, 16), i["k"]) and np.array_equal(i["V"][:, :, 0].reshape(3, 16), i["v"])
    assert out["lengths"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("step", STEPS, ids=["fp64", "fp32"])
def test_equal_keys_give_the_mean_of_the_values(step):
    i = _inputs(2, 2, 12, 300, seed=1)
    i["K"][:] = i["K"][:, :, :1]
    i["k"] = i["K"][:, :, 0].reshape(2, 24).copy()
    L = [6, 270]
    out = step(i["q"], i["k"], i["v"], i["K"], i["V"], L, x=i["x"], **i["gates"])
    for b in range(2):
        mean = i["V"][b, :, :L[b] + 1].astype(np.float64).mean(axis=1).reshape(-1)
        assert np.max(np.abs(out["ctx"][b] - mean)) <= (1e-12 if step is R.step64 else 2e-6)


@pytest.mark.parametrize("step", STEPS, ids=["fp64", "fp32"])
def test_a_score_200_above_the_rest_selects_its_value_without_overflow(step):
    i = _inputs(1, 1, 16, 300, seed=2)
    i["K"] *= np.float32(0.01)
    i["k"] *= np.float32(0.01)
    q = i["q"][0].astype(np.float64)
    i["K"][0, 0, 77] = (q * (230.0 * 4.0 / (q @ q))).astype(np.float32)          # z = 230 s with s >= 1
    out = step(i["q"], i["k"], i["v"], i["K"], i["V"], [260], x=i["x"], **i["gates"])
    assert np.all(np.isfinite(out["ctx"]))
    assert np.array_equal(out["ctx"][0].astype(np.float32), i["V"][0, 0, 77])


@pytest.mark.parametrize("step", STEPS, ids=["fp64", "fp32"])
def test_no_prosody_and_no_memory_gate_leave_the_query_alone(step):
    i = _inputs(2, 2, 8, 9, seed=3)
    out = step(i["q"], i["k"], i["v"], i["K"], i["V"], [3, 8], x=i["x"])
    assert np.all(out["scale"] == 1.0)
    two = step(i["q"], i["k"], i["v"], i["K"], i["V"], [3, 8], x=None, advance=False)
    assert np.array_equal(out["ctx"], two["ctx"]) and two["lengths"].tolist() == [3, 8]
    assert np.all(R.scale32(2, 2) == 1.0) and np.all(R.scale64(2, 2) == 1.0)


@pytest.mark.parametrize("step", STEPS, ids=["fp64", "fp32"])
def test_inactive_rows_are_zero_and_write_nothing(step):
    i = _inputs(4, 1, 4, 6, seed=4)
    K0, V0 = i["K"].copy(), i["V"].copy()
    out = step(i["q"], i["k"], i["v"], i["K"], i["V"], [-1, 6, 7, 5], x=i["x"], **i["gates"])
    assert np.all(out["ctx"][:3] == 0) and np.all(out["scale"][:3] == 0) and np.any(out["ctx"][3] != 0)
    assert np.array_equal(i["K"][:3], K0[:3]) and np.array_equal(i["V"][:3], V0[:3])
    assert out["lengths"].tolist() == [-1, 6, 7, 6]
    # a chunk count too small for a length makes the row inactive instead of wrong
    big = _inputs(1, 1, 4, 600, seed=5)
    out = step(big["q"], big["k"], big["v"], big["K"], big["V"], [300], n_chunks=1)
    assert np.all(out["ctx"] == 0) and out["lengths"].tolist() == [300]


def test_the_fp32_restatement_is_within_the_derived_bounds_of_fp64():
    for seed, (B, H, dh, cap, L) in enumerate([(2, 2, 4, 70, [0, 66]), (2, 1, 48, 300, [255, 256]),
                                               (1, 2, 128, 520, [513]), (2, 3, 32, 40, [1, 39])]):
        i = _inputs(B, H, dh, cap, seed=10 + seed)
        want = R.step64(i["q"], i["k"], i["v"], i["K"].copy(), i["V"].copy(), L, x=i["x"], with_bound=True, **i["gates"])
        got = R.step32(i["q"], i["k"], i["v"], i["K"].copy(), i["V"].copy(), L, x=i["x"], **i["gates"])
        assert np.all(np.abs(got["ctx"] - want["ctx"]) <= want["bound"])
        assert np.all(np.abs(got["scale"] - want["scale"]) <= want["scale_bound"])
        assert float(want["bound"].max()) < 2e-3, "the bound must stay far below a wiring error"


def test_geometry_of_the_rule_and_the_library_agree():
    from aura_snn_rag_amd import _lib, ops
    assert [R.gp_of(dh) for dh in (4, 8, 12, 32, 48, 64, 100, 128)] == [1, 2, 4, 8, 16, 16, 32, 32]
    assert [R.slots_of(dh) for dh in (4, 48, 128)] == [64, 4, 2]
    assert [ops.attn_decode_chunks(c) for c in (1, 256, 257, 32768)] == [1, 1, 2, 128]
    lib = _lib.load()
    for B, H, dh, nc in ((1, 1, 4, 1), (3, 2, 48, 2), (32, 12, 64, 9), (7, 16, 128, 128)):
        assert lib.aura_attn_decode_workspace_bytes(B, H, dh, nc) == 4 * ops.attn_decode_workspace_floats(B, H, dh, nc)
    assert lib.aura_attn_decode_workspace_bytes(1, 1, 6, 1) == -1 and lib.aura_attn_decode_workspace_bytes(1, 1, 4, 129) == -1


# ------------------------------------------------------------------------------------- the golden fixture
def _golden():
    return torch.load(GOLDEN, weights_only=True)


def _stepped64(case, variant):
    """The rule in fp64, one position at a time, over a golden case: [B, S, D]."""
    B, S, D, H = case["shape"]
    W = {k: v.double().numpy() for k, v in case["state_dict"].items()}
    hid = case["hidden"].double().numpy()
    prosody = None if variant == "no_prosody" else case["prosody"].double().numpy()
    memory = variant != "no_memory"
    lin = lambda n, t: t @ W[n + ".weight"].T + W[n + ".bias"]
    K, V = np.zeros((B, H, S, D // H)), np.zeros((B, H, S, D // H))
    L = np.zeros(B, np.int32)
    out = np.zeros((B, S, D))
    for t in range(S):
        x = hid[:, t]
        r = R.step64(lin("q_proj", x), lin("k_proj", x), lin("v_proj", x), K, V, L, x=x,
                     prosody=None if prosody is None else prosody[:, t], Wp=W["prosody_gate.weight"],
                     bp=W["prosody_gate.bias"], wm=W["memory_gate.weight"] if memory else None,
                     bm=W["memory_gate.bias"] if memory else None)
        L = r["lengths"]
        out[:, t] = lin("o_proj", r["ctx"])
    assert L.tolist() == [S] * B
    return out


def test_the_golden_fixture_has_the_cases_of_the_issue():
    g = _golden()
    assert [tuple(c["shape"]) for c in g["cases"]] == GOLDEN_SHAPES
    for c in g["cases"]:
        assert sorted(c["state_dict"]) == KEYS and sorted(c["outputs"]) == ["no_memory", "no_prosody", "prosody"]
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("variant", ["prosody", "no_prosody", "no_memory"])
def test_the_rule_stepped_in_fp64_matches_the_reference_outputs(n, variant):
    case = _golden()["cases"][n]
    want = case["outputs"][variant].double().numpy()
    got = _stepped64(case, variant)
    err, top = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print(f"golden {tuple(case['shape'])} {variant}: {err:.2e} on a maximum of {top:.2f}")
    assert err <= 5e-6 * top
    # and the whole-sequence fp64 formula is the same function
    W = {k: v.numpy() for k, v in case["state_dict"].items()}
    whole = R.forward64(case["hidden"].numpy(), W, case["shape"][3],
                        None if variant == "no_prosody" else case["prosody"].numpy(), variant != "no_memory")
    assert float(np.max(np.abs(whole - got))) <= 1e-12 * max(top, 1.0)


def test_the_golden_fixture_is_what_the_reference_computes():
    from oracle import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    from tools import gen_golden_attention
    fresh = gen_golden_attention.build(_ref_loader.load("core.language_zone.hippocampal_attention"))
    for a, b in zip(fresh["cases"], _golden()["cases"]):
        assert torch.equal(a["hidden"], b["hidden"]) and torch.equal(a["prosody"], b["prosody"])
        for k in KEYS:
            assert torch.equal(a["state_dict"][k], b["state_dict"][k]), k
        for k, v in a["outputs"].items():
            assert torch.allclose(v, b["outputs"][k], atol=1e-6, rtol=0), k


# ------------------------------------------------------------------------------------- host-side refusals
def _op_args(B=2, H=2, dh=8, cap=20):
    from aura_snn_rag_amd import ops
    D = H * dh
    z = lambda *s: torch.zeros(*s)
    return dict(q=z(B, D), k_new=z(B, D), v_new=z(B, D), x=z(B, D), prosody=z(B, 4), Wp=z(H, 4), bp=z(H), wm=z(1, D),
                bm=z(1), lengths=torch.zeros(B, dtype=torch.int32), k_cache=z(B, H, cap, dh), v_cache=z(B, H, cap, dh),
                workspace=z(ops.attn_decode_workspace_floats(B, H, dh, ops.attn_decode_chunks(cap))), n_chunks=None)


def _op(a):
    from aura_snn_rag_amd import ops
    return ops.attn_decode_step(a["q"], a["k_new"], a["v_new"], a["x"], a["prosody"], a["Wp"], a["bp"], a["wm"], a["bm"],
                                a["lengths"], a["k_cache"], a["v_cache"], a["workspace"], n_chunks=a["n_chunks"])


def test_the_op_refuses_bad_arguments_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    z = torch.zeros
    bad = [
        (dict(q=z(2, 15)), ValueError, "q shape"),
        (dict(k_new=z(3, 16)), ValueError, "k_new batch"),
        (dict(v_new=z(16)), ValueError, "v_new rank"),
        (dict(q=None), ValueError, "missing q"),
        (dict(q=z(2, 16).half()), TypeError, "fp16 q"),
        (dict(k_cache=z(2, 2, 20, 8).bfloat16()), TypeError, "bf16 cache"),
        (dict(q=z(2, 32)[:, ::2]), ValueError, "non-contiguous q"),
        (dict(k_cache=z(2, 2, 20)), ValueError, "cache rank"),
        (dict(v_cache=z(2, 2, 21, 8)), ValueError, "v_cache shape"),
        (dict(k_cache=z(2, 2, 20, 6), v_cache=z(2, 2, 20, 6), q=z(2, 12), k_new=z(2, 12), v_new=z(2, 12)), ValueError,
         "dh % 4"),
        (dict(k_cache=z(2, 1, 20, 132), v_cache=z(2, 1, 20, 132), q=z(2, 132), k_new=z(2, 132), v_new=z(2, 132)),
         ValueError, "dh > 128"),
        (dict(k_cache=z(1, 17, 2, 128), v_cache=z(1, 17, 2, 128), q=z(1, 2176), k_new=z(1, 2176), v_new=z(1, 2176)),
         ValueError, "D > 2048"),
        (dict(k_cache=z(2, 2, 0, 8), v_cache=z(2, 2, 0, 8)), ValueError, "cap < 1"),
        (dict(k_cache=z(1, 1, 32769, 4), v_cache=z(1, 1, 32769, 4), q=z(1, 4), k_new=z(1, 4), v_new=z(1, 4)), ValueError,
         "cap > 32768"),
        (dict(lengths=torch.zeros(2, dtype=torch.int64)), TypeError, "int64 lengths"),
        (dict(lengths=torch.zeros(3, dtype=torch.int32)), ValueError, "lengths shape"),
        (dict(lengths=[0, 0]), TypeError, "lengths as a list"),
        (dict(lengths=None), ValueError, "missing lengths"),
        (dict(prosody=z(2, 3)), ValueError, "prosody shape"),
        (dict(Wp=z(4, 2)), ValueError, "Wp shape"),
        (dict(bp=None), ValueError, "prosody without bp"),
        (dict(wm=None), ValueError, "bm without wm"),
        (dict(bm=None), ValueError, "wm without bm"),
        (dict(wm=z(15)), ValueError, "wm length"),
        (dict(bm=z(2)), ValueError, "bm length"),
        (dict(x=None), ValueError, "wm without x"),
        (dict(x=z(2, 8)), ValueError, "x shape"),
        (dict(n_chunks=0), ValueError, "n_chunks < 1"),
        (dict(n_chunks=2), ValueError, "256 n_chunks > cap + 255"),
        (dict(n_chunks=1.0), TypeError, "float n_chunks"),
        (dict(workspace=z(10)), ValueError, "workspace too small"),
        (dict(workspace=None), ValueError, "missing workspace"),
        (dict(workspace=z(1000).double()), TypeError, "fp64 workspace"),
    ]
    for change, exc, why in bad:
        a = _op_args()
        a.update(change)
        with pytest.raises(exc):
            _op(a)
            pytest.fail(f"accepted: {why}")
    # valid calls get as far as the device check, still without the library: CPU tensors are refused
    for change in (dict(), dict(prosody=None, Wp=None, bp=None), dict(wm=None, bm=None, x=None)):
        a = _op_args()
        a.update(change)
        with pytest.raises(ops.AuraDeviceError):
            _op(a)


def test_the_library_refuses_bad_geometry_and_pointers_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 0x10000                                           # never dereferenced: every call below returns on the host

    def call(B=2, H=2, dh=8, cap=20, nc=1, ws_bytes=1 << 20, **ptr):
        p = dict(q=P, k_new=P, v_new=P, x=P, prosody=P, Wp=P, bp=P, wm=P, bm=P, lengths=P, Kc=P, Vc=P, ws=P, ctx=P,
                 scale=None)
        p.update(ptr)
        return lib.aura_attn_decode_step(p["q"], p["k_new"], p["v_new"], p["x"], p["prosody"], p["Wp"], p["bp"], p["wm"],
                                         p["bm"], p["lengths"], p["Kc"], p["Vc"], B, H, dh, cap, nc, 1, p["ws"], ws_bytes,
                                         p["ctx"], p["scale"], None)
    INVAL, ALIGN = -1, -3
    for kw in (dict(B=-1), dict(H=0), dict(dh=6), dict(dh=0), dict(dh=132), dict(H=17, dh=128), dict(cap=0),
               dict(cap=32769), dict(nc=0), dict(nc=2), dict(B=2 ** 31), dict(ws_bytes=64), dict(q=None), dict(Kc=None),
               dict(lengths=None), dict(ws=None), dict(ctx=None), dict(Wp=None), dict(bp=None), dict(wm=None),
               dict(bm=None), dict(x=None)):
        assert call(**kw) == INVAL, kw
    for name in ("q", "k_new", "v_new", "x", "wm", "Kc", "Vc", "ws", "ctx"):
        assert call(**{name: P + 4}) == ALIGN, name
    for name in ("prosody", "Wp", "bp", "bm", "lengths", "scale"):
        assert call(**{name: P + 2}) == ALIGN, name
    assert call(B=0) == 0, "B == 0 launches nothing"


def test_the_cache_refuses_bad_geometry_and_a_step_on_a_full_cache(monkeypatch):
    from aura_snn_rag_amd import AttentionCache, HippocampalProsodyAttention
    ops = STUB.install(monkeypatch)
    for kw, exc in ((dict(capacity=0), ValueError), (dict(capacity=32769), ValueError), (dict(capacity=4.0), TypeError),
                    (dict(batch=-1), ValueError), (dict(batch=True), TypeError)):
        a = dict(batch=2, heads=2, capacity=8, head_dim=8)
        a.update(kw)
        with pytest.raises(exc):
            AttentionCache(**a)
    with pytest.raises(ValueError):
        HippocampalProsodyAttention(_config(20, 2), None).new_cache(1, 8)              # head_dim 10
    with pytest.raises(ValueError):
        HippocampalProsodyAttention(_config(4096, 32), None).new_cache(1, 8)           # D > 2048
    torch.manual_seed(0)
    att = HippocampalProsodyAttention(_config(16, 2), object()).eval()
    cache = att.new_cache(2, 5)
    assert tuple(cache.k.shape) == (2, 2, 5, 8) and cache.lengths.dtype == torch.int32 and cache.max_length == 0
    assert cache.workspace.numel() == ops.attn_decode_workspace_floats(2, 2, 8, 1)
    hidden = torch.randn(2, 6, 16)
    bad = [
        (lambda: att.prefill(hidden, cache=cache), ValueError),                        # 6 positions into 5
        (lambda: att.prefill(hidden[:, :4], cache=None), TypeError),
        (lambda: att.prefill(hidden[:1, :4], cache=cache), ValueError),                # batch
        (lambda: att.prefill(hidden[:, :4, :8], cache=cache), ValueError),
        (lambda: att.prefill(hidden[:, :4].double(), cache=cache), TypeError),
        (lambda: att.prefill(hidden[:, :4], cache=cache, lengths=[4, 5]), ValueError),   # longer than the prompt
        (lambda: att.prefill(hidden[:, :4], cache=cache, lengths=[4]), ValueError),
        (lambda: att.prefill(hidden[:, :4], cache=cache, lengths=[1.0, 2.0]), ValueError),
        (lambda: att.step(hidden[:, 0, :8], cache=cache), ValueError),
        (lambda: att.step(hidden[:, :2], cache=cache), ValueError),                    # two tokens
        (lambda: att.step(hidden[:, 0].half(), cache=cache), TypeError),
        (lambda: att.step(hidden[:, 0], prosody=torch.zeros(2, 3), cache=cache), ValueError),
        (lambda: att.step(hidden[:1, 0], cache=cache), ValueError),
        (lambda: att.step(hidden[:, 0], cache=att.new_cache(2, 5).k), TypeError),
    ]
    for fn, exc in bad:
        with pytest.raises(exc):
            fn()
    assert STUB.CALLS["step"] == 0
    att.prefill(hidden[:, :4], cache=cache)
    att.step(hidden[:, 4], cache=cache)
    assert cache.max_length == 5 and cache.lengths.tolist() == [5, 5]
    with pytest.raises(RuntimeError, match="full"):
        att.step(hidden[:, 5], cache=cache)
    assert STUB.CALLS["step"] == 1, "a step past the capacity must raise before the op"


def test_a_step_refuses_cpu_tensors_without_the_stub():
    from aura_snn_rag_amd import HippocampalProsodyAttention, ops
    att = HippocampalProsodyAttention(_config(16, 2), object()).eval()
    cache = att.new_cache(1, 4)
    with pytest.raises(ops.AuraDeviceError):
        att.step(torch.zeros(1, 16), cache=cache)


# ------------------------------------------------------------------------------------- the modules
def test_the_modules_keep_the_reference_surface():
    from aura_snn_rag_amd import HippocampalProsodyAttention, HippocampalTransformerLayer
    case = _golden()["cases"][0]
    B, S, D, H = case["shape"]
    att = HippocampalProsodyAttention(_config(D, H), object()).eval()
    assert sorted(att.state_dict()) == KEYS and len(KEYS) == 12
    att.load_state_dict(case["state_dict"], strict=True)
    assert (att.hidden_size, att.num_heads, att.head_dim, att.dropout) == (D, H, D // H, 0.0)
    with torch.no_grad():
        for variant, kw in (("prosody", dict(prosody=case["prosody"])), ("no_prosody", dict()),
                            ("no_memory", dict(prosody=case["prosody"], use_memory=False))):
            out, weights = att(case["hidden"], **kw)
            assert weights is None
            assert torch.allclose(out, case["outputs"][variant], atol=2e-6, rtol=0), variant
        # without a hippocampus the memory gate is off, as upstream
        none = HippocampalProsodyAttention(_config(D, H), None).eval()
        none.load_state_dict(case["state_dict"], strict=True)
        assert torch.allclose(none(case["hidden"], prosody=case["prosody"])[0], case["outputs"]["no_memory"], atol=2e-6,
                              rtol=0)
    layer = HippocampalTransformerLayer(_config(D, H), object())
    want = {"attention_norm.weight", "attention_norm.bias", "ffn_norm.weight", "ffn_norm.bias", "ffn.0.weight",
            "ffn.0.bias", "ffn.2.weight", "ffn.2.bias"} | {"attention." + k for k in KEYS}
    assert set(layer.state_dict()) == want
    # gradients flow through forward and prefill
    hidden = case["hidden"].clone().requires_grad_(True)
    att(hidden, prosody=case["prosody"])[0].sum().backward()
    assert hidden.grad is not None and all(p.grad is not None for p in att.parameters())


def _module(which, D=32, H=4, seed=0):
    from aura_snn_rag_amd import HippocampalProsodyAttention, HippocampalTransformerLayer
    torch.manual_seed(seed)
    cls = HippocampalProsodyAttention if which == "attention" else HippocampalTransformerLayer
    return cls(_config(D, H), object()).eval()


def _first(out):
    return out[0] if isinstance(out, tuple) else out


@pytest.mark.parametrize("which", ["attention", "layer"])
@pytest.mark.parametrize("variant", ["prosody", "no_prosody", "no_memory"])
def test_prefill_and_steps_equal_forward_at_every_position(monkeypatch, which, variant):
    STUB.install(monkeypatch)
    mod = _module(which)
    B, S, P, D = 3, 11, 5, 32
    hidden, prosody = torch.randn(B, S, D), 1.5 * torch.randn(B, S, 4)
    pro = (lambda a, b: None) if variant == "no_prosody" else (lambda a, b: prosody[:, a:b])
    mem = variant != "no_memory"
    with torch.no_grad():
        full = _first(mod(hidden, prosody=pro(0, S), use_memory=mem))
        cache = mod.new_cache(B, 16)
        rows = [_first(mod.prefill(hidden[:, :P], prosody=pro(0, P), use_memory=mem, cache=cache))]
        for t in range(P, S):
            step_in = hidden[:, t:t + 1] if t % 2 else hidden[:, t]                 # [B, 1, D] and [B, D]
            rows.append(mod.step(step_in, prosody=pro(t, t + 1), use_memory=mem, cache=cache)[:, None])
    stepped = torch.cat(rows, dim=1)
    assert stepped.shape == full.shape
    assert float((stepped - full).abs().max()) <= 2e-5 * max(1.0, float(full.abs().max()))
    assert STUB.CALLS["step"] == S - P and cache.lengths.tolist() == [S] * B and cache.max_length == S
    assert STUB.LAST["prosody"] == (variant != "no_prosody") and STUB.LAST["memory"] == mem
    mod.prefill(hidden[:, :P].clone().requires_grad_(True), cache=cache)            # prefill keeps autograd usable


@pytest.mark.parametrize("which", ["attention", "layer"])
def test_right_padded_prompts_step_to_the_same_outputs(monkeypatch, which):
    STUB.install(monkeypatch)
    mod = _module(which, seed=1)
    B, D, P, n_new = 3, 32, 6, 4
    lens = [6, 3, 1]
    seqs = [torch.randn(L + n_new, D) for L in lens]                                 # each row's true sequence
    pros = [1.5 * torch.randn(L + n_new, 4) for L in lens]
    with torch.no_grad():
        want = [_first(mod(s[None], prosody=p[None]))[0] for s, p in zip(seqs, pros)]
        prompt, pp = torch.zeros(B, P, D), torch.zeros(B, P, 4)
        for b, L in enumerate(lens):
            prompt[b, :L], pp[b, :L] = seqs[b][:L], pros[b][:L]
            prompt[b, L:] = 7.0                                                       # padding that would show
        cache = mod.new_cache(B, 12)
        pre = _first(mod.prefill(prompt, prosody=pp, cache=cache, lengths=lens))
        assert cache.lengths.tolist() == lens and cache.max_length == P
        for b, L in enumerate(lens):
            assert float((pre[b, :L] - want[b][:L]).abs().max()) <= 2e-5
        for i in range(n_new):
            tok = torch.stack([seqs[b][L + i] for b, L in enumerate(lens)])
            pr = torch.stack([pros[b][L + i] for b, L in enumerate(lens)])
            out = mod.step(tok, prosody=pr, cache=cache)
            for b, L in enumerate(lens):
                assert float((out[b] - want[b][L + i]).abs().max()) <= 2e-5, (b, i)
    assert cache.lengths.tolist() == [L + n_new for L in lens] and cache.max_length == P + n_new


def test_a_retired_row_returns_zeros_and_keeps_its_cache(monkeypatch):
    STUB.install(monkeypatch)
    att = _module("attention", seed=2)
    hidden = torch.randn(3, 7, 32)
    with torch.no_grad():
        cache = att.new_cache(3, 10)
        att.prefill(hidden[:, :5], cache=cache)
        cache.retire([1])
        k0, v0 = cache.k.clone(), cache.v.clone()
        out = att.step(hidden[:, 5], cache=cache)
        ctx_zero = att.o_proj(torch.zeros(1, 32))[0]                                   # zeros through o_proj: its bias
        assert torch.equal(out[1], ctx_zero) and not torch.equal(out[0], ctx_zero)
        assert torch.equal(cache.k[1], k0[1]) and torch.equal(cache.v[1], v0[1])
        assert not torch.equal(cache.k[0], k0[0])
        assert cache.lengths.tolist() == [6, -1, 6]
        full = att(hidden[:, :6])[0]
        assert float((out[0] - full[0, 5]).abs().max()) <= 2e-5
