"""``MemoryAugmentedLayer`` and ``SNNRAGTransformer`` on the CPU: the ``state_dict`` surface against the reference's
(tests/golden/snn_rag_transformer_keys.json), ``forward(memory=context)`` of the MLP layers against the reference's
recorded outputs (tests/golden/memory_augmented_layer.pt, written by tools/gen_golden_snn_rag.py), the host-side refusals
of ``ops.row_linear_gate`` and of ``step(fused=True)``, and the cached step and ``generate`` on CPU stand-ins of the ops
(tests/cpu_stub_*.py) with a small stand-in bank.

Parity with the recorded outputs.  The fixture's outputs are the reference's fp32 evaluation; ours is another fp32
evaluation of the same formula (a batched softmax-weighted sum instead of a loop, the library's attention).  The
yardstick is the recorded output's own distance from the module in double precision; ours must be within 4 times that,
the margin tests/test_gpu_fused_step.py uses for the same reason: two fp32 evaluations that differ in summation order.
Both distances go to the parity record."""
import json
import os
import types

import pytest
import torch

from tests import cpu_stub_decode_attention as DECODE
from tests import cpu_stub_place_code as PLACE
from tests import cpu_stub_row_linear as ROWLIN
from tests import cpu_stub_row_linear_epilogue as GATE
from tests import cpu_stub_sampling as SAMPLE
from tests import cpu_stub_theta_gamma as THETA
from tests import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = os.path.join(HERE, "golden", "snn_rag_transformer_keys.json")
LAYERS = os.path.join(HERE, "golden", "memory_augmented_layer.pt")
INJECTIONS = ("cross_attention", "concat", "gate")


class StandInBank:
    """The three members of ``HippocampalFormation`` the batched retrieval touches, on the CPU: exact cosine top-k."""

    def __init__(self, features):
        self.features = features
        self.memory_count = features.shape[0]
        self.recalls = 0

    def recall_batch(self, query, k=5, **kw):
        self.recalls += 1
        unit = torch.nn.functional.normalize(self.features, dim=-1)
        scores, rows = torch.topk(torch.nn.functional.normalize(query, dim=-1) @ unit.T, k, dim=-1)
        return scores, rows.to(torch.int32)

    def gather_features(self, rows):
        return self.features[rows.long()]


def _config(D=96, H=4, dropout=0.0, **kw):
    return types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=dropout, intermediate_size=2 * D, **kw)


def _layer(inj="gate", snn=False, bank=None, D=96, H=4, dropout=0.0, seed=0):
    from aura_snn_rag_amd import MemoryAugmentedLayer
    torch.manual_seed(seed)
    return MemoryAugmentedLayer(_config(D, H, dropout), bank, use_snn_ffn=snn, memory_injection=inj).eval()


def _context(B=3, k=5, D=96, seed=9):
    from aura_snn_rag_amd import MemoryContext
    g = torch.Generator().manual_seed(seed)
    return MemoryContext(torch.randn(B, k, D, generator=g), torch.rand(B, k, generator=g), None)


# ------------------------------------------------------------------------------------------------ the reference's surface
def test_the_state_dict_keys_and_shapes_are_the_references():
    from aura_snn_rag_amd import MemoryAugmentedLayer, SNNRAGTransformer
    golden = json.load(open(KEYS))
    cfg = types.SimpleNamespace(**golden["config"])
    shapes = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert {k: len(v) for k, v in golden["models"].items()} == dict(cross_attention=76, concat=64, gate=72)
    for inj in INJECTIONS:
        model = SNNRAGTransformer(cfg, None, memory_injection=inj)
        assert shapes(model) == golden["models"][inj], inj
        assert model.output_head.weight is model.semantic_encoder.token_embedding.weight, "the head is tied"
        assert model.snn_layers == {0} and [l.use_snn_ffn for l in model.layers] == [True, False]
        for snn in (False, True):
            layer = MemoryAugmentedLayer(cfg, None, use_snn_ffn=snn, memory_injection=inj)
            assert shapes(layer) == golden["layers"][f"{inj}-{'snn' if snn else 'mlp'}"], (inj, snn)
    with pytest.raises(ValueError):
        MemoryAugmentedLayer(cfg, None, memory_injection="prepend")
    # defaults and switches of the constructors
    assert SNNRAGTransformer(cfg, None).layers[0].memory_injection == "gate"
    assert [l.use_snn_ffn for l in SNNRAGTransformer(cfg, None, use_snn_ffn=False).layers] == [False, False]
    assert [l.use_snn_ffn for l in SNNRAGTransformer(cfg, None, snn_layers=[1]).layers] == [False, True]
    assert MemoryAugmentedLayer(cfg, None).memory_injection == "cross_attention"


def test_the_constructors_print_nothing(capsys):
    from aura_snn_rag_amd import SNNRAGTransformer
    SNNRAGTransformer(types.SimpleNamespace(**json.load(open(KEYS))["config"]), None)
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("inj", INJECTIONS)
def test_forward_with_a_given_context_is_the_references_forward(inj):
    from aura_snn_rag_amd import MemoryAugmentedLayer, MemoryContext
    data = torch.load(LAYERS)
    B, S, D, H, K = data["shape"]
    case = data["cases"][inj]
    layer = MemoryAugmentedLayer(_config(D, H), object(), use_snn_ffn=False, memory_injection=inj,
                                 num_retrieved=K).eval()
    layer.load_state_dict(case["state_dict"])
    ctx = MemoryContext(case["features"], case["scores"], None)
    with torch.no_grad():
        ours = {"memory": layer(case["hidden"], prosody=case["prosody"], use_memory=True, memory=ctx),
                "no_memory": layer(case["hidden"], prosody=case["prosody"], use_memory=False, memory=ctx)}
        layer.double()
        ctx64 = MemoryContext(ctx.features.double(), ctx.scores.double(), None)
        ref64 = {"memory": layer(case["hidden"].double(), prosody=case["prosody"].double(), use_memory=True,
                                 memory=ctx64),
                 "no_memory": layer(case["hidden"].double(), prosody=case["prosody"].double(), use_memory=False)}
    assert float((ref64["memory"] - ref64["no_memory"]).abs().max()) > 1e-2, "the memories reach the output"
    for name in ("memory", "no_memory"):
        recorded = float((case["outputs"][name].double() - ref64[name]).abs().max())
        mine = float((ours[name].double() - ref64[name]).abs().max())
        print(f"memory layer {inj} {name}: recorded {recorded:.3e}, ours {mine:.3e} from fp64")
        helpers.record_parity(f"memory layer fixture {inj} {name}", int(mine <= 4.0 * recorded), 1,
                              recorded_error=recorded, our_error=mine,
                              magnitude=float(ref64[name].abs().max()))
        assert ours[name].shape == (B, S, D) and mine <= 4.0 * recorded


@pytest.mark.parametrize("inj", INJECTIONS)
def test_without_a_bank_the_layer_is_attention_and_feed_forward(inj):
    from aura_snn_rag_amd import HippocampalTransformerLayer
    layer = _layer(inj, seed=2)
    plain = HippocampalTransformerLayer(_config(), None).eval()
    theirs = plain.state_dict()
    plain.load_state_dict({k: v for k, v in layer.state_dict().items() if k in theirs})
    hidden, prosody = torch.randn(2, 6, 96), torch.randn(2, 6, 4)
    with torch.no_grad():
        assert layer.retrieve_context(hidden) is None
        assert torch.equal(layer(hidden, prosody=prosody), plain(hidden, prosody=prosody))
    empty = _layer(inj, bank=StandInBank(torch.zeros(0, 96)), seed=2)
    assert empty.retrieve_context(hidden) is None


@pytest.mark.parametrize("inj", INJECTIONS)
def test_retrieval_is_one_batched_recall_and_a_given_context_skips_it(inj):
    from aura_snn_rag_amd import MemoryContext
    bank = StandInBank(torch.randn(40, 96, generator=torch.Generator().manual_seed(1)))
    layer = _layer(inj, bank=bank, seed=3)
    hidden = torch.randn(3, 6, 96)
    with torch.no_grad():
        want = layer(hidden)                                                # the reference's behaviour: retrieve, inject
        assert bank.recalls == 1
        attn = hidden + layer.attention(layer.attention_norm(hidden))[0]
        ctx = layer.retrieve_context(attn)
        assert isinstance(ctx, MemoryContext) and ctx.features.shape == (3, 5, 96) and ctx.scores.shape == (3, 5)
        assert bank.recalls == 2
        assert torch.equal(layer(hidden, memory=ctx), want) and bank.recalls == 2, "a given context retrieves nothing"
        # with the context fixed the layer is causal; with retrieval from the mean it is not
        assert float((layer(hidden[:, :4], memory=ctx) - want[:, :4]).abs().max()) <= 1e-5
        assert float((layer(hidden[:, :4]) - want[:, :4]).abs().max()) > 1e-4
    with pytest.raises(TypeError):
        layer(hidden, memory=(ctx.features, ctx.scores))
    with pytest.raises(ValueError):
        layer(hidden[:2], memory=ctx)


def test_store_memory_reaches_the_bank_in_training_only_and_in_the_last_layer():
    from aura_snn_rag_amd import SNNRAGTransformer
    stored = []
    bank = StandInBank(torch.randn(8, 96))
    bank.create_episodic_memories = lambda ids, feats, **kw: stored.append((len(ids), tuple(feats.shape)))
    layer = _layer("concat", bank=bank)
    hidden = torch.randn(2, 4, 96)
    layer(hidden, store_memory=True)
    assert stored == [], "eval mode stores nothing, as upstream"
    layer.train()(hidden, store_memory=True)
    assert stored == [(2, (2, 96))]
    calls = []
    cfg = types.SimpleNamespace(**json.load(open(KEYS))["config"])
    model = SNNRAGTransformer(cfg, None, use_snn_ffn=False)
    for i, l in enumerate(model.layers):
        l.forward = lambda h, _i=i, **kw: calls.append((_i, kw["store_memory"])) or h
    import aura_snn_rag_amd.core.language_zone.snn_rag_transformer as M
    real = M.embed_tokens
    try:
        M.embed_tokens = lambda ids, *a, **kw: (torch.zeros(ids.shape[0], ids.shape[1], 96), None)
        model(torch.zeros(2, 3, dtype=torch.int64), store_memory=True)
    finally:
        M.embed_tokens = real
    assert calls == [(0, False), (1, True)]


# ------------------------------------------------------------------------------------------------ refusals on the host
def _gate_args(R=3, K=16, N=5):
    z = torch.zeros
    return dict(x=z(R, K), weight=z(N, 2 * K)[:, :K], bias=z(N), u=z(R, N), c=z(R, N), residual=z(R, N))


def test_row_linear_gate_refuses_bad_arguments_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    z = torch.zeros
    bad = [
        (dict(x=z(33, 16), u=z(33, 5), c=z(33, 5), residual=z(33, 5)), ValueError, "R = 33"),
        (dict(x=z(0, 16)), ValueError, "R = 0"),
        (dict(x=z(3, 18), weight=z(5, 18)), ValueError, "K % 4"),
        (dict(x=z(3, 8196), weight=z(5, 8196)), ValueError, "K = 8196"),
        (dict(x=z(3, 16).half()), TypeError, "fp16 x"),
        (dict(x=z(16)), ValueError, "x rank"),
        (dict(x=None), ValueError, "missing x"),
        (dict(weight=None), ValueError, "missing weight"),
        (dict(weight=z(5, 16).bfloat16()), TypeError, "bf16 weight"),
        (dict(weight=[[0.0] * 16] * 5), TypeError, "a weight that is no tensor"),
        (dict(weight=z(5, 12)), ValueError, "weight K"),
        (dict(weight=z(0, 16)), ValueError, "N = 0"),
        (dict(weight=z(5, 16, 1)), ValueError, "weight rank"),
        (dict(weight=z(5, 32)[:, ::2]), ValueError, "a row that is not dense"),
        (dict(weight=z(5, 18)[:, :16]), ValueError, "a row stride that is no multiple of 4"),
        (dict(weight=z(16, 5).T), ValueError, "a transposed weight"),
        (dict(bias=z(6)), ValueError, "bias length"),
        (dict(bias=z(5).double()), TypeError, "fp64 bias"),
        (dict(u=None), ValueError, "missing u"),
        (dict(c=None), ValueError, "missing c"),
        (dict(residual=None), ValueError, "missing residual"),
        (dict(u=z(3, 6)), ValueError, "u shape"),
        (dict(c=z(2, 5)), ValueError, "c shape"),
        (dict(residual=z(3, 10)[:, ::2]), ValueError, "non-contiguous residual"),
        (dict(c=z(3, 5).half()), TypeError, "fp16 c"),
        (dict(out=z(3, 6)), ValueError, "out shape"),
    ]
    for change, exc, why in bad:
        a = dict(_gate_args(), out=None)
        a.update(change)
        out = a.pop("out")
        with pytest.raises(exc):
            ops.row_linear_gate(a["x"], a["weight"], a["bias"], a["u"], a["c"], a["residual"], out=out)
            pytest.fail(f"accepted: {why}")
    # valid calls get as far as the device check, still without the library: CPU tensors are refused
    for a in (_gate_args(), _gate_args(R=32, K=8192, N=1), dict(_gate_args(), bias=None),
              dict(_gate_args(), weight=z(5, 16))):
        with pytest.raises(ops.AuraDeviceError):
            ops.row_linear_gate(a["x"], a["weight"], a["bias"], a["u"], a["c"], a["residual"])
    assert ops._row_linear_gate_args(**dict(_gate_args(), out=None)) == (3, 16, 5, 32)


def test_the_library_refuses_bad_gate_geometry_and_pointers_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 0x10000                                           # never dereferenced: every call below returns on the host

    def call(R=3, K=16, N=5, ldw=32, **ptr):
        p = dict(x=P, W=P, b=P, u=P, c=P, res=P, y=P)
        p.update(ptr)
        return lib.aura_row_linear_gate(p["x"], R, K, p["W"], ldw, p["b"], p["u"], p["c"], p["res"], p["y"], N, 0, None)
    INVAL, ALIGN = -1, -3
    for kw in (dict(R=0), dict(R=33), dict(K=0), dict(K=18, ldw=20), dict(K=8196, ldw=8196), dict(x=None), dict(W=None),
               dict(u=None), dict(c=None), dict(res=None), dict(y=None), dict(N=0), dict(N=2 ** 31), dict(ldw=12),
               dict(ldw=18), dict(ldw=0)):
        assert call(**kw) == INVAL, kw
    for name in ("x", "W"):
        assert call(**{name: P + 4}) == ALIGN, name
    for name in ("b", "u", "c", "res", "y"):
        assert call(**{name: P + 2}) == ALIGN, name


def _stubs(monkeypatch):
    for stub in (ROWLIN, DECODE, GATE):
        stub.install(monkeypatch)


def test_the_layer_refuses_what_the_fused_step_does_not_cover(monkeypatch):
    _stubs(monkeypatch)
    hidden = torch.randn(3, 8, 96)
    ctx = _context()

    def prefilled(layer, B=3, h=hidden, memory=ctx):
        cache = layer.new_cache(B, 12)
        layer.prefill(h[:, :4], cache=cache, memory=memory)
        return cache
    cross = _layer("cross_attention", bank=object())
    cache = prefilled(cross)
    with pytest.raises(ValueError, match="cross_attention"):
        cross.step(hidden[:, 4], cache=cache, fused=True)
    cross.step(hidden[:, 4], cache=cache)                               # the unfused step takes every injection
    training = _layer("gate", bank=object(), dropout=0.1).train()
    cache = prefilled(training)
    with pytest.raises(RuntimeError, match="dropout"):
        training.step(hidden[:, 4], cache=cache, fused=True)
    training.eval().step(hidden[:, 4], cache=cache, fused=True)         # the same layer in eval mode steps
    assert GATE.CALLS["row_linear_gate"] == 1 and ROWLIN.CALLS["row_linear"] == 4
    tanh = _layer("gate", bank=object())
    tanh.ffn[1] = torch.nn.GELU(approximate="tanh")
    cache = prefilled(tanh)
    with pytest.raises(ValueError, match="GELU"):
        tanh.step(hidden[:, 4], cache=cache, fused=True)
    hybrid = _layer("gate", snn=True, bank=object(), dropout=0.1).train()
    with pytest.raises(RuntimeError, match="dropout"):
        hybrid.step(hidden[:, 4], cache=hybrid.new_cache(3, 12), fused=True)
    wide = _layer("concat", bank=object(), D=16, H=2)
    cache = wide.new_cache(33, 4)
    wide.prefill(torch.randn(33, 2, 16), cache=cache, memory=_context(B=33, D=16))
    with pytest.raises(ValueError, match="32"):
        wide.step(torch.randn(33, 16), cache=cache, fused=True)
    assert GATE.CALLS["row_linear_gate"] == 1 and ROWLIN.CALLS["row_linear"] == 4, "refused before any op"
    with pytest.raises(TypeError):
        wide.step(torch.randn(2, 16), cache=wide.attention.new_cache(2, 4))   # an attention cache is not a layer cache


def test_a_fused_step_refuses_cpu_tensors_without_the_stubs():
    from aura_snn_rag_amd import ops
    layer = _layer("gate", bank=object(), D=16, H=2)
    cache = layer.new_cache(1, 4)
    layer._pin(cache, _context(B=1, D=16))
    with pytest.raises(ops.AuraDeviceError):
        layer.step(torch.zeros(1, 16), cache=cache, fused=True)


# ------------------------------------------------------------------------------------------------ the modules on the stubs
@pytest.mark.parametrize("inj", INJECTIONS)
def test_prefill_and_steps_equal_forward_with_the_pinned_context(monkeypatch, inj):
    _stubs(monkeypatch)
    bank = StandInBank(torch.randn(40, 96, generator=torch.Generator().manual_seed(1)))
    layer = _layer(inj, bank=bank, seed=3)
    with torch.no_grad():                                               # norms that are not the identity
        for n in (layer.attention_norm, layer.ffn_norm):
            n.weight.add_(0.3 * torch.randn(96))
            n.bias.add_(0.3 * torch.randn(96))
    B, P, n_new, D = 3, 7, 6, 96
    S = P + n_new
    hidden, prosody = torch.randn(B, S, D), 1.5 * torch.randn(B, S, 4)
    with torch.no_grad():
        plain = layer.new_cache(B, 16)
        first = layer.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=plain)
        ctx = plain.memory
        assert bank.recalls == 1 and ctx is not None and ctx.features.shape == (B, 5, D)
        assert (plain.c is None) == (inj == "cross_attention") and (plain.u is not None) == (inj == "gate")
        full = layer(hidden, prosody=prosody, memory=ctx)
        tol = 2e-5 * max(1.0, float(full.abs().max()))
        assert float((first - full[:, :P]).abs().max()) <= tol
        fused = layer.new_cache(B, 16)
        layer.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=fused, memory=ctx)
        assert bank.recalls == 1, "a given context is pinned as it is"
        for t in range(P, S):
            step_in = hidden[:, t:t + 1] if t % 2 else hidden[:, t]     # [B, 1, D] and [B, D]
            a = layer.step(step_in, prosody=prosody[:, t], cache=plain)
            assert a.shape == (B, D) and float((a - full[:, t]).abs().max()) <= tol, t
            if inj == "cross_attention":
                continue
            before = ROWLIN.CALLS["row_linear"], DECODE.CALLS["step"], GATE.CALLS["row_linear_gate"]
            b = layer.step(step_in, prosody=prosody[:, t], cache=fused, fused=True)
            after = ROWLIN.CALLS["row_linear"], DECODE.CALLS["step"], GATE.CALLS["row_linear_gate"]
            assert tuple(y - x for x, y in zip(before, after)) == (4, 1, int(inj == "gate"))
            assert float((b - full[:, t]).abs().max()) <= tol, t
        assert bank.recalls == 1, "no step retrieves"
        assert plain.lengths.tolist() == [S] * B and plain.max_length == S
        # use_memory=False injects nothing, although the cache holds a context
        off = layer.new_cache(B, 16)
        layer.prefill(hidden[:, :P], prosody=prosody[:, :P], cache=off, use_memory=False)
        assert off.memory is None and bank.recalls == 1
    if inj == "gate":
        assert GATE.LAST == dict(R=B, K=D, N=D, ldw=2 * D, bias=False), "the left half of memory_gate.0, read in place"


def _model(monkeypatch, bank, **kw):
    for stub in (PLACE, THETA, DECODE, SAMPLE, ROWLIN, GATE):
        stub.install(monkeypatch)
    from aura_snn_rag_amd import SNNRAGTransformer
    torch.manual_seed(0)
    cfg = types.SimpleNamespace(vocab_size=61, embedding_dim=96, num_heads=2, num_layers=2, intermediate_size=192,
                                n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    m = SNNRAGTransformer(cfg, bank, snn_layers=[], **kw).eval()
    with torch.no_grad():
        m.semantic_encoder.token_embedding.weight.mul_(3.0)              # logits of order 1: decisive argmaxes
    return m


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_generate_pins_retrieval_at_the_prompt_and_equals_the_pinned_recompute_loop(monkeypatch, fused):
    bank = StandInBank(torch.randn(40, 96, generator=torch.Generator().manual_seed(1)))
    m = _model(monkeypatch, bank)
    ids = torch.randint(0, 61, (3, 5), generator=torch.Generator().manual_seed(1))
    states = []
    new_state = m.new_state
    monkeypatch.setattr(m, "new_state", lambda *a, **k: states.append(new_state(*a, **k)) or states[-1])
    got = m.generate(ids, max_new_tokens=9, temperature=0.0, repetition_penalty=1.0, fused_step=fused)
    assert bank.recalls == 2, "one recall per layer for the whole generation"
    pinned = m.pinned_memory(states[0])
    out = ids.clone()
    gaps = []
    with torch.no_grad():
        for _ in range(9):
            lg = m(out, memory=pinned)[0][:, -1]
            top2 = torch.topk(lg, 2, dim=-1).values
            gaps.append(float((top2[:, 0] - top2[:, 1]).min()))
            out = torch.cat([out, lg.argmax(-1, keepdim=True)], dim=1)
    assert min(gaps) > 1e-4, "the fixed seed must leave no argmax open"
    assert got.dtype == torch.int64 and torch.equal(got, out)
    assert bank.recalls == 2 and GATE.CALLS["row_linear_gate"] == (2 * 8 if fused else 0)
    with pytest.raises(ValueError, match="per layer"):
        m(ids, memory=pinned[:1])
    with pytest.raises(ValueError, match="32"):
        m.generate(torch.zeros(33, 4, dtype=torch.int64), max_new_tokens=2, fused_step=True)


# ------------------------------------------------------------------------------------------------ the GIF epilogue's host side
def _gif_args(R=8, K=16, N=5, T=4):
    z = torch.zeros
    return dict(x=z(R, K), weight=z(N, K), bias=z(N), T=T, decay=0.9, L=8, alpha=0.01, threshold=1.0,
                time_major=False, mix=None, out=None)


def test_row_linear_gif_refuses_bad_arguments_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    z = torch.zeros
    mix = (z(2, 5), z(2, 5), z(()))
    bad = [
        (dict(x=z(33, 16)), ValueError, "R = 33"),
        (dict(x=z(0, 16)), ValueError, "R = 0"),
        (dict(x=z(8, 18), weight=z(5, 18)), ValueError, "K % 4"),
        (dict(x=z(8, 8196), weight=z(5, 8196)), ValueError, "K = 8196"),
        (dict(x=z(8, 16).half()), TypeError, "fp16 x"),
        (dict(x=None), ValueError, "missing x"),
        (dict(weight=None), ValueError, "missing weight"),
        (dict(weight=z(5, 12)), ValueError, "weight K"),
        (dict(weight=z(0, 16)), ValueError, "N = 0"),
        (dict(weight=z(5, 32)[:, :16]), ValueError, "a strided weight"),
        (dict(bias=z(6)), ValueError, "bias length"),
        (dict(T=0), ValueError, "T = 0"),
        (dict(T=33), ValueError, "T = 33"),
        (dict(T=4.0), TypeError, "a float T"),
        (dict(L=0), ValueError, "L = 0"),
        (dict(decay="0.9"), TypeError, "a decay that is no number"),
        (dict(time_major=True, T=3), ValueError, "R % T"),
        (dict(mix=mix), ValueError, "the mix without time_major"),
        (dict(time_major=True, mix=mix[:2]), ValueError, "a mix of two"),
        (dict(time_major=True, mix=(mix[0], None, mix[2])), ValueError, "a mix with a hole"),
        (dict(time_major=True, mix=(z(2, 6), mix[1], mix[2])), ValueError, "mix residual shape"),
        (dict(time_major=True, mix=(mix[0], mix[1], z(2))), ValueError, "a gate of two floats"),
        (dict(time_major=True, mix=(mix[0], mix[1].double(), mix[2])), TypeError, "fp64 m"),
        (dict(out=z(8, 5)), ValueError, "out of the other form"),
        (dict(time_major=True, out=z(8, 4, 5)), ValueError, "out of the other form"),
    ]
    for change, exc, why in bad:
        a = _gif_args()
        a.update(change)
        x, w, b = a.pop("x"), a.pop("weight"), a.pop("bias")
        with pytest.raises(exc):
            ops.row_linear_gif(x, w, b, **a)
            pytest.fail(f"accepted: {why}")
    for change in ({}, dict(time_major=True), dict(time_major=True, mix=mix), dict(T=32), dict(T=1, time_major=True)):
        a = _gif_args()
        a.update(change)
        x, w, b = a.pop("x"), a.pop("weight"), a.pop("bias")
        with pytest.raises(ops.AuraDeviceError):
            ops.row_linear_gif(x, w, b, **a)


def test_the_library_refuses_bad_gif_geometry_and_pointers_before_any_launch():
    from aura_snn_rag_amd import _lib
    lib = _lib.load()
    P = 0x10000                                           # never dereferenced: every call below returns on the host

    def call(R=8, K=16, N=5, T=4, L=8, time_major=0, **ptr):
        p = dict(x=P, W=P, b=P, out=P, res=None, m=None, gate=None)
        p.update(ptr)
        return lib.aura_row_linear_gif(p["x"], R, K, p["W"], p["b"], p["out"], N, T, 0.9, L, 0.01, 1.0, time_major,
                                       p["res"], p["m"], p["gate"], 0, None)
    INVAL, ALIGN = -1, -3
    three = dict(res=P, m=P, gate=P)
    for kw in (dict(R=0), dict(R=33), dict(K=0), dict(K=18), dict(K=8196), dict(x=None), dict(W=None), dict(out=None),
               dict(N=0), dict(N=2 ** 31), dict(T=0), dict(T=33), dict(L=0), dict(time_major=1, T=3),
               dict(time_major=1, res=P), dict(time_major=1, res=P, m=P), dict(time_major=1, gate=P),
               dict(time_major=0, **three)):
        assert call(**kw) == INVAL, kw
    for name in ("x", "W"):
        assert call(**{name: P + 4}) == ALIGN, name
    for name in ("b", "out"):
        assert call(**{name: P + 2}) == ALIGN, name
    for name in ("res", "m", "gate"):
        assert call(time_major=1, **dict(three, **{name: P + 2})) == ALIGN, name


def test_the_numpy_gif_rule_is_the_oracles_loop():
    import numpy as np
    from oracle import aura_oracle as O
    from tests import row_linear_epilogue_rule as EPI
    g = torch.Generator().manual_seed(2)
    for T, L, scale in ((1, 8, 1.0), (4, 8, 3.0), (8, 16, 100.0), (4, 16, 0.01)):
        c = scale * torch.randn(6 * T, 33, generator=g)
        v, theta = O.gif_initial_state(6, 33, 1.0)
        spikes = O.gif_run(c.view(6, T, 33), v, theta, O.gif_decay(), L, 0.01, 1.0)[0]
        want = spikes.mean(dim=1).numpy()
        got = EPI.gif_mean32(c.numpy(), T, O.gif_decay(), L, 0.01, 1.0)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (T, L, scale)
    y = EPI.hybrid_mix32(np.float32([1.0]), np.float32([2.0]), np.float32([4.0]), 0.0)
    assert float(y[0]) == 4.0                                            # 1 + (0.5 * 2 + 0.5 * 4)


def test_the_fused_hybrid_step_is_eleven_launches_and_the_modules_formula(monkeypatch):
    from oracle import aura_oracle as O
    _stubs(monkeypatch)
    layer = _layer("gate", snn=True, bank=object(), seed=6)
    B, P, D = 3, 4, 96
    hidden, ctx = torch.randn(B, P + 2, D), _context()
    with torch.no_grad():
        cache = layer.new_cache(B, 8)
        layer.attention.prefill(layer.attention_norm(hidden[:, :P]), cache=cache.attention)
        layer._pin(cache, ctx)
        before = ROWLIN.CALLS["row_linear"], DECODE.CALLS["step"], GATE.CALLS["row_linear_gate"], GATE.CALLS["row_linear_gif"]
        got = layer.step(hidden[:, P], cache=cache, fused=True)
        after = ROWLIN.CALLS["row_linear"], DECODE.CALLS["step"], GATE.CALLS["row_linear_gate"], GATE.CALLS["row_linear_gif"]
        # row_linear: q/k/v, o_proj, mlp.0, mlp.2, syn1, syn2; the decode step is two launches: eleven in all
        assert tuple(y - x for x, y in zip(before, after)) == (6, 1, 1, 2)
        assert GATE.LAST["time_major"] and GATE.LAST["mix"] and GATE.LAST["R"] == B * 4
        # the module's formula on the same attention output
        full_att = layer.attention(layer.attention_norm(hidden[:, :P + 1]))[0][:, P]
        h = hidden[:, P] + full_att
        h = layer.inject_memories(h[:, None], ctx.features, ctx.scores)[:, 0]
        x = layer.ffn_norm(h)
        snn = layer.ffn.snn
        c1 = snn.neuron1.linear(snn.syn1(x[:, None])[0])                          # [B, 1, I]
        v, th = O.gif_initial_state(B, snn.hidden_dim, 1.0)
        s1 = O.gif_run(c1.expand(B, 4, snn.hidden_dim), v, th, snn.neuron1.decay, snn.neuron1.L, 0.01, 1.0)[0]
        c2 = snn.neuron2.linear(snn.syn2(s1)[0])
        v, th = O.gif_initial_state(B, D, 1.0)
        s2 = O.gif_run(c2, v, th, snn.neuron2.decay, snn.neuron2.L, 0.01, 1.0)[0].mean(dim=1)
        g = torch.sigmoid(layer.ffn.gate)
        want = h + ((1 - g) * layer.ffn.mlp(x) + g * s2)
        # both sides take their currents from torch's own sums here, so no spike can flip between them
        assert float((got - want).abs().max()) <= 1e-4
