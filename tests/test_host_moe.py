"""The MoE language zone on the CPU: the ``state_dict`` surface against the reference's
(tests/golden/moe_zone_keys.json), the fp64 rule and its fp32 restatement (tests/moe_rule.py) against the reference's
recorded outputs (tests/golden/moe_zone.pt, written by tools/gen_golden_moe.py), the host-side refusals of the ops, and
the modules' plumbing on CPU stand-ins of the ops (tests/cpu_stub_moe.py)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cpu_stub_moe as STUB
from tests import moe_rule as RULE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = os.path.join(HERE, "golden", "moe_zone_keys.json")
CASES = os.path.join(HERE, "golden", "moe_zone.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(CASES, weights_only=True)["cases"]


def _router_args(sd):
    return [sd[k].numpy() for k in ("cell.U.weight", "cell.U.bias", "cell.W.bias", "gate_proj.weight", "gate_proj.bias")]


def _expert_lists(sd, layers=2):
    """The flat parameter list of ``ops.moe_expert_table`` from an expert's ``state_dict`` and the default settings."""
    from aura_snn_rag_amd.core.language_zone.snn_expert import SNNExpert
    proto = SNNExpert(4, 4, 4, num_layers=layers)
    tensors = []
    for l in range(layers):
        tensors += [sd[f"layers.{2 * l}.weight"], sd[f"layers.{2 * l}.bias"], sd[f"layers.{2 * l + 1}.linear.weight"],
                    sd[f"layers.{2 * l + 1}.linear.bias"]]
    tensors += [sd["readout.weight"], sd["readout.bias"]]
    return [t.numpy() for t in tensors], proto.fused_parameters()[1]


# ------------------------------------------------------------------------------------------------ the reference's surface
def test_the_state_dict_keys_and_shapes_are_the_references():
    from aura_snn_rag_amd.core.language_zone.moe_language_zone import MoELanguageZone
    from aura_snn_rag_amd.core.language_zone.snn_expert import SNNExpert
    from aura_snn_rag_amd.core.liquid_moe import LiquidGatingNetwork, LiquidMoERouter
    g = json.load(open(KEYS))
    keys = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]
    zone = MoELanguageZone(**g["zone_args"])
    assert keys(zone) == g["zone"]
    assert keys(LiquidMoERouter(**g["router_args"])) == g["router"]
    assert keys(LiquidGatingNetwork(**g["router_args"])) == g["router"]
    assert keys(SNNExpert(**g["expert_args"])) == g["expert"]
    # a checkpoint of those keys loads strictly
    zone.load_state_dict({k: torch.zeros(shape) for k, shape in g["zone"]}, strict=True)
    for name in ("vocab_size", "embed_dim", "hidden_dim", "moe_hidden_dim", "top_k", "num_experts", "embeddings",
                 "encoder", "spike_to_continuous", "experts", "moe_router", "continuous_to_spike", "decoder",
                 "output_proj"):
        assert hasattr(zone, name), name
    assert zone.moe_router.temperature == 1.0 and zone.moe_router.expert_usage.shape == (4,)


def test_the_loaded_golden_router_state_fits_our_router(golden):
    from aura_snn_rag_amd.core.liquid_moe import LiquidMoERouter
    s = golden["e4"]["shape"]
    router = LiquidMoERouter(s["Dm"], s["Hr"], s["E"], s["top_k"])
    router.load_state_dict(golden["e4"]["router"], strict=True)


# ------------------------------------------------------------------------------------------------ the rule against the record
@pytest.mark.parametrize("case", ["e4", "e1"])
@pytest.mark.parametrize("gain", [False, True])
def test_the_route_rule_reproduces_the_recorded_router(golden, case, gain):
    c = golden[case]
    s = c["shape"]
    k = min(s["top_k"], s["E"])
    rec = c["route_gain" if gain else "route"]
    g = c["attn_gain"].numpy() if gain else None
    r64 = RULE.route64(c["x"].numpy(), *_router_args(c["router"]), 0.02, k, 1.0, g)
    assert (r64["order_margin"] > 0).all(), "the fixture's seed leaves no order open"
    assert np.array_equal(r64["indices"], rec["indices"].numpy())
    for name, bound in (("probs", "dprobs"), ("weights", "dweights")):
        share = np.abs(rec[name].numpy().astype(np.float64) - r64[name]) / r64[bound]
        assert share.max() <= 1.0, (name, share.max())
    r32 = RULE.route32(c["x"].numpy(), *_router_args(c["router"]), 0.02, k, 1.0, g)
    assert np.array_equal(r32["indices"], r64["indices"])
    for name, bound in (("probs", "dprobs"), ("weights", "dweights")):
        share = np.abs(r32[name].astype(np.float64) - r64[name]) / r64[bound]
        assert share.max() <= 0.5, (name, share.max())
    if gain:                                                    # both clamps are in the fixture
        t = 1.0 / (g + 1e-6)
        assert (t > 5.0).any() and (t < 0.1).any()


@pytest.mark.parametrize("case", ["e4", "e1"])
def test_the_expert_rule_reproduces_the_recorded_experts_and_the_dense_sum(golden, case):
    c = golden[case]
    s = c["shape"]
    k = min(s["top_k"], s["E"])
    x = c["x"].numpy()
    y64, dy, y32 = [], [], []
    for e in range(s["E"]):
        params, gif = _expert_lists(c["experts"][e])
        r = RULE.expert64(x, params, gif)
        assert not r["open"].any(), "the fixture's seed leaves no spike open"
        share = np.abs(c["predict"][e].numpy().astype(np.float64) - r["y"]) / r["bound"]
        assert share.max() <= 1.0, (e, share.max())
        ours, _ = RULE.expert32(x, params, gif)
        assert (np.abs(ours.astype(np.float64) - r["y"]) / r["bound"]).max() <= 0.5
        y64.append(r["y"]); dy.append(r["bound"]); y32.append(ours)
    r64 = RULE.route64(x, *_router_args(c["router"]), 0.02, k)
    idx = r64["indices"]
    rows = np.arange(x.shape[0])[:, None]
    pick = lambda per_expert: np.stack(per_expert)[idx, rows]                       # [N, k, Dm]
    comb = RULE.combine64(pick(y64), pick(dy), r64["weights"], r64["dweights"])
    share = np.abs(c["dense"].numpy().astype(np.float64) - comb["out"]) / comb["bound"]
    assert share.max() <= 1.0, share.max()
    r32 = RULE.route32(x, *_router_args(c["router"]), 0.02, k)
    ours = RULE.combine32(pick(y32), r32["weights"], r32["indices"])
    assert (np.abs(ours.astype(np.float64) - comb["out"]) / comb["bound"]).max() <= 0.5


def test_the_tie_rule_and_the_exact_restatements():
    p = np.array([[0.25, 0.25, 0.25, 0.25], [0.1, np.nan, 0.6, 0.3], [0.0, 0.5, 0.5, 0.0]], dtype=np.float32)
    assert RULE.topk_order(p, 2).tolist() == [[0, 1], [1, 2], [1, 2]]
    w = RULE.weights32(p, RULE.topk_order(p, 2))
    assert w[0].tolist() == [0.5, 0.5] and np.isnan(w[1]).all()
    # ascending expert id, whatever the rank order: 3 * 1 then + 2 * 10
    y = np.array([[[10.0], [1.0]]], dtype=np.float32)
    out = RULE.combine32(y, np.array([[2.0, 3.0]], dtype=np.float32), np.array([[5, 1]]))
    assert out.tolist() == [[23.0]]


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_bad_arguments_are_refused_before_the_library_is_loaded(monkeypatch):
    from aura_snn_rag_amd import _lib, ops
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    x, U, b = torch.zeros(5, 8), torch.zeros(6, 8), torch.zeros(6)
    G, gb = torch.zeros(3, 6), torch.zeros(3)
    ok = dict(dt=0.02, k=2)
    with pytest.raises(ops.AuraDeviceError):
        ops.moe_route(x, U, b, b, G, gb, **ok)
    for bad in (lambda: ops.moe_route(torch.zeros(5, 6), torch.zeros(6, 6), b, b, G, gb, **ok),      # Dm % 4
                lambda: ops.moe_route(torch.zeros(5, 260), torch.zeros(6, 260), b, b, G, gb, **ok),  # Dm > 256
                lambda: ops.moe_route(x, torch.zeros(6, 12), b, b, G, gb, **ok),                      # U's width
                lambda: ops.moe_route(x, torch.zeros(300, 8), torch.zeros(300), torch.zeros(300),
                                      torch.zeros(3, 300), gb, **ok),                                 # Hr > 256
                lambda: ops.moe_route(x, U, b, b, torch.zeros(65, 6), torch.zeros(65), **ok),         # E > 64
                lambda: ops.moe_route(x, U, b, b, G, gb, dt=0.02, k=4),                               # k > E
                lambda: ops.moe_route(x, U, b, b, torch.zeros(16, 6), torch.zeros(16), dt=0.02, k=9), # k > 8
                lambda: ops.moe_route(x, U, b, b, G, gb, dt=0.02, k=2, attn_gain=torch.zeros(4)),
                lambda: ops.moe_route(x.t().contiguous().t(), U, b, b, G, gb, **ok)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.moe_route(x.double(), U, b, b, G, gb, **ok)

    def expert(Dm=8, Hh=12, layers=1, L=16):
        ts = []
        for l in range(layers):
            ts += [torch.zeros(Hh, Dm if l == 0 else Hh), torch.zeros(Hh), torch.zeros(Hh, Hh), torch.zeros(Hh)]
        return ts + [torch.zeros(Dm, Hh), torch.zeros(Dm)], [(0.9, L, 0.01, 1.0)] * layers

    for kw in (dict(Hh=10), dict(Hh=516), dict(Dm=260), dict(layers=5), dict(L=65), dict(L=0)):
        ts, g = expert(**kw)
        with pytest.raises(ValueError):
            ops.moe_expert_table([ts], [g])
    ts, g = expert()
    with pytest.raises(ValueError):
        ops.moe_expert_table([ts, expert(Hh=16)[0]], [g, g])                                          # unequal experts
    with pytest.raises(ValueError):
        ops.moe_expert_table([ts[:2] + [None] + ts[3:]], [g])                                         # no bias
    with pytest.raises(ops.AuraDeviceError):
        ops.moe_expert_table([ts], [g])
    with pytest.raises(TypeError):
        ops.moe_experts(x, "routing", None)


# ------------------------------------------------------------------------------------------------ plumbing on the stubs
def _cpu_gif(monkeypatch):
    """The GIF loop of the encoder and the decoder in torch on the CPU (the rule of ``ops.gif_run`` in fp32)."""
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.language_zone import gif_neuron

    def gif_run(h, out, v, theta, decay, L, alpha, threshold, T, time_invariant=False, mean_out=False):
        assert not time_invariant and not mean_out
        for t in range(T):
            v.mul_(decay).add_(h[:, t])
            cl = L * theta * 2.0
            v.copy_(torch.minimum(torch.maximum(v, -cl), cl))
            s = torch.clamp(torch.floor(v / (theta + 1e-6)), 0, L)
            v.sub_(s * theta)
            if alpha > 0:
                theta.copy_(theta + alpha * s - alpha * (theta - threshold))
            out[:, t] = s

    monkeypatch.setattr(ops, "gif_run", gif_run)
    monkeypatch.setattr(gif_neuron, "_check_input", lambda x, who: None)


def _zone(seed=0, **kw):
    from aura_snn_rag_amd.core.language_zone.moe_language_zone import MoELanguageZone
    torch.manual_seed(seed)
    args = dict(vocab_size=50, embed_dim=12, hidden_dim=16, num_experts=4, top_k=2, moe_hidden_dim=8)
    args.update(kw)
    zone = MoELanguageZone(**args)
    with torch.no_grad():
        zone.moe_router.gate_proj.weight.mul_(100.0)
    return zone


def test_forward_on_the_stubs_shapes_usage_and_the_table(monkeypatch):
    STUB.install(monkeypatch)
    _cpu_gif(monkeypatch)
    zone = _zone().eval()
    ids = torch.randint(0, 50, (2, 5))
    with torch.no_grad():
        logits, extra = zone(ids)
    assert logits.shape == (2, 5, 50) and extra["probs"].shape == (2, 5, 4)
    assert torch.allclose(extra["probs"].sum(-1), torch.ones(2, 5), atol=1e-5)
    assert STUB.CALLS == {"moe_route": 1, "moe_expert_table": 1, "moe_experts": 1}
    assert torch.equal(zone.moe_router.expert_usage, torch.zeros(4)), "eval leaves expert_usage alone"
    # the table is kept ...
    with torch.no_grad():
        zone(ids)
    assert STUB.CALLS["moe_expert_table"] == 1
    # ... and rebuilt after a parameter write, a new storage or a changed neuron setting
    with torch.no_grad():
        zone.experts["expert_2"].readout.bias.add_(1.0)
        zone(ids)
    assert STUB.CALLS["moe_expert_table"] == 2
    zone.experts["expert_0"].layers[0].weight.data = zone.experts["expert_0"].layers[0].weight.data.clone()
    zone.experts["expert_1"].layers[1].threshold = 0.5
    with torch.no_grad():
        zone(ids)
    assert STUB.CALLS["moe_expert_table"] == 3
    # training under no_grad updates the usage from the indices: every token adds k = 2 selections
    zone.train()
    with torch.no_grad():
        out = zone.route_experts(torch.randn(10, 8), return_trace=True)
    assert out.trace.shape == (10, 2, 2, 8) and out.indices.dtype == torch.int64
    usage = zone.moe_router.expert_usage
    assert abs(float(usage.sum()) - 0.01 * 2.0) < 1e-6
    counts = torch.bincount(out.indices.flatten(), minlength=4).float()
    assert torch.allclose(usage, 0.01 * counts / 10)


def test_the_stub_route_experts_equals_the_dense_loop_over_all_tokens(monkeypatch):
    """The sparse result on the stand-ins against the reference's dense formulation from the same modules' parameters:
    every expert over all tokens, masked by the routing weight (the stand-ins' own fp32 restatement)."""
    STUB.install(monkeypatch)
    zone = _zone(seed=3).eval()
    x = torch.randn(40, 8)
    with torch.no_grad():
        out = zone.route_experts(x)
    dense = torch.zeros(40, 8)
    for i in range(4):
        ts, gif = zone.experts[f"expert_{i}"].fused_parameters()
        y, _ = RULE.expert32(x.numpy(), [t.detach().numpy() for t in ts], gif)
        w = (out.weights * (out.indices == i).float()).sum(1, keepdim=True)
        dense += torch.from_numpy(y) * w
    assert torch.allclose(out.expert_outputs, dense, atol=1e-5, rtol=1e-5)
    assert len(set(out.indices.flatten().tolist())) > 1


# ------------------------------------------------------------------------------------------------ the generated code
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_no_valu_write_right_before_an_mfma_in_the_experts_kernel(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_mfma_hazards as chk
    asm = tmp_path / "aura_moe.s"
    src = os.path.join(ROOT, "aura_snn_rag_amd", "csrc", "aura_moe.hip")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                           "-Wno-unused-function", "--cuda-device-only", "-S", src, "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    n, bad = chk.check(str(asm), kernels=("moe_experts_kernel",))
    assert n >= 12, "the experts kernel's MFMAs were not found in the generated code"
    assert not bad, bad[:3]
    text = asm.read_text()
    assert "v_mfma_f32_32x32x2_f32" in text or "v_mfma_f32_32x32x2f32" in text
