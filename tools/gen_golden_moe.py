"""Writes the two fixtures of the MoE language zone from the reference's classes, on the CPU.

    python tools/gen_golden_moe.py [--dir tests/golden]

Runs on the build machine only, where the reference checkout is present (oracle/_ref_loader.py loads its modules by
path; nothing of it is copied).  Both files hold data alone.
  * ``moe_zone_keys.json``: the ``state_dict`` key names and shapes of the reference's ``MoELanguageZone``,
    ``LiquidMoERouter`` and ``SNNExpert``, with the arguments they were built from.
  * ``moe_zone.pt``: two cases, (N, Dm, Hr, Hh, E, top_k) = (64, 16, 12, 24, 4, 2) and the same with E = 1: the router's
    and every expert's ``state_dict``, the input ``x``, an ``attn_gain``, and the recorded CPU outputs of the router
    (with and without the gain), of every expert's ``predict`` over all rows and of the dense weighted sum the zone's
    loop forms from them.  ``gate_proj.weight`` is scaled up so that the routing varies between tokens: at the
    reference's initialisation the cell's state is at most dt = 0.02 and the bias alone would decide.
The seed of a case is the first for which, in the fp64 rule of tests/moe_rule.py, no top-k order and no spike decision
lies within its bound of flipping (asserted): the recorded fp32 outputs then have one admissible value."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ZONE_ARGS = dict(vocab_size=97, embed_dim=24, hidden_dim=48, num_experts=4, top_k=2, moe_hidden_dim=16)
N, DM, HR, HH, TOP_K = 64, 16, 12, 24, 2
GATE_SCALE = 150.0


def _keys(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def expert_params(expert):
    """The flat parameter list and neuron settings in the order of ``ops.moe_expert_table``."""
    tensors, gif = [], []
    for syn, neuron in zip(expert.layers[0::2], expert.layers[1::2]):
        tensors += [syn.weight, syn.bias, neuron.linear.weight, neuron.linear.bias]
        gif.append((float(neuron.decay), int(neuron.L), float(neuron.alpha), float(neuron.threshold)))
    tensors += [expert.readout.weight, expert.readout.bias]
    return [t.detach().numpy() for t in tensors], gif


def decided(router, experts, x, gain):
    """True when the fp64 rule leaves no top-k order and no spike open for this case."""
    from tests import moe_rule as RULE
    c = router.cell
    args = [t.detach().numpy() for t in (x, c.U.weight, c.U.bias, c.W.bias, router.gate_proj.weight,
                                         router.gate_proj.bias)]
    k = min(router.top_k, router.num_experts)
    for g in (None, gain.numpy()):
        r = RULE.route64(*args, c.dt, k, router.temperature, g)
        if not (r["order_margin"] > 0).all():
            return False
    for ex in experts:
        params, gif = expert_params(ex)
        if RULE.expert64(x.numpy(), params, gif)["open"].any():
            return False
    return True


def build_case(moe_mod, expert_mod, E):
    for seed in range(400, 464):
        torch.manual_seed(seed)
        router = moe_mod.LiquidMoERouter(in_dim=DM, hidden_dim=HR, num_experts=E, top_k=TOP_K).eval()
        experts = [expert_mod.SNNExpert(input_dim=DM, hidden_dim=HH, output_dim=DM).eval() for _ in range(E)]
        with torch.no_grad():
            router.gate_proj.weight.mul_(GATE_SCALE)
        x = torch.randn(N, DM)
        gain = torch.cat([torch.full((8,), 1e-3), torch.full((8,), 50.0), 0.25 + 3.0 * torch.rand(N - 16)])
        if decided(router, experts, x, gain):
            break
    else:
        raise SystemExit("no seed leaves every decision farther than its bound")
    assert decided(router, experts, x, gain)
    with torch.no_grad():
        plain, gained = router(x), router(x, gain)
        predict = torch.stack([ex.predict(x) for ex in experts])                        # [E, N, Dm]
        dense = torch.zeros(N, DM)
        for i in range(E):                                                               # ascending expert id
            w = (plain["weights"] * (plain["indices"] == i).float()).sum(dim=1, keepdim=True)
            dense += predict[i] * w
    used = sorted(set(plain["indices"].flatten().tolist()))
    assert E == 1 or len(used) > 1, "the routing does not vary between tokens"
    clone = lambda sd: {k: v.clone() for k, v in sd.items()}
    return {"seed": seed, "shape": dict(N=N, Dm=DM, Hr=HR, Hh=HH, E=E, top_k=TOP_K), "x": x, "attn_gain": gain,
            "router": clone(router.state_dict()), "experts": [clone(ex.state_dict()) for ex in experts],
            "route": {k: v.clone() for k, v in plain.items()}, "route_gain": {k: v.clone() for k, v in gained.items()},
            "predict": predict, "dense": dense}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    from oracle import _ref_loader
    if not _ref_loader.available():
        raise SystemExit("gen_golden_moe.py needs the reference checkout (oracle/_ref_loader.py); not found")
    moe_mod = _ref_loader.load("src.core.liquid_moe")
    expert_mod = _ref_loader.load("src.core.language_zone.snn_expert")
    zone_mod = _ref_loader.load("src.core.language_zone.moe_language_zone")
    keys = {"zone_args": ZONE_ARGS, "zone": _keys(zone_mod.MoELanguageZone(**ZONE_ARGS)),
            "router_args": dict(in_dim=DM, hidden_dim=HR, num_experts=4, top_k=TOP_K),
            "router": _keys(moe_mod.LiquidMoERouter(in_dim=DM, hidden_dim=HR, num_experts=4, top_k=TOP_K)),
            "expert_args": dict(input_dim=DM, hidden_dim=HH, output_dim=DM),
            "expert": _keys(expert_mod.SNNExpert(input_dim=DM, hidden_dim=HH, output_dim=DM))}
    path = os.path.join(a.dir, "moe_zone_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(keys['zone'])} zone keys")
    data = {"cases": {"e4": build_case(moe_mod, expert_mod, 4), "e1": build_case(moe_mod, expert_mod, 1)}}
    path = os.path.join(a.dir, "moe_zone.pt")
    torch.save(data, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, seeds { {k: c['seed'] for k, c in data['cases'].items()} }")
    return 0


if __name__ == "__main__":
    sys.exit(main())
