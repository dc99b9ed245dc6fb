"""Stand-ins for ``ops.moe_route``, ``ops.moe_expert_table``, ``ops.moe_experts`` and ``ops.moe_forward`` on the CPU --
TEST INFRASTRUCTURE ONLY.

The fp32 restatement of ``tests/moe_rule.py`` behind the ops' entry points: for plumbing tests of the modules, not for
bits.  Each runs the op's own host checks first, so a call the real op would refuse on the host is refused here too.
``install(monkeypatch)`` swaps them into ``aura_snn_rag_amd.ops`` and counts the calls."""
import numpy as np
import torch

from tests import moe_rule as RULE

CALLS = {"moe_route": 0, "moe_expert_table": 0, "moe_experts": 0}


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def moe_route(x, U, bU, bW, gate_w, gate_b, *, dt, k, temperature=1.0, attn_gain=None):
    from aura_snn_rag_amd import ops
    N, Dm, Hr, E, k = ops._moe_route_args(x, U, bU, bW, gate_w, gate_b, dt, k, temperature, attn_gain)
    CALLS["moe_route"] += 1
    r = RULE.route32(_np(x), _np(U), _np(bU), _np(bW), _np(gate_w), _np(gate_b), dt, k, temperature, _np(attn_gain))
    return ops.MoeRouting(torch.from_numpy(r["indices"].astype(np.int32)), torch.from_numpy(r["weights"]),
                          torch.from_numpy(r["probs"]), None, E, k)


def moe_expert_table(experts, gif):
    from aura_snn_rag_amd import ops
    E, layers, Dm, Hh = ops._moe_expert_params(experts, gif)
    CALLS["moe_expert_table"] += 1
    return ops.MoeExpertTable(None, [list(g) for g in gif], E, layers, Dm, Hh, [list(ts) for ts in experts])


def moe_experts(x, routing, table, *, out=None, return_trace=False):
    from aura_snn_rag_amd import ops
    N, Dm, P = ops._moe_experts_args(x, routing, table, out, return_trace)
    CALLS["moe_experts"] += 1
    k = routing.k
    xs, idx = _np(x), routing.indices.numpy()
    y = np.zeros((N, k, Dm), dtype=np.float32)
    trace = np.zeros((N, k, table.layers, table.Hh), dtype=np.float32)
    for e in range(table.E):
        rows, slots = np.nonzero(idx == e)
        if rows.size == 0:
            continue
        ye, tr = RULE.expert32(xs[rows], [_np(t) for t in table.held[e]], table.gif[e])
        y[rows, slots] = ye
        for l, s in enumerate(tr):
            trace[rows, slots, l] = s
    res = torch.from_numpy(RULE.combine32(y, routing.weights.numpy(), idx))
    if out is not None:
        res = out.copy_(res)
    return res, torch.from_numpy(y), torch.from_numpy(trace) if return_trace else None


def moe_forward(x, U, bU, bW, gate_w, gate_b, table, *, dt, k, temperature=1.0, attn_gain=None, out=None,
                return_trace=False):
    routing = moe_route(x, U, bU, bW, gate_w, gate_b, dt=dt, k=k, temperature=temperature, attn_gain=attn_gain)
    res, y, trace = moe_experts(x, routing, table, out=out, return_trace=return_trace)
    return res, routing, y, trace


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    for name in CALLS:
        CALLS[name] = 0
    for fn in (moe_route, moe_expert_table, moe_experts, moe_forward):
        monkeypatch.setattr(ops, fn.__name__, fn)
    return ops
