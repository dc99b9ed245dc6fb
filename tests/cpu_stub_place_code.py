"""Stand-ins for ``ops.place_code`` / ``ops.place_code_backward`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Place code") with the winners of ``tests/place_code_rule.py`` and fp32 arithmetic
in the rule's order (a sequential ``fmaf``-free chain is not reproduced: the stub is for plumbing tests, not for bits).
``install(monkeypatch)`` swaps them into ``aura_snn_rag_amd.ops`` and counts the calls."""
import numpy as np
import torch

from tests import place_code_rule as R

CALLS = {"forward": 0, "backward": 0}
LAST = {}


def place_code(z, e, w2t, b2, k, dense=True):
    from aura_snn_rag_amd import ops
    N, P, D, k = ops._place_shapes(z, e, w2t, b2, k)
    CALLS["forward"] += 1
    LAST.update(w2t=w2t, dense=dense, shapes=(N, P, D, k))
    idx = torch.from_numpy(R.winners(z.detach().numpy(), k))
    act = torch.sigmoid(torch.gather(z.detach(), 1, idx.long()))
    code = torch.zeros(N, P).scatter_(1, idx.long(), act)
    out = e.detach() + 0.1 * (code @ w2t.detach() + b2.detach())
    return out, idx, act, (code if dense else None)


def place_code_backward(g_out, g_dense, idx, act, w2t):
    from aura_snn_rag_amd import ops
    N, P, D, k = ops._place_backward_shapes(g_out, g_dense, idx, act, w2t)
    CALLS["backward"] += 1
    g_act = 0.1 * torch.einsum("nd,nkd->nk", g_out, w2t[idx.long()])
    if g_dense is not None:
        g_act = g_act + torch.gather(g_dense, 1, idx.long())
    return torch.zeros(N, P).scatter_(1, idx.long(), g_act * act * (1.0 - act))


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(forward=0, backward=0)
    LAST.clear()
    monkeypatch.setattr(ops, "place_code", place_code)
    monkeypatch.setattr(ops, "place_code_backward", place_code_backward)
    return ops
