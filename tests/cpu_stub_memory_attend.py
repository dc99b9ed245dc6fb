"""A stand-in for ``ops.memory_attend`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Memory attend") from torch ops with torch's own sums: the stub is for plumbing tests
of the modules, not for bits.  It runs the op's own host checks first, so a call the real op would refuse on the host is
refused here too.  ``install(monkeypatch)`` swaps it into ``aura_snn_rag_amd.ops`` and counts the calls."""
import torch
import torch.nn.functional as F

CALLS = {"memory_attend": 0}
LAST = {}


def memory_attend(x, norm, G, s0, U, bias=None, *, eps=1e-5, out=None):
    from aura_snn_rag_amd import ops
    R, D, H, M, gamma, beta = ops._memory_attend_args(x, norm, G, s0, U, bias, eps, out)
    CALLS["memory_attend"] += 1
    LAST.update(R=R, D=D, H=H, M=M, bias=bias is not None, eps=eps)
    with torch.no_grad():
        xh = F.layer_norm(x, (D,), gamma, beta, eps)
        p = torch.softmax(torch.einsum("rhmd,rd->rhm", G, xh) + s0, dim=-1)
        acc = torch.einsum("rhm,rhmd->rd", p, U)
        y = x + (acc if bias is None else bias + acc)
    return y if out is None else out.copy_(y)


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(memory_attend=0)
    LAST.clear()
    monkeypatch.setattr(ops, "memory_attend", memory_attend)
    return ops
