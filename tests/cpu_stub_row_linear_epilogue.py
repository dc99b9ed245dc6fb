"""Stand-ins for ``ops.row_linear_gate`` and ``ops.row_linear_gif`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rules of ``include/aura_hip.h`` ("Row linear: gate epilogue", "Row linear: GIF epilogue") from torch ops with torch's
own sums and the oracle's GIF loop: the stubs are for plumbing tests of the modules, not for bits.  Each runs the op's own
host checks first, so a call the real op would refuse on the host is refused here too.  ``install(monkeypatch)`` swaps
them into ``aura_snn_rag_amd.ops`` and counts the calls."""
import torch
import torch.nn.functional as F

CALLS = {"row_linear_gate": 0, "row_linear_gif": 0}
LAST = {}


def row_linear_gate(x, weight, bias, u, c, residual, *, out=None):
    from aura_snn_rag_amd import ops
    R, K, N, ldw = ops._row_linear_gate_args(x, weight, bias, u, c, residual, out)
    CALLS["row_linear_gate"] += 1
    LAST.update(R=R, K=K, N=N, ldw=ldw, bias=bias is not None)
    with torch.no_grad():
        y = residual + torch.sigmoid(F.linear(x, weight, bias) + u) * c
    return y if out is None else out.copy_(y)


def row_linear_gif(x, weight, bias=None, *, T, decay, L, alpha, threshold, time_major=False, mix=None, out=None):
    from aura_snn_rag_amd import ops
    from oracle import aura_oracle as O
    R, K, N, out_shape, (res, m, gate) = ops._row_linear_gif_args(x, weight, bias, T, decay, L, alpha, threshold,
                                                                    time_major, mix, out)
    CALLS["row_linear_gif"] += 1
    LAST.update(R=R, K=K, N=N, T=T, time_major=bool(time_major), mix=mix is not None)
    with torch.no_grad():
        c = F.linear(x, weight, bias)
        h = c.view(R // T, T, N) if time_major else c[:, None, :].expand(R, T, N)
        v, theta = O.gif_initial_state(h.shape[0], N, threshold)
        y = O.gif_run(h, v, theta, decay, L, alpha, threshold)[0]
        if time_major:
            y = y.mean(dim=1)
            if mix is not None:
                g = torch.sigmoid(gate.detach())
                y = res + ((1 - g) * m + g * y)
    return y if out is None else out.copy_(y)


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(row_linear_gate=0, row_linear_gif=0)
    LAST.clear()
    monkeypatch.setattr(ops, "row_linear_gate", row_linear_gate)
    monkeypatch.setattr(ops, "row_linear_gif", row_linear_gif)
    return ops
