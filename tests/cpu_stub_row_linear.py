"""Stand-in for ``ops.row_linear`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Row linear") from torch ops with torch's own sums: the stub is for plumbing tests
of the modules, not for bits.  It runs the op's own ``_row_linear_args`` first, so a call the real op would refuse on
the host is refused here too.  ``install(monkeypatch)`` swaps it into ``aura_snn_rag_amd.ops`` and counts the calls."""
import torch
import torch.nn.functional as F

CALLS = {"row_linear": 0}
LAST = {}


def row_linear(x, weights, biases=None, *, norm=None, eps=1e-5, activation=None, residual=None, return_normed=False,
               out=None):
    from aura_snn_rag_amd import ops
    R, K, W, b, outs, gamma, beta, single = ops._row_linear_args(x, weights, biases, norm, eps, activation, residual,
                                                                  return_normed, out)
    CALLS["row_linear"] += 1
    LAST.update(R=R, K=K, N=tuple(w.shape[0] for w in W if w is not None), norm=norm is not None,
                activation=activation, residual=residual is not None, return_normed=bool(return_normed))
    with torch.no_grad():
        xh = F.layer_norm(x, (K,), gamma, beta, float(eps)) if norm is not None else x
        ys = []
        for w, bias, o in zip(W, b, outs):
            if w is None:
                continue
            y = F.linear(xh, w, bias)
            if activation == "gelu":
                y = F.gelu(y)
            if residual is not None:
                y = y + residual
            ys.append(y if o is None else o.copy_(y))
    y = ys[0] if single else tuple(ys)
    return (y, xh.clone()) if return_normed else y


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(row_linear=0)
    LAST.clear()
    monkeypatch.setattr(ops, "row_linear", row_linear)
    return ops
