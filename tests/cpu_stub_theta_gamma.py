"""Stand-ins for ``ops.theta_gamma_table`` / ``theta_gamma_norm`` / ``theta_gamma_norm_backward`` in torch fp32 on the
CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Theta-gamma") in torch ops, in the rule's order of operations but with torch's own
sums: the stub is for plumbing tests, not for bits.  ``install(monkeypatch)`` swaps them into ``aura_snn_rag_amd.ops``
and counts the calls."""
import math

import torch

CALLS = {"table": 0, "derivatives": 0, "forward": 0, "backward": 0}
LAST = {}


def theta_gamma_table(theta_off, gamma_off, amp, max_seq_len, ratio, positions=None, start=0, rows=None,
                      derivatives=False, pe=True):
    from aura_snn_rag_amd import ops
    R, D = ops._theta_table_shapes(theta_off, gamma_off, amp, max_seq_len, positions, start, rows)
    CALLS["derivatives" if derivatives else "table"] += 1
    p = positions if positions is not None else torch.arange(start, start + R).to(torch.float32)
    phi = ((p / float(max(max_seq_len - 1, 1))) * torch.tensor(2.0 * math.pi, dtype=torch.float32))[:, None]
    a = phi + theta_off.detach()
    g = phi * torch.tensor(ratio, dtype=torch.float32) + gamma_off.detach()
    A = (torch.cos(a) + 1.0) * 0.5
    q = torch.sin(a) + 0.5 * (A * torch.sin(g))
    m = amp.detach()
    out = q * m if pe else None
    LAST.update(table=out, rows=R)
    if not derivatives:
        return out
    return out, m * (torch.cos(a) - (0.25 * torch.sin(a)) * torch.sin(g)), m * ((0.5 * A) * torch.cos(g)), q


def _rows(N, S, R):
    return torch.arange(N) if R == N else torch.arange(N) % S


def theta_gamma_norm(x, table, w, b, seq_len, eps=1e-5):
    from aura_snn_rag_amd import ops
    N, S, R, D = ops._theta_norm_shapes("theta_gamma_norm", x, table, w, b, seq_len, eps)
    CALLS["forward"] += 1
    LAST.update(shapes=(N, S, R, D), used_table=table)
    h = x.detach() + table[_rows(N, S, R)]
    mean = h.mean(1)
    rstd = 1.0 / torch.sqrt(((h - mean[:, None]) ** 2).mean(1) + eps)
    return ((h - mean[:, None]) * rstd[:, None]) * w.detach() + b.detach(), mean, rstd


def theta_gamma_norm_backward(g_y, x, table, derivatives, mean, rstd, w, seq_len, column_sums=True):
    from aura_snn_rag_amd import ops
    N, S, R, D = ops._theta_backward_shapes(g_y, x, table, derivatives, mean, rstd, w, seq_len)
    CALLS["backward"] += 1
    LAST.update(derivatives=derivatives is not None, column_sums=column_sums)
    rows = _rows(N, S, R)
    n = ((x.detach() + table[rows]) - mean[:, None]) * rstd[:, None]
    wg = w.detach() * g_y
    g_h = rstd[:, None] * ((wg - wg.mean(1, keepdim=True)) - n * (wg * n).mean(1, keepdim=True))
    if not column_sums:
        return g_h, None
    grads = [(g_y * n).sum(0), g_y.sum(0)]
    if derivatives is not None:
        grads += [(g_h * d[rows]).sum(0) for d in derivatives]
    return g_h, torch.stack(grads)


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(table=0, derivatives=0, forward=0, backward=0)
    LAST.clear()
    monkeypatch.setattr(ops, "theta_gamma_table", theta_gamma_table)
    monkeypatch.setattr(ops, "theta_gamma_norm", theta_gamma_norm)
    monkeypatch.setattr(ops, "theta_gamma_norm_backward", theta_gamma_norm_backward)
    return ops
