"""Stand-in for ``ops.attn_decode_step`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Decode attention") from torch ops with torch's own sums and a plain softmax: the
stub is for plumbing tests of the modules, not for bits.  It runs the op's own ``_attn_decode_shapes`` first, so a call
the real op would refuse on the host is refused here too.  ``install(monkeypatch)`` swaps it into
``aura_snn_rag_amd.ops`` and counts the calls."""
import math

import torch

CALLS = {"step": 0}
LAST = {}


def attn_decode_step(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace, n_chunks=None,
                     advance=True, return_scale=False):
    from aura_snn_rag_amd import ops
    B, H, dh, cap, n_chunks = ops._attn_decode_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache,
                                                       v_cache, workspace, n_chunks)
    CALLS["step"] += 1
    LAST.update(shapes=(B, H, dh, cap, n_chunks), prosody=prosody is not None, memory=wm is not None)
    s = torch.ones(B, H)
    if prosody is not None:
        s = (1.0 + torch.sigmoid(prosody @ Wp.detach().T + bp.detach())) * (1.0 + 0.2 * torch.tanh(prosody[:, 0:1])) \
            * (1.0 + 0.05 * torch.tanh(prosody[:, 1:2]))
    if wm is not None:
        s = s * (1.0 + 0.5 * torch.sigmoid(x @ wm.detach().reshape(-1) + bm.detach().reshape(-1)[0]))[:, None]
    ctx = torch.zeros(B, H, dh)
    scale = torch.zeros(B, H)
    lim = min(cap, ops.DECODE_CHUNK * n_chunks)
    for b in range(B):
        L = int(lengths[b])
        if L < 0 or L >= lim:
            continue
        k_cache[b, :, L] = k_new[b].detach().view(H, dh)
        v_cache[b, :, L] = v_new[b].detach().view(H, dh)
        qs = q[b].detach().view(H, dh) * s[b][:, None]
        z = torch.einsum("hd,htd->ht", qs, k_cache[b, :, :L + 1]) * (1.0 / math.sqrt(dh))
        ctx[b] = torch.einsum("ht,htd->hd", torch.softmax(z, dim=-1), v_cache[b, :, :L + 1])
        scale[b] = s[b]
        if advance:
            lengths[b] += 1
    ctx = ctx.reshape(B, H * dh)
    return (ctx, scale) if return_scale else ctx


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(step=0)
    LAST.clear()
    monkeypatch.setattr(ops, "attn_decode_step", attn_decode_step)
    return ops
