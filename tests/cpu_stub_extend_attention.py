"""Stand-in for ``ops.attn_decode_extend`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Decode attention: extend") from torch ops with torch's own sums and a plain
softmax: the stub is for plumbing tests of the modules, not for bits.  It runs the op's own
``_attn_decode_extend_shapes`` first, so a call the real op would refuse on the host is refused here too.
``install(monkeypatch)`` swaps it into ``aura_snn_rag_amd.ops`` and counts the calls."""
import math

import torch

CALLS = {"extend": 0}
LAST = {}


def attn_decode_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace,
                       n_chunks=None, advance=True, return_scale=False):
    from aura_snn_rag_amd import ops
    B, m, H, dh, cap, n_chunks = ops._attn_decode_extend_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths,
                                                                k_cache, v_cache, workspace, n_chunks)
    CALLS["extend"] += 1
    LAST.update(shapes=(B, m, H, dh, cap, n_chunks), prosody=prosody is not None, memory=wm is not None)
    s = torch.ones(B, m, H)
    if prosody is not None:
        s = (1.0 + torch.sigmoid(prosody @ Wp.detach().T + bp.detach())) * (1.0 + 0.2 * torch.tanh(prosody[..., 0:1])) \
            * (1.0 + 0.05 * torch.tanh(prosody[..., 1:2]))
    if wm is not None:
        s = s * (1.0 + 0.5 * torch.sigmoid(x @ wm.detach().reshape(-1) + bm.detach().reshape(-1)[0]))[..., None]
    ctx = torch.zeros(B, m, H, dh)
    scale = torch.zeros(B, m, H)
    lim = min(cap, ops.DECODE_CHUNK * n_chunks)
    for b in range(B):
        L = int(lengths[b])
        if L < 0 or L + m > lim:
            continue
        k_cache[b, :, L:L + m] = k_new[b].detach().view(m, H, dh).transpose(0, 1)
        v_cache[b, :, L:L + m] = v_new[b].detach().view(m, H, dh).transpose(0, 1)
        for j in range(m):
            qs = q[b, j].detach().view(H, dh) * s[b, j][:, None]
            z = torch.einsum("hd,htd->ht", qs, k_cache[b, :, :L + j + 1]) * (1.0 / math.sqrt(dh))
            ctx[b, j] = torch.einsum("ht,htd->hd", torch.softmax(z, dim=-1), v_cache[b, :, :L + j + 1])
        scale[b] = s[b]
        if advance:
            lengths[b] += m
    ctx = ctx.reshape(B, m, H * dh)
    return (ctx, scale) if return_scale else ctx


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(extend=0)
    LAST.clear()
    monkeypatch.setattr(ops, "attn_decode_extend", attn_decode_extend)
    return ops
