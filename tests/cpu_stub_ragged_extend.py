"""Stand-in for ``ops.attn_decode_extend(.., counts=)`` in torch fp32 on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Decode attention: extend with per-row counts") from torch ops with torch's own sums
and a plain softmax: for plumbing tests of the modules, not for bits.  It runs the op's own host checks first, so a
call the real op would refuse on the host is refused here too, and it never reads a row ``j >= counts[b]`` of ``q``,
``k_new``, ``v_new``, ``x`` or ``prosody``.  Without ``counts`` it is ``tests/cpu_stub_extend_attention.py``'s stub.
``install(monkeypatch)`` swaps it into ``aura_snn_rag_amd.ops`` (after that stub, which keeps counting the calls without
counts) and records the counts of every ragged call."""
import math

import torch

from tests import cpu_stub_extend_attention as EXTEND

CALLS = {"ragged": 0}
COUNTS = []                                                             # the counts of every ragged call, in order


def attn_decode_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache, workspace,
                       n_chunks=None, advance=True, return_scale=False, counts=None):
    if counts is None:
        return EXTEND.attn_decode_extend(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths, k_cache, v_cache,
                                         workspace, n_chunks=n_chunks, advance=advance, return_scale=return_scale)
    from aura_snn_rag_amd import ops
    B, m, H, dh, cap, n_chunks = ops._attn_decode_extend_shapes(q, k_new, v_new, x, prosody, Wp, bp, wm, bm, lengths,
                                                                k_cache, v_cache, workspace, n_chunks)
    ops._attn_decode_extend_counts(counts, lengths)
    CALLS["ragged"] += 1
    COUNTS.append(counts.tolist())
    ctx = torch.zeros(B, m, H, dh)
    scale = torch.zeros(B, m, H)
    lim = min(cap, ops.DECODE_CHUNK * n_chunks)
    for b in range(B):
        L, mb = int(lengths[b]), int(counts[b])
        if L < 0 or mb < 0 or mb > m or L + mb > lim:
            continue
        s = torch.ones(mb, H)
        if prosody is not None:
            p = prosody[b, :mb]
            s = (1.0 + torch.sigmoid(p @ Wp.detach().T + bp.detach())) * (1.0 + 0.2 * torch.tanh(p[..., 0:1])) \
                * (1.0 + 0.05 * torch.tanh(p[..., 1:2]))
        if wm is not None:
            s = s * (1.0 + 0.5 * torch.sigmoid(x[b, :mb] @ wm.detach().reshape(-1) + bm.detach().reshape(-1)[0]))[..., None]
        k_cache[b, :, L:L + mb] = k_new[b, :mb].detach().view(mb, H, dh).transpose(0, 1)
        v_cache[b, :, L:L + mb] = v_new[b, :mb].detach().view(mb, H, dh).transpose(0, 1)
        for j in range(mb):
            qs = q[b, j].detach().view(H, dh) * s[j][:, None]
            z = torch.einsum("hd,htd->ht", qs, k_cache[b, :, :L + j + 1]) * (1.0 / math.sqrt(dh))
            ctx[b, j] = torch.einsum("ht,htd->hd", torch.softmax(z, dim=-1), v_cache[b, :, :L + j + 1])
        scale[b, :mb] = s
        if advance:
            lengths[b] += mb
    ctx = ctx.reshape(B, m, H * dh)
    return (ctx, scale) if return_scale else ctx


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(ragged=0)
    COUNTS.clear()
    monkeypatch.setattr(ops, "attn_decode_extend", attn_decode_extend)
    return ops
