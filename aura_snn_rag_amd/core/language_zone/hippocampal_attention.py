"""HippocampalProsodyAttention: the reference's prosody- and memory-gated causal self-attention, with a K/V cache and a
fused one-token decoding step.

API-compatible with the reference's ``src/core/language_zone/hippocampal_attention.py``: the constructor, the twelve
``state_dict`` keys (``q_proj`` / ``k_proj`` / ``v_proj`` / ``o_proj`` / ``prosody_gate`` / ``memory_gate``, weight and
bias each) and ``forward(hidden, prosody=None, use_memory=True) -> (output, None)``.  ``forward`` is the reference's
arithmetic from torch ops with the library's causal attention (the projections and the S x S attention
are library GEMMs), gradients included.

New on this module: ``new_cache`` / ``prefill`` / ``step`` / ``extend``.  The causal forward at position t is a function of the rows
0 .. t alone, so ``prefill`` over a prompt followed by one ``step`` per new token computes what ``forward`` over the
whole sequence computes, without recomputing the context: a step is the three projections of the new row (library
calls), ``ops.attn_decode_step`` (``csrc/aura_decode.hip``, the rule: ``include/aura_hip.h``, "Decode attention") and
``o_proj``.  The step is fp32, runs under ``no_grad`` and has no CPU fallback: CPU tensors raise ``AuraDeviceError``.
``step(fused=True)`` replaces the library calls by ``ops.row_linear`` (``csrc/aura_rowlin.hip``, "Row linear"): the three
projections in one launch, with the layer's LayerNorm in front, and ``o_proj`` with the residual behind.
``extend`` appends ``m`` tokens to a cache that already holds a context: the three projections of the ``B m`` rows,
``ops.attn_decode_extend`` (one pass over K and V for all ``m`` queries; "Decode attention: extend") and ``o_proj``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops


def row_counts(who: str, name: str, counts, B: int, lo: int, hi: int, device, dtype=torch.int32):
    """Per-row counts [B] for a ragged call -> ``(tensor of dtype on device, host values or None)``.  A host sequence
    (list, tuple, CPU tensor) is checked against ``lo <= c <= hi`` here and its values are returned; a tensor that is
    already on another device is only shaped and typed: its values are never read on the host."""
    if isinstance(counts, torch.Tensor):
        if counts.dtype not in (torch.int32, torch.int64) or tuple(counts.shape) != (B,):
            raise ValueError(f"{who}: {name} is [B] = ({B},) integers, got {counts.dtype} {tuple(counts.shape)}")
        known = counts.tolist() if counts.device.type == "cpu" else None
    else:
        known = list(counts)
        if len(known) != B or any(isinstance(c, bool) or not isinstance(c, int) for c in known):
            raise ValueError(f"{who}: {name} is [B] = ({B},) integers, got {counts!r}")
        counts = torch.tensor(known, dtype=dtype)
    if known is not None and any(not lo <= c <= hi for c in known):
        raise ValueError(f"{who}: {name} {known} must lie in [{lo}, {hi}]")
    return counts.to(device=device, dtype=dtype).contiguous(), known


class AttentionCache:
    """The K/V cache of one attention module: ``k`` and ``v`` [B, H, capacity, dh] fp32, ``lengths`` int32 [B] on the
    device (the next position of each row; -1 retires a row: its steps return zeros and leave its cache alone), the
    partials ``workspace`` of the step, allocated once, and ``max_length``: a host-side upper bound of the lengths
    (prompt length plus steps taken), so that a step past ``capacity`` raises without reading the device.
    ``extend_workspace`` is the partials workspace of ``extend``, allocated at first use and grown when a later call
    feeds more tokens at once."""
    __slots__ = ("k", "v", "lengths", "workspace", "n_chunks", "capacity", "max_length", "extend_workspace")

    def __init__(self, batch: int, heads: int, capacity: int, head_dim: int, device=None):
        for n, v in (("batch", batch), ("capacity", capacity)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"AttentionCache: {n} must be an int, got {type(v)}")
        if batch < 0:
            raise ValueError(f"AttentionCache: batch={batch} must not be negative")
        if not 1 <= capacity <= ops.DECODE_MAX_CAP:
            raise ValueError(f"AttentionCache: capacity={capacity} must be in [1, {ops.DECODE_MAX_CAP}]")
        self.capacity = capacity
        self.n_chunks = ops.attn_decode_chunks(capacity)
        self.k = torch.zeros(batch, heads, capacity, head_dim, dtype=torch.float32, device=device)
        self.v = torch.zeros_like(self.k)
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)
        self.workspace = torch.empty(ops.attn_decode_workspace_floats(batch, heads, head_dim, self.n_chunks),
                                     dtype=torch.float32, device=device)
        self.max_length = 0
        self.extend_workspace = None

    @property
    def batch(self) -> int:
        return self.k.shape[0]

    def extend_workspace_for(self, m: int) -> torch.Tensor:
        """The workspace of an extend of ``m`` tokens: kept between calls, re-allocated only to grow."""
        B, H, _, dh = self.k.shape
        need = ops.attn_decode_extend_workspace_floats(B, m, H, dh, self.n_chunks)
        if self.extend_workspace is None or self.extend_workspace.numel() < need:
            self.extend_workspace = torch.empty(need, dtype=torch.float32, device=self.k.device)
        return self.extend_workspace

    def retire(self, rows) -> None:
        """Marks rows as finished (``lengths = -1``): their steps return zeros and write nothing."""
        self.lengths[torch.as_tensor(rows, dtype=torch.long, device=self.lengths.device)] = -1


class HippocampalProsodyAttention(nn.Module):
    def __init__(self, config, hippocampus):
        super().__init__()
        self.config = config
        self.hippocampus = hippocampus
        self.hidden_size = config.embedding_dim
        self.num_heads = config.num_heads
        self.head_dim = self.hidden_size // self.num_heads
        self.q_proj = nn.Linear(self.hidden_size, self.hidden_size)
        self.k_proj = nn.Linear(self.hidden_size, self.hidden_size)
        self.v_proj = nn.Linear(self.hidden_size, self.hidden_size)
        self.o_proj = nn.Linear(self.hidden_size, self.hidden_size)
        self.prosody_gate = nn.Linear(4, self.num_heads)
        self.memory_gate = nn.Linear(self.hidden_size, 1)
        self.dropout = config.dropout

    # ------------------------------------------------------------------------------------------------ full sequences
    def _heads(self, t: torch.Tensor) -> torch.Tensor:
        B, S, _ = t.shape
        return t.view(B, S, self.num_heads, self.head_dim).transpose(1, 2)

    def _memory_on(self, use_memory: bool) -> bool:
        return bool(use_memory) and self.hippocampus is not None

    def _attend(self, hidden, prosody, use_memory):
        """The reference's forward up to the output; also returns the keys and values [B, H, S, dh]."""
        B, S, _ = hidden.shape
        query = self._heads(self.q_proj(hidden))
        key = self._heads(self.k_proj(hidden))
        value = self._heads(self.v_proj(hidden))
        if prosody is not None:
            gain = torch.sigmoid(self.prosody_gate(prosody)).transpose(1, 2).unsqueeze(-1)
            arousal_boost = 1.0 + 0.2 * torch.tanh(prosody[..., 0:1])
            valence_gain = 1.0 + 0.05 * torch.tanh(prosody[..., 1:2])
            query = query * (1.0 + gain) * arousal_boost.unsqueeze(1) * valence_gain.unsqueeze(1)
        if self._memory_on(use_memory):
            memory_weight = torch.sigmoid(self.memory_gate(hidden))
            query = query * (1.0 + memory_weight.transpose(1, 2).unsqueeze(-1) * 0.5)
        context = F.scaled_dot_product_attention(query, key, value,
                                                 dropout_p=self.dropout if self.training else 0.0, is_causal=True)
        context = context.transpose(1, 2).contiguous().view(B, S, self.hidden_size)
        return self.o_proj(context), key, value

    def forward(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None,
                use_memory: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        return self._attend(hidden_states, prosody, use_memory)[0], None

    # ------------------------------------------------------------------------------------------------ cached decoding
    def new_cache(self, batch: int, capacity: int) -> AttentionCache:
        """An empty cache for ``batch`` sequences of at most ``capacity`` positions, on the module's device."""
        if self.head_dim * self.num_heads != self.hidden_size or self.head_dim % 4 or not \
                4 <= self.head_dim <= ops.DECODE_MAX_HEAD or self.hidden_size > ops.DECODE_MAX_D:
            raise ValueError(f"HippocampalProsodyAttention: the decode step needs embedding_dim = num_heads * head_dim "
                             f"<= {ops.DECODE_MAX_D} with head_dim a multiple of 4 in [4, {ops.DECODE_MAX_HEAD}]; got "
                             f"{self.hidden_size} = {self.num_heads} * {self.head_dim}")
        return AttentionCache(batch, self.num_heads, capacity, self.head_dim, device=self.q_proj.weight.device)

    def _check_cache(self, who: str, cache, B: int) -> None:
        if not isinstance(cache, AttentionCache):
            raise TypeError(f"{who}: cache must be an AttentionCache (new_cache), got {type(cache)}")
        if tuple(cache.k.shape) != (B, self.num_heads, cache.capacity, self.head_dim):
            raise ValueError(f"{who}: the cache is {tuple(cache.k.shape)}, this call needs "
                             f"({B}, {self.num_heads}, capacity, {self.head_dim})")

    def prefill(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
                cache: Optional[AttentionCache] = None, lengths=None):
        """``forward`` over a prompt [B, S, D] that also leaves K and V of positions < S in ``cache`` and sets its
        lengths: S, or ``lengths`` [B] (ints, at most S) for right-padded rows, whose valid outputs causality keeps
        unaffected and whose tail the steps overwrite.  Returns what ``forward`` returns."""
        who = "HippocampalProsodyAttention.prefill"
        if hidden_states.dim() != 3 or hidden_states.shape[-1] != self.hidden_size:
            raise ValueError(f"{who}: hidden is [B, S, {self.hidden_size}], got {tuple(hidden_states.shape)}")
        B, S, _ = hidden_states.shape
        self._check_cache(who, cache, B)
        if hidden_states.dtype != torch.float32:
            raise TypeError(f"{who}: hidden is {hidden_states.dtype}; the cache is fp32")
        if not 1 <= S <= cache.capacity:
            raise ValueError(f"{who}: a prompt of {S} positions does not fit a cache of capacity {cache.capacity}")
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            if lengths.dtype not in (torch.int32, torch.int64) or tuple(lengths.shape) != (B,):
                raise ValueError(f"{who}: lengths is [B] = ({B},) integers, got {lengths.dtype} {tuple(lengths.shape)}")
            if not lengths.is_cuda and int(lengths.max()) > S:
                raise ValueError(f"{who}: lengths {lengths.tolist()} exceed the prompt's {S} positions")
        output, key, value = self._attend(hidden_states, prosody, use_memory)
        with torch.no_grad():
            cache.k[:, :, :S].copy_(key.detach())
            cache.v[:, :, :S].copy_(value.detach())
            if lengths is None:
                cache.lengths.fill_(S)
            else:
                cache.lengths.copy_(lengths.to(cache.lengths.device).clamp(max=S))
            cache.max_length = S
        return output, None

    @torch.no_grad()
    def step(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
             cache: Optional[AttentionCache] = None, advance: bool = True, *, fused: bool = False,
             residual: Optional[torch.Tensor] = None, norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        """One new token: hidden [B, D] or [B, 1, D] (the normed row the layer feeds ``forward``), prosody [B, 4] or
        [B, 1, 4] or ``None``.  Appends the token's key and value at each row's length, attends over the cache and
        returns the attention output [B, D]; the lengths advance on the device unless ``advance=False`` (caches that
        share one lengths tensor: only the last of them advances it).  Raises when the cache may be full.

        ``fused=True`` (B <= 32) makes the step four launches: one ``ops.row_linear`` for the three projections, the
        two of ``ops.attn_decode_step`` and one ``ops.row_linear`` for ``o_proj``.  With ``norm`` (the layer's
        ``attention_norm``) hidden is the un-normalised row and the LayerNorm runs inside the first launch; with
        ``residual`` [B, D] the last launch adds it to the output.  Both need ``fused=True``."""
        who = "HippocampalProsodyAttention.step"
        if hidden_states.dim() == 3 and hidden_states.shape[1] == 1:
            hidden_states = hidden_states[:, 0]
        if hidden_states.dim() != 2 or hidden_states.shape[-1] != self.hidden_size:
            raise ValueError(f"{who}: hidden is [B, {self.hidden_size}] or [B, 1, {self.hidden_size}], got "
                             f"{tuple(hidden_states.shape)}")
        B = hidden_states.shape[0]
        self._check_cache(who, cache, B)
        if hidden_states.dtype != torch.float32:
            raise TypeError(f"{who}: hidden is {hidden_states.dtype}; the decode step runs in fp32 only")
        if prosody is not None:
            if prosody.dim() == 3 and prosody.shape[1] == 1:
                prosody = prosody[:, 0]
            if tuple(prosody.shape) != (B, 4):
                raise ValueError(f"{who}: prosody is [B, 4] or [B, 1, 4] with B={B}, got {tuple(prosody.shape)}")
            prosody = prosody.contiguous()
        if cache.max_length >= cache.capacity:
            raise RuntimeError(f"{who}: the cache is full ({cache.max_length} of {cache.capacity} positions); a sliding "
                               f"cache is not part of this module")
        x = hidden_states.contiguous()
        memory = self._memory_on(use_memory)
        if not fused and (residual is not None or norm is not None):
            raise ValueError(f"{who}: residual and norm are the fused step's arguments (fused=True)")
        if fused:
            if B > ops.ROW_LINEAR_MAX_ROWS:
                raise ValueError(f"{who}: the fused step takes at most {ops.ROW_LINEAR_MAX_ROWS} rows, got B={B}; "
                                 f"use fused=False")
            if norm is not None and not isinstance(norm, nn.LayerNorm):
                raise TypeError(f"{who}: norm must be the nn.LayerNorm in front of the attention, got {type(norm)}")
            if norm is not None and (norm.weight is None or norm.bias is None):
                raise ValueError(f"{who}: the fused prologue needs a LayerNorm with weight and bias")
            weights = (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight)
            biases = (self.q_proj.bias, self.k_proj.bias, self.v_proj.bias)
            if norm is not None:
                (q, k, v), x = ops.row_linear(x, weights, biases, norm=(norm.weight, norm.bias), eps=norm.eps,
                                              return_normed=True)
            else:
                q, k, v = ops.row_linear(x, weights, biases)
            ctx = ops.attn_decode_step(q, k, v, x if memory else None, prosody,
                                       self.prosody_gate.weight, self.prosody_gate.bias,
                                       self.memory_gate.weight if memory else None,
                                       self.memory_gate.bias if memory else None,
                                       cache.lengths, cache.k, cache.v, cache.workspace, n_chunks=cache.n_chunks,
                                       advance=bool(advance))
            cache.max_length += 1
            return ops.row_linear(ctx, self.o_proj.weight, self.o_proj.bias,
                                  residual=None if residual is None else residual.contiguous())
        ctx = ops.attn_decode_step(self.q_proj(x), self.k_proj(x), self.v_proj(x), x if memory else None, prosody,
                                   self.prosody_gate.weight, self.prosody_gate.bias,
                                   self.memory_gate.weight if memory else None,
                                   self.memory_gate.bias if memory else None,
                                   cache.lengths, cache.k, cache.v, cache.workspace, n_chunks=cache.n_chunks,
                                   advance=bool(advance))
        cache.max_length += 1
        return self.o_proj(ctx)

    @torch.no_grad()
    def extend(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
               cache: Optional[AttentionCache] = None, advance: bool = True, counts=None,
               count_bound: Optional[int] = None) -> torch.Tensor:
        """``m`` new tokens per row: hidden [B, m, D] (the normed rows), prosody [B, m, 4] or ``None``, ``1 <= m <=
        ops.DECODE_EXTEND_MAX``.  Appends their keys and values at each row's length, attends (token ``j`` over the
        cache and the new tokens up to itself) and returns the attention output [B, m, D]: what ``m`` calls of ``step``
        return, from one pass over the cache.  The lengths advance by ``m`` on the device unless ``advance=False``.
        Raises when the cache may not hold ``m`` more positions.

        ``counts`` [B] (ints in ``[0, m]``; a host sequence or a tensor): row ``b`` is right-padded and only its first
        ``counts[b]`` tokens are new; the padded places are read by nobody, append nothing and return ``o_proj``'s
        bias.  The lengths advance by ``counts[b]``.  The host-side bound ``max_length`` advances by the largest count
        where the host knows it (a host sequence, or ``count_bound``), by ``m`` otherwise; the same number is what the
        capacity check asks room for."""
        who = "HippocampalProsodyAttention.extend"
        if hidden_states.dim() != 3 or hidden_states.shape[-1] != self.hidden_size:
            raise ValueError(f"{who}: hidden is [B, m, {self.hidden_size}], got {tuple(hidden_states.shape)}")
        B, m, _ = hidden_states.shape
        if not 1 <= m <= ops.DECODE_EXTEND_MAX:
            raise ValueError(f"{who}: m={m} new tokens must be in [1, {ops.DECODE_EXTEND_MAX}]")
        self._check_cache(who, cache, B)
        if hidden_states.dtype != torch.float32:
            raise TypeError(f"{who}: hidden is {hidden_states.dtype}; the decode extend runs in fp32 only")
        if prosody is not None:
            if tuple(prosody.shape) != (B, m, 4):
                raise ValueError(f"{who}: prosody is [B, m, 4] = ({B}, {m}, 4), got {tuple(prosody.shape)}")
            prosody = prosody.contiguous()
        need = m
        if counts is not None:
            counts, known = row_counts(who, "counts", counts, B, 0, m, cache.lengths.device)
            if known is not None:
                need = max(known, default=0)
            if count_bound is not None:
                need = min(need, int(count_bound))
        elif count_bound is not None:
            raise ValueError(f"{who}: count_bound bounds counts; there are none")
        if cache.max_length + need > cache.capacity:
            raise RuntimeError(f"{who}: {need} more positions do not fit the cache ({cache.max_length} of "
                               f"{cache.capacity} may be held); a sliding cache is not part of this module")
        x = hidden_states.contiguous()
        memory = self._memory_on(use_memory)
        ragged = {} if counts is None else dict(counts=counts)          # without counts: the call as it was
        ctx = ops.attn_decode_extend(self.q_proj(x), self.k_proj(x), self.v_proj(x), x if memory else None, prosody,
                                     self.prosody_gate.weight, self.prosody_gate.bias,
                                     self.memory_gate.weight if memory else None,
                                     self.memory_gate.bias if memory else None,
                                     cache.lengths, cache.k, cache.v, cache.extend_workspace_for(m),
                                     n_chunks=cache.n_chunks, advance=bool(advance), **ragged)
        cache.max_length += need
        return self.o_proj(ctx)
