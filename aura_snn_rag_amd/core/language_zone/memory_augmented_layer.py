"""MemoryAugmentedLayer: self-attention, retrieval from the hippocampus and injection, then an MLP or a HybridFFN, with a
cached decoding step whose retrieved memories are pinned for the generation.

API-compatible with the reference's ``src/core/language_zone/memory_augmented_layer.py``: the constructor ``(config,
hippocampus, use_snn_ffn=False, memory_injection="cross_attention", num_retrieved=5)``, the submodule names and
``state_dict`` keys for the three injections and both FFN kinds, ``retrieve_memories`` / ``store_memory`` /
``inject_memories`` and ``forward(hidden_states, prosody=None, use_memory=True, store_memory=False)``.  Retrieval and
storage are the batched functions of ``memory_ops`` (one recall and one row gather per call instead of a Python loop
over the batch), with their extra keywords passed through.  The constructor prints nothing.

New on this module.  The reference retrieves from the mean over the whole context, in every layer and for every token,
which makes the layer non-causal: the function at earlier positions changes as the context grows, so nothing can be
cached.  Here a generation retrieves once per layer, from the prompt, and holds the result (``MemoryContext``).  With
the memories fixed the layer is causal, and ``prefill`` plus ``step`` computes what ``forward(.., memory=context)`` over
the whole sequence computes.  Re-retrieval during a generation is not part of this module.
  * ``retrieve_context(hidden_states)`` -> ``MemoryContext`` or ``None`` (no bank, or an empty one);
  * ``forward(.., memory=context)`` injects the given context as it is and retrieves nothing;
  * ``new_cache`` / ``prefill`` / ``step`` / ``extend``: ``prefill`` pins the context (retrieved from the prompt, or
    given) in the cache together with the constants of the generation, ``step`` is one token through the layer,
    ``extend`` several at once (``ops.attn_decode_extend``).  ``step(fused=True)`` replaces the strings of small torch
    launches by ``ops.row_linear``, for the ``gate`` injection ``ops.row_linear_gate`` and for the spiking FFN
    ``ops.row_linear_gif`` (``csrc/aura_rowlin.hip``); it raises where it does not apply and never falls back.
  * ``fold_memory(cache)`` -> ``FoldedMemory`` or ``None``: the pinned memories of a ``cross_attention`` layer folded
    through both projections of ``memory_attention``, once per generation; the fused step's injection is then one
    launch (``ops.memory_attend``, ``csrc/aura_memattend.hip``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from .hippocampal_attention import AttentionCache, HippocampalProsodyAttention
from .memory_ops import BatchedMemoryMixin, inject_concat, inject_cross_attention, inject_gate
from .snn_ffn import HybridFFN

INJECTIONS = ("cross_attention", "concat", "gate")


class MemoryContext(NamedTuple):
    """The memories one layer holds for a generation: ``features`` [B, k, D], ``scores`` [B, k] and, where the caller
    kept them, the bank ``rows`` int32 [B, k] they came from (-1: an empty slot)."""
    features: torch.Tensor
    scores: torch.Tensor
    rows: Optional[torch.Tensor] = None


class FoldedMemory(NamedTuple):
    """The pinned memories of a ``cross_attention`` layer folded through ``memory_attention``'s projections (the rule:
    ``include/aura_hip.h``, "Memory attend"): ``G`` [B, H, k, D] and ``s0`` [B, H, k], the keys met with the query
    projection and the softmax scale, and ``U`` [B, H, k, D], the values carried through ``out_proj``'s weight."""
    G: torch.Tensor
    s0: torch.Tensor
    U: torch.Tensor


class MemoryLayerCache:
    """What one ``MemoryAugmentedLayer`` carries through a generation: the ``attention`` cache, the pinned ``memory``
    (a ``MemoryContext`` or ``None``: nothing is injected) and the per-row constants the pinned memories make of the
    injection: ``c`` [B, D], the score-weighted context (``gate``: projected by ``memory_proj``), and for ``gate``
    ``u = W_g[:, D:] c + b_g`` [B, D], the half of the gate's pre-activation that does not depend on the token.
    ``fold`` (``cross_attention``): the ``FoldedMemory`` tables, built by ``fold_memory`` on demand, ``None`` until then.
    ``lengths``, ``capacity``, ``max_length`` and ``retire`` are the attention cache's."""
    __slots__ = ("attention", "memory", "c", "u", "fold")

    def __init__(self, attention: AttentionCache):
        self.attention = attention
        self.memory = None
        self.c = None
        self.u = None
        self.fold = None

    @property
    def lengths(self):
        return self.attention.lengths

    @lengths.setter
    def lengths(self, value):
        self.attention.lengths = value

    @property
    def capacity(self) -> int:
        return self.attention.capacity

    @property
    def max_length(self) -> int:
        return self.attention.max_length

    @property
    def batch(self) -> int:
        return self.attention.batch

    def retire(self, rows) -> None:
        self.attention.retire(rows)


class MemoryAugmentedLayer(BatchedMemoryMixin, nn.Module):
    def __init__(self, config, hippocampus, use_snn_ffn: bool = False, memory_injection: str = "cross_attention",
                 num_retrieved: int = 5):
        super().__init__()
        if memory_injection not in INJECTIONS:
            raise ValueError(f"MemoryAugmentedLayer: memory_injection must be one of {INJECTIONS}, got "
                             f"{memory_injection!r}")
        self.config = config
        self.hippocampus = hippocampus
        self.memory_injection = memory_injection
        self.num_retrieved = num_retrieved
        self.use_snn_ffn = use_snn_ffn
        D = config.embedding_dim
        self.attention_norm = nn.LayerNorm(D)
        self.attention = HippocampalProsodyAttention(config, hippocampus)
        if memory_injection == "cross_attention":
            self.memory_norm = nn.LayerNorm(D)
            self.memory_attention = nn.MultiheadAttention(embed_dim=D, num_heads=config.num_heads,
                                                          dropout=config.dropout, batch_first=True)
        elif memory_injection == "gate":
            self.memory_gate = nn.Sequential(nn.Linear(D * 2, D), nn.Sigmoid())
            self.memory_proj = nn.Linear(D, D)
        self.ffn_norm = nn.LayerNorm(D)
        if use_snn_ffn:
            self.ffn = HybridFFN(input_dim=D, hidden_dim=config.intermediate_size, snn_ratio=0.5,
                                 dropout=config.dropout)
        else:
            self.ffn = nn.Sequential(nn.Linear(D, config.intermediate_size), nn.GELU(),
                                     nn.Linear(config.intermediate_size, D), nn.Dropout(config.dropout))
        self.dropout = nn.Dropout(config.dropout)
        self.query_proj = nn.Linear(D, D)

    # ------------------------------------------------------------------------------------------------ memory
    def _bank_holds_memories(self) -> bool:
        return self.hippocampus is not None and self.hippocampus.memory_count > 0

    def inject_memories(self, hidden_states, memory_features, memory_scores):
        if self.memory_injection == "cross_attention":
            return inject_cross_attention(hidden_states, memory_features, self.memory_norm, self.memory_attention,
                                          self.dropout)
        if self.memory_injection == "concat":
            return inject_concat(hidden_states, memory_features, memory_scores)
        return inject_gate(hidden_states, memory_features, memory_scores, self.memory_proj, self.memory_gate)

    def retrieve_context(self, hidden_states: torch.Tensor, lengths=None, **retrieve_kw) -> Optional[MemoryContext]:
        """The memories ``forward`` would retrieve for ``hidden_states`` [B, S, D] (the states after the attention
        sublayer), as a ``MemoryContext`` to hold; ``None`` without a bank or with an empty one.  ``lengths`` [B]
        (a tensor, ``1 <= lengths[b] <= S``): the rows are right-padded and a row's query is the mean over its own
        ``lengths[b]`` positions (``memory_ops.masked_mean``), so that it pins what the row alone pins."""
        if not self._bank_holds_memories():
            return None
        if lengths is not None:
            retrieve_kw["lengths"] = lengths
        features, scores = self.retrieve_memories(hidden_states, k=self.num_retrieved, **retrieve_kw)
        return MemoryContext(features, scores, None)

    def _check_context(self, who: str, memory, B: int) -> MemoryContext:
        if not isinstance(memory, MemoryContext):
            raise TypeError(f"{who}: memory must be a MemoryContext (retrieve_context), got {type(memory)}")
        D = self.config.embedding_dim
        f, s = memory.features, memory.scores
        if f.dim() != 3 or f.shape[0] != B or f.shape[2] != D or tuple(s.shape) != (B, f.shape[1]):
            raise ValueError(f"{who}: memory is features [B, k, D] = ({B}, k, {D}) and scores [B, k], got "
                             f"{tuple(f.shape)} and {tuple(s.shape)}")
        return memory

    def _after_attention(self, hidden_states, use_memory, memory):
        """The injection and the feed-forward sublayer: everything behind the attention's residual."""
        if use_memory:
            if memory is not None:
                hidden_states = self.inject_memories(hidden_states, memory.features, memory.scores)
            elif self._bank_holds_memories():
                features, scores = self.retrieve_memories(hidden_states, k=self.num_retrieved)
                hidden_states = self.inject_memories(hidden_states, features, scores)
        return hidden_states + self.ffn(self.ffn_norm(hidden_states))

    # ------------------------------------------------------------------------------------------------ full sequences
    def forward(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
                store_memory: bool = False, *, memory: Optional[MemoryContext] = None) -> torch.Tensor:
        """The reference's forward.  ``memory`` (a ``MemoryContext``): with ``use_memory`` it is injected as it is and
        no retrieval runs, so that the layer is causal; ``None`` retrieves from the mean of ``hidden_states`` as the
        reference does."""
        if memory is not None:
            self._check_context("MemoryAugmentedLayer.forward", memory, hidden_states.shape[0])
        attn_output, _ = self.attention(self.attention_norm(hidden_states), prosody=prosody, use_memory=use_memory)
        hidden_states = self._after_attention(hidden_states + self.dropout(attn_output), use_memory, memory)
        if store_memory and self.training:
            self.store_memory(hidden_states)
        return hidden_states

    # ------------------------------------------------------------------------------------------------ cached decoding
    def new_cache(self, batch: int, capacity: int) -> MemoryLayerCache:
        return MemoryLayerCache(self.attention.new_cache(batch, capacity))

    def _check_cache(self, who: str, cache) -> None:
        if not isinstance(cache, MemoryLayerCache):
            raise TypeError(f"{who}: cache must be a MemoryLayerCache (new_cache), got {type(cache)}")

    @torch.no_grad()
    def _pin(self, cache: MemoryLayerCache, memory: Optional[MemoryContext]) -> None:
        """Holds ``memory`` in the cache with the constants it makes of the injection (see ``MemoryLayerCache``)."""
        cache.memory, cache.c, cache.u, cache.fold = memory, None, None, None
        if memory is None or self.memory_injection == "cross_attention":
            return
        weights = F.softmax(memory.scores, dim=-1).unsqueeze(-1)
        context = (memory.features * weights).sum(dim=1)                       # [B, D]
        if self.memory_injection == "gate":
            D = self.config.embedding_dim
            gate = self.memory_gate[0]
            context = self.memory_proj(context)
            cache.u = F.linear(context, gate.weight[:, D:], gate.bias).contiguous()
        cache.c = context.contiguous()

    def _check_foldable(self, who: str) -> None:
        """What the fold assumes of ``memory_attention``: one packed ``in_proj_weight`` and nothing appended to the keys
        and values."""
        att = self.memory_attention
        if not att._qkv_same_embed_dim:
            raise ValueError(f"{who}: memory_attention must hold one packed in_proj_weight (kdim = vdim = embed_dim)")
        if att.bias_k is not None or att.bias_v is not None or att.add_zero_attn:
            raise ValueError(f"{who}: memory_attention with bias_k, bias_v or add_zero_attn attends rows that are not "
                             f"memories; the fold does not cover them")

    @torch.no_grad()
    def fold_memory(self, cache: MemoryLayerCache) -> Optional[FoldedMemory]:
        """Folds the pinned memories of a ``cross_attention`` layer through ``memory_attention``'s projections into the
        tables ``ops.memory_attend`` reads (``FoldedMemory``; the rule: ``include/aura_hip.h``, "Memory attend") and
        holds them in ``cache.fold``: what ``step(fused=True)`` needs.  Once per generation: computed in fp64 from the
        fp32 parameters and rounded once, so every table element carries a single rounding; torch ops only, on the
        device the memories are on.  A second call returns the tables it holds.  ``None``, and nothing done, for the
        other injections and when nothing is pinned.  The zero rows of empty slots are folded like any memory."""
        who = "MemoryAugmentedLayer.fold_memory"
        self._check_cache(who, cache)
        if self.memory_injection != "cross_attention" or cache.memory is None:
            return None
        if cache.fold is not None:
            return cache.fold
        self._check_foldable(who)
        att = self.memory_attention
        features = cache.memory.features
        B, M, D = features.shape
        H = att.num_heads
        dh = D // H
        if D % 4 != 0 or not 4 <= D <= ops.MEMORY_ATTEND_MAX_D or not 1 <= M <= ops.MEMORY_ATTEND_MAX_M \
                or H * M > ops.MEMORY_ATTEND_MAX_HM:
            raise ValueError(f"{who}: D={D}, H={H} and k={M} are outside ops.memory_attend's limits (D % 4 == 0, D <= "
                             f"{ops.MEMORY_ATTEND_MAX_D}, k <= {ops.MEMORY_ATTEND_MAX_M}, H k <= "
                             f"{ops.MEMORY_ATTEND_MAX_HM}); use fused=False")
        W = att.in_proj_weight.double()
        b = torch.zeros(3 * D, dtype=torch.float64, device=W.device) if att.in_proj_bias is None \
            else att.in_proj_bias.double()
        mem = features.double()
        keys = (mem @ W[D:2 * D].T + b[D:2 * D]).view(B, M, H, dh)
        values = (mem @ W[2 * D:].T + b[2 * D:]).view(B, M, H, dh)
        root = float(dh) ** 0.5
        G = torch.einsum("bmhj,hjd->bhmd", keys, W[:D].view(H, dh, D)) / root
        s0 = torch.einsum("bmhj,hj->bhm", keys, b[:D].view(H, dh)) / root
        U = torch.einsum("bmhj,dhj->bhmd", values, att.out_proj.weight.double().view(D, H, dh))
        cache.fold = FoldedMemory(G.float().contiguous(), s0.float().contiguous(), U.float().contiguous())
        return cache.fold

    def prefill(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
                cache: Optional[MemoryLayerCache] = None, memory: Optional[MemoryContext] = None,
                lengths=None) -> torch.Tensor:
        """``forward`` over a prompt [B, S, D] that also fills the attention cache and pins the memory context for the
        steps that follow: ``memory`` if given, else what ``retrieve_context`` finds for the prompt; nothing with
        ``use_memory=False``.  Returns what ``forward(.., memory=<the pinned context>)`` returns.  ``lengths`` [B]:
        right-padded rows; the cache takes them as the attention's ``prefill`` does and the retrieval query is each
        row's mean over its own positions."""
        who = "MemoryAugmentedLayer.prefill"
        self._check_cache(who, cache)
        if memory is not None:
            self._check_context(who, memory, hidden_states.shape[0])
        ragged = {} if lengths is None else dict(lengths=torch.as_tensor(lengths))
        attn_output, _ = self.attention.prefill(self.attention_norm(hidden_states), prosody=prosody,
                                                use_memory=use_memory, cache=cache.attention, **ragged)
        hidden_states = hidden_states + self.dropout(attn_output)
        if not use_memory:
            memory = None
        elif memory is None:
            memory = self.retrieve_context(hidden_states, **ragged)
        self._pin(cache, memory)
        return self._after_attention(hidden_states, memory is not None, memory)

    @torch.no_grad()
    def step(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
             cache: Optional[MemoryLayerCache] = None, advance: bool = True, *, fused: bool = False) -> torch.Tensor:
        """One new token through the layer: hidden [B, D] or [B, 1, D] -> [B, D], with the memories ``prefill`` pinned
        (``use_memory=False`` injects nothing).  ``advance=False`` leaves the cache's lengths alone.

        ``fused=False`` is the layer's formula from torch ops around ``attention.step``.  ``fused=True`` (B <= 32, eval
        mode or no dropout, the exact GELU) makes an MLP layer seven launches: four of the attention's fused step, one
        for the injection (``gate``: ``ops.row_linear_gate``; ``cross_attention``: ``ops.memory_attend`` over the tables
        ``fold_memory(cache)`` made, which must have been called: the step never folds; ``concat``: one torch add),
        LayerNorm + ``ffn.0`` + GELU, ``ffn.2`` + residual.  A HybridFFN layer is eleven: the MLP branch without its residual, then
        the four of the spiking branch (``_snn_branch``: ``ops.row_linear`` and ``ops.row_linear_gif``, the ``B * T``
        rows of ``syn2`` and ``neuron2.linear`` in groups of whole tokens of at most 32 rows), the last of which mixes
        the branches and adds the residual.  It raises where it does not apply; it never falls back."""
        who = "MemoryAugmentedLayer.step"
        self._check_cache(who, cache)
        if hidden_states.dim() == 3 and hidden_states.shape[1] == 1:
            hidden_states = hidden_states[:, 0]
        memory = cache.memory if use_memory else None
        if fused:
            return self._fused_step(hidden_states, prosody, use_memory, cache, advance, memory)
        attn_output = self.attention.step(self.attention_norm(hidden_states), prosody=prosody, use_memory=use_memory,
                                          cache=cache.attention, advance=advance)
        hidden_states = (hidden_states + self.dropout(attn_output))[:, None]
        return self._after_attention(hidden_states, memory is not None, memory)[:, 0]

    @torch.no_grad()
    def extend(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
               cache: Optional[MemoryLayerCache] = None, advance: bool = True, counts=None,
               count_bound: Optional[int] = None) -> torch.Tensor:
        """``m`` new tokens through the layer: hidden [B, m, D] -> [B, m, D], the layer's formula around the
        attention's ``extend``, with the memories ``prefill`` pinned injected at every new position
        (``use_memory=False`` injects nothing).  ``counts`` [B]: right-padded rows (see the attention's ``extend``);
        what the padded places return is unspecified."""
        self._check_cache("MemoryAugmentedLayer.extend", cache)
        memory = cache.memory if use_memory else None
        ragged = {} if counts is None and count_bound is None else dict(counts=counts, count_bound=count_bound)
        attn_output = self.attention.extend(self.attention_norm(hidden_states), prosody=prosody,
                                            use_memory=use_memory, cache=cache.attention, advance=advance, **ragged)
        return self._after_attention(hidden_states + self.dropout(attn_output), memory is not None, memory)

    def _mlp(self):
        return self.ffn.mlp if self.use_snn_ffn else self.ffn

    def _fused_step(self, hidden_states, prosody, use_memory, cache, advance, memory) -> torch.Tensor:
        who = "MemoryAugmentedLayer.step(fused=True)"
        cross = self.memory_injection == "cross_attention"
        mlp = self._mlp()
        drops = [self.dropout.p, mlp[3].p] + ([self.ffn.snn.dropout.p] if self.use_snn_ffn else [])
        if cross:
            drops.append(self.memory_attention.dropout)
        if self.training and any(p > 0 for p in drops):
            raise RuntimeError(f"{who}: the fused step has no dropout; call eval() first (dropout={max(drops)})")
        if not isinstance(mlp[1], nn.GELU) or getattr(mlp[1], "approximate", "none") != "none":
            raise ValueError(f"{who}: the MLP's activation must be the exact nn.GELU(), got {mlp[1]!r}")
        if hidden_states.dim() == 2 and hidden_states.shape[0] > ops.ROW_LINEAR_MAX_ROWS:
            raise ValueError(f"{who}: at most {ops.ROW_LINEAR_MAX_ROWS} rows, got B={hidden_states.shape[0]}; use "
                             f"fused=False")
        if self.ffn_norm.weight is None or self.ffn_norm.bias is None:
            raise ValueError(f"{who}: the fused prologue needs a LayerNorm with weight and bias")
        if cross and memory is not None:
            if self.memory_norm.weight is None or self.memory_norm.bias is None:
                raise ValueError(f"{who}: the fused cross_attention injection needs a memory_norm with weight and bias")
            self._check_foldable(who)
            if cache.fold is None:
                raise ValueError(f"{who}: the cross_attention injection steps fused from the folded tables of the "
                                 f"pinned memories: call fold_memory(cache) once after prefill, or use fused=False")
        hidden = self.attention.step(hidden_states, prosody=prosody, use_memory=use_memory, cache=cache.attention,
                                     advance=advance, fused=True, residual=hidden_states, norm=self.attention_norm)
        if memory is not None:
            if cross:
                fold, mn = cache.fold, self.memory_norm
                hidden = ops.memory_attend(hidden, (mn.weight, mn.bias), fold.G, fold.s0, fold.U,
                                           self.memory_attention.out_proj.bias, eps=mn.eps)
            elif self.memory_injection == "gate":
                D = self.config.embedding_dim
                hidden = ops.row_linear_gate(hidden, self.memory_gate[0].weight[:, :D], None, cache.u, cache.c, hidden)
            else:
                hidden = hidden + 0.1 * cache.c
        norm = (self.ffn_norm.weight, self.ffn_norm.bias)
        if not self.use_snn_ffn:
            mid = ops.row_linear(hidden, mlp[0].weight, mlp[0].bias, norm=norm, eps=self.ffn_norm.eps,
                                 activation="gelu")
            return ops.row_linear(mid, mlp[2].weight, mlp[2].bias, residual=hidden)
        mid, normed = ops.row_linear(hidden, mlp[0].weight, mlp[0].bias, norm=norm, eps=self.ffn_norm.eps,
                                     activation="gelu", return_normed=True)
        mlp_out = ops.row_linear(mid, mlp[2].weight, mlp[2].bias)
        return self._snn_branch(normed, mix=(hidden, mlp_out))

    def _snn_branch(self, x: torch.Tensor, mix=None, group_rows: int = ops.ROW_LINEAR_MAX_ROWS) -> torch.Tensor:
        """``SNNFFN``'s eval forward for the rows x [B, D] of one decoding step in four launches: ``syn1``;
        ``neuron1.linear`` with its T-step loop (``ops.row_linear_gif``, the currents are the same at every step);
        ``syn2`` over the ``B * T`` spike rows; ``neuron2.linear`` with its loop and the mean over T.  The last two go in
        groups of whole tokens of at most ``group_rows`` rows (a row's bits do not depend on the grouping).  Every token
        starts from fresh neuron state, as ``SNNFFN`` does.  ``mix=(residual, mlp_out)``: the last launch also finishes
        the layer, ``residual + ((1 - g) * mlp_out + g * mean)`` with ``g = sigmoid(ffn.gate)`` read on the device."""
        who = "MemoryAugmentedLayer.step(fused=True)"
        snn = self.ffn.snn
        n1, n2, T = snn.neuron1, snn.neuron2, snn.num_timesteps
        if snn.plasticity:
            raise ValueError(f"{who}: a plastic SNNFFN keeps traces; use fused=False")
        if not 1 <= T <= group_rows:
            raise ValueError(f"{who}: num_timesteps={T} must be in [1, {group_rows}]")
        B = x.shape[0]
        h1 = ops.row_linear(x, snn.syn1.weight, snn.syn1.bias)
        spikes1 = ops.row_linear_gif(h1, n1.linear.weight, n1.linear.bias, T=T, decay=n1.decay, L=n1.L, alpha=n1.alpha,
                                     threshold=n1.threshold)
        rows = spikes1.view(B * T, snn.hidden_dim)
        out = torch.empty(B, snn.output_dim, dtype=torch.float32, device=x.device)
        tokens = group_rows // T
        for t0 in range(0, B, tokens):
            t1 = min(B, t0 + tokens)
            h2 = ops.row_linear(rows[t0 * T:t1 * T], snn.syn2.weight, snn.syn2.bias)
            part = None if mix is None else (mix[0][t0:t1], mix[1][t0:t1], self.ffn.gate)
            ops.row_linear_gif(h2, n2.linear.weight, n2.linear.bias, T=T, decay=n2.decay, L=n2.L, alpha=n2.alpha,
                               threshold=n2.threshold, time_major=True, mix=part, out=out[t0:t1])
        return out
