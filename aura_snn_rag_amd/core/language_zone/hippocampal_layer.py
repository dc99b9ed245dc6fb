"""HippocampalTransformerLayer: pre-norm attention and feed-forward sublayers around HippocampalProsodyAttention.

API-compatible with the reference's ``src/core/language_zone/hippocampal_layer.py`` (constructor, ``state_dict`` keys
``attention_norm`` / ``attention.*`` / ``ffn_norm`` / ``ffn.0`` / ``ffn.2``, ``forward``).  New on this module:
``new_cache`` / ``prefill`` / ``step`` / ``extend`` wrap the norms, the residuals and the feed-forward around the attention's, so
that a stack of layers decodes one token at a time, layer by layer, each with its own cache.  ``step(fused=True)`` is
the same step in six launches (``ops.row_linear``, ``csrc/aura_rowlin.hip``)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ... import ops
from .hippocampal_attention import AttentionCache, HippocampalProsodyAttention


class HippocampalTransformerLayer(nn.Module):
    def __init__(self, config, hippocampus):
        super().__init__()
        self.config = config
        self.attention_norm = nn.LayerNorm(config.embedding_dim)
        self.attention = HippocampalProsodyAttention(config, hippocampus)
        self.ffn_norm = nn.LayerNorm(config.embedding_dim)
        self.ffn = nn.Sequential(
            nn.Linear(config.embedding_dim, config.intermediate_size),
            nn.GELU(),
            nn.Linear(config.intermediate_size, config.embedding_dim),
            nn.Dropout(config.dropout),
        )
        self.dropout = nn.Dropout(config.dropout)

    def _feed_forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return hidden_states + self.ffn(self.ffn_norm(hidden_states))

    def forward(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None,
                use_memory: bool = True) -> torch.Tensor:
        attn_output, _ = self.attention(self.attention_norm(hidden_states), prosody=prosody, use_memory=use_memory)
        return self._feed_forward(hidden_states + self.dropout(attn_output))

    def new_cache(self, batch: int, capacity: int) -> AttentionCache:
        return self.attention.new_cache(batch, capacity)

    def prefill(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
                cache: Optional[AttentionCache] = None, lengths=None) -> torch.Tensor:
        """``forward`` over a prompt [B, S, D] that also fills ``cache`` (see the attention's ``prefill``)."""
        attn_output, _ = self.attention.prefill(self.attention_norm(hidden_states), prosody=prosody,
                                                use_memory=use_memory, cache=cache, lengths=lengths)
        return self._feed_forward(hidden_states + self.dropout(attn_output))

    @torch.no_grad()
    def step(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
             cache: Optional[AttentionCache] = None, advance: bool = True, *, fused: bool = False) -> torch.Tensor:
        """One new token through the layer: hidden [B, D] or [B, 1, D] -> [B, D].  ``advance=False`` leaves the
        cache's lengths alone (a model whose layers share one lengths tensor advances it in its last layer).

        ``fused=True`` (B <= 32, eval mode or no dropout, the exact GELU) is the same function in six launches instead
        of fourteen: LayerNorm + Q/K/V, the two of the decode step, ``o_proj`` + residual, LayerNorm + ``ffn.0`` + GELU,
        ``ffn.2`` + residual (``ops.row_linear``).  It raises where it does not apply; it never falls back."""
        if hidden_states.dim() == 3 and hidden_states.shape[1] == 1:
            hidden_states = hidden_states[:, 0]
        if fused:
            return self._fused_step(hidden_states, prosody, use_memory, cache, advance)
        attn_output = self.attention.step(self.attention_norm(hidden_states), prosody=prosody, use_memory=use_memory,
                                          cache=cache, advance=advance)
        return self._feed_forward(hidden_states + self.dropout(attn_output))

    @torch.no_grad()
    def extend(self, hidden_states: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
               cache: Optional[AttentionCache] = None, advance: bool = True, counts=None,
               count_bound: Optional[int] = None) -> torch.Tensor:
        """``m`` new tokens through the layer: hidden [B, m, D] -> [B, m, D], the layer's formula around the
        attention's ``extend``.  ``counts`` [B]: right-padded rows (see the attention's ``extend``); what the padded
        places return is unspecified."""
        ragged = {} if counts is None and count_bound is None else dict(counts=counts, count_bound=count_bound)
        attn_output = self.attention.extend(self.attention_norm(hidden_states), prosody=prosody,
                                            use_memory=use_memory, cache=cache, advance=advance, **ragged)
        return self._feed_forward(hidden_states + self.dropout(attn_output))

    def _fused_step(self, hidden_states, prosody, use_memory, cache, advance) -> torch.Tensor:
        who = "HippocampalTransformerLayer.step(fused=True)"
        if self.training and (self.dropout.p > 0 or self.ffn[3].p > 0):
            raise RuntimeError(f"{who}: the fused step has no dropout; call eval() first (dropout={self.dropout.p})")
        act = self.ffn[1]
        if not isinstance(act, nn.GELU) or getattr(act, "approximate", "none") != "none":
            raise ValueError(f"{who}: ffn.1 must be the exact nn.GELU(), got {act!r}")
        if hidden_states.dim() == 2 and hidden_states.shape[0] > ops.ROW_LINEAR_MAX_ROWS:
            raise ValueError(f"{who}: at most {ops.ROW_LINEAR_MAX_ROWS} rows, got B={hidden_states.shape[0]}; use "
                             f"fused=False")
        if self.ffn_norm.weight is None or self.ffn_norm.bias is None:
            raise ValueError(f"{who}: the fused prologue needs a LayerNorm with weight and bias")
        hidden = self.attention.step(hidden_states, prosody=prosody, use_memory=use_memory, cache=cache,
                                     advance=advance, fused=True, residual=hidden_states, norm=self.attention_norm)
        mid = ops.row_linear(hidden, self.ffn[0].weight, self.ffn[0].bias,
                             norm=(self.ffn_norm.weight, self.ffn_norm.bias), eps=self.ffn_norm.eps, activation="gelu")
        return ops.row_linear(mid, self.ffn[2].weight, self.ffn[2].bias, residual=hidden)
