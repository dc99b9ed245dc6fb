"""HippocampalTransformerLayer: pre-norm attention and feed-forward sublayers around HippocampalProsodyAttention.

API-compatible with the reference's ``src/core/language_zone/hippocampal_layer.py`` (constructor, ``state_dict`` keys
``attention_norm`` / ``attention.*`` / ``ffn_norm`` / ``ffn.0`` / ``ffn.2``, ``forward``).  New on this module:
``new_cache`` / ``prefill`` / ``step`` wrap the norms, the residuals and the feed-forward around the attention's, so
that a stack of layers decodes one token at a time, layer by layer, each with its own cache."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

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
             cache: Optional[AttentionCache] = None, advance: bool = True) -> torch.Tensor:
        """One new token through the layer: hidden [B, D] or [B, 1, D] -> [B, D].  ``advance=False`` leaves the
        cache's lengths alone (a model whose layers share one lengths tensor advances it in its last layer)."""
        if hidden_states.dim() == 3 and hidden_states.shape[1] == 1:
            hidden_states = hidden_states[:, 0]
        attn_output = self.attention.step(self.attention_norm(hidden_states), prosody=prosody, use_memory=use_memory,
                                          cache=cache, advance=advance)
        return self._feed_forward(hidden_states + self.dropout(attn_output))
