"""SNNRAGTransformer: the place-code front end, a stack of ``MemoryAugmentedLayer``s (self-attention, retrieval from the
hippocampus and injection, MLP or HybridFFN with the spiking FFN) and the tied head, with cached generation.

API-compatible with the reference's ``src/core/language_zone/snn_rag_transformer.py``: the constructor ``(config,
hippocampus, use_snn_ffn=True, snn_layers=None, memory_injection="gate", num_retrieved=5)`` (it prints nothing), the
attribute names (``pos_encoder``, ``semantic_encoder``, ``dropout``, ``layer_norm``, ``layers``, ``output_head``,
``snn_layers``), the ``state_dict`` keys, the tied head, ``set_gradient_checkpointing`` and ``forward(input_ids,
prosody=None, use_memory=True, store_memory=False) -> (logits, place_cell_activity)``.  The front end is
``embed_tokens``, as in ``HippocampalTransformer``; ``store_memory`` reaches the last layer only, as upstream.

New on this module: ``forward(.., memory=[context per layer])`` and ``new_state`` / ``prefill`` / ``step`` /
``generate``, the last three with the signature and semantics of ``HippocampalTransformer``'s (the decode loop is the
same code: ``CachedDecodingMixin``).  One more deliberate difference from the reference's loop comes on top of those
listed there: **retrieval is pinned at the prompt**.  The reference re-retrieves in every layer, for every token, from the
mean of the growing context: a bank recall per layer and token, and a function that changes at earlier positions, so that
nothing can be cached.  Here ``prefill`` retrieves once per layer from the prompt and every later step injects those
memories, as retrieval-augmented generation usually does; ``generate`` then equals the loop that recomputes
``forward(context, memory=pinned)``.  Re-retrieval during a generation is not built.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from .hippocampal_transformer import CachedDecodingMixin, DecodeState
from .memory_augmented_layer import MemoryAugmentedLayer, MemoryContext
from .place_cell_encoder import PlaceCellSemanticEncoder
from .theta_gamma_encoding import ThetaGammaPositionalEncoding, embed_tokens


class SNNRAGTransformer(CachedDecodingMixin, nn.Module):
    def __init__(self, config, hippocampus, use_snn_ffn: bool = True, snn_layers: Optional[List[int]] = None,
                 memory_injection: str = "gate", num_retrieved: int = 5):
        super().__init__()
        self.config = config
        self.hippocampus = hippocampus
        self.use_gradient_checkpointing = getattr(config, 'use_gradient_checkpointing', False)
        if snn_layers is None:
            snn_layers = list(range(0, config.num_layers, 2))                   # every other layer, as upstream
        self.snn_layers = set(snn_layers)
        self.pos_encoder = ThetaGammaPositionalEncoding(config)
        self.semantic_encoder = PlaceCellSemanticEncoder(config, hippocampus)
        self.dropout = nn.Dropout(config.dropout)
        self.layer_norm = nn.LayerNorm(config.embedding_dim)
        self.layers = nn.ModuleList([
            MemoryAugmentedLayer(config=config, hippocampus=hippocampus,
                                 use_snn_ffn=(use_snn_ffn and i in self.snn_layers),
                                 memory_injection=memory_injection, num_retrieved=num_retrieved)
            for i in range(config.num_layers)])
        self.output_head = nn.Linear(config.embedding_dim, config.vocab_size, bias=False)
        self.output_head.weight = self.semantic_encoder.token_embedding.weight      # tied, as upstream

    def set_gradient_checkpointing(self, enable: bool = True):
        self.use_gradient_checkpointing = enable

    def _layer_forward(self, layer, hidden_states, prosody, use_memory, store_memory, memory=None):
        return layer(hidden_states, prosody=prosody, use_memory=use_memory, store_memory=store_memory, memory=memory)

    def _layer_contexts(self, who: str, memory) -> Sequence[Optional[MemoryContext]]:
        if memory is None:
            return [None] * len(self.layers)
        if not isinstance(memory, (list, tuple)) or len(memory) != len(self.layers):
            raise ValueError(f"{who}: memory is a list of one MemoryContext (or None) per layer, {len(self.layers)} here")
        return memory

    # ------------------------------------------------------------------------------------------------ full sequences
    def forward(self, input_ids: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
                store_memory: bool = False, memory=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``memory``: a list with one ``MemoryContext`` (or ``None``) per layer; a layer with one injects it and
        retrieves nothing (``pinned_memory`` of a ``prefill``'s state gives the list a generation holds)."""
        contexts = self._layer_contexts("SNNRAGTransformer.forward", memory)
        hidden_states, place_cell_activity = embed_tokens(input_ids, self.semantic_encoder, self.pos_encoder,
                                                          self.layer_norm)
        hidden_states = self.dropout(hidden_states)
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            should_store = store_memory and i == last
            if self.training and self.use_gradient_checkpointing:
                hidden_states = checkpoint(self._layer_forward, layer, hidden_states, prosody, use_memory,
                                           should_store, contexts[i], use_reentrant=False)
            else:
                hidden_states = layer(hidden_states, prosody=prosody, use_memory=use_memory,
                                      store_memory=should_store, memory=contexts[i])
        return self.output_head(hidden_states), place_cell_activity

    # ------------------------------------------------------------------------------------------------ cached decoding
    def prefill(self, input_ids: torch.Tensor, prosody: Optional[torch.Tensor] = None,
                state: Optional[DecodeState] = None, use_memory: bool = True, memory=None,
                lengths=None) -> torch.Tensor:
        """``forward`` over a prompt [B, S] that also fills every layer's cache, pins every layer's memory context
        (``memory``: the list to pin; ``None``: each layer retrieves from the prompt) and marks the prompt's tokens in
        ``state.seen``.  Returns the logits [B, S, V].  ``lengths`` [B] (ints, ``1 <= lengths[b] <= S``, on the host or
        the device): the rows are right-padded; the caches hold each row's own positions, every layer retrieves from
        the mean over a row's own positions, only its own tokens are marked, the state becomes ``ragged`` and the
        logits at the padded places are unspecified."""
        return self.output_head(self._prefill_hidden("SNNRAGTransformer.prefill", input_ids, prosody, state,
                                                     use_memory, lengths, memory))

    def _prefill_layer_kwargs(self, who: str, memory) -> Sequence[dict]:
        return [dict(memory=context) for context in self._layer_contexts(who, memory)]

    @staticmethod
    def pinned_memory(state: DecodeState) -> List[Optional[MemoryContext]]:
        """The contexts the layers hold in ``state`` after ``prefill``: what ``forward(.., memory=)`` takes."""
        return [cache.memory for cache in state.caches]

    def fold_memory(self, state: DecodeState) -> list:
        """Folds every layer's pinned memories into the tables its fused ``cross_attention`` step reads
        (``MemoryAugmentedLayer.fold_memory``): one ``FoldedMemory`` or ``None`` per layer.  Idempotent; nothing to do
        for ``gate`` and ``concat``."""
        self._check_state("SNNRAGTransformer.fold_memory", state, state.batch)
        return [layer.fold_memory(cache) for layer, cache in zip(self.layers, state.caches)]

    def _before_fused_steps(self, state: DecodeState) -> None:
        self.fold_memory(state)
