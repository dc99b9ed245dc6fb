"""Batched memory retrieval / storage / injection for the RAG transformer layer.

The immediate caller of the hot path in the reference is ``MemoryAugmentedLayer``
(``src/core/language_zone/memory_augmented_layer.py:86-203``): it loops over the batch in Python,
issues one ``retrieve_similar_memories`` per row and then copies ``k`` bank rows one by one.
These functions keep the method signatures and results of that layer and do the work in one
batched recall + one row gather.

Use either as free functions or through ``BatchedMemoryMixin``::

    class FastLayer(BatchedMemoryMixin, MemoryAugmentedLayer):   # reference layer, HIP memory path
        pass
"""
from __future__ import annotations

import uuid
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F


def retrieve_memories(hippocampus, query: torch.Tensor, k: int = 5, dtype=None,
                      reinforce: Optional[float] = None, reinforce_cap: float = 1.0,
                      diversity: Optional[float] = None, max_similarity: Optional[float] = None,
                      fetch_k: Optional[int] = None, tags=None, newer_than: Optional[float] = None,
                      older_than: Optional[float] = None,
                      min_strength: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``query`` [B, D] (already projected) -> (memory_features [B, k, D], memory_scores [B, k]).

    Same contract as the reference loop (``memory_augmented_layer.py:106-130``): slots beyond the
    number of hits stay zero.  ``reinforce`` (default off): strengthen the retrieved rows by that amount up to
    ``reinforce_cap`` (``HippocampalFormation.recall_batch(reinforce=...)``).  ``diversity`` / ``max_similarity`` /
    ``fetch_k`` (default off): diverse recall, so that near-copies of one memory do not fill the k slots
    (``HippocampalFormation.recall_batch(diversity=..., max_similarity=...)``).  ``tags`` (an int, or one per batch
    item) / ``newer_than`` / ``older_than`` / ``min_strength`` (default off): scoped recall -- only memories of that
    tag, time window and strength are retrieved, exactly (``HippocampalFormation.recall_batch(tags=...)``)."""
    B, D = query.shape
    dtype = dtype or query.dtype
    dev = query.device
    feats = torch.zeros(B, k, D, device=dev, dtype=dtype)
    scores = torch.zeros(B, k, device=dev, dtype=dtype)
    if hippocampus is None or hippocampus.memory_count == 0:
        return feats, scores
    kw = {} if reinforce is None else dict(reinforce=reinforce, reinforce_cap=reinforce_cap)
    if diversity is not None or max_similarity is not None:
        kw.update(diversity=diversity, max_similarity=max_similarity, fetch_k=fetch_k)
    for name, v in (("tags", tags), ("newer_than", newer_than), ("older_than", older_than), ("min_strength", min_strength)):
        if v is not None:
            kw[name] = v
    s, rows = hippocampus.recall_batch(query.detach().float(), k=k, **kw)      # [B, k'] (k' <= k)
    kk = s.shape[1]
    valid = rows >= 0
    feats[:, :kk] = hippocampus.gather_features(rows).to(dtype)            # -1 rows gather zeros
    scores[:, :kk] = torch.where(valid, s, torch.zeros_like(s)).to(dtype)
    return feats, scores


def store_memory(hippocampus, hidden_states: torch.Tensor, event_tag: str = "layer",
                 merge_similarity: Optional[float] = None, tag=None, merge_within_tags: Optional[bool] = None,
                 merge_blend: Optional[float] = None):
    """Mean-pool each batch item and store it (``memory_augmented_layer.py:132-153``).  ``merge_similarity`` (default
    off): a consolidating write -- a pooled row that repeats a held memory at that cosine strengthens it instead of
    taking a slot (``HippocampalFormation.create_episodic_memories(merge_similarity=...)``, whose report is returned);
    a bank constructed with a threshold consolidates without it.  ``tag`` (default off; an int, or one per batch item):
    the stored memories carry it (``HippocampalFormation.create_episodic_memories(tags=...)``) and
    ``retrieve_memories(tags=...)`` recalls within it; together with a consolidating write only when the consolidation
    stays within tags.  ``merge_within_tags`` (default None: what the bank was constructed with): a pooled row then
    merges only into a memory of its own tag (``create_episodic_memories(merge_within_tags=...)``).  ``merge_blend``
    (default None: what the bank was constructed with): the rate at which a repeated memory moves toward the pooled rows
    that repeat it (``create_episodic_memories(merge_blend=...)``)."""
    if hippocampus is None:
        return None
    feats = hidden_states.detach().float().mean(dim=1)                      # [B, D]
    ids = [str(uuid.uuid4())[:8] for _ in range(feats.shape[0])]
    kw = {} if tag is None else dict(tags=tag)
    if merge_within_tags is not None:
        kw["merge_within_tags"] = merge_within_tags
    if merge_blend is not None:
        kw["merge_blend"] = merge_blend
    if merge_similarity is None:
        return hippocampus.create_episodic_memories(ids, feats, **kw)
    return hippocampus.create_episodic_memories(ids, feats, merge_similarity=merge_similarity, **kw)


def inject_concat(hidden_states, memory_features, memory_scores):
    """``memory_injection == "concat"`` (``:178-184``)."""
    w = F.softmax(memory_scores, dim=-1).unsqueeze(-1)
    ctx = (memory_features * w).sum(dim=1, keepdim=True).expand(-1, hidden_states.shape[1], -1)
    return hidden_states + 0.1 * ctx


def inject_gate(hidden_states, memory_features, memory_scores, memory_proj, memory_gate):
    """``memory_injection == "gate"`` (``:186-198``): the score-weighted memory context, projected, enters
    through a sigmoid gate computed from [hidden, context]."""
    w = F.softmax(memory_scores, dim=-1).unsqueeze(-1)
    ctx = (memory_features * w).sum(dim=1, keepdim=True).expand(-1, hidden_states.shape[1], -1)
    ctx = memory_proj(ctx)
    gate = memory_gate(torch.cat([hidden_states, ctx], dim=-1))
    return hidden_states + gate * ctx


def inject_cross_attention(hidden_states, memory_features, memory_norm, memory_attention, dropout):
    """``memory_injection == "cross_attention"`` (``:171-179``): the normed hidden states attend to the
    k retrieved rows."""
    attn_out, _ = memory_attention(query=memory_norm(hidden_states), key=memory_features, value=memory_features)
    return hidden_states + dropout(attn_out)


class MemoryInjection(nn.Module):
    """The injection half of ``MemoryAugmentedLayer`` (``memory_augmented_layer.py:47-60,155-203``) as
    a module of its own, with the reference's submodule names (``memory_norm``, ``memory_attention``,
    ``memory_gate``, ``memory_proj``, ``query_proj``) so that a layer checkpoint's keys load with
    ``strict=False``.  ``forward(hidden_states)`` = batched recall + row gather on the HIP bank
    (``retrieve_memories``) followed by the configured injection."""

    def __init__(self, hippocampus, embedding_dim: int, num_heads: int = 8, dropout: float = 0.1,
                 memory_injection: str = "cross_attention", num_retrieved: int = 5):
        super().__init__()
        if memory_injection not in ("cross_attention", "concat", "gate"):
            raise ValueError("memory_injection must be 'cross_attention', 'concat' or 'gate'")
        self.hippocampus = hippocampus
        self.memory_injection = memory_injection
        self.num_retrieved = num_retrieved
        if memory_injection == "cross_attention":
            self.memory_norm = nn.LayerNorm(embedding_dim)
            self.memory_attention = nn.MultiheadAttention(embed_dim=embedding_dim, num_heads=num_heads,
                                                          dropout=dropout, batch_first=True)
        elif memory_injection == "gate":
            self.memory_gate = nn.Sequential(nn.Linear(embedding_dim * 2, embedding_dim), nn.Sigmoid())
            self.memory_proj = nn.Linear(embedding_dim, embedding_dim)
        self.dropout = nn.Dropout(dropout)
        self.query_proj = nn.Linear(embedding_dim, embedding_dim)

    def retrieve_memories(self, hidden_states: torch.Tensor, k: int = 5, reinforce: Optional[float] = None,
                          reinforce_cap: float = 1.0, *, diversity: Optional[float] = None,
                          max_similarity: Optional[float] = None, fetch_k: Optional[int] = None, tags=None,
                          newer_than: Optional[float] = None, older_than: Optional[float] = None,
                          min_strength: Optional[float] = None):
        query = self.query_proj(hidden_states.mean(dim=1))
        return retrieve_memories(self.hippocampus, query, k=k, dtype=hidden_states.dtype, reinforce=reinforce,
                                 reinforce_cap=reinforce_cap, diversity=diversity, max_similarity=max_similarity,
                                 fetch_k=fetch_k, tags=tags, newer_than=newer_than, older_than=older_than,
                                 min_strength=min_strength)

    def store_memory(self, hidden_states: torch.Tensor, merge_similarity: Optional[float] = None, tag=None,
                     merge_within_tags: Optional[bool] = None, merge_blend: Optional[float] = None):
        return store_memory(self.hippocampus, hidden_states, event_tag=f"layer_{id(self)}",
                            merge_similarity=merge_similarity, tag=tag, merge_within_tags=merge_within_tags,
                            merge_blend=merge_blend)

    def inject_memories(self, hidden_states, memory_features, memory_scores):
        if self.memory_injection == "cross_attention":
            return inject_cross_attention(hidden_states, memory_features, self.memory_norm, self.memory_attention,
                                          self.dropout)
        if self.memory_injection == "concat":
            return inject_concat(hidden_states, memory_features, memory_scores)
        return inject_gate(hidden_states, memory_features, memory_scores, self.memory_proj, self.memory_gate)

    def consolidate_memory(self, similarity: Optional[float] = None, within_tags: Optional[bool] = None,
                           blend: Optional[float] = None):
        """Merge the near-copies the bank holds (``HippocampalFormation.consolidate``); ``within_tags`` (None: the
        bank's default): only among memories of one tag; ``blend`` (None: the bank's default): the rate at which a
        kept memory moves toward the rows merged into it."""
        kw = {} if within_tags is None else dict(within_tags=within_tags)
        if blend is not None:
            kw["blend"] = blend
        return self.hippocampus.consolidate(similarity=similarity, **kw)

    def replay_memories(self, n: int, **kw):
        """``(features [n, D], rows int32 [n])``: ``n`` held memories drawn by priority for a sleep phase
        (``HippocampalFormation.replay`` and its keywords: scope, ``alpha``, ``seed`` / ``draw``, ``reinforce``,
        ``touch``); zeros / ``-1`` where the scope held fewer."""
        s = self.hippocampus.replay(n, **kw)
        return s.features, s.rows

    def forward(self, hidden_states: torch.Tensor, use_memory: bool = True) -> torch.Tensor:
        if use_memory and self.hippocampus is not None and self.hippocampus.memory_count > 0:
            mf, ms = self.retrieve_memories(hidden_states, k=self.num_retrieved)
            hidden_states = self.inject_memories(hidden_states, mf, ms)
        return hidden_states


def masked_mean(hidden_states: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """The mean of every row of ``hidden_states`` [B, S, D] over its first ``lengths[b]`` positions: the valid
    positions summed in fp32 (the padded ones selected out, so that nothing they hold, NaN included, counts) and
    divided by the row's length.  Device ops only; ``lengths[b] >= 1`` is the caller's to ensure."""
    lengths = lengths.to(hidden_states.device)
    valid = torch.arange(hidden_states.shape[1], device=hidden_states.device)[None, :] < lengths[:, None]
    total = torch.where(valid[..., None], hidden_states.float(), 0.0).sum(dim=1)
    return (total / lengths.to(torch.float32)[:, None]).to(hidden_states.dtype)


class BatchedMemoryMixin:
    """Overrides ``retrieve_memories`` / ``store_memory`` of the reference layer with the batched
    HIP path; ``inject_memories`` and everything else stay the layer's own."""

    def retrieve_memories(self, hidden_states: torch.Tensor, k: int = 5, reinforce: Optional[float] = None,
                          reinforce_cap: float = 1.0, *, diversity: Optional[float] = None,
                          max_similarity: Optional[float] = None, fetch_k: Optional[int] = None, tags=None,
                          newer_than: Optional[float] = None, older_than: Optional[float] = None,
                          min_strength: Optional[float] = None, lengths=None):
        """``lengths`` [B]: right-padded rows; the query is each row's mean over its own positions."""
        pooled = hidden_states.mean(dim=1) if lengths is None else masked_mean(hidden_states, lengths)
        query = self.query_proj(pooled)
        return retrieve_memories(self.hippocampus, query, k=k, dtype=hidden_states.dtype, reinforce=reinforce,
                                 reinforce_cap=reinforce_cap, diversity=diversity, max_similarity=max_similarity,
                                 fetch_k=fetch_k, tags=tags, newer_than=newer_than, older_than=older_than,
                                 min_strength=min_strength)

    def store_memory(self, hidden_states: torch.Tensor, merge_similarity: Optional[float] = None, tag=None,
                     merge_within_tags: Optional[bool] = None, merge_blend: Optional[float] = None):
        return store_memory(self.hippocampus, hidden_states, event_tag=f"layer_{id(self)}",
                            merge_similarity=merge_similarity, tag=tag, merge_within_tags=merge_within_tags,
                            merge_blend=merge_blend)

    def consolidate_memory(self, similarity: Optional[float] = None, within_tags: Optional[bool] = None,
                           blend: Optional[float] = None):
        """Merge the near-copies the bank holds (``HippocampalFormation.consolidate``); ``within_tags`` (None: the
        bank's default): only among memories of one tag; ``blend`` (None: the bank's default): the rate at which a
        kept memory moves toward the rows merged into it."""
        kw = {} if within_tags is None else dict(within_tags=within_tags)
        if blend is not None:
            kw["blend"] = blend
        return self.hippocampus.consolidate(similarity=similarity, **kw)

    def replay_memories(self, n: int, **kw):
        """``(features [n, D], rows int32 [n])``: ``n`` held memories drawn by priority for a sleep phase
        (``HippocampalFormation.replay`` and its keywords: scope, ``alpha``, ``seed`` / ``draw``, ``reinforce``,
        ``touch``); zeros / ``-1`` where the scope held fewer."""
        s = self.hippocampus.replay(n, **kw)
        return s.features, s.rows
