"""PlaceCellSemanticEncoder: tokens -> sparse place-cell code -> semantic embedding.

API-compatible with the reference's ``src/core/language_zone/place_cell_encoder.py`` (constructor, ``state_dict`` keys,
``sparsity`` / ``k``, ``forward`` returning ``(semantic_embedding, place_cell_activity)``, ``get_place_cell_pattern``,
``extra_repr``).  The embedding lookup and ``Linear(D -> P)`` stay torch (a table read and a library GEMM); everything
after the logits -- the reference's ``topk``, ``sigmoid``, ``zeros_like``, ``scatter``, the dense ``Linear(P -> D)`` over
a 97 %-zero tensor and the residual -- is one HIP launch (``csrc/aura_place.hip``; the rule: ``include/aura_hip.h``,
"Place code"), and its backward another.  Where the reference's ``torch.topk`` leaves the order of equal logits open,
the lower cell index wins here.

New on this module: ``forward_sparse`` (the code as ``PlaceCode(indices, values, n_cells)``; no [N, P] tensor is
written) and ``encode_logits`` for callers that hold logits already.  fp32 only; CPU tensors raise ``AuraDeviceError``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from ... import ops


class PlaceCode(NamedTuple):
    """A sparse place-cell code: per token the ``k`` active cells in ascending order (``indices`` [..., k] int32) and
    their activations (``values`` [..., k]) out of ``n_cells``."""
    indices: torch.Tensor
    values: torch.Tensor
    n_cells: int

    def to_dense(self) -> torch.Tensor:
        """[..., n_cells]: zeros with ``values`` at ``indices`` (what ``forward`` returns as place_cell_activity)."""
        dense = torch.zeros(*self.indices.shape[:-1], self.n_cells, dtype=self.values.dtype, device=self.values.device)
        return dense.scatter(-1, self.indices.long(), self.values)


class PlaceCellSemanticEncoder(nn.Module):
    def __init__(self, config, hippocampus):
        super().__init__()
        self.config = config
        self.hippocampus = hippocampus
        self.token_embedding = nn.Embedding(config.vocab_size, config.embedding_dim)
        nn.init.normal_(self.token_embedding.weight, mean=0.0, std=0.02)
        self.semantic_projection = nn.Linear(config.embedding_dim, config.n_place_cells)
        self.place_to_semantic = nn.Linear(config.n_place_cells, config.embedding_dim)
        self.sparsity = 0.03
        self.k = int(config.n_place_cells * self.sparsity)
        if not 1 <= self.k <= ops.PLACE_MAX_K or config.n_place_cells > ops.PLACE_MAX_CELLS:
            raise ValueError(f"n_place_cells={config.n_place_cells} gives k={self.k}: the place-code kernel needs "
                             f"1 <= k <= {ops.PLACE_MAX_K} and at most {ops.PLACE_MAX_CELLS} cells")
        self._w2t: Optional[torch.Tensor] = None       # [P, D]: place_to_semantic.weight transposed, detached
        self._w2t_key = None

    def _table(self) -> torch.Tensor:
        """The [P, D] transpose of ``place_to_semantic.weight``, rebuilt when the weight was written in place
        (``_version``), re-allocated or moved."""
        w = self.place_to_semantic.weight
        key = (w._version, w.data_ptr(), w.device, w.dtype)
        if self._w2t is None or key != self._w2t_key:
            self._w2t = w.detach().t().contiguous()
            self._w2t_key = key
        return self._w2t

    def encode_logits(self, z: torch.Tensor, e: torch.Tensor, dense: bool = True):
        """From place-cell logits ``z`` [..., P] and embeddings ``e`` [..., D]: ``(semantic_embedding [..., D],
        PlaceCode, place_cell_activity [..., P] or None)``.  Differentiable in ``z``, ``e`` and the read-out's weight
        and bias."""
        P, D = self.config.n_place_cells, self.config.embedding_dim
        if z.shape[-1] != P or e.shape[-1] != D or z.shape[:-1] != e.shape[:-1]:
            raise ValueError(f"encode_logits: z [..., {P}] and e [..., {D}] with equal leading shapes; got "
                             f"{tuple(z.shape)} and {tuple(e.shape)}")
        lead = z.shape[:-1]
        w = self.place_to_semantic.weight
        out, idx, act, code = ops.PlaceCodeFunction.apply(
            z.reshape(-1, P).contiguous(), e.reshape(-1, D).contiguous(), self._table(), self.place_to_semantic.bias,
            self.k, bool(dense), w if (torch.is_grad_enabled() and w.requires_grad) else None)
        sparse = PlaceCode(idx.reshape(*lead, self.k), act.reshape(*lead, self.k), P)
        return out.reshape(*lead, D), sparse, (code.reshape(*lead, P) if dense else None)

    def _logits(self, input_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        token_embeds = self.token_embedding(input_ids)
        return self.semantic_projection(token_embeds), token_embeds

    def forward(self, input_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """input_ids [batch, seq_len] -> (semantic_embedding [batch, seq_len, D], place_cell_activity
        [batch, seq_len, P])."""
        z, e = self._logits(input_ids)
        out, _, code = self.encode_logits(z, e, dense=True)
        return out, code

    def forward_sparse(self, input_ids: torch.Tensor) -> Tuple[torch.Tensor, PlaceCode]:
        """As ``forward`` with the code left sparse: no [batch, seq_len, P] tensor is written."""
        z, e = self._logits(input_ids)
        out, sparse, _ = self.encode_logits(z, e, dense=False)
        return out, sparse

    def get_place_cell_pattern(self, token_id: int) -> torch.Tensor:
        """[n_place_cells]: the sparse activation pattern of one token."""
        input_ids = torch.tensor([[token_id]], device=next(self.parameters()).device)
        _, place_activity = self.forward(input_ids)
        return place_activity[0, 0]

    def extra_repr(self) -> str:
        return (f'vocab_size={self.config.vocab_size}, '
                f'embedding_dim={self.config.embedding_dim}, '
                f'n_place_cells={self.config.n_place_cells}, '
                f'sparsity={self.sparsity:.1%} (k={self.k})')
