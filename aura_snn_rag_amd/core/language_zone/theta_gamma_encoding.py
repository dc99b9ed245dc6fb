"""ThetaGammaPositionalEncoding: positions -> theta-gamma phase code, and the two lines that consume it.

API-compatible with the reference's ``src/core/language_zone/theta_gamma_encoding.py`` (constructor, the parameters and
``state_dict`` keys ``theta_phase_offsets`` / ``gamma_phase_offsets`` / ``amplitude_modulation`` with their
initialisation, ``embedding_dim`` / ``theta_freq`` / ``gamma_freq`` / ``max_seq_len``, ``forward(positions,
seq_length)``, ``extra_repr``).  ``forward`` is the table kernel of ``csrc/aura_theta.hip`` (the rule:
``include/aura_hip.h``, "Theta-gamma"): one sine / cosine evaluation per (position, column), never per token.

New on this module: ``encode_add_norm(hidden, norm, ..)`` -- ``LayerNorm(hidden + pe)``, the next two lines of both
reference models' ``forward``, in one launch that never writes ``hidden + pe`` -- and the module-level ``embed_tokens``,
a model's whole front end (tokens to first hidden state) on the package's own kernels.  fp32 only; CPU tensors raise
``AuraDeviceError``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ... import ops


class _PhaseTable(torch.autograd.Function):
    """``pe`` [R, D] at explicit fp32 positions [R], differentiable in the three parameters: the gradient is the
    derivative tables of a second table call times ``g``, summed over the rows (small tensors, torch ops)."""

    @staticmethod
    def forward(ctx, positions, theta_off, gamma_off, amp, max_seq_len: int, ratio: float):
        ctx.save_for_backward(positions, theta_off, gamma_off, amp)
        ctx.geometry = (max_seq_len, ratio)
        return ops.theta_gamma_table(theta_off, gamma_off, amp, max_seq_len, ratio, positions=positions)

    @staticmethod
    def backward(ctx, g):
        positions, theta_off, gamma_off, amp = ctx.saved_tensors
        if not any(ctx.needs_input_grad[1:4]):
            return (None,) * 6
        derivs = ops.theta_gamma_table(theta_off, gamma_off, amp, *ctx.geometry, positions=positions, derivatives=True,
                                       pe=False)[1:]
        grads = [(g * d).sum(0) if need else None for d, need in zip(derivs, ctx.needs_input_grad[1:4])]
        return (None, *grads, None, None)


class ThetaGammaPositionalEncoding(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.embedding_dim = config.embedding_dim
        self.theta_freq = float(config.theta_frequency)
        self.gamma_freq = float(config.gamma_frequency)
        self.theta_phase_offsets = nn.Parameter(torch.randn(config.embedding_dim) * 0.1)
        self.gamma_phase_offsets = nn.Parameter(torch.randn(config.embedding_dim) * 0.1)
        # the phase of a position is fixed by max_seq_len, not by the length of a call: stable during generation
        self.max_seq_len = getattr(config, 'max_seq_len', 512)
        self.amplitude_modulation = nn.Parameter(torch.ones(config.embedding_dim))
        if not 1 <= self.embedding_dim <= ops.THETA_MAX_D:
            raise ValueError(f"embedding_dim={self.embedding_dim}: the theta-gamma kernels need 1 <= D <= "
                             f"{ops.THETA_MAX_D}")
        self._pe: Optional[torch.Tensor] = None         # [S, D] for positions start .. start + S - 1, detached
        self._pe_key = None

    def _params(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.theta_phase_offsets, self.gamma_phase_offsets, self.amplitude_modulation

    def _geometry(self) -> Tuple[int, float]:
        return int(self.max_seq_len), ops.theta_gamma_ratio(self.theta_freq, self.gamma_freq)

    def forward(self, positions: torch.Tensor, seq_length: int) -> torch.Tensor:
        """positions [...] (integer or float) -> [..., D].  ``seq_length`` is ignored, as upstream: the phase is
        normalised by ``max_seq_len``.  Differentiable in the three parameters."""
        flat = positions.reshape(-1).to(torch.float32).contiguous()
        pe = _PhaseTable.apply(flat, *self._params(), *self._geometry())
        return pe.reshape(*positions.shape, self.embedding_dim)

    def _range_table(self, start: int, S: int) -> torch.Tensor:
        """The detached [S, D] table of positions ``start .. start + S - 1``.  Kept between calls under ``no_grad``
        and rebuilt when a parameter was written in place (``_version``), re-allocated or moved."""
        max_seq_len, ratio = self._geometry()
        params = tuple(p.detach() for p in self._params())
        build = lambda: ops.theta_gamma_table(*params, max_seq_len, ratio, start=start, rows=S)
        if torch.is_grad_enabled():
            return build()
        key = (start, S, max_seq_len, ratio) + tuple((p._version, p.data_ptr(), p.device) for p in self._params())
        if self._pe is None or key != self._pe_key:
            self._pe = build()
            self._pe_key = key
        return self._pe

    def encode_add_norm(self, hidden: torch.Tensor, norm: nn.LayerNorm, positions: Optional[torch.Tensor] = None,
                        start: int = 0) -> torch.Tensor:
        """``norm(hidden + pe)`` for ``hidden`` [B, S, D] in one launch.  ``positions``: ``None`` for ``start,
        start + 1, ..``; [S] or [1, S] shared by the batch; [B, S] per item (integer or float).  Differentiable in
        ``hidden``, the three parameters, ``norm.weight`` and ``norm.bias``."""
        D = self.embedding_dim
        if not isinstance(norm, nn.LayerNorm) or tuple(norm.normalized_shape) != (D,) or norm.weight is None \
                or norm.bias is None:
            raise TypeError(f"encode_add_norm: norm must be an nn.LayerNorm(({D},)) with weight and bias, got {norm!r}")
        if hidden.dim() != 3 or hidden.shape[-1] != D:
            raise ValueError(f"encode_add_norm: hidden is [B, S, {D}], got {tuple(hidden.shape)}")
        B, S, _ = hidden.shape
        max_seq_len, ratio = self._geometry()
        if positions is None:
            if isinstance(start, bool) or not isinstance(start, int):
                raise TypeError(f"encode_add_norm: start must be an int, got {type(start)}")
            flat = None
            table = self._range_table(start, S)
        else:
            if start != 0:
                raise ValueError("encode_add_norm: give positions or start, not both")
            if tuple(positions.shape) in ((S,), (1, S)) or tuple(positions.shape) == (B, S):
                flat = positions.reshape(-1).to(torch.float32).contiguous()
            else:
                raise ValueError(f"encode_add_norm: positions is [{S}], [1, {S}] or [{B}, {S}], got "
                                 f"{tuple(positions.shape)}")
            table = ops.theta_gamma_table(*(p.detach() for p in self._params()), max_seq_len, ratio, positions=flat)
        y = ops.ThetaGammaNormFunction.apply(hidden.reshape(B * S, D).contiguous(), table, *self._params(),
                                             norm.weight, norm.bias, S, float(norm.eps),
                                             (flat, start, max_seq_len, ratio))
        return y.reshape(B, S, D)

    def extra_repr(self) -> str:
        return (f'embedding_dim={self.embedding_dim}, '
                f'theta_freq={self.theta_freq:.1f}Hz, '
                f'gamma_freq={self.gamma_freq:.1f}Hz')


def embed_tokens(input_ids: torch.Tensor, semantic_encoder, pos_encoder: ThetaGammaPositionalEncoding,
                 norm: nn.LayerNorm, start: int = 0, dense: bool = True, positions: Optional[torch.Tensor] = None):
    """The front end of both reference models, tokens to first hidden state (up to, not including, dropout):
    ``semantic, code = semantic_encoder(input_ids)``, ``hidden = norm(semantic + pos_encoder(arange(S)))``.  Returns
    ``(hidden [B, S, D], place_cell_activity [B, S, P])``, or with ``dense=False`` the code as a ``PlaceCode``.
    ``positions`` [B, S] (instead of ``start``) gives every row its own positions, as ``encode_add_norm`` takes them."""
    semantic, code = semantic_encoder(input_ids) if dense else semantic_encoder.forward_sparse(input_ids)
    if positions is not None:
        return pos_encoder.encode_add_norm(semantic, norm, positions=positions), code
    return pos_encoder.encode_add_norm(semantic, norm, start=start), code
