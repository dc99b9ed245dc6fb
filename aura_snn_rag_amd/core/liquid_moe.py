"""Liquid MoE routing behind the reference's names (``src/core/liquid_moe.py``): ``LiquidCellConfig``, ``LiquidCell``,
``LiquidMoERouter`` and its alias ``LiquidGatingNetwork``, with the reference's constructors, attribute names and
``state_dict`` keys.  ``BanditGating`` (host NumPy) is not part of this package.

When autograd is not recording, ``LiquidMoERouter`` is the fused ``ops.moe_route`` (the rule: ``include/aura_hip.h``,
"MoE zone"): one launch for logits, softmax, top-k and weights, two more for the plan that ``ops.moe_experts`` reads.
The router's state starts at zero, so the time constant (``V``, softplus, clamp) and ``W.weight`` cannot reach its
output and are not read.  When autograd is recording, the same module is the composition from torch ops below, ``V``
path included, so training works and every parameter the reference trains receives its gradient."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


@dataclass
class LiquidCellConfig:
    in_dim: int
    hidden_dim: int
    dt: float = 0.02
    tau_min: float = 0.02
    tau_max: float = 2.0


class LiquidCell(nn.Module):
    """One Euler step of a liquid time-constant cell: ``h' = h + dt (-h / (tau(x) + 1e-6) + tanh(W h + U x))`` with
    ``tau(x) = min(tau_min + softplus(V x), tau_max)``.  ``h_prev=None`` is the zero state."""

    def __init__(self, config: LiquidCellConfig):
        super().__init__()
        self.hidden_dim = config.hidden_dim
        self.dt = config.dt
        self.tau_min = config.tau_min
        self.tau_max = config.tau_max
        self.W = nn.Linear(config.hidden_dim, config.hidden_dim)
        self.U = nn.Linear(config.in_dim, config.hidden_dim)
        self.V = nn.Linear(config.in_dim, config.hidden_dim)
        for lin in (self.W, self.U, self.V):
            nn.init.xavier_uniform_(lin.weight)

    def forward(self, x: torch.Tensor, h_prev: Optional[torch.Tensor] = None) -> torch.Tensor:
        if h_prev is None:
            h_prev = x.new_zeros(x.size(0), self.hidden_dim)
        tau = torch.clamp(self.tau_min + F.softplus(self.V(x)), max=self.tau_max)
        gates = torch.tanh(self.W(h_prev) + self.U(x))
        return h_prev + self.dt * (-h_prev / (tau + 1e-6) + gates)


def _recording(module: nn.Module, *tensors) -> bool:
    if not torch.is_grad_enabled():
        return False
    return any(t is not None and t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters())


class LiquidMoERouter(nn.Module):
    def __init__(self, in_dim: int, hidden_dim: int, num_experts: int, top_k: int = 2):
        super().__init__()
        self.top_k = top_k
        self.num_experts = num_experts
        self.config = LiquidCellConfig(in_dim, hidden_dim)
        self.cell = LiquidCell(self.config)
        self.gate_proj = nn.Linear(hidden_dim, num_experts)
        self.register_buffer('expert_usage', torch.zeros(num_experts))
        self.temperature = 1.0

    @property
    def k(self) -> int:
        return min(self.top_k, self.num_experts)

    def _gain(self, x, attn_gain):
        if attn_gain is None:
            return None
        if attn_gain.dim() == 2 and attn_gain.shape[1] == 1:
            attn_gain = attn_gain[:, 0]
        if attn_gain.dim() != 1 or attn_gain.shape[0] != x.shape[0]:
            raise ValueError(f"LiquidMoERouter: attn_gain is one gain per row ([N] or [N, 1]), got {tuple(attn_gain.shape)}")
        return attn_gain.detach().to(torch.float32).contiguous()

    def route(self, x: torch.Tensor, attn_gain: Optional[torch.Tensor] = None) -> "ops.MoeRouting":
        """The fused router on ``x`` [N, in_dim] (no autograd): ``ops.MoeRouting`` with int32 ``indices`` and the plan
        of the expert launch.  Updates ``expert_usage`` when training."""
        with torch.no_grad():
            routing = ops.moe_route(x.detach().contiguous(), self.cell.U.weight.detach(), self.cell.U.bias.detach(),
                                    self.cell.W.bias.detach(), self.gate_proj.weight.detach(),
                                    self.gate_proj.bias.detach(), dt=float(self.cell.dt), k=self.k,
                                    temperature=float(self.temperature), attn_gain=self._gain(x, attn_gain))
            if self.training:
                self._count(routing.indices, x.size(0))
        return routing

    def _count(self, indices: torch.Tensor, rows: int) -> None:
        """The running share of tokens per expert: 0.99 of the old value and 0.01 of this batch's."""
        batch = torch.zeros_like(self.expert_usage)
        flat = indices.reshape(-1).long()
        batch.index_add_(0, flat, torch.ones(flat.numel(), device=flat.device, dtype=batch.dtype))
        self.expert_usage.mul_(0.99).add_(batch / max(rows, 1), alpha=0.01)

    def compose(self, x: torch.Tensor, attn_gain: Optional[torch.Tensor] = None) -> Dict[str, Any]:
        """The router from torch ops (differentiable; the time-constant path included)."""
        logits = self.gate_proj(self.cell(x, h_prev=None))
        if attn_gain is None:
            logits = logits / self.temperature
        else:
            gain = attn_gain.unsqueeze(1) if attn_gain.dim() == 1 else attn_gain
            logits = logits / torch.clamp(self.temperature / (gain + 1e-6), min=0.1, max=5.0)
        probs = F.softmax(logits, dim=-1)
        top_p, top_i = torch.topk(probs, self.k, dim=-1)
        weights = top_p / (top_p.sum(dim=-1, keepdim=True) + 1e-8)
        if self.training:
            with torch.no_grad():
                self._count(top_i, x.size(0))
        return {'weights': weights, 'indices': top_i, 'probs': probs}

    def forward(self, x: torch.Tensor, attn_gain: Optional[torch.Tensor] = None) -> Dict[str, Any]:
        if _recording(self, x, attn_gain):
            return self.compose(x, attn_gain)
        r = self.route(x, attn_gain)
        return {'weights': r.weights, 'indices': r.indices.long(), 'probs': r.probs}


class LiquidGatingNetwork(LiquidMoERouter):
    """The older name of ``LiquidMoERouter``."""
