"""Synapsis: dense synapse ``currents = W . spikes + b`` over a flattened (B*T, in) batch.

API-compatible with the reference's ``src/core/language_zone/synapsis.py`` (constructor keywords,
``weight`` / ``bias`` parameter names, ``(currents, state)`` return, optional trace state).  The
contraction is a plain library GEMM on the matrix cores ("only the
T-dedup is new" -- that lives in ``SNNFFN``).  The one hand-written kernel behind this module is the timestep STDP of
``stdp_update`` (``csrc/aura_stdp.hip``); ``apply_stdp_update`` stays the reference's rate rule on time-mean activity.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops

Trace = Tuple[torch.Tensor, torch.Tensor]


class StdpState(NamedTuple):
    """The carried traces of ``Synapsis.stdp_update``: ``x`` [B, in] of the inputs, ``y`` [B, out] of the outputs (fp32)."""
    x: torch.Tensor
    y: torch.Tensor


class Synapsis(nn.Module):
    def __init__(self, in_features, out_features, enable_plasticity=False, stdp_lr=0.001,
                 trace_decay=0.95, target_firing_rate=0.3, bias=True, stdp_a_plus=1.0, stdp_a_minus=1.05,
                 stdp_tau_decay=None, stdp_bounds=(-10.0, 10.0)):
        super().__init__()
        # timestep STDP (stdp_update): amplitudes, trace decay per step -- None: trace_decay for both traces, a number
        # for both, or a (pre, post) pair -- and the weight clip (the reference's [-10, 10])
        self.stdp_a_plus, self.stdp_a_minus = float(stdp_a_plus), float(stdp_a_minus)
        self.stdp_tau_decay = stdp_tau_decay
        self.stdp_bounds = (float(stdp_bounds[0]), float(stdp_bounds[1]))
        if not self.stdp_bounds[0] <= self.stdp_bounds[1]:
            raise ValueError(f"stdp_bounds={stdp_bounds}: the lower bound exceeds the upper")
        self.in_features, self.out_features = in_features, out_features
        self.enable_plasticity, self.stdp_lr = enable_plasticity, stdp_lr
        self.trace_decay, self.target_firing_rate = trace_decay, target_firing_rate
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.register_parameter('bias', nn.Parameter(torch.empty(out_features)) if bias else None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        # spiking-regime init: sparser input spikes (lower firing rate) get larger weights
        nn.init.normal_(self.weight, 0.0, 1.0 / math.sqrt(self.in_features * self.target_firing_rate))
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _fresh_traces(self, like: torch.Tensor, batch: int) -> Trace:
        def z(n):
            return torch.zeros(batch, n, device=like.device, dtype=like.dtype)
        return z(self.in_features), z(self.out_features)

    def forward(self, spikes: torch.Tensor, state: Optional[Trace] = None):
        batch, steps, _ = spikes.shape
        currents = F.linear(spikes.reshape(batch * steps, self.in_features), self.weight, self.bias)
        currents = currents.reshape(batch, steps, self.out_features)
        if not self.enable_plasticity:
            return currents, None
        pre, post = state if state is not None else self._fresh_traces(spikes, batch)
        return currents, self._update_traces(spikes, currents, (pre, post))

    def _update_traces(self, pre_spikes, post_currents, state: Trace) -> Trace:
        """Exponential moving averages of the time-mean pre / post activity."""
        keep, take = self.trace_decay, 1 - self.trace_decay
        return (keep * state[0] + take * pre_spikes.mean(dim=1),
                keep * state[1] + take * post_currents.mean(dim=1))

    def apply_stdp_update(self, pre_trace, post_trace) -> None:
        """dW = lr * outer(mean post trace, mean pre trace), weights clipped to [-10, 10]."""
        if self.enable_plasticity:
            with torch.no_grad():
                self.weight.add_(self.stdp_lr * torch.outer(post_trace.mean(dim=0), pre_trace.mean(dim=0)))
                self.weight.clamp_(-10.0, 10.0)

    def stdp_decays(self) -> Tuple[float, float]:
        """``(lambda_pre, lambda_post)`` of ``stdp_update``."""
        d = self.trace_decay if self.stdp_tau_decay is None else self.stdp_tau_decay
        if isinstance(d, (tuple, list)):
            return float(d[0]), float(d[1])
        return float(d), float(d)

    def stdp_update(self, pre: torch.Tensor, post: torch.Tensor, state: Optional[StdpState] = None, *,
                    apply: bool = True, return_dw: bool = False):
        """Timestep STDP (the rule: ``include/aura_hip.h``, "STDP") from the activity on both sides of this synapse, in
        one fused HIP launch plus a small reduction: ``pre`` [B, T, in] (or [B, in]: an input that is the same at every
        step), ``post`` [B, T, out], fp32 or bf16 alike; ``state`` the ``StdpState`` of the previous call (``None``:
        zero traces).  Returns ``(StdpState, dW or None)``.  ``apply``: ``weight`` becomes
        ``clamp(weight + stdp_lr * dW, *stdp_bounds)`` in place; ``apply=False, return_dw=True`` hands back the raw dW
        (for a caller that gates it, say with a reward, before adding it).  Runs under ``no_grad``.  With
        ``enable_plasticity=False`` it returns ``(None, None)`` and launches nothing, as ``apply_stdp_update`` does."""
        if not self.enable_plasticity:
            return None, None
        if not apply and not return_dw:
            raise ValueError("Synapsis.stdp_update: apply=False needs return_dw=True (nothing would be computed)")
        if self.weight.dtype != torch.float32:
            raise TypeError(f"Synapsis.stdp_update needs an fp32 weight, got {self.weight.dtype}: keep fp32 master "
                            f"weights for plasticity and cast a copy for the forward pass")
        lam_pre, lam_post = self.stdp_decays()
        x_in, y_in = (None, None) if state is None else (state[0], state[1])
        with torch.no_grad():
            dw = torch.empty_like(self.weight) if return_dw else None
            x, y = ops.stdp_update(pre.detach(), post.detach(), x_in, y_in, self.weight if apply else None, dw,
                                   lambda_pre=lam_pre, lambda_post=lam_post, a_plus=self.stdp_a_plus,
                                   a_minus=self.stdp_a_minus, lr=self.stdp_lr, w_min=self.stdp_bounds[0],
                                   w_max=self.stdp_bounds[1], pre_time_invariant=pre.dim() == 2)
            if apply:
                # the kernel wrote through the data pointer: count it as the in-place op it is
                torch.autograd.graph.increment_version(self.weight)
        return StdpState(x, y), dw

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"plasticity={self.enable_plasticity}, bias={self.bias is not None}")
