"""``MoELanguageZone`` behind the reference's name (``src/core/language_zone/moe_language_zone.py``): embeddings, a GIF
encoder, the spike-to-continuous bridge, the liquid router over ``num_experts`` ``SNNExpert`` modules, the
continuous-to-spike bridge, a GIF decoder and the output projection.  The reference's constructor, attribute names and
``state_dict`` keys; ``forward(input_ids, attention_mask=None) -> (logits, {'probs': ...})``.

The reference runs every expert that any token selected over all ``B S`` tokens, about ten launches per expert, and
masks the result.  Here, when autograd is not recording, ``route_experts`` is five launches in all (``ops.moe_route``,
``ops.moe_experts``; the rule: ``include/aura_hip.h``, "MoE zone"): each expert runs on its own tokens only, with the
activations in LDS.  When autograd is recording, ``route_experts`` is ``route_experts_composed``: the same modules from
torch ops and the differentiable ``GIFNeuron``, each expert on its gathered tokens, so training works.

Not here: ``T > 1`` or carried state in the fused experts, bf16, a fused backward, ``generate``."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from ... import ops
from ..liquid_moe import LiquidMoERouter, _recording
from .gif_neuron import GIFNeuron
from .snn_expert import SNNExpert
from .spike_bridge import ContinuousToSpikeBridge, SpikeToContinuousBridge


class MoEOutput(NamedTuple):
    """``expert_outputs`` [N, Dm] the weighted sum; ``indices`` int64 [N, k]; ``weights`` [N, k]; ``probs`` [N, E];
    ``trace`` (``return_trace``) [N, k, layers, Hh] every layer's spikes of every (token, slot) pair, else ``None``;
    ``pair_outputs`` [N, k, Dm] every pair's expert output (fused path) or ``None``."""
    expert_outputs: torch.Tensor
    indices: torch.Tensor
    weights: torch.Tensor
    probs: torch.Tensor
    trace: Optional[torch.Tensor] = None
    pair_outputs: Optional[torch.Tensor] = None


class MoELanguageZone(nn.Module):
    def __init__(self, vocab_size: int, embed_dim: int, hidden_dim: int, num_experts: int = 8, top_k: int = 2,
                 moe_hidden_dim: int = 64):
        super().__init__()
        self.vocab_size = vocab_size
        self.embed_dim = embed_dim
        self.hidden_dim = hidden_dim
        self.moe_hidden_dim = moe_hidden_dim
        self.top_k = top_k
        self.num_experts = num_experts
        self.embeddings = nn.Embedding(vocab_size, embed_dim)
        self.encoder = GIFNeuron(embed_dim, hidden_dim, L=16)
        self.spike_to_continuous = SpikeToContinuousBridge(spike_dim=hidden_dim, output_dim=moe_hidden_dim,
                                                           encoding='rate', time_window=10)
        self.experts = nn.ModuleDict({
            f'expert_{i}': SNNExpert(input_dim=moe_hidden_dim, hidden_dim=hidden_dim // 2, output_dim=moe_hidden_dim)
            for i in range(num_experts)})
        self.moe_router = LiquidMoERouter(in_dim=moe_hidden_dim, hidden_dim=64, num_experts=num_experts, top_k=top_k)
        self.continuous_to_spike = ContinuousToSpikeBridge(input_dim=moe_hidden_dim, spike_dim=hidden_dim,
                                                           encoding='poisson')
        self.decoder = GIFNeuron(hidden_dim, embed_dim, L=16)
        self.output_proj = nn.Linear(embed_dim, vocab_size)
        self._table = None
        self._table_key = None

    # ---- the experts' pointer table --------------------------------------------------------------------------------
    def expert_table(self) -> "ops.MoeExpertTable":
        """The device table of the experts' parameter pointers, kept between calls and rebuilt when a parameter was
        written in place (``_version``), re-allocated or moved, or a neuron's setting changed."""
        tensors, gif = [], []
        for i in range(self.num_experts):
            t, g = self.experts[f'expert_{i}'].fused_parameters()
            tensors.append(t)
            gif.append(g)
        key = (tuple((p._version, p.data_ptr(), p.device) for ts in tensors for p in ts), tuple(map(tuple, gif)))
        if self._table is None or key != self._table_key:
            self._table = ops.moe_expert_table([[p.detach() for p in ts] for ts in tensors], gif)
            self._table_key = key
        return self._table

    # ---- routing and experts ---------------------------------------------------------------------------------------
    def route_experts(self, continuous: torch.Tensor, attn_gain: Optional[torch.Tensor] = None,
                      return_trace: bool = False) -> MoEOutput:
        """Router, selected experts and weighted sum on ``continuous`` [N, moe_hidden_dim]."""
        if _recording(self, continuous, attn_gain):
            if return_trace:
                raise ValueError("MoELanguageZone.route_experts: the trace is written by the fused launch; call it "
                                 "under torch.no_grad()")
            return self.route_experts_composed(continuous, attn_gain)
        with torch.no_grad():
            x = continuous.detach().contiguous()
            routing = self.moe_router.route(x, attn_gain)
            out, y, trace = ops.moe_experts(x, routing, self.expert_table(), return_trace=return_trace)
        return MoEOutput(out, routing.indices.long(), routing.weights, routing.probs, trace, y)

    def route_experts_composed(self, continuous: torch.Tensor, attn_gain: Optional[torch.Tensor] = None,
                               routing: Optional[Dict[str, torch.Tensor]] = None) -> MoEOutput:
        """The same from torch ops and this package's modules (differentiable): every selected expert's ``predict`` on
        its gathered tokens, added in ascending expert id.  ``routing``: a router's dict to use instead of routing."""
        route = routing if routing is not None else self.moe_router.compose(continuous, attn_gain)
        idx, w = route['indices'], route['weights']
        out = torch.zeros(continuous.shape[0], self.moe_hidden_dim, device=continuous.device, dtype=continuous.dtype)
        for i in range(self.num_experts):
            chosen = idx == i
            rows = torch.nonzero(chosen.any(dim=1)).flatten()
            if rows.numel() == 0:
                continue
            y = self.experts[f'expert_{i}'].predict(continuous.index_select(0, rows))
            wi = (w * chosen.to(w.dtype)).sum(dim=1).index_select(0, rows)
            out = out.index_add(0, rows, y * wi.unsqueeze(1))
        return MoEOutput(out, idx, w, route['probs'])

    # ---- the model -------------------------------------------------------------------------------------------------
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                keep_on_device: bool = False) -> Tuple[torch.Tensor, Dict]:
        B, S = input_ids.shape
        spikes, _ = self.encoder(self.embeddings(input_ids))
        continuous = self.spike_to_continuous(spikes.reshape(B * S, 1, self.hidden_dim))
        moe = self.route_experts(continuous)
        spikes_moe = self.continuous_to_spike(moe.expert_outputs)
        steps = spikes_moe.shape[1]
        decoded, _ = self.decoder(spikes_moe.view(B, S, steps, self.hidden_dim).mean(dim=2))
        logits = self.output_proj(decoded)
        probs = moe.probs.view(B, S, -1).detach()
        return logits, {'probs': probs if keep_on_device else probs.cpu()}

    def setup_moe_router(self, *args, **kwargs):
        pass

    def forward_async(self, *args, **kwargs):
        raise DeprecationWarning("MoELanguageZone.forward_async is gone: forward() runs on the GPU")
