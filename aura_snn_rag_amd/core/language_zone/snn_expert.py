"""``SNNExpert`` behind the reference's name (``src/core/language_zone/snn_expert.py``): ``num_layers`` pairs of
``Synapsis`` and ``GIFNeuron`` in ``layers`` and a ``readout`` linear over the time-mean spikes; the same constructor and
``state_dict`` keys.  ``forward`` and ``predict`` run from this package's modules (the GIF loop is the HIP kernel, its
gradient the surrogate kernels).  Inside ``MoELanguageZone`` with autograd off, ``predict`` of all experts on their own
tokens is one fused launch instead (``ops.moe_experts``), which reads this module's parameters where they are:
``fused_parameters`` lists them."""
from __future__ import annotations

from typing import Any, List, Optional

import torch
import torch.nn as nn

from .gif_neuron import GIFNeuron
from .synapsis import Synapsis


class SNNExpert(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim=1, num_layers=2, L=16):
        super().__init__()
        layers = []
        for i in range(num_layers):
            layers.append(Synapsis(input_dim if i == 0 else hidden_dim, hidden_dim))
            layers.append(GIFNeuron(hidden_dim, hidden_dim, L=L))
        self.layers = nn.ModuleList(layers)
        self.readout = nn.Linear(hidden_dim, output_dim)

    def forward(self, x: torch.Tensor, states: Optional[List[Any]] = None) -> torch.Tensor:
        """``x`` [B, T, input_dim]; ``states``: one entry per layer or ``None`` (fresh state).  Returns [B, output_dim]."""
        h = x
        for i, layer in enumerate(self.layers):
            h, _ = layer(h, state=states[i] if states else None)
        return self.readout(h.mean(dim=1))

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """One step from fresh state: ``x`` [B, input_dim] (or [B, T, input_dim])."""
        return self.forward(x.unsqueeze(1) if x.dim() == 2 else x, states=None)

    def fused_parameters(self):
        """``(tensors, neuron settings)`` in the order of ``ops.moe_expert_table``."""
        tensors, gif = [], []
        for syn, neuron in zip(self.layers[0::2], self.layers[1::2]):
            tensors += [syn.weight, syn.bias, neuron.linear.weight, neuron.linear.bias]
            gif.append((float(neuron.decay), int(neuron.L), float(neuron.alpha), float(neuron.threshold)))
        tensors += [self.readout.weight, self.readout.bias]
        return tensors, gif
