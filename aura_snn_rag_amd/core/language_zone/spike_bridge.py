"""The bridges between spike trains and continuous features behind the reference's names
(``src/core/language_zone/spike_bridge.py``), from torch ops: they are a reduction over a short window and one small
linear, which the library already does well.  ``proj`` is an ``nn.Linear`` (or ``nn.Identity`` when the sizes agree), so
the ``state_dict`` keys are the reference's.  The Poisson draw is ``torch.rand`` under torch's generator."""
from __future__ import annotations

import torch
import torch.nn as nn


class SpikeToContinuousBridge(nn.Module):
    """``spikes`` [B, T, spike_dim] -> [B, output_dim].  ``encoding``: ``'rate'`` the mean of the last ``time_window``
    steps; ``'temporal'`` a mean weighted by ``exp(t / time_window)``; ``'phase'`` the mean magnitude of the window's
    spectrum; anything else the mean over all steps."""

    def __init__(self, spike_dim, output_dim, encoding='rate', time_window=10):
        super().__init__()
        self.encoding = encoding
        self.time_window = time_window
        self.proj = nn.Linear(spike_dim, output_dim) if spike_dim != output_dim else nn.Identity()

    def features(self, spikes: torch.Tensor) -> torch.Tensor:
        if self.encoding == 'rate':
            return spikes[:, -self.time_window:, :].mean(dim=1)
        if self.encoding == 'temporal':
            steps = torch.arange(spikes.shape[1], device=spikes.device).float()
            w = torch.exp(steps / self.time_window).view(1, -1, 1)
            return (spikes * w).sum(dim=1) / (w.sum() + 1e-6)
        if self.encoding == 'phase':
            return torch.abs(torch.fft.rfft(spikes[:, -self.time_window:, :], dim=1)).mean(dim=1)
        return spikes.mean(dim=1)

    def forward(self, spikes: torch.Tensor) -> torch.Tensor:
        return self.proj(self.features(spikes))


class ContinuousToSpikeBridge(nn.Module):
    """``x`` [B, input_dim] -> spikes [B, num_timesteps, spike_dim].  ``'poisson'``: a spike where a uniform draw is
    below ``sigmoid(proj(x))``; ``'temporal'``: the first ``sigmoid(proj(x)) num_timesteps`` steps spike; anything
    else: no spikes."""

    def __init__(self, input_dim, spike_dim, encoding='poisson', num_timesteps=10):
        super().__init__()
        self.encoding = encoding
        self.num_timesteps = num_timesteps
        self.proj = nn.Linear(input_dim, spike_dim) if input_dim != spike_dim else nn.Identity()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        feat = self.proj(x)
        rows, dim = feat.shape
        T = self.num_timesteps
        if self.encoding == 'poisson':
            draw = torch.rand(rows, T, dim, device=x.device, dtype=x.dtype)
            return (draw < torch.sigmoid(feat).unsqueeze(1)).to(x.dtype)
        if self.encoding == 'temporal':
            steps = torch.arange(T, device=x.device, dtype=x.dtype).view(1, -1, 1)
            return ((torch.sigmoid(feat) * T).unsqueeze(1) > steps).to(x.dtype)
        return torch.zeros(rows, T, dim, device=x.device, dtype=x.dtype)
