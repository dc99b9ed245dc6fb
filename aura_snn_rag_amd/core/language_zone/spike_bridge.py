"""The bridges between spike trains and continuous features behind the reference's names
(``src/core/language_zone/spike_bridge.py``), from torch ops: they are a reduction over a short window and one small
linear, which the library already does well.  ``proj`` is an ``nn.Linear`` (or ``nn.Identity`` when the sizes agree), so
the ``state_dict`` keys are the reference's.

The Poisson draw of ``ContinuousToSpikeBridge`` comes two ways.  Without a seed it is ``torch.rand`` under torch's
generator, as in the reference: it depends on the call's shape and on the generator's history.  With ``seed=`` it is
``ops.poisson_rate`` (``csrc/aura_bridge.hip``; the rule: ``include/aura_hip.h``, "Poisson bridge"): the projection, the
sigmoid, a Philox draw keyed by (channel, timestep, position, stream) and, for ``rate_code``, the mean over the
timesteps in one launch, so that a token's spikes are the same in a forward over a sequence and in a one-token step.
The comparison carries no autograd history in the reference either; the seeded path is a constant and has no
backward."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ... import ops


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
    else: no spikes.  ``forward(x, seed=, streams=, rows_per_stream=, start=)`` ('poisson' with a projection only)
    returns the seeded train; ``rate_code`` its mean over the timesteps."""

    def __init__(self, input_dim, spike_dim, encoding='poisson', num_timesteps=10):
        super().__init__()
        self.encoding = encoding
        self.num_timesteps = num_timesteps
        self.proj = nn.Linear(input_dim, spike_dim) if input_dim != spike_dim else nn.Identity()

    def _seeded(self, who: str, x: torch.Tensor, seed, streams, rows_per_stream, start, **outputs):
        if self.encoding != 'poisson':
            raise ValueError(f"ContinuousToSpikeBridge.{who}: a seed goes with encoding='poisson', this bridge has "
                             f"encoding={self.encoding!r}")
        if not isinstance(self.proj, nn.Linear):
            raise ValueError(f"ContinuousToSpikeBridge.{who}: the seeded draw is fused with the projection; this bridge "
                             f"has none (input_dim == spike_dim)")
        with torch.no_grad():
            bias = None if self.proj.bias is None else self.proj.bias.detach()
            return ops.poisson_rate(x.detach().contiguous(), self.proj.weight.detach(), bias, T=self.num_timesteps,
                                    seed=seed, streams=streams, rows_per_stream=rows_per_stream, start=start, **outputs)

    def rate_code(self, x: torch.Tensor, *, seed: int, streams=None, rows_per_stream: Optional[int] = None,
                  start=0) -> torch.Tensor:
        """``x`` [N, input_dim] -> [N, spike_dim]: the mean over the timesteps of the seeded train, the bits of
        ``forward(x, seed=..).mean(dim=1)``, in one launch that writes neither the uniforms nor the train.  The
        arguments are ``ops.poisson_rate``'s."""
        return self._seeded("rate_code", x, seed, streams, rows_per_stream, start)

    def forward(self, x: torch.Tensor, *, seed: Optional[int] = None, streams=None,
                rows_per_stream: Optional[int] = None, start=0) -> torch.Tensor:
        if seed is not None:
            return self._seeded("forward", x, seed, streams, rows_per_stream, start, return_spikes=True)[1]
        if streams is not None or rows_per_stream is not None or not (isinstance(start, int) and start == 0):
            raise ValueError("ContinuousToSpikeBridge.forward: streams, rows_per_stream and start go with a seed")
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
