"""Prosody attention: token ids -> the attention gains that ``ProsodyModulatedGIF`` consumes.

API-compatible with the reference's ``src/core/language_zone/multi_channel_attention.py`` and ``prosody_attention.py``:
``MultiChannelSpikingAttention`` (constructor, the ``decay`` / ``weights`` buffers and with them the ``state_dict`` keys,
``forward(amp, pitch, boundary)`` and its dict ``mu_scalar`` / ``salience`` / ``winners``), ``prosody_channels_from_text``
and ``ProsodyAttentionBridge(k_winners)`` with ``forward(input_ids, token_strings=None) -> (attention_gains, result)``.
Everything runs in the one launch of ``csrc/aura_prosody.hip`` (the rule: ``include/aura_hip.h``, "Prosody attention"):
the bridge goes from ids to gains without a [B, S] intermediate passing through torch.  Forward only, as upstream (the
spikes are a comparison); fp32 only; CPU tensors raise ``AuraDeviceError``.

Where the reference leaves something open, the rule fixes it: among equal salience values the lower position wins, and
``winners`` come in rank order.  New here: ``lengths`` (rows that end early), ``state`` (the three membranes, carried
between calls), the ``attention_preset`` keyword of the bridge, and the extra entries ``gains``, ``state`` and (on
request) ``spikes`` of the result dict.

Chunked use: feeding a sequence in pieces, each call's ``result['state']`` passed to the next, gives the spikes of the
whole run bit for bit.  Salience normalisation, smoothing at the chunk's edges, winners, ``mu_scalar`` and the gains are
per call by definition: they describe the piece they were computed on.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from ... import ops

# the argument set that the reference's optimized_prosody_attention.py spells out for this name
ATTENTION_PRESETS = {
    "analytical_balanced": dict(k_winners=5, w_amp=0.8, w_pitch=1.2, w_bound=1.0, smoothing=2, normalize_salience=True,
                                gain_up=1.5, gain_down=0.7),
}


class MultiChannelSpikingAttention(nn.Module):
    def __init__(self, k_winners=5, decay_amp=0.7, decay_pitch=0.7, decay_bound=0.7,
                 w_amp=1.0, w_pitch=1.0, w_bound=1.0, gain_up=1.8, gain_down=0.6,
                 min_gain=0.5, max_gain=2.5, smoothing=0, normalize_salience=True):
        super().__init__()
        self.k_winners = k_winners
        self.register_buffer('decay', torch.tensor([decay_amp, decay_pitch, decay_bound], dtype=torch.float32))
        self.register_buffer('weights', torch.tensor([w_amp, w_pitch, w_bound], dtype=torch.float32))
        self.gain_up = gain_up
        self.gain_down = gain_down          # stored and unused, as upstream
        self.min_gain = min_gain
        self.max_gain = max_gain
        self.smoothing = smoothing
        self.normalize_salience = normalize_salience
        self.validate = True                # read the range of ids / lengths before the launch (a host sync)

    def _run(self, ids, channels, lengths, state, want_spikes: bool) -> ops.ProsodyAttention:
        return ops.prosody_attention(ids, channels, k=int(self.k_winners), decay=self.decay, weights=self.weights,
                                     gain_up=self.gain_up, min_gain=self.min_gain, max_gain=self.max_gain,
                                     smoothing=int(self.smoothing), normalize=bool(self.normalize_salience),
                                     lengths=lengths, state=state, want_spikes=want_spikes, validate=self.validate)

    @staticmethod
    def _result(r: ops.ProsodyAttention) -> Dict[str, torch.Tensor]:
        out = {"mu_scalar": r.mu, "salience": r.salience, "winners": r.winners.long(), "gains": r.gains,
               "state": r.state}
        if r.spikes is not None:
            out["spikes"] = r.spikes
        return out

    def forward(self, amp, pitch, boundary, lengths: Optional[torch.Tensor] = None,
                state: Optional[torch.Tensor] = None, return_spikes: bool = False) -> Dict[str, torch.Tensor]:
        """amp, pitch, boundary [B, S] fp32 -> ``{mu_scalar [B], salience [B, S], winners [B, k] int64 (rank order, -1
        beyond a short row), gains [B, S], state [B, 3]}`` and, with ``return_spikes``, ``spikes`` [3, B, S]."""
        return self._result(self._run(None, (amp, pitch, boundary), lengths, state, return_spikes))


def prosody_channels_from_text(token_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Deterministic prosody from token IDs [B, S]: ``(amp, pitch, boundary)``, each [B, S] fp32."""
    ch = ops.prosody_channels(token_ids)
    return ch[0], ch[1], ch[2]


class ProsodyAttentionBridge(nn.Module):
    def __init__(self, k_winners: int = 5, attention_preset: Optional[str] = None, **attention_kwargs):
        super().__init__()
        if attention_preset is not None:
            if attention_preset not in ATTENTION_PRESETS:
                raise ValueError(f"attention_preset={attention_preset!r}: known presets are {sorted(ATTENTION_PRESETS)}")
            if attention_kwargs:
                raise ValueError("ProsodyAttentionBridge: give attention_preset or attention keywords, not both")
            self.attention = MultiChannelSpikingAttention(**ATTENTION_PRESETS[attention_preset])
        else:
            self.attention = MultiChannelSpikingAttention(k_winners=k_winners, **attention_kwargs)

    def forward(self, input_ids: torch.Tensor, token_strings=None, lengths: Optional[torch.Tensor] = None,
                state: Optional[torch.Tensor] = None, return_spikes: bool = False):
        """input_ids [B, S] -> ``(attention_gains [B, S], result)`` in one launch; ``token_strings`` is ignored, as
        upstream.  ``result`` is the attention's dict; ``attention_gains`` is its ``gains``: ``mu (1 + salience)``."""
        r = self.attention._run(input_ids, None, lengths, state, return_spikes)
        return r.gains, self.attention._result(r)
