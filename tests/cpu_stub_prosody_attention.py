"""Stand-ins for ``ops.prosody_attention`` / ``ops.prosody_channels`` on the CPU -- TEST INFRASTRUCTURE ONLY.

Built from the rule of ``tests/prosody_attention_rule.py`` (the fp32 restatement of ``include/aura_hip.h``, "Prosody
attention"); the channels from ids are the rule's fp64 values rounded to fp32.  They run the ops' own host checks first,
so a plumbing test sees the same refusals.  ``install(monkeypatch)`` swaps them into ``aura_snn_rag_amd.ops`` and
counts the calls."""
import numpy as np
import torch

from tests import prosody_attention_rule as R

CALLS = {"attention": 0, "channels": 0}
LAST = {}


def _channels(ids):
    a, p, b, _ = R.channels(ids.numpy())
    return a.astype(np.float32), p.astype(np.float32), b


def prosody_attention(ids=None, channels=None, *, k, decay, weights, gain_up=1.8, min_gain=0.5, max_gain=2.5,
                      smoothing=0, normalize=True, lengths=None, state=None, want_spikes=False, want_channels=False,
                      validate=True):
    from aura_snn_rag_amd import ops
    B, S, k, m = ops._prosody_shapes(ids, channels, k, decay, weights, gain_up, min_gain, max_gain, smoothing, lengths,
                                     state)
    if validate:
        ops._prosody_values("prosody_attention", ids, lengths, S)
    CALLS["attention"] += 1
    LAST.update(from_ids=ids is not None, k=k, m=m, lengths=lengths, state=state)
    ch = _channels(ids) if ids is not None else tuple(c.numpy() for c in channels)
    f = R.forward(*ch, decay.numpy(), weights.numpy(), k, m, normalize, gain_up, min_gain, max_gain,
                  None if lengths is None else lengths.numpy(), None if state is None else state.numpy())
    t = torch.from_numpy
    return ops.ProsodyAttention(t(f["gains"]), t(f["salience"]), t(f["mu"]), t(f["winners"]), t(f["v_out"]),
                                t(f["spikes"]) if want_spikes else None,
                                t(np.stack(ch)) if want_channels else None)


def prosody_channels(ids, validate=True):
    from aura_snn_rag_amd import ops
    _, S = ops._prosody_ids("prosody_channels", ids)
    if validate:
        ops._prosody_values("prosody_channels", ids, None, S)
    CALLS["channels"] += 1
    return torch.from_numpy(np.stack(_channels(ids)))


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(attention=0, channels=0)
    LAST.clear()
    monkeypatch.setattr(ops, "prosody_attention", prosody_attention)
    monkeypatch.setattr(ops, "prosody_channels", prosody_channels)
    return ops
