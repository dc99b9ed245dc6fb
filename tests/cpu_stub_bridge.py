"""Stand-in for ``ops.poisson_rate`` on the CPU -- TEST INFRASTRUCTURE ONLY.

The fp32 restatement of ``tests/poisson_bridge_rule.py`` behind the op's entry point: the generator, the uniforms and
the decisions are the rule's, the last bit of ``q`` is not the device's and the rate is torch's CPU mean of the train.  It runs the op's own host checks first, so a
call the real op would refuse on the host is refused here too.  ``install(monkeypatch)`` swaps it into
``aura_snn_rag_amd.ops`` and counts the calls."""
import numpy as np
import torch

from tests import poisson_bridge_rule as RULE

CALLS = {"poisson_rate": 0}
LAST = {}


def poisson_rate(x, weight, bias=None, *, T, seed, streams=None, rows_per_stream=None, start=0, return_probs=False,
                 return_spikes=False, out=None):
    from aura_snn_rag_amd import ops
    N, K, H, T, seed, B, S, start0 = ops._poisson_rate_args(x, weight, bias, T, seed, streams, rows_per_stream, start,
                                                           return_probs, return_spikes, out)
    CALLS["poisson_rate"] += 1
    LAST.update(N=N, K=K, H=H, T=T, seed=seed, S=S, device_start=isinstance(start, torch.Tensor))
    if streams is not None:
        streams = streams.numpy() if isinstance(streams, torch.Tensor) else np.asarray(streams)
    st = start.numpy() if isinstance(start, torch.Tensor) else start0
    rate, q, spikes = RULE.bridge(x.detach().numpy(), weight.detach().numpy(),
                                  None if bias is None else bias.detach().numpy(), T, seed, streams,
                                  None if streams is None else S, st)
    rate = torch.from_numpy(spikes).mean(dim=1)     # torch's CPU mean (count / T), so that the modules' parts agree here
    if out is not None:
        rate = out.copy_(rate)
    extra = ((torch.from_numpy(q),) if return_probs else ()) + ((torch.from_numpy(spikes),) if return_spikes else ())
    return (rate,) + extra if extra else rate


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(poisson_rate=0)
    LAST.clear()
    monkeypatch.setattr(ops, "poisson_rate", poisson_rate)
    return ops
