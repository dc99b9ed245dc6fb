"""Stand-in for ``ops.sample_next`` in NumPy on the CPU -- TEST INFRASTRUCTURE ONLY.

The rule of ``include/aura_hip.h`` ("Next token") as ``tests/sampling_rule.py`` restates it, with the Philox words and
the uniforms of ``tests/cpu_stub_replay.py`` and NumPy's fp32 ``exp`` / ``log`` in place of the device's: the decisions
are the rule's, the last bits of ``cum`` and ``d`` are not the device's.  It runs the op's own ``_sample_args`` first,
so a call the real op would refuse on the host is refused here too, and it keeps the row state (``seen``, ``finished``,
``out``) as the kernel does.  ``install(monkeypatch)`` swaps it into ``aura_snn_rag_amd.ops`` and counts the calls."""
import numpy as np
import torch

from tests import sampling_rule as R

CALLS = {"sample": 0}
LAST = {}


def sample_next(logits, *, seen=None, finished=None, stream_ids=None, penalty=1.0, penalty_rule="divide",
                temperature=1.0, top_k=50, top_p=0.9, seed=0, step=0, eos_id=None, pad_id=0, out=None,
                return_candidates=False):
    from aura_snn_rag_amd import ops
    B, V, _, scalars = ops._sample_args(logits, seen, finished, stream_ids, penalty, penalty_rule, temperature, top_k,
                                        top_p, seed, step, eos_id, pad_id, out)
    penalty, _, temperature, top_k, top_p, seed, step, eos, pad = scalars
    CALLS["sample"] += 1
    LAST.update(shape=(B, V), step=step, seed=seed, top_k=top_k, temperature=temperature)
    streams = np.arange(B) if stream_ids is None else np.asarray(
        stream_ids.cpu().numpy() if isinstance(stream_ids, torch.Tensor) else stream_ids)
    r = R.sample(logits.detach().numpy(), None if seen is None else seen.numpy(), streams, penalty=penalty,
                 rule=penalty_rule, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, step=step)
    done = np.zeros(B, dtype=bool) if finished is None else finished.numpy() != 0
    token = np.where(done, pad, r["token"]).astype(np.int64)
    tokens = torch.empty(B, dtype=torch.int64) if out is None else out
    tokens.copy_(torch.from_numpy(token))
    for b in np.nonzero(~done & (token >= 0))[0]:
        if seen is not None:
            seen[b, token[b]] = 1
        if finished is not None and eos >= 0 and token[b] == eos:
            finished[b] = 1
    if not return_candidates:
        return tokens
    fill = dict(ids=-1, z=-np.inf, cum=-np.inf, d=-np.inf, n_kept=0)
    cand = {}
    for name in ("ids", "z", "cum", "d", "n_kept"):
        if name in r:
            v = np.array(r[name], copy=True)
            v[done] = fill[name]
            cand[name] = torch.from_numpy(v)
    return tokens, cand


def draws(row, steps, *, stream=0, **kw):
    """The stub's tokens for one logit row [V] at every step of ``steps`` (one vectorised pass of the same rule code)."""
    steps = np.asarray(steps, dtype=np.uint64)
    z = np.broadcast_to(np.asarray(row, dtype=np.float32), (steps.size, len(row)))
    return R.sample(z, None, np.full(steps.size, stream), step=steps, **kw)["token"]


def install(monkeypatch):
    from aura_snn_rag_amd import ops
    CALLS.update(sample=0)
    LAST.clear()
    monkeypatch.setattr(ops, "sample_next", sample_next)
    return ops
