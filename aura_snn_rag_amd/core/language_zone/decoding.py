"""What ``generate`` of the three language models shares, each piece once: the seed check, the start of a turn from a
returned state, the sample/step loop and the trim to the step at which the last row finished.  Plain functions over a
state that carries ``seen``, ``finished``, ``seed``, ``step``, ``stream_ids`` and ``pending`` (``DecodeState`` and
``ZoneState`` both do); what differs between the models comes in as arguments: how one column of tokens becomes the next
logits, and whether a finished row is retired from the attention caches."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from ... import ops

_UNSET = object()


def check_seed(who: str, seed) -> int:
    """``seed`` as an int; raises unless it is an ``int`` or ``np.integer`` (no bool) in [0, 2^64)."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < (1 << 64):
        raise ValueError(f"{who}: seed must be an int in [0, 2^64), got {seed!r}")
    return int(seed)


def start_turn(state, input_ids: torch.Tensor, seed: Optional[int], stream_ids) -> torch.Tensor:
    """Starts a turn on a state that ``generate(.., return_state=True)`` returned: ``seed`` (checked by the caller) and
    ``stream_ids`` replace the state's where they are given, and the turn's tokens ``[pending, input_ids]`` [B, 1 + S]
    are returned with ``pending`` cleared."""
    if seed is not None:
        state.seed = seed
    if stream_ids is not None:
        state.stream_ids = stream_ids
    turn = torch.cat([state.pending.to(input_ids.device)[:, None], input_ids.to(torch.int64)], dim=1)
    state.pending = None
    return turn


def decode_loop(logits: torch.Tensor, state, new: torch.Tensor, sampling: dict, eos: Optional[int], pad: int,
                sync_every: int, step: Callable[[torch.Tensor], torch.Tensor], retire: bool) -> int:
    """Samples up to ``new.shape[1]`` tokens per row into the columns of ``new`` [B, max_new_tokens] int64, the first
    from ``logits`` [B, V] and every later one from ``step(previous column)``; returns the number of columns written.
    Per token: one ``ops.sample_next`` under ``state.seed`` / ``state.step`` / ``state.stream_ids`` with the keyword
    arguments ``sampling`` (it marks ``state.seen`` and ``state.finished``), then ``state.step += 1``.  With an ``eos``
    the host looks at ``finished`` every ``sync_every`` columns and stops when every row has finished; ``retire`` sets a
    finished row's ``state.lengths`` to -1 before the next step, which takes the row out of the attention caches."""
    n = 0
    while True:
        column = new[:, n]
        ops.sample_next(logits, seen=state.seen, finished=state.finished, stream_ids=state.stream_ids, seed=state.seed,
                        step=state.step, eos_id=eos, pad_id=pad, out=column, **sampling)
        state.step += 1
        n += 1
        if n == new.shape[1]:
            return n
        if eos is not None:
            if retire:
                state.lengths.masked_fill_(state.finished.bool(), -1)
            if n % sync_every == 0 and bool(state.finished.all()):
                return n
        logits = step(column)


def trim_to_last_finish(new: torch.Tensor, eos: Optional[int]) -> int:
    """The number of columns of ``new`` [B, n] up to the step at which the last row finished: a column is padding when
    every row had drawn ``eos`` before it.  ``n`` without an ``eos`` (no device read), else one host sync."""
    if eos is None:
        return new.shape[1]
    done_before = ((new == eos).cumsum(1) - (new == eos).to(torch.int64)) > 0
    return int((~done_before.all(0)).sum().item())
