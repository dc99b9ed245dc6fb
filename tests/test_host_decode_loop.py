"""The pieces ``generate`` of the three language models shares (``core/language_zone/decoding.py``), alone: the
sample/step loop on a step callable that plays back prepared logits and the sampler's CPU stand-in
(tests/cpu_stub_sampling.py), the seed check and the trim to the step at which the last row finished.  No model."""
import types

import numpy as np
import pytest
import torch

from tests import cpu_stub_sampling as SAMPLE

V, PAD = 12, 11
GREEDY = dict(penalty=1.0, penalty_rule="divide", temperature=0.0, top_k=5, top_p=0.9)


def _state(B, step=0, lengths=None):
    return types.SimpleNamespace(seen=torch.zeros(B, V, dtype=torch.uint8), finished=torch.zeros(B, dtype=torch.uint8),
                                 seed=3, step=step, stream_ids=None, pending=None,
                                 lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int32))


def _logits(columns):
    """One [B, V] block per column of token ids: every row's logit is largest at its token."""
    return [torch.zeros(len(col), V).scatter_(1, torch.tensor(col)[:, None], 4.0) for col in columns]


def _run(monkeypatch, columns, state, max_new_tokens, eos=None, sync_every=8, retire=False):
    """Runs the loop over the prepared columns -> (n, the [B, max_new_tokens] block, what every step call saw)."""
    from aura_snn_rag_amd.core.language_zone.decoding import decode_loop
    SAMPLE.install(monkeypatch)
    blocks = _logits(columns)
    new = torch.full((len(columns[0]), max_new_tokens), -5, dtype=torch.int64)
    seen = []

    def step(column):
        seen.append(dict(tokens=column.tolist(), step=state.step,
                         lengths=None if state.lengths is None else state.lengths.tolist()))
        return blocks[len(seen)]
    n = decode_loop(blocks[0], state, new, GREEDY, eos, PAD, sync_every, step, retire)
    return n, new, seen


def test_without_an_eos_every_column_is_sampled_and_the_last_one_is_not_stepped(monkeypatch):
    columns = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10]]
    state = _state(2, step=3)
    n, new, calls = _run(monkeypatch, columns, state, 5)
    assert n == 5 and len(calls) == 4 and state.step == 3 + 5 and SAMPLE.CALLS["sample"] == 5
    assert new.tolist() == [[1, 3, 5, 7, 9], [2, 4, 6, 8, 10]]
    assert [c["tokens"] for c in calls] == columns[:4], "every step is fed the column sampled before it"
    assert [c["step"] for c in calls] == [4, 5, 6, 7]
    assert state.seen.sum(1).tolist() == [5, 5] and state.finished.tolist() == [0, 0]
    # a one-column destination: the first logits are sampled and nothing is stepped
    n, new, calls = _run(monkeypatch, columns, _state(2), 1, eos=9, sync_every=1)
    assert n == 1 and calls == [] and new.tolist() == [[1], [2]]


def test_the_host_looks_at_finished_every_sync_every_columns_only(monkeypatch):
    from aura_snn_rag_amd.core.language_zone.decoding import trim_to_last_finish
    eos = 7
    columns = [[1, 2], [eos, eos]] + [[3, 4]] * 7                       # both rows draw the EOS at new token 2
    late = _state(2)
    n, new, calls = _run(monkeypatch, columns, late, 9, eos=eos, sync_every=4)
    assert n == 4 and len(calls) == 3, "all rows had finished at n = 2; the host looked at n = 4"
    assert new[:, :4].tolist() == [[1, eos, PAD, PAD]] * 1 + [[2, eos, PAD, PAD]] and late.step == 4
    assert bool((new[:, 4:] == -5).all()), "nothing is written past the stop"
    assert trim_to_last_finish(new[:, :n], eos) == 2
    soon = _state(2)
    n1, new1, calls1 = _run(monkeypatch, columns, soon, 9, eos=eos, sync_every=1)
    assert n1 == 2 and len(calls1) == 1 and soon.step == 2
    assert trim_to_last_finish(new1[:, :n1], eos) == 2 and torch.equal(new1[:, :2], new[:, :2])
    # without an EOS the flags are never read: the loop runs to the end whatever they hold
    flagged = _state(2)
    flagged.finished.fill_(1)
    assert _run(monkeypatch, columns, flagged, 9, eos=None, sync_every=1)[0] == 9


@pytest.mark.parametrize("retire", [True, False])
def test_retirement_sets_a_finished_rows_length_to_minus_one_before_the_next_step(monkeypatch, retire):
    eos = 7
    columns = [[eos, 2], [3, 4], [5, 6]]                                # row 0 finishes with its first token
    state = _state(2, lengths=[5, 9])
    n, new, calls = _run(monkeypatch, columns, state, 3, eos=eos, retire=retire)
    assert n == 3 and new.tolist() == [[eos, PAD, PAD], [2, 4, 6]] and state.finished.tolist() == [1, 0]
    assert [c["lengths"] for c in calls] == [[-1 if retire else 5, 9]] * 2
    # without an EOS nothing can finish and nothing is retired
    free = _state(2, lengths=[5, 9])
    _run(monkeypatch, columns, free, 3, eos=None, retire=retire)
    assert free.lengths.tolist() == [5, 9]


def test_the_seed_check_takes_python_and_numpy_integers_in_range():
    from aura_snn_rag_amd.core.language_zone.decoding import check_seed
    for good in (0, 2 ** 64 - 1, np.int64(3)):
        got = check_seed("Model.generate", good)
        assert type(got) is int and got == int(good)
    for bad in (True, -1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match=r"^Model\.generate: seed"):
            check_seed("Model.generate", bad)


def test_the_trim_keeps_the_columns_up_to_the_last_rows_finish():
    from aura_snn_rag_amd.core.language_zone.decoding import trim_to_last_finish
    eos = 7
    block = torch.tensor([[1, eos, PAD, PAD, PAD, PAD],                 # finishes at column 1
                          [2, 3, 4, 5, eos, PAD],                       # finishes at column 4
                          [6, 8, 9, 10, 0, 1]])                         # never finishes
    assert trim_to_last_finish(block, eos) == 6, "a row that never finishes keeps every column"
    assert trim_to_last_finish(block[:2], eos) == 5, "up to and including the column of the last EOS"
    assert trim_to_last_finish(block[:1], eos) == 2
    assert trim_to_last_finish(block, None) == 6 and trim_to_last_finish(block[:2], None) == 6
    assert trim_to_last_finish(block[:, :0], eos) == 0
