"""Host-side logic of diverse recall on the CPU (``ops`` replaced by tests/cpu_stub_diverse.py, which restates
the rule in torch fp64): the defaults and clamps of ``fetch_k``, the argument errors, that a call without the new
arguments launches nothing new and passes the recall today's arguments, that ``reinforce`` is applied once and after
the selection, what ``_last_flag`` holds, and the pass-through of the layer helpers."""
import inspect

import pytest
import torch

from tests import cpu_stub_diverse as stub

NOW = 1.7e9 + 5.0


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", lambda: NOW)
    for k in stub.CALLS:
        stub.CALLS[k] = 0
    stub.LAST.clear()
    return H


def _hf(H, n, D=16, M=256, seed=0):
    hf = H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=M, feature_dim=D,
                                device="cpu", use_centroid_index=False)
    g = torch.Generator().manual_seed(seed)
    hf.create_episodic_memories([f"m{i}" for i in range(n)], torch.randn(n, D, generator=g))
    return hf


def _recorded_knn(monkeypatch):
    calls = []
    real = stub.knn_search

    def knn_search(*a, **kw):
        calls.append((a[4], dict(kw)))                  # (k, keyword arguments)
        return real(*a, **kw)
    monkeypatch.setattr(stub, "knn_search", knn_search)
    return calls


def test_the_rule_on_four_memories():
    # A and A' are near-copies, B and C stand apart; scores descend A, A', B, C
    a = torch.tensor([1.0, 0.0, 0.0, 0.0])
    bank = torch.stack([a, a + torch.tensor([0.0, 0.02, 0.0, 0.0]), torch.tensor([0.3, 1.0, 0.0, 0.0]),
                        torch.tensor([0.2, 0.0, 1.0, 0.0])])
    inv = 1.0 / bank.norm(dim=1)
    rows = torch.tensor([[0, 1, 2, 3]], dtype=torch.int32)
    scores = torch.tensor([[0.9, 0.89, 0.5, 0.4]])
    s, r = stub.diverse_select(bank, inv, 4, rows, scores, 3, 0.0, None)
    assert r.tolist() == [[0, 1, 2]] and torch.equal(s, scores[:, :3])
    s, r = stub.diverse_select(bank, inv, 4, rows, scores, 3, 0.0, 0.9)
    assert r.tolist() == [[0, 2, 3]] and s.tolist() == [[scores[0, 0].item(), scores[0, 2].item(), scores[0, 3].item()]]
    s, r = stub.diverse_select(bank, inv, 4, rows, scores, 2, 1.0, None)     # pure diversity: the least similar to A
    assert r.tolist() == [[0, 3]]
    s, r = stub.diverse_select(bank, inv, 4, rows[:, :2].contiguous(), scores[:, :2].contiguous(), 2, 0.0, 0.9)
    assert r.tolist() == [[0, -1]] and s[0, 1].item() == float("-inf")       # runs short: padding
    # invalid candidates are ignored: -1, a row outside the bank, a NaN score
    rows2 = torch.tensor([[0, -1, 9, 1, 2, 3]], dtype=torch.int32)
    scores2 = torch.tensor([[0.9, 0.95, 0.95, 0.89, float("nan"), 0.4]])
    s, r = stub.diverse_select(bank, inv, 4, rows2, scores2, 3, 0.0, 0.9)
    assert r.tolist() == [[0, 3, -1]]


def test_fetch_k_defaults_and_clamps(hmod):
    hf = _hf(hmod, 200)
    q = torch.randn(3, 16)
    for k, fetch, want_F, want_k in ((5, None, 32, 5), (10, None, 40, 10), (40, None, 128, 40), (5, 64, 64, 5),
                                     (5, 500, 128, 5), (5, 5, 5, 5), (5, 0, 32, 5)):
        s, r = hf.recall_batch(q, k=k, now=NOW, max_similarity=0.9, fetch_k=fetch)
        assert (stub.LAST["F"], stub.LAST["k"]) == (want_F, want_k), (k, fetch)
        assert s.shape == (3, want_k) and r.shape == (3, want_k) and r.dtype == torch.int32
    small = _hf(hmod, 20)
    small.recall_batch(q, k=5, now=NOW, diversity=0.5)
    assert (stub.LAST["F"], stub.LAST["k"], stub.LAST["max_similarity"]) == (20, 5, None)     # clamped to the count
    s, r = small.recall_batch(q, k=30, now=NOW, diversity=0.5)
    assert (stub.LAST["F"], stub.LAST["k"]) == (20, 20) and r.shape == (3, 20)
    assert stub.LAST["diversity"] == 0.5 and stub.LAST["count"] == 20


def test_argument_errors(hmod):
    hf = _hf(hmod, 200)
    q = torch.randn(2, 16)
    before = dict(stub.CALLS)
    for kw in (dict(diversity=-0.1), dict(diversity=1.5), dict(diversity=float("nan")),
               dict(max_similarity=-1.0), dict(max_similarity=1.01), dict(max_similarity=float("nan")),
               dict(max_similarity=0.9, fetch_k=4),                 # F < k
               dict(max_similarity=0.9, fetch_k=-3),
               dict(diversity=0.5, bound_exchange=(lambda b: b[:, 0], 2))):
        with pytest.raises(ValueError):
            hf.recall_batch(q, k=5, now=NOW, **kw)
    with pytest.raises(ValueError):
        hf.recall_batch(q, k=150, now=NOW, diversity=0.5)           # k' = 150 > 128 candidates
    assert stub.CALLS == before                                      # refused before anything ran
    hf.recall_batch(q, k=5, now=NOW, max_similarity=1.0, diversity=0.0)
    hf.recall_batch(q, k=5, now=NOW, max_similarity=-0.5, diversity=1.0)
    empty = hmod.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=8, feature_dim=16,
                                      device="cpu")
    s, r = empty.recall_batch(q, k=5, diversity=0.5)
    assert s.shape == (2, 0) and r.shape == (2, 0)


def test_without_the_arguments_nothing_changes(hmod, monkeypatch):
    hf = _hf(hmod, 60)
    q = torch.randn(4, 16)
    calls = _recorded_knn(monkeypatch)
    s0, r0 = hf.recall_batch(q, k=3, now=NOW)
    assert stub.CALLS["diverse"] == 0 and len(calls) == 1 and calls[0][0] == 3
    plain_kw = calls[0][1]
    s1, r1 = hf.recall_batch(q, k=3, now=NOW, diversity=0.0)        # same rows: d = 0 without a limit
    assert stub.CALLS["diverse"] == 1 and len(calls) == 2
    assert calls[1][0] == 32                                         # the inner recall fetches F rows ...
    assert {k: v for k, v in calls[1][1].items()} .keys() == plain_kw.keys()      # ... with today's arguments
    assert all(calls[1][1][k] is plain_kw[k] or calls[1][1][k] == plain_kw[k] for k in plain_kw)
    assert torch.equal(r0, r1) and torch.equal(s0, s1)
    # the candidates handed to the selection are the plain top-F
    sF, rF = hf.recall_batch(q, k=32, now=NOW)
    assert torch.equal(stub.LAST["cand_rows"], rF) and torch.equal(stub.LAST["cand_scores"], sF)
    assert hf.retrieve_similar_memories(q[0], None, 3) == [(hf.id_of_row(int(r)), float(s)) for s, r in zip(s0[0], r0[0])]
    assert stub.CALLS["diverse"] == 1


def test_near_copies_leave_the_result(hmod):
    g = torch.Generator().manual_seed(3)
    base = torch.randn(30, 16, generator=g)
    feats = torch.cat([base[:6].repeat_interleave(5, 0) + 0.01 * torch.randn(30, 16, generator=g), base[6:]])
    hf = hmod.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=64, feature_dim=16,
                                   device="cpu", use_centroid_index=False)
    hf.create_episodic_memories([f"m{i}" for i in range(54)], feats)
    label = torch.cat([torch.arange(6).repeat_interleave(5), 6 + torch.arange(24)])
    q = base[:6] + 0.05 * torch.randn(6, 16, generator=g)
    _, plain = hf.recall_batch(q, k=4, now=NOW)
    _, div = hf.recall_batch(q, k=4, now=NOW, max_similarity=0.9)
    assert all(len(set(label[r.long()].tolist())) == 1 for r in plain)       # four copies of one memory
    assert all(len(set(label[r.long()].tolist())) == 4 for r in div)
    assert torch.equal(plain[:, 0], div[:, 0])                               # the first pick is the best candidate
    ids = hf.retrieve_similar_memories(q[0], k=4, max_similarity=0.9, fetch_k=40)
    assert [i for i, _ in ids] == [hf.id_of_row(int(r)) for r in div[0]]


def test_reinforce_is_applied_once_after_the_selection(hmod):
    hf = _hf(hmod, 100)
    hf.decay_memories(0.5)
    q = torch.randn(5, 16)
    s, r = hf.recall_batch(q, k=4, now=NOW, diversity=0.7, max_similarity=0.95, reinforce=0.25)
    assert stub.CALLS["reinforce"] == 1 and stub.CALLS["diverse"] == 1
    hit = torch.zeros(100, dtype=torch.bool)
    hit[r[r >= 0].long()] = True
    assert torch.equal(hf.memory_metadata[:100, 0], torch.where(hit, torch.tensor(0.75), torch.tensor(0.5)))
    fetched = torch.zeros(100, dtype=torch.bool)
    fetched[stub.LAST["cand_rows"].reshape(-1).long()] = True
    assert int(fetched.sum()) > int(hit.sum())                                # the F fetched rows were not reinforced
    # the candidates were scored before the reinforcement
    assert bool((stub.LAST["cand_scores"] <= 0.5 * (0.5 + 0.2) + 1e-6).all())


def test_last_flag_is_what_the_inner_recall_left(hmod):
    class Flagged(hmod.HippocampalFormation):
        def recall_batch(self, queries, k=5, **kw):
            out = super().recall_batch(queries, k=k, **kw)
            if kw.get("diversity") is None and kw.get("max_similarity") is None:
                self._last_flag = 64 + k                                      # what a candidate-mode recall would leave
            return out
    hf = Flagged(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=64, feature_dim=16, device="cpu",
                 use_centroid_index=False)
    hf.create_episodic_memories([f"m{i}" for i in range(50)], torch.randn(50, 16))
    hf.recall_batch(torch.randn(2, 16), k=3, now=NOW, max_similarity=0.9)
    assert hf._last_flag == 64 + 32


def test_layer_helpers_pass_the_arguments_on(hmod):
    from aura_snn_rag_amd.core.language_zone import memory_ops as MO
    from aura_snn_rag_amd.sharded import ShardedHippocampus
    hf = _hf(hmod, 40)
    q = torch.randn(3, 16)
    f0, s0 = MO.retrieve_memories(hf, q, k=4)
    assert stub.CALLS["diverse"] == 0
    f1, s1 = MO.retrieve_memories(hf, q, k=4, diversity=0.5, fetch_k=16)
    assert stub.CALLS["diverse"] == 1 and (stub.LAST["F"], stub.LAST["k"], stub.LAST["diversity"]) == (16, 4, 0.5)
    assert f1.shape == (3, 4, 16) and s1.shape == (3, 4)
    f2, s2 = MO.retrieve_memories(hf, q, k=4, max_similarity=-0.99)            # nearly everything is too similar
    assert stub.CALLS["diverse"] == 2 and bool((s2[:, -1] == 0).all()) and bool((f2[:, -1] == 0).all())
    assert bool((s2[:, 0] != 0).all())
    inj = MO.MemoryInjection(hf, 16, num_heads=2, memory_injection="concat")
    h = torch.randn(3, 7, 16)
    inj.retrieve_memories(h, k=4)
    assert stub.CALLS["diverse"] == 2
    mf, ms = inj.retrieve_memories(h, k=4, max_similarity=0.9, fetch_k=20)
    assert stub.CALLS["diverse"] == 3 and stub.LAST["F"] == 20 and mf.shape == (3, 4, 16)

    class Layer(MO.BatchedMemoryMixin):
        hippocampus, query_proj = hf, inj.query_proj
    Layer().retrieve_memories(h, 4, diversity=0.25)
    assert stub.CALLS["diverse"] == 4 and stub.LAST["diversity"] == 0.25
    for fn in (MO.retrieve_memories, MO.MemoryInjection.retrieve_memories, MO.BatchedMemoryMixin.retrieve_memories,
               hmod.HippocampalFormation.recall_batch, hmod.HippocampalFormation.retrieve_similar_memories):
        p = inspect.signature(fn).parameters
        assert all(p[n].default is None for n in ("diversity", "max_similarity", "fetch_k")), fn
    # candidate rows of a sharded bank live on other ranks: its recall has no such argument
    assert "diversity" not in inspect.signature(ShardedHippocampus.recall_batch).parameters
    # positional use of the reference's signature is unchanged
    assert list(inspect.signature(hmod.HippocampalFormation.retrieve_similar_memories).parameters)[:4] == \
        ["self", "query_features", "location", "k"]
