"""Random operation sequences on the CPU (``ops`` replaced by tests/cpu_stub_scoped.py, the stub chain that carries
every op) against the fp64 bank model of tests/bank_model.py: after every operation the structure is compared exactly,
every recall path with the model, and the bank with a bank rebuilt from its checkpoint.  The point here is the host
logic -- slots, cursor, id maps, implicit id ranges, tags, the lists' dirty flags, the checkpoint -- on a bank small
enough to fill, wrap, empty and refill many times in 60 steps: D = 16, 96 rows, 4 centroids rebuilt every 16 writes.

The near-copies of D = 16 rows are kept 0.02 away from the merge threshold by construction (``bank_model.Pool`` leaves
out a row that comes close to an earlier one, and asserts the gap in fp64).

``test_tag_sequences`` runs the tag-aware cases (per-tag quotas, merging within tags) on tests/cpu_stub_quota.py.

The deterministic cases below are the smallest ones that show what the sequences found (see each docstring)."""
import numpy as np
import pytest
import torch

from tests import bank_model as B
from tests import cpu_stub_quota as qstub
from tests import cpu_stub_scoped as stub

SEEDS = 4                       # (x 3 policies x index on / off; 10 seeds pass too and take 3.5 minutes on the stubs)
# (cost with 4 seeds, measured alone on 8 cores: the six cases of test_sequences 8 - 23 s each, 90 s together; the five
# tag-aware cases of test_tag_sequences 21 - 33 s each, 140 s together -- the largest share of the suite without a GPU.
# A profile of one seed of quotas-index: 95 % is the checks after each step, nearly all of it in the torch stand-ins of
# the recalls; the recalls every case runs take about 60 % and the tag-aware extras, after every other step, 35 %)
STEPS = 60
SIZES = dict(M=96, D=16, batches=(1, 2, 7, 16, 30), pool_rows=900, pool_groups=40)
TOTAL = {}


@pytest.fixture()
def hmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    clock = B.Clock()
    monkeypatch.setattr(H, "ops", stub)
    monkeypatch.setattr(H.time, "time", clock)
    return H, clock


def _factory(H, policy, index, interval=16, **kw):
    def make():
        hf = H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=SIZES["M"],
                                    feature_dim=SIZES["D"], device="cpu", use_centroid_index=index, overflow=policy, **kw)
        hf.centroids_k, hf.centroids_update_interval = 4, interval
        hf.centroid_counts = torch.zeros(4)                 # (shrunk centroids_k: the counts buffer follows, as a rebuild leaves it)
        return hf
    return make


@pytest.mark.parametrize("index", [False, True], ids=["exact", "index"])
@pytest.mark.parametrize("policy", ["reference", "fifo", "weakest"])
def test_sequences(hmod, policy, index):
    H, clock = hmod
    tot = dict(queries=0, near_ties=0, differed=0, exact=0)
    seen = set()
    for seed in range(SEEDS):
        sizes = dict(SIZES, policy=policy, index=index, pool_seed=seed % 3)
        seq = B.run_sequence(_factory(H, policy, index), stub, seed, STEPS, sizes, clock)
        for k in tot:
            tot[k] += seq.stats[k]
        seen |= {e["op"] for e in seq.log}
        seen |= {"overwrote"} if any(e.get("over") for e in seq.log) else set()
        seen |= {"indexed"} if any(e.get("indexed_recall_checked") for e in seq.log) else set()
    # the alphabet was used, the bank filled and overwrote, the index was consulted
    want = {"write", "write_merge", "bulk", "decay", "reinforce", "recall_reinforce", "touch", "retag", "edit", "forget",
            "prune", "consolidate", "checkpoint", "overwrote"} | ({"rebuild", "indexed"} if index else set())
    assert want <= seen, f"never happened: {sorted(want - seen)}"
    # (d) the model's own near-ties: topk_equivalent's allowance must not be what makes the comparisons pass
    assert tot["near_ties"] <= 0.05 * tot["queries"], tot
    B.helpers.record_parity(f"host sequences {policy} {'index' if index else 'exact'}", tot["exact"], tot["queries"],
                            tot["near_ties"], positions_differed=tot["differed"])


# ------------------------------------------------------------------------ per-tag quotas and merging within tags
# The same machine on tests/cpu_stub_quota.py (the end of the stub chain): tagged writes under quotas, consolidating
# writes and consolidate() within tags, set_tag_quota, enforce_tag_quotas, and the tie origins through every compaction
# and the checkpoint.  The centroids are rebuilt every 20 writes here: an interval that does not divide the 96 rows, so
# that a full bank with an index writes whole runs (with 16 every run of a full bank is one row, and no run could take
# a tag victim and a global victim).  The int-quota case names a quota of 9 for the one tag whose ties the plan uses
# (``mid_quota``): with 2 rows per tag the next victim from any origin is one of two rows, and no write could show that
# the origin, and not row 0 or the cursor, ranked them; every other tag keeps the int quota of 2.  The repeat searches
# and the diverse recall run after every other step (``extra_every``; their draws are their own).
NAMED = {1: 10, 2: 3, 3: 30, 4: 1}
TAG_CASES = {
    "quotas-exact": ("weakest", False, lambda seed: B.tagcase({**NAMED, **({0: 40} if seed % 2 else {})}, range(6),
                                                               [0.2, 0.15, 0.2, 0.2, 0.1, 0.15], small=2, mid=3, over=1, free=5)),
    "quotas-index": ("weakest", True, lambda seed: B.tagcase({**NAMED, **({0: 40} if seed % 2 else {})}, range(6),
                                                              [0.2, 0.15, 0.2, 0.2, 0.1, 0.15], small=2, mid=3, over=1, free=5)),
    "int-quota-index": ("weakest", True, lambda seed: B.tagcase(2, range(1, 13), [1 / 12] * 12, small=1, mid=2, over=3, free=0,
                                                                mid_quota=9)),
    "merging-fifo": ("fifo", True, lambda seed: B.tagcase(None, range(4), [0.25] * 4, small=1, mid=2, over=3, free=0)),
    "merging-reference": ("reference", True, lambda seed: B.tagcase(None, range(4), [0.25] * 4, small=1, mid=2, over=3, free=0)),
}


@pytest.fixture()
def qmod(monkeypatch):
    from aura_snn_rag_amd.core import hippocampal as H
    clock = B.Clock()
    monkeypatch.setattr(H, "ops", qstub)
    monkeypatch.setattr(H.time, "time", clock)
    return H, clock


def run_tag_case(H, clock, name, seed, steps=STEPS):
    policy, index, case = TAG_CASES[name]
    tc = case(seed)
    sizes = dict(SIZES, policy=policy, index=index, pool_seed=seed % 3, tagcase=tc, extra_every=2)
    kw = {} if tc["quota"] is None else dict(tag_quota=tc["quota"])
    return B.run_sequence(_factory(H, policy, index, interval=20, **kw), qstub, seed, steps, sizes, clock,
                          plan=B.TagPlan(steps, tc, index, SIZES["M"]))


@pytest.mark.parametrize("name", list(TAG_CASES))
def test_tag_sequences(qmod, name):
    H, clock = qmod
    keys = ("queries", "near_ties", "differed", "exact", "repeat_rows", "repeat_near_ties")
    tot = dict.fromkeys(keys, 0)
    for seed in range(SEEDS):
        seq = run_tag_case(H, clock, name, seed)
        for k in keys:
            tot[k] += seq.stats[k]
        # every seed holds every planned event
        missing = [what for what, ok in B.tag_events(seq).items() if not ok]
        assert not missing, f"seed {seed}: never happened: {missing}\n" + "\n".join(str(e) for e in seq.log)
    assert tot["near_ties"] <= 0.05 * tot["queries"], tot
    # the near-ties of the repeat search that were allowed either target, counted from the model alone
    assert tot["repeat_near_ties"] <= 0.01 * tot["repeat_rows"], tot
    B.helpers.record_parity(f"host tag sequences {name}", tot["exact"], tot["queries"], tot["near_ties"],
                            positions_differed=tot["differed"], repeat_rows=tot["repeat_rows"],
                            repeat_near_ties_accepted=tot["repeat_near_ties"])
