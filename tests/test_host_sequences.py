"""Random operation sequences on the CPU (``ops`` replaced by tests/cpu_stub_scoped.py, the stub chain that carries
every op) against the fp64 bank model of tests/bank_model.py: after every operation the structure is compared exactly,
every recall path with the model, and the bank with a bank rebuilt from its checkpoint.  The point here is the host
logic -- slots, cursor, id maps, implicit id ranges, tags, the lists' dirty flags, the checkpoint -- on a bank small
enough to fill, wrap, empty and refill many times in 60 steps: D = 16, 96 rows, 4 centroids rebuilt every 16 writes.

The near-copies of D = 16 rows are kept 0.02 away from the merge threshold by construction (``bank_model.Pool`` leaves
out a row that comes close to an earlier one, and asserts the gap in fp64).

The deterministic cases below are the smallest ones that show what the sequences found (see each docstring)."""
import numpy as np
import pytest
import torch

from tests import bank_model as B
from tests import cpu_stub_scoped as stub

SEEDS = 4                       # (x 3 policies x index on / off; 10 seeds pass too and take 3.5 minutes on the stubs)
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


def _factory(H, policy, index):
    def make():
        hf = H.HippocampalFormation(n_place_cells=4, n_time_cells=3, n_grid_cells=3, max_memories=SIZES["M"],
                                    feature_dim=SIZES["D"], device="cpu", use_centroid_index=index, overflow=policy)
        hf.centroids_k, hf.centroids_update_interval = 4, 16
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
