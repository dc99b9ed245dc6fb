"""Random operation sequences on the kernels against the fp64 bank model of tests/bank_model.py: one seed, 40 steps,
for every overflow policy x {no index, 256 centroids} x D in {64, 100}.  After every operation the structure is compared
exactly, every recall path (the exact scan, the probe-masked scan, the inverted lists through a batch of 544 queries,
a scoped recall) with the model's fp64 scores, and the bank -- rows, score bits, ``_inv_norm``, the bf16 shadow and its
residuals -- with a bank rebuilt from ``state_dict()`` + ``bank_state()``.

Sizes: 10 000 rows, first filled to 9000 by ``bulk_write``: the smallest bank in which the bf16 shadow and the
list-sorted image are live (``SHADOW_MIN_ROWS`` = 8192) and which can still fill up.  The centroids are rebuilt every
1024 inserts: an interval that does not divide the full bank, so a full bank writes whole runs instead of rebuilding
after every row.  D = 100 is a row width that is no multiple of 16; no bf16 image is kept at that width
(``feature_dim % 8``), so the events that concern the image are asserted at D = 64 only.

Part of every sequence is planned (``_Plan``) so that each case crosses 8192 rows downwards by a ``forget`` and by a
``prune`` and upwards again, fills the bank and overwrites, recalls through the index right after a ``forget`` with no
rebuild in between, overwrites rows the sorted image holds, appends more than ``ops.ivf2_slack(interval)`` rows between
two re-packs, and goes on after a checkpoint round trip; the rest is drawn.  Each event is asserted from the op log.

``test_tag_sequence`` runs the same machine over the tag-aware state: per-tag quotas (tagged writes, ``set_tag_quota``,
``enforce_tag_quotas``, the tie origins through every compaction and the checkpoint) and merging within tags
(consolidating writes and ``consolidate`` within tags), with the planned part of ``bank_model.TagPlan`` and the events
of ``bank_model.tag_events``; after every operation -- after every other one in the four cases with an index
(``extra_every``) -- it adds the scoped and the scope-blind repeat search over the next 48 rows of the pool against the
fp64 rule, and those searches and a diverse recall against the rebuilt bank.

Nothing here provokes a fault: every operation keeps to the documented contracts (quotas only with ``'weakest'``, no run
asks for more victims than rows held, tags stay in [0, 2^24))."""
import time

import pytest
import torch

from tests import bank_model as B

pytestmark = pytest.mark.gpu
M, FILL, STEPS, SEED = 10_000, 9000, 40, 5
LIVE = 8192
INTERVAL = 1024
SIZES = dict(M=M, batches=(1, 7, 64, 300, 1500), batch_weights=(3, 3, 3, 2, 1), pool_rows=22_000, pool_groups=400)


@pytest.fixture(scope="module")
def hmod():
    from aura_snn_rag_amd.core import hippocampal as H
    clock = B.Clock()
    mp = pytest.MonkeyPatch()
    mp.setattr(H.time, "time", clock)
    yield H, clock
    mp.undo()


class _Plan:
    """The planned part of a sequence: goals in order, each reached by one operation once its precondition holds
    (otherwise that step works towards the precondition and the goal stays); a drawn operation in between."""

    def __init__(self, index):
        self.index = index
        self.goals = ["fill0", "append_a", "append_b", "still_decay", "still_reinforce", "still_touch", "still_recall",
                      "fill", "overwrite", "checkpoint", "down", "up", "edit", "down_prune", "up"]
        # these follow their predecessor with nothing in between; the still_ ones run at the `now` of the checks before
        # them, on a live image with appended rows: only the operation itself can tell the cached score constants
        self.sticky = {"append_b", "overwrite", "still_decay", "still_reinforce", "still_touch", "still_recall"}
        self.drawn_last = True

    def __call__(self, seq):
        left = STEPS - (seq.step + 1)
        if not self.goals:
            return None
        if not (self.drawn_last or self.goals[0] in self.sticky or left <= 2 * len(self.goals) + 4):
            self.drawn_last = True
            return None
        forced = getattr(self, "_" + self.goals[0])(seq)
        self.drawn_last = forced is None
        return forced

    def _done(self, op, fn):
        self.goals.pop(0)
        return op, fn

    def _live_with_room(self, seq, room):
        """Towards a bank of at least 8192 rows with ``room`` free ones, or None when it is one."""
        n = seq.model.count
        if n < LIVE:
            return "bulk", lambda: seq.op_bulk(FILL - n, self.index, True)
        if M - n < room:
            return "forget", lambda: seq.op_forget("rows", n=n - (M - room - 200))
        return None

    def _fill0(self, seq):
        return self._done("bulk", lambda: seq.op_bulk(FILL, self.index, True))

    def _append_a(self, seq):
        return self._live_with_room(seq, 700) or self._done("bulk", lambda: seq.op_bulk(300, False, False))

    def _append_b(self, seq):
        return self._done("bulk", lambda: seq.op_bulk(300, False, True))

    def _still_decay(self, seq):
        return self._done("decay", seq.op_decay) + (True,)

    def _still_reinforce(self, seq):
        return self._done("reinforce", seq.op_reinforce) + (True,)

    def _still_touch(self, seq):
        return self._done("touch", seq.op_touch) + (True,)

    def _still_recall(self, seq):
        return self._done("recall_reinforce", lambda: seq.op_recall_reinforce(True)) + (True,)

    def _fill(self, seq):
        room = M - seq.model.count
        if room > 1400:
            return "bulk", lambda: seq.op_bulk(room - 1000, False, True)
        return self._done("write", lambda: seq.op_write(room + 64, True))

    def _overwrite(self, seq):
        return self._done("write", lambda: seq.op_write(300, False))

    def _checkpoint(self, seq):
        return self._done("checkpoint", seq.op_checkpoint)

    def _down(self, seq):
        return self._live_with_room(seq, 0) or self._done("forget", lambda: seq.op_forget("rows", n=seq.model.count - 7900))

    def _up(self, seq):
        if seq.model.count >= LIVE:                         # (a drawn write has crossed already)
            self.goals.pop(0)
            return None
        return self._done("write", lambda: seq.op_write(1500, False))

    def _edit(self, seq):
        return self._done("edit", seq.op_edit)

    def _down_prune(self, seq):
        n = seq.model.count
        return self._live_with_room(seq, 0) or self._done("prune", lambda: seq.op_prune(False, frac=(n - 8000) / n))


def _events(seq, image):
    """The mandatory events, from the op log alone."""
    log = seq.log
    slack = seq.ops.ivf2_slack(INTERVAL)
    down = [e for e in log if e["op"] in ("forget", "prune") and e["count_before"] >= LIVE > e["count_after"]]
    ev = {
        "crosses 8192 downwards by a forget": any(e["op"] == "forget" for e in down),
        "crosses 8192 downwards by a prune": any(e["op"] == "prune" for e in down),
        "crosses 8192 upwards again": any(e["count_before"] < LIVE <= e["count_after"] and e["step"] > down[0]["step"]
                                          for e in log) if down else False,
        "fills the bank and overwrites": any(e.get("over") and e["count_after"] == M for e in log),
        "goes on after a checkpoint round trip": any(e["op"] == "checkpoint" and e["step"] < STEPS - 1 for e in log),
    }
    if seq.z["index"]:
        ev["recalls through the index after a forget, no rebuild in between"] = any(
            e["op"] == "forget" and e.get("removed") and e["indexed_recall_checked"] for e in log)
    still = {e["op"] for e in log if e["still"] and (e["image_live_before"] or not image)}
    ev["decays, reinforces, touches and recalls with reinforcement while the clock stands still"] = \
        {"decay", "reinforce", "touch", "recall_reinforce"} <= still
    if image:
        ev["overwrites rows the sorted image holds"] = any(e.get("over") and e["image_live_before"] and
                                                           e["image_appended"] > 0 for e in log)
        ev[f"appends more than {slack} rows between two re-packs"] = any(e["image_appended"] > slack for e in log)
    return ev


@pytest.mark.parametrize("D", [64, 100])
@pytest.mark.parametrize("index", [False, True], ids=["exact", "index"])
@pytest.mark.parametrize("policy", ["reference", "fifo", "weakest"])
def test_sequence(dev, hmod, policy, index, D):
    H, clock = hmod
    from aura_snn_rag_amd import ops

    def factory():
        hf = H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                    device="cuda", use_centroid_index=index, overflow=policy)
        hf.centroids_update_interval = INTERVAL
        return hf

    sizes = dict(SIZES, D=D, policy=policy, index=index)
    t0 = time.perf_counter()
    seq = B.run_sequence(factory, ops, SEED, STEPS, sizes, clock, plan=_Plan(index))
    st = seq.stats
    print(f"sequence {policy} index={index} D={D}: {time.perf_counter() - t0:.1f} s; {st}; ops {[e['op'] for e in seq.log]}; "
          f"counts {[e['count_after'] for e in seq.log]}")
    B.helpers.record_parity(f"sequence {policy} {'index' if index else 'exact'} D={D}", st["exact"], st["queries"],
                            st["near_ties"], positions_differed=st["differed"])
    missing = [name for name, ok in _events(seq, image=index and seq.hf._use_shadow).items() if not ok]
    assert not missing, f"never happened: {missing}\n" + "\n".join(str(e) for e in seq.log)
    # (d) the model's own near-ties: topk_equivalent's allowance must not be what makes the comparisons pass
    assert st["near_ties"] <= 0.05 * st["queries"], st


# ------------------------------------------------------------------------ per-tag quotas and merging within tags
QUOTAS = {1: 300, 2: 60, 3: 1500, 4: 5}
TAG_PROBS = [0.45, 0.15, 0.05, 0.2, 0.004, 0.146]            # tags 0 and 5 are unlimited: they fill the bank


def _named():
    return B.tagcase(QUOTAS, range(6), TAG_PROBS, small=2, mid=3, over=1, free=5)


def _every_tag():
    # tag_quota=40 for each of the tags 1 .. 100 (81 rows each after the first fill), a tenth of the rows untagged; one planned batch carries all 100 limited
    # tags (two library calls that share one bitmap); the plan names a quota of 600 for the tag whose ties it uses
    return B.tagcase(40, range(101), [0.1] + [0.009] * 100, small=1, mid=2, over=3, free=0, many=True, mid_quota=600)


def _merging():
    return B.tagcase(None, range(6), TAG_PROBS, small=2, mid=3, over=1, free=5)


TAG_CASES = {
    "quotas-exact-64": ("weakest", False, 64, _named),
    "quotas-index-64": ("weakest", True, 64, _named),
    "quotas-index-100": ("weakest", True, 100, _named),   # no bf16 image: the scoped search is the dense fp32 scan
    "every-tag-index-64": ("weakest", True, 64, _every_tag),
    "merging-fifo-index-64": ("fifo", True, 64, _merging),
    "merging-reference-exact-64": ("reference", False, 64, _merging),
}


def run_tag_case(H, clock, ops, name, device="cuda"):
    """One tag-aware case (``ops`` None: the library; on the CPU, tests/cpu_stub_quota.py with ``device='cpu'``)."""
    policy, index, D, case = TAG_CASES[name]
    tc = case()

    def factory():
        kw = {} if tc["quota"] is None else dict(tag_quota=tc["quota"])
        hf = H.HippocampalFormation(feature_dim=D, max_memories=M, n_place_cells=8, n_time_cells=4, n_grid_cells=4,
                                    device=device, use_centroid_index=index, overflow=policy, **kw)
        hf.centroids_update_interval = INTERVAL
        return hf

    # (the plan refills twice: a larger pool.  The cases with an index cost three to four times their test_sequence
    # counterpart with the repeat searches and the diverse recall after every step: there they run after every other one)
    sizes = dict(SIZES, D=D, policy=policy, index=index, tagcase=tc, pool_rows=26_000, extra_every=2 if index else 1)
    t0 = time.perf_counter()
    seq = B.run_sequence(factory, ops, SEED, STEPS, sizes, clock, plan=B.TagPlan(STEPS, tc, index, M, fill=FILL))
    return seq, time.perf_counter() - t0


@pytest.mark.parametrize("name", list(TAG_CASES))
def test_tag_sequence(dev, hmod, name):
    H, clock = hmod
    from aura_snn_rag_amd import ops
    seq, wall = run_tag_case(H, clock, ops, name)
    st = seq.stats
    print(f"tag sequence {name}: {wall:.1f} s; {st}; ops {[e['op'] for e in seq.log]}; "
          f"counts {[e['count_after'] for e in seq.log]}")
    B.helpers.record_parity(f"tag sequence {name}", st["exact"], st["queries"], st["near_ties"],
                            positions_differed=st["differed"], repeat_rows=st["repeat_rows"],
                            repeat_near_ties_accepted=st["repeat_near_ties"], wall_s=round(wall, 1))
    image = TAG_CASES[name][1] and seq.hf._use_shadow
    missing = [what for what, ok in B.tag_events(seq, live=LIVE if image else None).items() if not ok]
    assert not missing, f"never happened: {missing}\n" + "\n".join(str(e) for e in seq.log)
    assert st["near_ties"] <= 0.05 * st["queries"], st
    assert st["repeat_near_ties"] <= 0.01 * st["repeat_rows"], st
