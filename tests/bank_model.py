"""A plain model of the episodic bank and a driver that runs random operation sequences against it -- TEST
INFRASTRUCTURE ONLY (``tests/test_host_sequences.py`` on the CPU stubs, ``tests/test_gpu_sequences.py`` on the kernels).

The model (``BankModel``) holds the memories in order -- id, the fp32 feature row as written, location, strength,
fp32 timestamp, tag, centroid id -- and restates the documented rules with NumPy and torch fp64; no product code is in
it.  ``run_sequence`` draws a seeded sequence of operations, applies each to the bank and to the model, and after every
mutating operation checks

  (a) structure, exact: count, cursor, the id of every row, ``id_to_idx`` of the live ids, tags, feature / location /
      strength / timestamp bits, a zero tail;
  (b) every recall path against the model's fp64 scores (``helpers.topk_equivalent``: 1e-5 on scores, a position may
      differ only where the model's own scores are within 2e-6);
  (c) the bank against a bank rebuilt from ``state_dict()`` + ``bank_state()``: rows and score bits of the same
      recalls, ``_inv_norm``, the bf16 shadow and its residuals, bit for bit -- derived state kept current by hand
      must equal derived state built from nothing;
  (d) how many queries the model itself sees as near-ties (two adjacent fp64 scores of the top k + 1 within 2e-6):
      counted from the model alone, capped by the tests at 5 % so that (b)'s allowance cannot hide a wrong row.

Two kinds of decision are tested elsewhere with their own tolerances, and here the model checks that the device's
choice is admissible and then follows it: centroid ids (``memory_metadata[:, 2]`` and ``probe()`` are taken as given;
what is asserted is that an indexed recall returns the fp64 top-k among exactly the rows whose stored centroid id is
one of the query's probed lists, the full scan where that set is empty) and ``'weakest'`` victims (fp64 keys: every
victim within 1e-5 relative of the n-th smallest key, every clearly smaller key a victim, exact ties in ring order from
the cursor; 1e-5 is the fp32 rounding of ``strength * expf(x)``, a few ulp, with room).  ``prune(min_key=)`` is
followed in the same band.

A failure raises ``SequenceFailure`` with the seed, the step, the operation and the whole log, so a device failure can
be replayed on the CPU stubs."""
import numpy as np
import torch

from tests import helpers
from tests.cpu_stub_consolidate import rule as consolidate_rule
from tests.cpu_stub_retention import reinforce_reference
from tests.cpu_stub_scoped import scope_mask

TAU = 0.9
GAP = 0.02                      # the data keeps every cosine at least this far from TAU
NEAR_TIE = 2e-6
VICTIM_BAND = 1e-5
T0 = 1.7e9                      # a multiple of 128: every clock value is exact in fp32
NQ = 32
INF = float("inf")


class SequenceFailure(AssertionError):
    pass


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _unit64(x):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


# --------------------------------------------------------------------------------------------------------- the data
class Pool:
    """Rows in the order the sequence writes them: ``n_groups`` independent centres with 6 near-copies each
    (``centre + 0.05 randn``), the rest plain ``randn``; a group's members lie close together in the stream, so a batch
    holds new rows, near-copies of held rows and near-copies of each other."""

    def __init__(self, D, n_rows, n_groups, seed, device="cpu"):
        g = torch.Generator().manual_seed(seed)
        centres = torch.randn(n_groups, D, generator=g)
        copies = centres.repeat_interleave(6, 0) + 0.05 * torch.randn(6 * n_groups, D, generator=g)
        feats = torch.cat([copies, torch.randn(n_rows - 6 * n_groups, D, generator=g)])
        label = torch.cat([torch.arange(n_groups).repeat_interleave(6), n_groups + torch.arange(n_rows - 6 * n_groups)])
        if n_rows <= 4096:
            # few dimensions: two independent rows may come close to TAU; take the units (a group, a plain row) one
            # by one and leave out a unit that comes within 0.85 of what was taken before
            u = _unit64(feats)
            cos = (u @ u.t()).numpy()
            lab = label.numpy()
            taken = np.zeros(n_rows, dtype=bool)
            for unit in np.unique(lab):
                rows = np.nonzero(lab == unit)[0]
                if not taken.any() or cos[rows][:, taken].max() <= 0.85:
                    taken[rows] = True
            keep = torch.from_numpy(np.nonzero(taken)[0])
            feats, label = feats[keep], label[keep]
        n = feats.shape[0]
        base = torch.rand(int(label.max()) + 1, generator=g)
        key = base[label] + 0.02 * torch.rand(n, generator=g)
        order = torch.argsort(key)
        self.feats = feats[order].contiguous().to(device)
        self.label = label[order].to(device)
        self.centres = centres
        self.D, self.n, self.used = D, n, 0
        self.within, self.across = self._gap()
        assert self.within >= TAU + GAP and self.across <= TAU - GAP, \
            f"pool D={D} seed={seed}: smallest cosine inside a group {self.within:.4f}, largest across {self.across:.4f}"
        q = torch.cat([centres[torch.randint(0, n_groups, (NQ // 2,), generator=g)] + 0.3 * torch.randn(NQ // 2, D, generator=g),
                       torch.randn(NQ - NQ // 2, D, generator=g)])
        self.queries = q.contiguous().to(device)

    def _gap(self):
        """fp64: (smallest cosine inside a group, largest cosine between rows of different groups), every pair."""
        u = _unit64(self.feats)
        within, across = 1.0, -1.0
        for lo in range(0, self.n, 2048):
            c = u[lo:lo + 2048] @ u.t()
            same = self.label[lo:lo + 2048, None] == self.label[None, :]
            within = min(within, float(torch.where(same, c, torch.ones_like(c)).min()))
            across = max(across, float(torch.where(same, -torch.ones_like(c), c).max()))
        return within, across

    def left(self):
        return self.n - self.used

    def take(self, n):
        assert self.left() >= n
        f = self.feats[self.used:self.used + n].clone()
        self.used += n
        return f


_POOLS = {}


def pool_for(D, n_rows, n_groups, seed, device="cpu"):
    """One pool per (shape, seed, device), built and checked once; every sequence reads it from the start."""
    key = (D, n_rows, n_groups, seed, str(device))
    if key not in _POOLS:
        _POOLS[key] = Pool(D, n_rows, n_groups, seed, device)
    p = _POOLS[key]
    p.used = 0
    return p


# -------------------------------------------------------------------------------------------------------- the model
class BankModel:
    def __init__(self, M, D, S, policy, device, merge_reinforce=0.1, merge_cap=1.0):
        self.M, self.D, self.policy, self.dev = M, D, policy, torch.device(device)
        self.merge_reinforce, self.merge_cap = merge_reinforce, merge_cap
        z = dict(device=self.dev)
        self.feats = torch.zeros(M, D, **z)
        self.loc = torch.zeros(M, S, **z)
        self.strength = torch.zeros(M, **z)
        self.ts = torch.zeros(M, **z)
        self.tag = torch.zeros(M, dtype=torch.int64, **z)
        self.cid = torch.full((M,), -1.0, **z)              # copied from the device, never computed
        self.ids = [None] * M
        self.explicit = [False] * M
        self.count = 0
        self.cursor = 0

    # -- writes
    def _store(self, slots, ids, explicit, feats, loc, now, tags):
        last = {}
        for i, s in enumerate(slots):                       # a slot named twice: the last write wins
            last[int(s)] = i
        dst = torch.tensor(list(last.keys()), dtype=torch.int64, device=self.dev)
        src = torch.tensor(list(last.values()), dtype=torch.int64, device=self.dev)
        self.feats[dst] = feats[src]
        self.loc[dst] = loc.to(self.dev)
        self.strength[dst] = 1.0
        self.ts[dst] = float(np.float32(now))
        self.tag[dst] = 0 if tags is None else torch.as_tensor(np.asarray(tags), dtype=torch.int64, device=self.dev)[src]
        self.cid[dst] = -1.0
        for s, i in last.items():
            self.ids[s], self.explicit[s] = ids[i], explicit

    def write(self, ids, feats, loc, now, tags=None, explicit=True, select=None):
        """Rows go behind the held ones while there is room; then ``'reference'`` rewrites slot 0, ``'fifo'`` the ring
        from the cursor on, ``'weakest'`` the slots ``select(self, rows left, now)`` names (the device's victims,
        checked there).  Returns the number of rows that overwrote."""
        n, i, over = len(ids), 0, 0
        tags = None if tags is None else np.asarray(tags)
        while i < n:
            room = self.M - self.count
            if room > 0:
                m = min(room, n - i)
                slots = np.arange(self.count, self.count + m)
                self.count += m
            elif self.policy == "reference":
                m = n - i
                slots = np.zeros(m, dtype=np.int64)
            elif self.policy == "fifo":
                m = n - i
                slots = (self.cursor + np.arange(m)) % self.M
                self.cursor = (self.cursor + m) % self.M
            else:
                slots = select(self, n - i, now)
                m = len(slots)
                self.cursor = (self.cursor + m) % self.M
            over += 0 if room > 0 else m
            self._store(slots, ids[i:i + m], explicit, feats[i:i + m], loc, now, None if tags is None else tags[i:i + m])
            i += m
        return over

    def keys64(self, now, n=None):
        n = self.count if n is None else n
        now32 = float(np.float32(now))
        return self.strength[:n].double() * torch.exp(-(now32 - self.ts[:n].double()) / 3600.0)

    def check_victims(self, rows, count, cursor, now):
        """The device's ``n`` victims among the first ``count`` rows, in its order, against the fp64 keys."""
        rows = np.asarray(rows, dtype=np.int64)
        n = rows.size
        assert n and np.unique(rows).size == n and rows.min() >= 0 and rows.max() < count, "victims: not n distinct held rows"
        keys = self.keys64(now, count).cpu().numpy()
        ring = (np.arange(count) - cursor % count) % count
        order = np.lexsort((ring, keys))
        kth = keys[order[n - 1]]
        victim = np.zeros(count, dtype=bool)
        victim[rows] = True
        assert (keys[rows] <= kth * (1 + VICTIM_BAND)).all(), "a victim's key is above the n-th smallest"
        assert victim[keys < kth * (1 - VICTIM_BAND)].all(), "a row with a clearly smaller key was spared"
        ideal = order[:n]
        for i in np.nonzero(rows != ideal)[0].tolist():
            a, b = keys[rows[i]], keys[ideal[i]]
            assert a != b, f"victim {i}: equal keys out of ring order (row {rows[i]}, expected {ideal[i]})"
            assert abs(a - b) <= VICTIM_BAND * max(a, b), f"victim {i}: row {rows[i]} (key {a}) before row {ideal[i]} (key {b})"

    def _best_held(self, fn, held):
        """(largest cosine of every row of ``fn`` to the unit rows ``held``, the LOWEST row that attains it)."""
        n = fn.shape[0]
        if held.shape[0] == 0:
            return torch.full((n, 1), -INF, dtype=torch.float64), torch.zeros(n, dtype=torch.int64)
        cs = fn @ held.t()
        best = cs.max(1).values
        arg = (cs == best[:, None]).to(torch.int8).argmax(1)
        return best[:, None].cpu(), arg.cpu()

    def _decide(self, fn, held, tau):
        best, arg = self._best_held(fn, held)
        stored, leader, _ = consolidate_rule(best, (fn @ fn.t()).cpu(), tau)      # column 0 stands for the best held row
        return torch.where(stored >= 0, arg, stored).numpy(), leader.numpy()

    def write_merge(self, ids, feats, loc, now, tau, select=None):
        """A consolidating write, in chunks of 1024: the rule on fp64 cosines; the distinct stored targets are
        reinforced and take the write's timestamp BEFORE the kept rows are written."""
        kept_ids, over = [], 0
        for lo in range(0, len(ids), 1024):
            f = feats[lo:lo + 1024]
            stored, leader = self._decide(_unit64(f), _unit64(self.feats[:self.count]), tau)
            targets = np.unique(stored[stored >= 0])
            if targets.size:
                self.reinforce(targets, self.merge_reinforce, self.merge_cap)
                self.touch(targets, now)
            kept = np.nonzero((stored < 0) & (leader < 0))[0]
            if kept.size:
                kid = [ids[lo + i] for i in kept.tolist()]
                over += self.write(kid, f[torch.from_numpy(kept).to(f.device)], loc, now, select=select)
                kept_ids += kid
        return kept_ids, over

    # -- strengths, timestamps, tags
    def _held(self, rows):
        r = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
        return r[(r >= 0) & (r < self.count)]

    def decay(self, rate):
        self.strength[:self.count] *= float(np.float32(1.0) - np.float32(rate))       # fp32, as the kernel

    def reinforce(self, rows, amount, cap=1.0):
        r = torch.as_tensor(np.asarray(rows, dtype=np.int64).reshape(-1))
        meta = reinforce_reference(self.strength.cpu()[:, None].clone(), self.count, r, amount, cap)
        self.strength.copy_(meta[:, 0])

    def touch(self, rows, now):
        self.ts[torch.from_numpy(self._held(rows)).to(self.dev)] = float(np.float32(now))

    def retag(self, rows, tag):
        self.tag[torch.from_numpy(self._held(rows)).to(self.dev)] = int(tag)

    def rows_of_ids(self, ids):
        where = {mid: r for r, mid in enumerate(self.ids[:self.count]) if self.explicit[r]}
        return np.asarray([where[m] for m in ids], dtype=np.int64)

    # -- compaction
    def _ring_start(self):
        return self.cursor % self.M if self.policy in ("fifo", "weakest") and self.count == self.M else 0

    def _reorder(self, order):
        o = torch.from_numpy(np.asarray(order, dtype=np.int64)).to(self.dev)
        k = o.numel()
        for name in ("feats", "loc", "strength", "ts", "tag", "cid"):
            a = getattr(self, name)
            moved = a[o].clone()
            a[:self.count] = 0
            a[:k] = moved
        ids = [self.ids[r] for r in order]
        ex = [self.explicit[r] for r in order]
        self.ids = ids + [None] * (self.M - k)
        self.explicit = ex + [False] * (self.M - k)
        self.count, self.cursor = k, 0

    def forget(self, kill):
        """Take the rows ``kill`` out: the survivors in ring order, oldest first; the cursor is 0."""
        kill = self._held(kill)
        if kill.size == 0:
            return 0
        keep = np.ones(self.count, dtype=bool)
        keep[kill] = False
        start = self._ring_start()
        self._reorder(np.concatenate([start + np.nonzero(keep[start:])[0], np.nonzero(keep[:start])[0]]))
        return int(kill.size)

    def rows_with_tags(self, tags):
        return np.nonzero(np.isin(self.tag[:self.count].cpu().numpy(), np.asarray(tags)))[0]

    def consolidate(self, tau):
        """What writing the rows, oldest first, into an empty bank through consolidating writes in chunks of 1024
        leaves: a kept row takes the largest strength and the latest timestamp of the rows merged into it, then the
        distinct stored targets of a chunk are reinforced once."""
        start = self._ring_start()
        if start:
            self._reorder(np.concatenate([np.arange(start, self.count), np.arange(start)]))
        count = self.count
        if count == 0:
            return 0
        u = _unit64(self.feats[:count])
        S, T = self.strength.cpu().clone(), self.ts.cpu().clone()
        kept_rows = []
        for lo in range(0, count, 1024):
            hi = min(count, lo + 1024)
            prefix = torch.as_tensor(kept_rows, dtype=torch.int64, device=self.dev)
            stored, leader = self._decide(u[lo:hi], u[prefix], tau)
            for i in np.nonzero((stored >= 0) | (leader >= 0))[0].tolist():
                t = kept_rows[stored[i]] if stored[i] >= 0 else lo + int(leader[i])
                S[t], T[t] = max(S[t], S[lo + i]), max(T[t], T[lo + i])
            targets = np.unique(stored[stored >= 0])
            if targets.size:
                t = torch.as_tensor([kept_rows[j] for j in targets.tolist()])
                S = reinforce_reference(S[:, None].clone(), count, t, self.merge_reinforce, self.merge_cap)[:, 0]
            kept_rows += (lo + np.nonzero((stored < 0) & (leader < 0))[0]).tolist()
        self.strength.copy_(S)
        self.ts.copy_(T)
        self._reorder(kept_rows)
        return count - len(kept_rows)

    # -- scoring
    def meta(self):
        n = self.count
        return torch.stack([self.strength[:n], self.ts[:n], self.cid[:n], self.tag[:n].float()], dim=1)

    def scores(self, q, now):
        """fp64 [nq, count]: ``(0.5 cos + 0.3 * 0 + 0.2 exp(-(now - t) / 3600)) * strength`` (no query location)."""
        n = self.count
        cos = _unit64(q) @ _unit64(self.feats[:n]).t()
        temporal = torch.exp(-(float(np.float32(now)) - self.ts[:n].double()) / 3600.0)
        return (0.5 * cos + 0.2 * temporal[None, :]) * self.strength[:n].double()[None, :]

    @staticmethod
    def topk(masked, k):
        """Descending, equal scores to the lower row, ``-inf`` / ``-1`` where a query has fewer than k rows."""
        vals, idx = torch.sort(masked, dim=1, descending=True, stable=True)
        vals, idx = vals[:, :k], idx[:, :k]
        return vals, torch.where(vals == -INF, torch.full_like(idx, -1), idx)


# ------------------------------------------------------------------------------------------------------- the driver
class _Spy:
    """Records what ``ops.bank_select_weakest`` answers while a write runs (the model follows those victims)."""

    def __init__(self, ops):
        self.ops, self.calls = ops, []

    def __enter__(self):
        self.orig = self.ops.bank_select_weakest

        def spy(meta, count, now, cursor, n):
            rows, keys = self.orig(meta, count, now, cursor, n)
            self.calls.append(dict(count=int(count), now=now, cursor=int(cursor), n=int(n),
                                   rows=rows.detach().cpu().numpy().astype(np.int64).copy()))
            return rows, keys
        self.ops.bank_select_weakest = spy
        return self

    def __exit__(self, *exc):
        self.ops.bank_select_weakest = self.orig


class Clock:
    """The fake ``time.time`` of a test module: ``H.time.time`` is patched to ``clock``."""

    def __init__(self):
        self.now = T0

    def __call__(self):
        return self.now


class Sequence:
    def __init__(self, hf_factory, ops, seed, sizes, clock):
        if ops is None:
            from aura_snn_rag_amd import ops
        self.factory, self.ops, self.seed, self.z, self.clock = hf_factory, ops, seed, sizes, clock
        self.rng = np.random.default_rng(seed)
        torch.manual_seed(seed)
        clock.now = T0
        self.hf = hf_factory()
        self.dev = self.hf.memory_features.device
        self.cuda = self.dev.type == "cuda"
        z = sizes
        self.model = BankModel(z["M"], z["D"], self.hf.memory_locations.shape[1], z["policy"], self.dev)
        self.pool = pool_for(z["D"], z["pool_rows"], z["pool_groups"], z.get("pool_seed", 0), self.dev)
        self.q = self.pool.queries
        self.k = 8
        self.log = []
        self.next_id = 0
        self.next_bulk = 0
        self.stats = dict(queries=0, near_ties=0, differed=0, exact=0)
        self.step = -1

    # -- helpers
    def _ids(self, n):
        out = [f"s{self.seed}-m{self.next_id + i}" for i in range(n)]
        self.next_id += n
        return out

    def _move(self):
        loc = torch.from_numpy(self.rng.standard_normal(self.model.loc.shape[1]).astype(np.float32))
        self.hf.update_spatial_state(loc.to(self.dev))
        return loc

    def _select(self, spy):
        def select(model, left, now):
            assert spy.calls, "the write asked for no victims where the model needs some"
            c = spy.calls.pop(0)
            assert c["n"] <= left and c["cursor"] == model.cursor and c["count"] <= model.count, f"victim request {c}"
            if not self.z["index"]:
                assert c["n"] == min(left, model.M), "without an index a batch is one run"
            model.check_victims(c["rows"], c["count"], c["cursor"], c["now"])
            return c["rows"]
        return select

    def _rows(self, n, wild=False):
        r = self.rng.integers(0, self.model.count, size=n)
        if wild:                                            # -1, rows outside the bank, duplicates: all ignored
            r = np.concatenate([r, [-1, self.model.count, self.model.M + 5], r[:2]])
        return r

    def _ivf(self):
        st = getattr(self.hf, "_ivf", None)
        return st if st is not None and st.valid else None

    # -- operations: each applies itself to the bank and to the model and returns what the log should say
    def op_write(self, n, tagged):
        ids, f, loc, now = self._ids(n), self.pool.take(n), self._move(), self.clock.now
        tags = self.rng.integers(1, 5, size=n) if tagged else None
        with _Spy(self.ops) as spy:
            self.hf.create_episodic_memories(ids, f, tags=tags)
            over = self.model.write(ids, f, loc, now, tags=tags, select=self._select(spy))
            assert not spy.calls, "the write asked for more victims than the model placed"
        return dict(n=n, tagged=tagged, over=over)

    def op_write_merge(self, n):
        ids, f, loc, now = self._ids(n), self.pool.take(n), self._move(), self.clock.now
        with _Spy(self.ops) as spy:
            rep = self.hf.create_episodic_memories(ids, f, merge_similarity=TAU)
            kept, over = self.model.write_merge(ids, f, loc, now, TAU, select=self._select(spy))
            assert not spy.calls, "the write asked for more victims than the model placed"
        assert rep.n_stored == len(kept) and [i for i, m in zip(ids, rep.merged.tolist()) if not m] == kept, \
            f"the write kept {rep.n_stored} rows, the fp64 rule keeps {len(kept)}"
        return dict(n=n, kept=len(kept), over=over)

    def op_bulk(self, n, rebuild, tagged):
        f, loc, now = self.pool.take(n), self._move(), self.clock.now
        prefix, first = f"s{self.seed}-b{self.next_bulk}-", int(self.rng.integers(0, 1000))
        self.next_bulk += 1
        tags = self.rng.integers(0, 5, size=n) if tagged else None
        assert self.hf.bulk_write(f, id_prefix=prefix, first_index=first, rebuild=rebuild, tags=tags) == n
        m = self.model
        m._store(np.arange(m.count, m.count + n), [f"{prefix}{first + i}" for i in range(n)], False, f, loc, now, tags)
        m.count += n
        return dict(n=n, rebuild=rebuild, tagged=tagged)

    def op_decay(self):
        rate = float(self.rng.choice([0.0625, 0.125]))      # exact in binary: 1 - rate is the same in fp32 and fp64
        self.hf.decay_memories(rate)
        self.model.decay(rate)
        return dict(rate=rate)

    def op_reinforce(self):
        rows = self._rows(int(self.rng.integers(1, 40)), wild=True)
        self.hf.reinforce(torch.from_numpy(rows), amount=0.25, cap=1.0)
        self.model.reinforce(rows, 0.25, 1.0)
        return dict(rows=rows.size)

    def op_recall_reinforce(self, index):
        m, now = self.model, self.clock.now
        k = min(self.k, m.count)
        scores, rows = self.hf.recall_batch(self.q, k=self.k, now=now, use_candidates=index, reinforce=0.1)
        full = self._masked(self._cand_mask() if index and self.hf._candidate_mode() else None, now)
        self._compare("recall+reinforce", rows, scores, full, k)
        m.reinforce(rows.cpu().numpy(), 0.1, 1.0)           # (the rows the bank returned: the two stay in step)
        return dict(index=index)

    def op_touch(self):
        rows = self._rows(int(self.rng.integers(1, 40)), wild=True)
        self.hf.touch(torch.from_numpy(rows))
        self.model.touch(rows, self.clock.now)
        return dict(rows=rows.size)

    def op_retag(self, by_ids):
        m, tag = self.model, int(self.rng.integers(0, 5))
        live = [m.ids[r] for r in range(m.count) if m.explicit[r]]
        if by_ids and live:
            ids = [live[i] for i in self.rng.integers(0, len(live), size=min(5, len(live)))]
            assert self.hf.retag(ids=ids, tag=tag) == len(set(ids))
            m.retag(m.rows_of_ids(ids), tag)
            return dict(ids=len(ids), tag=tag)
        rows = self._rows(int(self.rng.integers(1, 40)), wild=True)
        assert self.hf.retag(rows=rows, tag=tag) == m._held(rows).size
        m.retag(rows, tag)
        return dict(rows=rows.size, tag=tag)

    def op_edit(self):
        m = self.model
        vals = torch.from_numpy((0.25 + 0.75 * self.rng.random(m.count)).astype(np.float32)).to(self.dev)
        self.hf.memory_metadata[:m.count, 0] = vals         # the documented way to set strengths, seen through _version
        m.strength[:m.count] = vals
        return {}

    def _forget(self, kind, kill, **kw):
        m = self.model
        c0 = m.count
        rep = self.hf.forget(**kw)
        n = m.forget(kill)
        assert rep.n_removed == n and rep.old_to_new.shape == (c0,) and int((rep.old_to_new < 0).sum()) == n
        return dict(kind=kind, removed=n)

    def op_forget(self, kind, n=None):
        m = self.model
        if kind == "ids":
            live = [m.ids[r] for r in range(m.count) if m.explicit[r]]
            if live:
                ids = [live[i] for i in self.rng.integers(0, len(live), size=min(6, len(live)))]
                return self._forget(kind, m.rows_of_ids(ids), ids=ids)
            kind = "rows"
        if kind == "tags":
            tags = [int(self.rng.integers(1, 5))]
            return self._forget(kind, m.rows_with_tags(tags), tags=tags)
        n = int(self.rng.integers(1, max(2, m.count // 16))) if n is None else n
        rows = self.rng.choice(m.count, size=min(n, m.count), replace=False)
        rows = np.concatenate([rows, [-1, m.M + 1], rows[:1]])
        return self._forget(kind, rows, rows=torch.from_numpy(rows))

    def op_prune(self, by_key, frac=None):
        m, now = self.model, self.clock.now
        frac = float(self.rng.uniform(0.02, 0.15)) if frac is None else frac
        c0 = m.count
        if not by_key:
            thr = float(torch.quantile(m.strength[:c0].double(), frac, interpolation="lower"))   # a held fp32 value
            kill = np.nonzero((m.strength[:c0] < thr).cpu().numpy())[0]
            rep = self.hf.prune(min_strength=thr)
        else:
            keys = m.keys64(now).cpu().numpy()
            thr = float(np.quantile(keys, frac)) * (1 + 3e-5)
            rep = self.hf.prune(min_key=thr, now=now)
            kill = np.nonzero(rep.old_to_new < 0)[0]        # the device's fp32 comparison, followed inside the band
            gone = np.zeros(c0, dtype=bool)
            gone[kill] = True
            assert gone[keys < thr * (1 - VICTIM_BAND)].all(), "prune spared a row clearly below min_key"
            assert not gone[keys > thr * (1 + VICTIM_BAND)].any(), "prune removed a row clearly above min_key"
        n = m.forget(kill)
        assert rep.n_removed == n, f"prune removed {rep.n_removed} rows, the model {n}"
        return dict(by_key=by_key, removed=n)

    def op_consolidate(self, rebuild):
        rep = self.hf.consolidate(TAU, rebuild=rebuild)
        n = self.model.consolidate(TAU)
        assert rep.n_merged == n, f"consolidate merged {rep.n_merged} rows, the fp64 rule {n}"
        return dict(rebuild=rebuild, merged=n)

    def op_rebuild(self):
        self.hf.rebuild_centroids()
        return {}

    def _reloaded(self):
        new = self.factory()
        new.load_state_dict(self.hf.state_dict())
        new.load_bank_state(self.hf.bank_state())
        return new

    def op_checkpoint(self):
        self.hf = self._reloaded()
        return {}

    # -- the checks
    def _cand_mask(self):
        """bool [nq, count]: the rows whose stored centroid id is one of the query's probed lists (all rows where that
        set is empty: the full-scan fallback).  The probes are the device's; on the CPU, the stub's formula."""
        hf, m = self.hf, self.model
        probes = hf.probe(self.q)
        if probes is None:
            nprobe = min(8, hf.centroids_k)
            probes = torch.stack([torch.topk(-torch.norm(hf.centroids - self.q[i], dim=1), k=nprobe).indices
                                  for i in range(self.q.shape[0])])
        mask = (m.cid[None, :m.count, None] == probes[:, None, :].to(m.cid.dtype)).any(-1)
        return torch.where(mask.any(1, keepdim=True), mask, torch.ones_like(mask))

    def _masked(self, mask, now):
        s = self.model.scores(self.q, now)
        return s if mask is None else torch.where(mask, s, torch.full_like(s, -INF))

    def _compare(self, what, rows, scores, full, k):
        ref_s, ref_i = BankModel.topk(full, k)
        assert rows.shape == ref_i.shape, f"{what}: result shape {tuple(rows.shape)}, expected {tuple(ref_i.shape)}"
        exact, n, ok = helpers.topk_equivalent(rows, scores.double(), ref_i, ref_s.cpu(), full.cpu())
        top = torch.sort(full, dim=1, descending=True).values[:, :k + 1]
        gaps = top[:, :-1] - top[:, 1:]
        ties = int(((gaps < NEAR_TIE) & torch.isfinite(gaps)).any(1).sum())
        st = self.stats
        st["queries"] += n
        st["exact"] += exact
        st["near_ties"] += ties
        st["differed"] += int((rows.cpu().long() != ref_i.cpu()).sum())
        assert ok, f"{what} (k={k}): not the model's top-k ({exact} of {n} queries index-exact)"

    def _scope(self):
        """The scoped recall of this step: kwargs for ``recall_batch`` and the model's mask."""
        m, kind = self.model, self.step % 5
        meta = m.meta()
        if kind == 0:
            qt = np.asarray([(i % 6) - 1 for i in range(NQ)], dtype=np.int64)        # -1, 0 (untagged), 1 .. 4
            return dict(tags=qt), torch.stack([scope_mask(meta, m.count, int(t)) for t in qt])
        if kind == 1:
            kw = dict(tags=2)
        elif kind == 2:
            kw = dict(tags=-1)
        elif kind == 3:                                     # a window whose ends sit on stored timestamps
            t = torch.unique(m.ts[:m.count]).cpu().double()
            kw = dict(newer_than=float(t[(len(t) - 1) // 3]), older_than=float(t[(2 * len(t)) // 3]))
        else:
            kw = dict(min_strength=float(m.strength[:m.count].median()))
        one = scope_mask(meta, m.count, kw.get("tags", -1), kw.get("newer_than"), kw.get("older_than"), kw.get("min_strength"))
        return kw, one[None, :].expand(NQ, -1)

    def _recalls(self):
        """The recalls of this step: (name, k, kwargs, the model's mask or None, query replicas)."""
        hf, m = self.hf, self.model
        ks = [self.k] + ([1, 33] if self.step % 5 == 0 else [])
        out = [("exact", k, dict(use_candidates=False), None, 1) for k in ks]
        indexed = self.z["index"] and hf._candidate_mode()
        if indexed:
            mask = self._cand_mask()
            out += [("index", k, dict(use_candidates=True), mask, 1) for k in ks]
            if self.cuda:                                   # more than MASKED_SCAN_MAX_QUERIES: the inverted lists
                out += [("lists", k, dict(use_candidates=True), mask, 17) for k in ks]
        kw, mask = self._scope()
        out.append(("scoped:" + ",".join(kw), self.k, kw, mask, 1))
        return out, indexed

    def check(self):
        hf, m, now = self.hf, self.model, self.clock.now
        n, M = m.count, m.M
        # (a) structure, exact
        assert hf.memory_count == n, f"memory_count {hf.memory_count}, the model holds {n}"
        assert hf._write_cursor % M == m.cursor, f"write cursor {hf._write_cursor} (mod {M}), the model's {m.cursor}"
        got = [hf.id_of_row(r) for r in range(n)]
        if got != m.ids[:n]:
            r = next(i for i in range(n) if got[i] != m.ids[i])
            raise AssertionError(f"id_of_row({r}) = {got[r]!r}, the model holds {m.ids[r]!r}")
        for r in range(n):
            if m.explicit[r]:
                assert hf.id_to_idx.get(m.ids[r]) == r, f"id_to_idx[{m.ids[r]!r}] = {hf.id_to_idx.get(m.ids[r])}, held at row {r}"
        meta = hf.memory_metadata
        assert torch.equal(hf.memory_tags.long(), m.tag[:n]), "memory_tags differ"
        assert torch.equal(_bits(hf.memory_features[:n]), _bits(m.feats[:n])), "feature bits differ"
        assert torch.equal(_bits(hf.memory_locations[:n]), _bits(m.loc[:n])), "location bits differ"
        assert torch.equal(_bits(meta[:n, 0]), _bits(m.strength[:n])), \
            f"strength bits differ at rows {torch.nonzero(meta[:n, 0] != m.strength[:n]).flatten()[:8].tolist()}"
        assert torch.equal(_bits(meta[:n, 1]), _bits(m.ts[:n])), \
            f"timestamp bits differ at rows {torch.nonzero(meta[:n, 1] != m.ts[:n]).flatten()[:8].tolist()}"
        for name, a in (("features", hf.memory_features), ("locations", hf.memory_locations), ("metadata", meta)):
            assert not bool(a[n:].any()), f"the tail of {name} behind row {n} is not zero"
        m.cid[:n] = meta[:n, 2]
        if n == 0:
            return False
        # (b) every recall path against the model, (c) against a bank rebuilt from the checkpoint
        fresh = self._reloaded()
        recalls, indexed = self._recalls()
        for name, k, kw, mask, reps in recalls:
            q = self.q if reps == 1 else self.q.repeat(reps, 1)
            kk = min(k, n)
            s1, r1 = hf.recall_batch(q, k=k, now=now, **kw)
            s2, r2 = fresh.recall_batch(q, k=k, now=now, **kw)
            self._compare(name, r1[:NQ], s1[:NQ], self._masked(mask, now), kk)
            for j in range(1, reps):
                assert torch.equal(r1[j * NQ:(j + 1) * NQ], r1[:NQ]) and torch.equal(_bits(s1[j * NQ:(j + 1) * NQ]), _bits(s1[:NQ])), \
                    f"{name} (k={k}): the same query gives different results at two places of the batch"
            assert torch.equal(r1, r2), f"{name} (k={k}): rows differ from the bank rebuilt from the checkpoint"
            assert torch.equal(_bits(s1), _bits(s2)), f"{name} (k={k}): score bits differ from the bank rebuilt from the checkpoint"
        hf._ensure_norms()
        fresh._ensure_norms()
        if self.cuda:                                       # (the CPU stand-ins compute 1/||row|| two ways)
            assert torch.equal(_bits(hf._inv_norm[:n]), _bits(fresh._inv_norm[:n])), "_inv_norm differs from the rebuilt bank's"
        else:
            assert torch.allclose(hf._inv_norm[:n], fresh._inv_norm[:n], rtol=1e-6, atol=0), "_inv_norm differs from the rebuilt bank's"
        if hf._shadow is not None and fresh._shadow is not None:
            u = min(hf._shadow_valid_upto, fresh._shadow_valid_upto, n)
            assert torch.equal(_bits(hf._shadow[:u]), _bits(fresh._shadow[:u])), "the bf16 shadow differs from the rebuilt bank's"
            assert torch.equal(_bits(hf._rho[:u]), _bits(fresh._rho[:u])), "the shadow's residuals differ from the rebuilt bank's"
        return indexed

    # -- the sequence
    def random_op(self):
        m, z, rng = self.model, self.z, self.rng
        room = m.M - m.count
        batches = [b for b in z["batches"] if b <= self.pool.left()]
        w = {}
        if batches:
            w.update(write=5, write_merge=2)
            if room > 0:
                w["bulk"] = 2
        if m.count:
            w.update(decay=1, reinforce=1, recall_reinforce=2, touch=1, retag=2, edit=1, forget=3, prune=2,
                     consolidate=1, checkpoint=1)
            if z["index"]:
                w["rebuild"] = 1
        names = list(w)
        p = np.asarray([w[x] for x in names], dtype=np.float64)
        op = names[int(rng.choice(len(names), p=p / p.sum()))]
        bw = np.asarray(z.get("batch_weights", [1] * len(z["batches"]))[:len(batches)], dtype=np.float64)
        if op == "write":
            return op, lambda: self.op_write(int(rng.choice(batches, p=bw / bw.sum())), bool(rng.integers(0, 2)))
        if op == "write_merge":
            return op, lambda: self.op_write_merge(int(rng.choice(batches, p=bw / bw.sum())))
        if op == "bulk":
            return op, lambda: self.op_bulk(min(int(rng.choice(batches, p=bw / bw.sum())), room), bool(rng.integers(0, 2)),
                                            bool(rng.integers(0, 2)))
        if op == "recall_reinforce":
            return op, lambda: self.op_recall_reinforce(bool(rng.integers(0, 2)))
        if op == "retag":
            return op, lambda: self.op_retag(bool(rng.integers(0, 2)))
        if op == "forget":
            return op, lambda: self.op_forget(str(rng.choice(["rows", "ids", "tags"])))
        if op == "prune":
            return op, lambda: self.op_prune(bool(rng.integers(0, 2)))
        if op == "consolidate":
            return op, lambda: self.op_consolidate(bool(rng.integers(0, 2)))
        return op, getattr(self, "op_" + op)

    def run_step(self, op, fn, still=False):
        """One operation on the bank and the model, then the checks.  The clock moves first, by a multiple of 128 s (the
        spacing of fp32 timestamps today) -- every sixth time, and with ``still``, by nothing: what is cached per
        ``now`` then has to notice the operation by itself."""
        self.step += 1
        dt = 128.0 * int(self.rng.integers(0, 6))
        self.clock.now += 0.0 if still else dt
        m = self.model
        ivf = self._ivf()
        entry = dict(step=self.step, op=op, now=self.clock.now, still=still or dt == 0.0, count_before=m.count,
                     image_live_before=ivf is not None)
        self.log.append(entry)
        try:
            entry.update(fn() or {})
            entry["count_after"] = m.count
            entry["indexed_recall_checked"] = bool(self.check())
            ivf = self._ivf()
            entry["image_appended"] = ivf.appended if ivf is not None else 0
        except SequenceFailure:
            raise
        except Exception as e:
            lines = "\n".join(f"  {x}" for x in self.log)
            raise SequenceFailure(f"seed {self.seed}, step {self.step}, op {op!r} ({self.z['policy']}, index "
                                  f"{self.z['index']}, D={self.z['D']}): {type(e).__name__}: {e}\nop log:\n{lines}") from e


def run_sequence(hf_factory, ops, seed, steps, sizes, clock, plan=None):
    """Run ``steps`` operations of the seeded sequence on ``hf_factory()`` and on the model, with the checks after
    every one.  ``ops``: the module the bank's ``ops`` is patched to (None: the library's).  ``sizes``: ``M``, ``D``,
    ``policy``, ``index``, ``batches`` (+ ``batch_weights``), ``pool_rows`` / ``pool_groups`` / ``pool_seed``.
    ``plan(seq)``: called before every step; it may return ``(op name, callable)`` or ``(op name, callable, still)``
    to force that step's operation (``still``: the clock does not move before it).
    Returns the ``Sequence`` (``log``, ``stats``, ``hf``, ``model``)."""
    seq = Sequence(hf_factory, ops, seed, sizes, clock)
    for _ in range(steps):
        forced = plan(seq) if plan is not None else None
        seq.run_step(*(forced if forced is not None else seq.random_op()))
    return seq
