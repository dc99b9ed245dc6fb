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

The tag-aware cases (``sizes["tagcase"]``, see ``tagcase``) put per-tag quotas and merging within tags through the same
machine.  The model keeps ``quota`` and ``origin`` itself and restates the "Per-tag quotas" rule of
``include/aura_hip.h``: a write is followed run by run (``_RunSpy`` records the runs ``hf._write_rows`` sees and the
selections each asks for); every run obeys the cap ``min(rows left, M, quota prefix)`` and ends earlier only at a
centroid-rebuild boundary; ``held_t`` and ``x_t`` are exact; the tag victims are checked per tag in the band above, ties
in ring order from the tag's own origin, the global victims among the rows that are no tag victim of the run; slots,
origins (last victim + 1) and the cursor follow the rule.  ``forget``, ``prune``, ``consolidate`` and
``enforce_tag_quotas`` remap the origins by the rule as written (the number of survivors before the origin in ring
order); ``bulk_write``, ``retag``, a changed quota and a checkpoint leave them (a checkpoint taken with no quota set
carries none).  Merging within tags is the fp64 rule on cosines masked by tag equality.  (a) then also compares
``tag_counts()``, ``tag_quotas``, ``_tag_origin`` and the quota keys of ``bank_state()``; (b) a read-only repeat search,
scope-blind and with drawn tags, over the next 48 rows of the pool (``leader`` and merged / kept exact, ``stored``
exact unless the two best eligible held cosines are within 1e-6 in fp64 -- counted from the model alone, capped by the
tests at 1 % --, ``cos`` within 1e-5); (c) the same searches and one diverse recall against the rebuilt bank, bit for
bit.  ``TagPlan`` plans part of such a sequence and ``tag_events`` names what every case must contain.

A failure raises ``SequenceFailure`` with the seed, the step, the operation and the whole log (in the tag-aware cases
with the run lengths, the tag victims per scope, the global victims and the origins before and after), so a device
failure can be replayed on the CPU stubs."""
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
        self.quota = {}                                     # named tags (0 may be named)
        self.quota_default = None                           # every tag except 0
        self.origin = {}                                    # tie origin per tag (missing: 0)
        self.index_interval = None                          # set by the driver when the bank keeps a centroid index

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

    def check_victims(self, rows, count, cursor, now, among=None, what="victims"):
        """The device's ``n`` victims among the first ``count`` rows (``among``: bool [count], the rows that may be
        taken -- a tag's rows, or the rows that are no tag victim of the run; None: all), in its order, against the
        fp64 keys, ties in ring order from ``cursor`` (the bank's cursor, or the tag's origin)."""
        rows = np.asarray(rows, dtype=np.int64)
        n = rows.size
        cand = np.arange(count) if among is None else np.nonzero(among)[0]
        assert n and np.unique(rows).size == n and np.isin(rows, cand).all() and n <= cand.size, \
            f"{what}: not n distinct held rows that may be taken"
        keys = self.keys64(now, count).cpu().numpy()
        ring = (np.arange(count) - cursor % count) % count
        order = cand[np.lexsort((ring[cand], keys[cand]))]
        kth = keys[order[n - 1]]
        victim = np.zeros(count, dtype=bool)
        victim[rows] = True
        assert (keys[rows] <= kth * (1 + VICTIM_BAND)).all(), f"{what}: a victim's key is above the n-th smallest"
        assert victim[cand[keys[cand] < kth * (1 - VICTIM_BAND)]].all(), f"{what}: a row with a clearly smaller key was spared"
        ideal = order[:n]
        for i in np.nonzero(rows != ideal)[0].tolist():
            a, b = keys[rows[i]], keys[ideal[i]]
            assert a != b, f"{what} {i}: equal keys out of ring order (row {rows[i]}, expected {ideal[i]})"
            assert abs(a - b) <= VICTIM_BAND * max(a, b), f"{what} {i}: row {rows[i]} (key {a}) before row {ideal[i]} (key {b})"

    def exact_order(self, count, cursor, now, among, n):
        """The first ``n`` rows of ``among`` by (fp64 key, ring position from ``cursor``): what another origin would
        have taken (used to show that an origin mattered, never to judge the device)."""
        keys = self.keys64(now, count).cpu().numpy()
        cand = np.nonzero(among)[0]
        ring = (np.arange(count) - cursor % count) % count
        return cand[np.lexsort((ring[cand], keys[cand]))][:n]

    # -- per-tag quotas (the rule: include/aura_hip.h, "Per-tag quotas")
    def quota_of(self, t):
        q = self.quota.get(int(t))
        return self.quota_default if q is None and int(t) != 0 else q

    def set_quota(self, tag, q):
        if tag is None:
            self.quota_default = q
        elif q is None:
            self.quota.pop(int(tag), None)
        else:
            self.quota[int(tag)] = int(q)

    def quotas_view(self):
        return {**self.quota, **({None: self.quota_default} if self.quota_default is not None else {})}

    def has_quota(self):
        return bool(self.quota) or self.quota_default is not None

    def tags_np(self, count=None):
        return self.tag[:self.count if count is None else count].cpu().numpy()

    def limited_counts(self):
        """{tag: rows held} of the limited tags: the named ones, and with a default every tag but 0 that is held."""
        held = self.tags_np()
        tags = set(self.quota) | ({int(t) for t in np.unique(held) if t != 0} if self.quota_default is not None else set())
        return {t: int((held == t).sum()) for t in sorted(tags)}

    def quota_prefix(self, tags):
        """The longest prefix of ``tags`` with at most q(t) rows of each limited tag t."""
        seen = {}
        for i, t in enumerate(np.asarray(tags).tolist()):
            q = self.quota_of(t)
            if q is not None:
                seen[t] = seen.get(t, 0) + 1
                if seen[t] > q:
                    return i
        return len(tags)

    def write_runs(self, ids, feats, loc, now, tags, runs, explicit=True):
        """A write under ``'weakest'`` as the runs the bank made of it (``runs``: per ``_write_rows`` call its length
        and the selections it asked the device for).  Every run obeys the rule's steps 1 - 4 on the rows held before
        it; the device's victims are checked in the band and followed.  Returns one report per run."""
        n, M, i, out = len(ids), self.M, 0, []
        tg = np.zeros(n, dtype=np.int64) if tags is None else np.asarray(tags, dtype=np.int64)
        while i < n:
            assert runs, f"the bank wrote {i} of {n} rows and stopped"
            run = runs.pop(0)
            m, left, count = int(run["n"]), n - i, self.count
            whole = min(left, M)
            cap = min(whole, self.quota_prefix(tg[i:i + whole]))
            assert 1 <= m <= cap, f"a run of {m} rows where the cap is {cap}"
            if m < cap:                                     # only a centroid-rebuild boundary ends a run earlier
                iv = self.index_interval
                assert iv and ((count < M and m == min(iv - count % iv, M - count)) or
                               (count == M and M % iv == 0 and m == 1)), f"a run of {m} rows, cap {cap}, at count {count}"
            rt = tg[i:i + m]
            calls = list(run["calls"])
            limited = sorted({int(t) for t in rt.tolist() if self.quota_of(t) is not None})
            held_tags = self.tags_np(count)
            tagv, vic, new_origin, alt = [], {}, {}, {}
            if limited and count:
                assert calls and calls[0]["kind"] == "scoped", f"no scoped selection for a run with limited tags: {calls}"
                c = calls.pop(0)
                in_t = [int((rt == t).sum()) for t in limited]
                assert (c["count"], c["tags"], c["incoming"]) == (count, limited, in_t), f"scoped request {c}"
                assert c["quotas"] == [self.quota_of(t) for t in limited], f"scoped request {c}"
                assert [o % count for o in c["origins"]] == [self.origin.get(t, 0) % count for t in limited], \
                    f"scoped request: origins {c['origins']}, the model's {[self.origin.get(t, 0) for t in limited]}"
                for s, t in enumerate(limited):
                    mine = held_tags == t
                    held = int(mine.sum())
                    x = min(in_t[s], max(0, held + in_t[s] - self.quota_of(t)))
                    v = np.asarray(c["victims"][s], dtype=np.int64)
                    assert (int(c["held"][s]), int(c["x"][s]), v.size) == (held, x, x), \
                        f"tag {t}: held {c['held'][s]}, x {c['x'][s]}, {v.size} victims; the rule: held {held}, x {x}"
                    if x:
                        self.check_victims(v, count, self.origin.get(t, 0), c["now"], among=mine, what=f"tag {t} victims")
                        new_origin[t] = int(v[-1]) + 1
                        vic[t] = v.tolist()
                        alt[t] = (self.exact_order(count, 0, c["now"], mine, x).tolist(),
                                  self.exact_order(count, self.cursor, c["now"], mine, x).tolist())
                        tagv += v.tolist()
            rem = m - len(tagv)
            n_app = min(rem, M - count)
            g = rem - n_app
            glob = []
            if g:
                assert calls and calls[0]["kind"] in ("masked", "plain"), f"no global selection for {g} victims: {calls}"
                c = calls.pop(0)
                assert (c["n"], c["cursor"], c["count"]) == (g, self.cursor, count), f"victim request {c}"
                free = np.ones(count, dtype=bool)
                free[tagv] = False
                if c["kind"] == "masked":
                    assert c["masked"] == sorted(tagv), "the bitmap does not hold exactly the run's tag victims"
                self.check_victims(c["rows"], count, self.cursor, c["now"], among=free, what="global victims")
                glob = np.asarray(c["rows"], dtype=np.int64).tolist()
                self.cursor = (self.cursor + g) % M
            assert not calls, f"the run asked for selections the rule does not need: {calls}"
            slots = np.asarray(list(range(count, count + n_app)) + tagv + glob, dtype=np.int64)
            self.count += n_app
            self._store(slots, ids[i:i + m], explicit, feats[i:i + m], loc, now, None if tags is None else tg[i:i + m])
            self.origin.update(new_origin)
            out.append(dict(n=m, app=n_app, room=M - count, tag_victims=vic, alt=alt, glob=glob,
                            quota_cut=bool(m == cap < whole), x={t: len(v) for t, v in vic.items()}))
            i += m
        return out

    def _best_held(self, fn, held, ok=None):
        """(largest cosine of every row of ``fn`` to the unit rows ``held``, the LOWEST row that attains it, (the
        largest DIFFERENT cosine, the lowest row that attains that)); ``ok`` bool [n, held]: the pairs that are eligible (None: all)."""
        n = fn.shape[0]
        if held.shape[0] == 0:
            none = torch.full((n, 1), -INF, dtype=torch.float64)
            return none, torch.zeros(n, dtype=torch.int64), (none[:, 0], torch.zeros(n, dtype=torch.int64))
        cs = fn @ held.t()
        if ok is not None:
            cs = torch.where(ok.to(cs.device), cs, torch.full_like(cs, -INF))
        best = cs.max(1).values
        arg = (cs == best[:, None]).to(torch.int8).argmax(1)
        rest = torch.where(cs == best[:, None], torch.full_like(cs, -INF), cs)
        second = rest.max(1).values
        arg2 = (rest == second[:, None]).to(torch.int8).argmax(1)
        return best[:, None].cpu(), arg.cpu(), (second.cpu(), arg2.cpu())

    def _decide(self, fn, held, tau, tag_b=None, tag_h=None, full=False):
        """The rule on fp64 cosines; with ``tag_b`` / ``tag_h`` (int64 [n] / [held]) on the cosines masked by tag
        equality, held rows and in-batch rows alike."""
        ok = None
        cb = (fn @ fn.t()).cpu()
        if tag_b is not None:
            tb, th = torch.as_tensor(np.asarray(tag_b)), torch.as_tensor(np.asarray(tag_h))
            ok = tb[:, None] == th[None, :]
            cb = torch.where(tb[:, None] == tb[None, :], cb, torch.full_like(cb, -INF))
        best, arg, second = self._best_held(fn, held, ok)
        stored, leader, cos = consolidate_rule(best, cb, tau)                      # column 0 stands for the best held row
        stored = torch.where(stored >= 0, arg, stored).numpy()
        if full:
            return stored, leader.numpy(), cos.numpy(), best[:, 0].numpy(), second[0].numpy(), second[1].numpy()
        return stored, leader.numpy()

    def write_merge(self, ids, feats, loc, now, tau, select=None, tags=None, within=False, writer=None):
        """A consolidating write, in chunks of 1024: the rule on fp64 cosines; the distinct stored targets are
        reinforced and take the write's timestamp BEFORE the kept rows are written.  ``within``: on the cosines masked
        by tag equality (rows without a tag are tag 0); the kept rows are written with their tags before the next
        chunk decides.  ``writer(kept ids, feats, tags)``: writes the kept rows of a chunk (default: ``write``) and
        returns what it reports.  Returns ``(kept ids, writer reports or rows that overwrote, per chunk info)``."""
        kept_ids, over, info = [], 0, []
        tg = None if not within else (np.zeros(len(ids), dtype=np.int64) if tags is None else np.asarray(tags, dtype=np.int64))
        for lo in range(0, len(ids), 1024):
            f = feats[lo:lo + 1024]
            fn, hn = _unit64(f), _unit64(self.feats[:self.count])
            if within:
                t = tg[lo:lo + 1024]
                stored, leader = self._decide(fn, hn, tau, t, self.tags_np())
                b_stored, b_leader = self._decide(fn, hn, tau)
                merged = (stored >= 0) | (leader >= 0)
                lim = {}
                for u in sorted({int(x) for x in t.tolist() if self.quota_of(x) is not None}):
                    lim[u] = dict(held=int((self.tags_np() == u).sum()), q=self.quota_of(u), all=int((t == u).sum()),
                                  kept=int(((t == u) & ~merged).sum()))
                info.append(dict(stored=stored, leader=leader, limited=lim,
                                 kept_blind_merges=int((~merged & ((b_stored >= 0) | (b_leader >= 0))).sum())))
            else:
                stored, leader = self._decide(fn, hn, tau)
            targets = np.unique(stored[stored >= 0])
            if targets.size:
                self.reinforce(targets, self.merge_reinforce, self.merge_cap)
                self.touch(targets, now)
            kept = np.nonzero((stored < 0) & (leader < 0))[0]
            if kept.size:
                kid = [ids[lo + i] for i in kept.tolist()]
                kf = f[torch.from_numpy(kept).to(f.device)]
                kt = None if tags is None else np.asarray(tags)[lo:lo + 1024][kept]
                if writer is not None:
                    rep = writer(kid, kf, kt)
                    if info:
                        info[-1]["runs"] = rep
                else:
                    over += self.write(kid, kf, loc, now, tags=kt, select=select)
                kept_ids += kid
        return (kept_ids, over, info) if within else (kept_ids, over)

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

    def _reorder(self, order, start=0):
        """New row i holds what row ``order[i]`` held (``order``: in ring order from the ring's start ``start``).  A tie
        origin becomes the number of survivors that come before it in ring order from the ring's start."""
        c0 = self.count
        if self.origin and c0:
            alive = np.zeros(c0, dtype=bool)
            alive[np.asarray(order, dtype=np.int64)] = True
            walk = (start + np.arange(c0)) % c0             # the rows as the ring passes them, from its start
            for t, c in self.origin.items():
                # the origin's place on the ring is the row r with (r - c) mod count == 0, as the eviction order reads
                # it (an origin equal to the count is row 0's place); count the survivors the walk meets before it
                at = int(np.argmax((walk - c) % c0 == 0))
                self.origin[t] = int(alive[walk[:at]].sum())
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
        self._reorder(np.concatenate([start + np.nonzero(keep[start:])[0], np.nonzero(keep[:start])[0]]), start)
        return int(kill.size)

    def rows_with_tags(self, tags):
        return np.nonzero(np.isin(self.tag[:self.count].cpu().numpy(), np.asarray(tags)))[0]

    def enforce_plan(self):
        """``[(tag, held, quota)]`` of the limited tags that hold more than their quota, ascending by tag."""
        return [(t, h, self.quota_of(t)) for t, h in self.limited_counts().items() if h > self.quota_of(t)]

    def enforce(self, victims, now):
        """``enforce_tag_quotas``: per tag over its quota the first ``held - q`` rows of its eviction order go (the
        device's ``victims`` {tag: rows}, checked in the band and followed), its origin moves behind the last of them,
        then ONE forget, which remaps the origins."""
        kill = []
        for t, h, q in self.enforce_plan():
            v = np.asarray(victims[t], dtype=np.int64)
            assert v.size == h - q, f"tag {t}: {v.size} victims, {h} held and a quota of {q}"
            self.check_victims(v, self.count, self.origin.get(t, 0), now, among=self.tags_np() == t, what=f"tag {t} excess")
            self.origin[t] = int(v[-1]) + 1
            kill += v.tolist()
        return self.forget(np.asarray(kill, dtype=np.int64))

    def _consolidate_plan(self, tau, within):
        """(kept rows, strengths, timestamps) of a bank already in age order -- nothing is changed."""
        count = self.count
        u = _unit64(self.feats[:count])
        tg = self.tags_np()
        S, T = self.strength.cpu().clone(), self.ts.cpu().clone()
        kept_rows = []
        for lo in range(0, count, 1024):
            hi = min(count, lo + 1024)
            prefix = torch.as_tensor(kept_rows, dtype=torch.int64, device=self.dev)
            if within:
                stored, leader = self._decide(u[lo:hi], u[prefix], tau, tg[lo:hi], tg[np.asarray(kept_rows, dtype=np.int64)])
            else:
                stored, leader = self._decide(u[lo:hi], u[prefix], tau)
            for i in np.nonzero((stored >= 0) | (leader >= 0))[0].tolist():
                t = kept_rows[stored[i]] if stored[i] >= 0 else lo + int(leader[i])
                S[t], T[t] = max(S[t], S[lo + i]), max(T[t], T[lo + i])
            targets = np.unique(stored[stored >= 0])
            if targets.size:
                t = torch.as_tensor([kept_rows[j] for j in targets.tolist()])
                S = reinforce_reference(S[:, None].clone(), count, t, self.merge_reinforce, self.merge_cap)[:, 0]
            kept_rows += (lo + np.nonzero((stored < 0) & (leader < 0))[0]).tolist()
        return kept_rows, S, T

    def consolidate(self, tau, within=False, compare=False):
        """What writing the rows, oldest first, into an empty bank through consolidating writes in chunks of 1024
        leaves: a kept row takes the largest strength and the latest timestamp of the rows merged into it, then the
        distinct stored targets of a chunk are reinforced once.  ``within``: each row with its own tag, on the masked
        cosines; a kept row keeps its tag.  ``compare``: also returns whether the other rule keeps other rows."""
        start = self._ring_start()
        if start:
            self._reorder(np.concatenate([np.arange(start, self.count), np.arange(start)]), start)
        count = self.count
        if count == 0:
            return (0, False) if compare else 0
        kept_rows, S, T = self._consolidate_plan(tau, within)
        differs = compare and self._consolidate_plan(tau, not within)[0] != kept_rows
        self.strength.copy_(S)
        self.ts.copy_(T)
        self._reorder(kept_rows)
        return (count - len(kept_rows), differs) if compare else count - len(kept_rows)

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


class _RunSpy:
    """Records how a write is cut into runs (``hf._write_rows``, as tests/test_gpu_quota.py wraps it) and what every
    run asks the device to select: ``ops.bank_select_weakest_scoped`` (decoded with ``scoped_selection_decode``),
    ``ops.bank_select_weakest_masked`` and ``ops.bank_select_weakest``.  ``runs``: one ``dict(n, calls)`` per run;
    ``loose``: selections asked for outside a run (``enforce_tag_quotas``)."""
    NAMES = ("bank_select_weakest", "bank_select_weakest_masked", "bank_select_weakest_scoped")

    def __init__(self, ops, hf):
        self.ops, self.hf, self.runs, self.loose, self.cur = ops, hf, [], [], None

    def _note(self, **call):
        (self.loose if self.cur is None else self.cur["calls"]).append(call)

    def __enter__(self):
        self.orig = {n: getattr(self.ops, n) for n in self.NAMES if hasattr(self.ops, n)}
        rows_of = lambda t: t.detach().cpu().numpy().astype(np.int64).copy()

        def plain(meta, count, now, cursor, n):
            rows, keys = self.orig["bank_select_weakest"](meta, count, now, cursor, n)
            self._note(kind="plain", count=int(count), now=now, cursor=int(cursor), n=int(n), rows=rows_of(rows))
            return rows, keys

        def masked(meta, count, now, cursor, n, bitmap):
            rows, keys = self.orig["bank_select_weakest_masked"](meta, count, now, cursor, n, bitmap)
            b = bitmap.detach().cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            bits = ((b[:, None] >> np.arange(32)[None, :]) & 1).reshape(-1)[:count]
            self._note(kind="masked", count=int(count), now=now, cursor=int(cursor), n=int(n), rows=rows_of(rows),
                       masked=np.nonzero(bits)[0].tolist())
            return rows, keys

        def scoped(meta, count, now, scope_tags, origins, incoming, quotas, bitmap=None):
            packed, bm = self.orig["bank_select_weakest_scoped"](meta, count, now, scope_tags, origins, incoming, quotas,
                                                                 **({} if bitmap is None else dict(bitmap=bitmap)))
            held, x, victims = self.ops.scoped_selection_decode(packed.cpu(), incoming)
            ints = lambda v: [int(i) for i in np.asarray(v).reshape(-1)]
            self._note(kind="scoped", count=int(count), now=now, tags=ints(scope_tags), origins=ints(origins),
                       incoming=ints(incoming), quotas=ints(quotas), held=ints(held), x=ints(x),
                       victims=[ints(v) for v in victims])
            return packed, bm
        for n, f in (("bank_select_weakest", plain), ("bank_select_weakest_masked", masked),
                     ("bank_select_weakest_scoped", scoped)):
            if n in self.orig:
                setattr(self.ops, n, f)
        real = self.hf._write_rows

        def write_rows(ids, *a, **kw):
            self.cur = dict(n=len(ids), calls=[])
            self.runs.append(self.cur)
            try:
                return real(ids, *a, **kw)
            finally:
                self.cur = None
        self.hf._write_rows = write_rows
        return self

    def __exit__(self, *exc):
        del self.hf._write_rows
        for n, f in self.orig.items():
            setattr(self.ops, n, f)


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
        self.tc = sizes.get("tagcase")                      # the tag-aware cases: see ``tagcase``
        if self.tc is not None:
            self.stats.update(repeat_rows=0, repeat_near_ties=0)
            self.check_rng = np.random.default_rng([seed, 1])   # the checks' own draws: no check disturbs a sequence
            for t, q in self.tc["quota_map"].items():
                self.model.set_quota(t, q)
            self.model.index_interval = int(self.hf.centroids_update_interval) if sizes["index"] else None

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

    def op_forget(self, kind, n=None, tags=None, rows=None):
        m = self.model
        if rows is not None:
            return self._forget(kind, np.asarray(rows, dtype=np.int64), rows=torch.from_numpy(np.asarray(rows, dtype=np.int64)))
        if kind == "ids":
            live = [m.ids[r] for r in range(m.count) if m.explicit[r]]
            if live:
                ids = [live[i] for i in self.rng.integers(0, len(live), size=min(6, len(live)))]
                return self._forget(kind, m.rows_of_ids(ids), ids=ids)
            kind = "rows"
        if kind == "tags":
            tags = [int(self.rng.integers(1, 5))] if tags is None else tags
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
        if not self.model.has_quota():
            self.model.origin = {}                          # the tie origins travel with the quotas: none set, none kept
        return {}

    # -- the tag-aware operations (cases with ``sizes["tagcase"]``): per-tag quotas and merging within tags
    def _draw_tags(self, n):
        return self.rng.choice(np.asarray(self.tc["tags"]), size=n, p=np.asarray(self.tc["probs"], dtype=np.float64)).astype(np.int64)

    def _note_spy(self, spy):
        """What the bank did, into the log entry BEFORE the model judges it: a failing step keeps its run lengths and
        the victims of every selection."""
        brief = lambda c: {k: (np.asarray(v).tolist() if k == "rows" else v) for k, v in c.items()
                           if k in ("kind", "count", "cursor", "n", "tags", "origins", "incoming", "held", "x", "victims", "rows")}
        self.entry["runs"] = [r["n"] for r in spy.runs]
        self.entry["device_selections"] = [[brief(c) for c in r["calls"]] for r in spy.runs] + \
                                          ([[brief(c) for c in spy.loose]] if spy.loose else [])

    def _model_write(self, ids, f, loc, now, tags, spy):
        """The model's side of a plain write: the recorded runs under ``'weakest'``, the ring otherwise."""
        if self.model.policy == "weakest":
            return self.model.write_runs(ids, f, loc, now, tags, spy.runs)
        over = self.model.write(ids, f, loc, now, tags=tags)
        del spy.runs[:]
        return [dict(n=len(ids), over=over, tag_victims={}, alt={}, glob=[], app=len(ids) - over, room=0, quota_cut=False, x={})]

    @staticmethod
    def _run_log(runs, o0, o1):
        """What every log entry of a write says: the run lengths, the tag victims per scope, the global victims, the
        origins before and after."""
        return dict(runs=[r["n"] for r in runs], tag_victims=[r["tag_victims"] for r in runs], glob=[r["glob"] for r in runs],
                    origins_before=o0, origins_after=o1,
                    over=sum(r.get("over", len(r["glob"]) + sum(len(v) for v in r["tag_victims"].values())) for r in runs),
                    room_tag_victims=any(r["tag_victims"] and r["room"] > 0 for r in runs),
                    full_both=any(r["tag_victims"] and r["glob"] and r["room"] == 0 for r in runs),
                    quota_cut=any(r["quota_cut"] for r in runs),
                    origin_mattered=any(set(v) != set(r["alt"][t][0]) and set(v) != set(r["alt"][t][1])
                                        for r in runs for t, v in r["tag_victims"].items()))

    def op_twrite(self, n, tags="draw", feats=None):
        m = self.model
        tags = self._draw_tags(n) if isinstance(tags, str) else (None if tags is None else np.asarray(tags, dtype=np.int64))
        ids, f, loc, now = self._ids(n), (self.pool.take(n) if feats is None else feats), self._move(), self.clock.now
        o0, counts0 = dict(m.origin), m.limited_counts()
        with _RunSpy(self.ops, self.hf) as spy:
            self.hf.create_episodic_memories(ids, f, tags=tags)
            self._note_spy(spy)
            runs = self._model_write(ids, f, loc, now, tags, spy)
            assert not spy.runs and not spy.loose, "the write made more runs or selections than the rule needs"
        counts1 = m.limited_counts()
        stuck = [t for t in (set() if tags is None else set(tags.tolist())) if m.quota_of(t) is not None and
                 counts0.get(t, 0) > m.quota_of(t) and counts1.get(t) == counts0.get(t)]
        return dict(n=n, tagged=tags is not None, over_quota_unchanged=stuck, **self._run_log(runs, o0, dict(m.origin)))

    def _verbatim(self, f, tags):
        """Two rows for a consolidating write: a held row once more under the tag it carries (it must merge into that
        row, or the lowest bit-identical one of the tag) and once under another tag of the case that holds no row
        within ``TAU`` of it but bit-identical copies (it must be kept, or merge into the lowest such copy)."""
        m = self.model
        want = self.tc.get("focus")
        rows = np.nonzero(m.tags_np() == want)[0] if want is not None else np.zeros(0, dtype=np.int64)
        if rows.size == 0:
            rows = self.rng.permutation(m.count)
        u = _unit64(m.feats[:m.count])
        held = m.tags_np()
        for r in rows[:16].tolist():                        # (the first row whose copy has another tag to go to)
            t = int(m.tag[r])
            cos = (u @ u[r]).cpu().numpy()
            same = (m.feats[:m.count] == m.feats[r]).all(1).cpu().numpy()
            near = (_unit64(f) @ u[r]).cpu().numpy() >= TAU - GAP     # (rows of this batch count as held rows will)
            others = [int(x) for x in self.tc["tags"] if int(x) != t and not ((held == x) & (cos >= TAU - GAP) & ~same).any()
                      and not (near & (tags == x)).any()]
            if others:
                break
        t2 = others[int(self.rng.integers(0, len(others)))] if others else None
        return r, t, t2, same, held.copy()

    def op_write_merge_tagged(self, n, verbatim=False, tags="draw"):
        m = self.model
        tags = self._draw_tags(n) if isinstance(tags, str) else np.asarray(tags, dtype=np.int64)
        f = self.pool.take(n)
        vb = None
        if verbatim and m.count and n + 2 <= 1024:
            r, t, t2, same, tags0 = self._verbatim(f, tags)
            extra = [t] + ([t2] if t2 is not None else [])
            f = torch.cat([f] + [m.feats[r:r + 1].clone()] * len(extra))
            tags = np.concatenate([tags, extra])
            vb = (r, t, t2, same, tags0, n)
        N = len(tags)
        ids, loc, now = self._ids(N), self._move(), self.clock.now
        o0, ids0 = dict(m.origin), list(m.ids)
        with _RunSpy(self.ops, self.hf) as spy:
            rep = self.hf.create_episodic_memories(ids, f, merge_similarity=TAU, tags=tags, merge_within_tags=True)
            self._note_spy(spy)
            kept, _, info = m.write_merge(ids, f, loc, now, TAU, tags=tags, within=True,
                                          writer=lambda kid, kf, kt: self._model_write(kid, kf, loc, now, kt, spy))
            assert not spy.runs and not spy.loose, "the write made more runs or selections than the rule needs"
        assert rep.n_stored == len(kept) and [i for i, x in zip(ids, rep.merged.tolist()) if not x] == kept, \
            f"the write kept {rep.n_stored} rows, the fp64 rule within tags keeps {len(kept)}"
        runs = [r for c in info for r in c.get("runs", [])]
        out = dict(n=N, kept=len(kept), kept_blind_merges=sum(c["kept_blind_merges"] for c in info),
                   **self._run_log(runs, o0, dict(m.origin)))
        # rows a consolidating write merges are not stored and do not count towards in_t
        out["merged_not_counted"] = False
        for c in info:
            for t, d in c["limited"].items():
                x = sum(r["x"].get(t, 0) for r in c.get("runs", []))
                if d["all"] <= d["q"] and d["held"] >= d["q"] and x < min(d["all"], max(0, d["held"] + d["all"] - d["q"])):
                    out["merged_not_counted"] = True
        if vb is not None:
            r, t, t2, same, tags0, at = vb
            stored, leader = info[0]["stored"], info[0]["leader"]
            first = lambda tag: int(np.nonzero(same & (tags0 == tag))[0][0]) if (same & (tags0 == tag)).any() else -1
            assert stored[at] == first(t) >= 0, f"a held row written again under its tag {t} did not merge into it: {stored[at]}"

            def bank_row(i, target):
                """Where the bank's report must place batch row i: the row it merged into (``target`` >= 0) or the
                row it was stored at, -1 once this same call has overwritten that memory again."""
                if target >= 0:
                    return target if m.ids[target] == ids0[target] else -1
                return next((x for x in range(m.count) if m.ids[x] == ids[i]), -1)
            assert bool(rep.merged[at]) and int(rep.rows[at]) == bank_row(at, first(t)), \
                f"the copy under its own tag {t}: merged {bool(rep.merged[at])} into row {int(rep.rows[at])}, expected row {first(t)}"
            out["verbatim_same"] = True
            if t2 is not None:
                assert (stored[at + 1] == first(t2)) and leader[at + 1] < 0, \
                    f"row {r} (tag {t}) written again under tag {t2}: target {stored[at + 1]}, expected {first(t2)}"
                assert bool(rep.merged[at + 1]) == (first(t2) >= 0) and int(rep.rows[at + 1]) == bank_row(at + 1, first(t2)), \
                    f"the copy under tag {t2}: merged {bool(rep.merged[at + 1])}, row {int(rep.rows[at + 1])}, expected " \
                    f"{'row ' + str(first(t2)) if first(t2) >= 0 else 'a stored row'}"
                out["verbatim_other"] = True
        return out

    def op_tbulk(self, n, rebuild, tags="draw"):
        f, loc, now = self.pool.take(n), self._move(), self.clock.now
        prefix, first = f"s{self.seed}-b{self.next_bulk}-", int(self.rng.integers(0, 1000))
        self.next_bulk += 1
        tags = self._draw_tags(n) if isinstance(tags, str) else np.full(n, int(tags), dtype=np.int64)
        m = self.model
        o0 = dict(m.origin)
        assert self.hf.bulk_write(f, id_prefix=prefix, first_index=first, rebuild=rebuild, tags=tags) == n
        m._store(np.arange(m.count, m.count + n), [f"{prefix}{first + i}" for i in range(n)], False, f, loc, now, tags)
        m.count += n
        return dict(n=n, rebuild=rebuild, tagged=True, origins_before=o0, origins_after=dict(m.origin))

    def op_tretag(self):
        m, tag = self.model, int(self._draw_tags(1)[0])
        rows = self._rows(int(self.rng.integers(1, 40)), wild=True)
        assert self.hf.retag(rows=rows, tag=tag) == m._held(rows).size
        m.retag(rows, tag)
        return dict(rows=rows.size, tag=tag)

    def op_set_quota(self, changes=None):
        """Lower, raise or remove a quota, the default too (``changes``: {tag or None: quota or None})."""
        m = self.model
        if changes is None:
            named = [t for t in self.tc["quota_map"] if t is not None] or [int(t) for t in self.tc["tags"][:4]]
            tag = None if self.rng.integers(0, 4) == 0 else int(named[int(self.rng.integers(0, len(named)))])
            q0 = m.quota_default if tag is None else m.quota.get(tag)
            q = [None, 1, 2, None if q0 is None else max(1, q0 // 2), 5 if q0 is None else 2 * q0 + 1][int(self.rng.integers(0, 5))]
            changes = {tag: q}
        for tag, q in changes.items():
            self.hf.set_tag_quota(tag, q)
            m.set_quota(tag, q)
        return dict(changes=changes)

    def op_enforce(self):
        m, now = self.model, self.clock.now
        plan, o0 = m.enforce_plan(), dict(m.origin)
        with _RunSpy(self.ops, self.hf) as spy:
            rep = self.hf.enforce_tag_quotas(now=now)
        self._note_spy(spy)
        assert not spy.runs, "enforce_tag_quotas wrote rows"
        if not plan:
            assert rep.n_removed == 0 and not spy.loose
            return dict(removed=0, origins_before=o0, origins_after=dict(m.origin))
        assert len(spy.loose) == 1 and spy.loose[0]["kind"] == "scoped", f"enforce_tag_quotas selected {spy.loose}"
        c = spy.loose[0]
        assert (c["tags"], c["held"], c["x"]) == ([t for t, _, _ in plan], [h for _, h, _ in plan], [h - q for _, h, q in plan]), \
            f"enforce_tag_quotas: {c}, the model: {plan}"
        victims = dict(zip(c["tags"], c["victims"]))
        n = m.enforce(victims, c["now"])
        assert rep.n_removed == n, f"enforce_tag_quotas removed {rep.n_removed} rows, the model {n}"
        return dict(removed=n, tag_victims=victims, origins_before=o0, origins_after=dict(m.origin))

    def op_tconsolidate(self, rebuild, within):
        m = self.model
        o0 = dict(m.origin)
        rep = self.hf.consolidate(TAU, rebuild=rebuild, within_tags=within)
        n, differs = m.consolidate(TAU, within, compare=True)
        assert rep.n_merged == n, f"consolidate(within_tags={within}) merged {rep.n_merged} rows, the fp64 rule {n}"
        return dict(rebuild=rebuild, within=within, merged=n, differs_from_other_rule=bool(differs),
                    origins_before=o0, origins_after=dict(m.origin))

    def op_prune_weak(self, rows):
        """Weaken the held rows ``rows`` to a quarter of the weakest strength held (the documented in-place edit), then
        ``prune(min_strength=)`` half that strength: exactly these rows go, whatever else the bank holds."""
        m = self.model
        o0 = dict(m.origin)
        rows = m._held(rows)
        low = float(m.strength[:m.count].min())
        r = torch.from_numpy(rows).to(self.dev)
        self.hf.memory_metadata[r, 0] = low / 4
        m.strength[r] = low / 4
        thr = float(np.float32(low / 2))
        kill = np.nonzero((m.strength[:m.count] < thr).cpu().numpy())[0]
        rep = self.hf.prune(min_strength=thr)
        n = m.forget(kill)
        assert rep.n_removed == n == rows.size, f"prune removed {rep.n_removed} rows, the model {n}"
        return dict(by_key=False, removed=n, origins_before=o0, origins_after=dict(m.origin))

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
        if self.tc is not None:
            assert hf.tag_counts() == m.limited_counts(), f"tag_counts() {hf.tag_counts()}, the model's {m.limited_counts()}"
            assert dict(hf.tag_quotas) == m.quotas_view(), f"tag_quotas {dict(hf.tag_quotas)}, the model's {m.quotas_view()}"
            got = dict(hf._tag_origin)
            for t in set(got) | set(m.origin):              # (a tag the model holds at 0 may be absent on the bank)
                assert got.get(t, 0) == m.origin.get(t, 0), f"tie origins {got}, the model's {m.origin}"
            state = hf.bank_state()
            assert ("tag_quota" in state) == ("tag_origin" in state) == m.has_quota(), \
                f"bank_state() keys {sorted(state)} with quotas {m.quotas_view()}"
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
        if self.tc is not None and self.step % self.z.get("extra_every", 1) == 0:
            self._repeat_checks(fresh, now)
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

    def _repeat_checks(self, fresh, now):
        """Read-only: the repeat search over the next 48 rows of the pool (peeked, not consumed), scope-blind and with
        drawn tags, against the fp64 rule and against the rebuilt bank; one diverse recall against the rebuilt bank."""
        hf, m, st = self.hf, self.model, self.stats
        k = min(48, self.pool.left())
        if k:
            f = self.pool.feats[self.pool.used:self.pool.used + k].clone()
            fn, hn = _unit64(f), _unit64(m.feats[:m.count])
            drawn = self.check_rng.choice(np.asarray(self.tc["tags"]), size=k).astype(np.int64)
            for tags in (None, drawn):
                kw = {} if tags is None else dict(tags=tags)
                what = "find_repeats" + ("" if tags is None else "(tags=)")
                got = hf.find_repeats(f, TAU, **kw)
                again = fresh.find_repeats(f, TAU, **kw)
                for a, b in zip(got, again):
                    assert torch.equal(_bits(a), _bits(b)), f"{what} differs from the bank rebuilt from the checkpoint"
                gs, gl, gc = (x.numpy() for x in got)
                stored, leader, cos, best, second, arg2 = m._decide(fn, hn, TAU, tags, None if tags is None else m.tags_np(),
                                                                    full=True)
                assert np.array_equal(gl, leader), f"{what}: leaders {gl.tolist()}, the fp64 rule {leader.tolist()}"
                assert np.array_equal(gs >= 0, stored >= 0), f"{what}: merged / kept differs from the fp64 rule"
                with np.errstate(invalid="ignore"):
                    near = (stored >= 0) & (best - second <= 1e-6)
                ok = (gs == stored) | (near & (gs == arg2))
                assert ok.all(), f"{what}: stored targets {gs[~ok].tolist()}, the fp64 rule {stored[~ok].tolist()}"
                rep = (stored >= 0) | (leader >= 0)
                assert (np.abs(gc[rep].astype(np.float64) - cos[rep]) <= 1e-5).all() and np.isneginf(gc[~rep]).all(), \
                    f"{what}: cos differs from the fp64 value"
                st["repeat_rows"] += k
                st["repeat_near_ties"] += int(near.sum())
        kw = dict(k=self.k, now=now, diversity=0.3, max_similarity=0.9, fetch_k=32)
        s1, r1 = hf.recall_batch(self.q, **kw)
        s2, r2 = fresh.recall_batch(self.q, **kw)
        assert torch.equal(r1, r2) and torch.equal(_bits(s1), _bits(s2)), "diverse recall differs from the rebuilt bank's"

    # -- the sequence
    def random_op_tagged(self):
        """The draw of the tag-aware cases (the old cases keep ``random_op`` and its weights)."""
        m, z, rng, tc = self.model, self.z, self.rng, self.tc
        room = m.M - m.count
        batches = [b for b in z["batches"] if b <= self.pool.left() - 48]
        quota = z["policy"] == "weakest" and tc["quota"] is not None
        w = {}
        if batches:
            w.update(twrite=5, write_merge_tagged=3)
            if room > 0:
                w["tbulk"] = 2
        if m.count:
            w.update(decay=1, reinforce=1, recall_reinforce=1, touch=1, tretag=2, edit=1, forget=3, prune=2,
                     tconsolidate=2, checkpoint=1)
            if z["index"]:
                w["rebuild"] = 1
        if quota:
            w.update(set_quota=2, enforce=2)
        names = list(w)
        p = np.asarray([w[x] for x in names], dtype=np.float64)
        op = names[int(rng.choice(len(names), p=p / p.sum()))]
        bw = np.asarray(z.get("batch_weights", [1] * len(z["batches"]))[:len(batches)], dtype=np.float64)
        batch = lambda: int(rng.choice(batches, p=bw / bw.sum()))
        if op == "twrite":
            return "write", lambda: self.op_twrite(batch(), tags=None if rng.integers(0, 5) == 0 else "draw")
        if op == "write_merge_tagged":
            return op, lambda: self.op_write_merge_tagged(batch(), verbatim=bool(rng.integers(0, 4) == 0 and m.count >= m.M // 2))
        if op == "tbulk":
            return "bulk", lambda: self.op_tbulk(min(batch(), room), bool(rng.integers(0, 2)))
        if op == "tretag":
            return "retag", self.op_tretag
        if op == "tconsolidate":
            return "consolidate", lambda: self.op_tconsolidate(bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
        if op == "recall_reinforce":
            return op, lambda: self.op_recall_reinforce(bool(rng.integers(0, 2)))
        if op == "forget":
            kind = str(rng.choice(["rows", "ids", "tags"]))
            return op, lambda: self.op_forget(kind, tags=[int(self._draw_tags(1)[0])] if kind == "tags" else None)
        if op == "prune":
            def prune(by_key=bool(rng.integers(0, 2))):
                # (a bank of tied keys -- one bulk_write -- would lose every row to a quantile of its keys)
                keys = m.keys64(self.clock.now).cpu().numpy()
                tied = by_key and (keys <= np.quantile(keys, 0.15) * (1 + 3e-5)).mean() > 0.34
                return self.op_prune(by_key and not tied)
            return op, prune
        return op, getattr(self, "op_" + op)

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
        self.entry = entry
        if self.tc is not None:
            entry["origins_before"] = dict(m.origin)
        try:
            entry.update(fn() or {})
            if self.tc is not None:
                entry["origins_after"] = dict(m.origin)
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
    ``policy``, ``index``, ``batches`` (+ ``batch_weights``), ``pool_rows`` / ``pool_groups`` / ``pool_seed``;
    ``tagcase`` (see ``tagcase``) makes it a tag-aware case, and ``extra_every`` = 2 runs that case's repeat searches and
    diverse recall after every other step instead of after every step (they draw from a generator of their own, so the
    sequence is the same either way).
    ``plan(seq)``: called before every step; it may return ``(op name, callable)`` or ``(op name, callable, still)``
    to force that step's operation (``still``: the clock does not move before it).
    Returns the ``Sequence`` (``log``, ``stats``, ``hf``, ``model``)."""
    seq = Sequence(hf_factory, ops, seed, sizes, clock)
    for _ in range(steps):
        forced = plan(seq) if plan is not None else None
        seq.run_step(*(forced if forced is not None else (seq.random_op() if seq.tc is None else seq.random_op_tagged())))
    return seq


# ------------------------------------------------------------------------------- the tag-aware cases: plan and events
def tagcase(quota, tags, probs, small, mid, over, free, many=False, mid_quota=None):
    """``sizes["tagcase"]``: ``quota`` as the bank's ``tag_quota=`` (a mapping, an int for every tag but 0, None: merging
    within tags only), the tags the case draws with their probabilities, and the tags the planned part uses: ``small``
    (a small quota, overflowed inside one batch), ``mid`` (the tag whose tied rows show the origin), ``over`` (driven
    over its quota), ``free`` (unlimited: fills the bank).  ``mid_quota``: the quota the plan names for ``mid`` where the case's own (an int
    quota of 2) leaves too few tied rows for an origin to show.  ``many``: one planned batch with more than 64 limited tags."""
    qm = {} if quota is None else ({None: int(quota)} if isinstance(quota, int) else dict(quota))
    return dict(quota=quota, quota_map=qm, tags=list(tags), probs=list(probs), small=small, mid=mid, over=over,
                free=free, many=many, focus=None, mid_quota=mid_quota)


class TagPlan:
    """The planned part of a tag-aware sequence, in the manner of the GPU tests' ``_Plan``: goals in order, each
    reached by one operation once its precondition holds (otherwise the step works towards it), a drawn operation in
    between unless the goal is ``sticky`` (it follows its predecessor directly: the ``still_`` writes need the tied
    keys the steps before them left)."""

    def __init__(self, steps, tc, index, M, fill=None):
        self.steps, self.tc, self.index, self.M, self.fill0 = steps, tc, index, M, fill
        quota = tc["quota"] is not None
        g = ["fill0"] if fill else []
        if quota:
            g += (["many"] if tc["many"] else []) + ["cut", "over_bulk", "over_write", "enforce"]
        g += (["refill"] if fill else []) + ["verbatim", "cons_within", "cons_blind"] + (["refill"] if fill else [])
        if quota:
            g += ["restore", "tie_a", "tie_b", "c_forget", "tie_d", "c_prune", "tie_copies", "c_consolidate", "tie_d",
                  "c_checkpoint", "tie_d", "fill", "full_both"]
        self.goals = g
        self.sticky = {"over_write", "enforce", "cons_within", "cons_blind", "tie_a", "tie_b", "c_forget", "tie_d", "tie_copies", "c_prune",
                       "c_consolidate", "c_checkpoint", "full_both"}
        self.drawn_last = True

    def __call__(self, seq):
        left = self.steps - (seq.step + 1)
        if not self.goals:
            return None
        if not (self.drawn_last or self.goals[0] in self.sticky or left <= 2 * len(self.goals) + 4):
            self.drawn_last = True
            return None
        forced = getattr(self, "_" + self.goals[0])(seq)
        self.drawn_last = forced is None
        return forced

    def _done(self, op, fn, still=False):
        self.goals.pop(0)
        return op, fn, still

    # -- preconditions
    def _room(self, seq, need):
        m = seq.model
        if m.M - m.count >= need:
            return None
        return "forget", lambda: seq.op_forget("rows", n=need - (m.M - m.count) + 8)

    def _quotas(self, seq, tags):
        """The case's own quotas for ``tags`` (a drawn ``set_quota`` may have changed them)."""
        m, qm = seq.model, self.tc["quota_map"]
        want = {t: (qm[t] if t in qm else None) for t in list(tags) + ([None] if None in qm else [])}
        if self.tc["mid_quota"] and self.tc["mid"] in want:
            want[self.tc["mid"]] = self.tc["mid_quota"]
        have = {t: (m.quota_default if t is None else m.quota.get(t)) for t in want}
        if want == have:
            return None
        return "set_quota", lambda: seq.op_set_quota({t: q for t, q in want.items() if have[t] != q})

    def _held(self, seq, tag):
        return int((seq.model.tags_np() == tag).sum())

    # -- goals
    def _fill0(self, seq):
        return self._done("bulk", lambda: seq.op_tbulk(self.fill0, self.index))

    def _refill(self, seq):
        n = seq.model.count
        if n >= self.fill0 or seq.pool.left() < self.fill0 - n + 4000:      # (or the pool could not feed the rest)
            self.goals.pop(0)
            return None
        return self._done("bulk", lambda: seq.op_tbulk(self.fill0 - n, False, tags=self.tc["free"]))

    def _many(self, seq):
        tags = [t for t in self.tc["tags"] if seq.model.quota_of(t) is not None]
        return self._done("write", lambda: seq.op_twrite(2 * len(tags), tags=tags + tags))

    def _cut(self, seq):
        t = self.tc["small"]
        pre = self._quotas(seq, [t])
        if pre:
            return pre
        q = seq.model.quota_of(t)
        return self._room(seq, 2 * q + 1) or self._done("write", lambda: seq.op_twrite(2 * q + 1, tags=[t] * (2 * q + 1)))

    def _over_bulk(self, seq):
        t = self.tc["over"]
        pre = self._quotas(seq, [t])
        if pre:
            return pre
        q = seq.model.quota_of(t)
        if self._held(seq, t) > q:
            self.goals.pop(0)
            return self._over_write(seq)
        return self._room(seq, q + 5) or self._done("bulk", lambda: seq.op_tbulk(q + 5, False, tags=t))

    def _over_write(self, seq):
        t = self.tc["over"]
        return self._done("write", lambda: seq.op_twrite(4, tags=[t] * 4))

    def _enforce(self, seq):
        return self._done("enforce", seq.op_enforce)

    def _verbatim(self, seq):
        m, tc, t = seq.model, self.tc, self.tc["small"]
        if tc["quota"] is None:
            if m.count == 0:
                return "write", lambda: seq.op_twrite(16)
            return self._done("write_merge_tagged", lambda: seq.op_write_merge_tagged(6, verbatim=True))
        pre = self._quotas(seq, [t])
        if pre:
            return pre
        q = m.quota_of(t)
        if self._held(seq, t) < q:                         # bring the tag to its quota first
            return "write", lambda: seq.op_twrite(q, tags=[t] * q)
        if self._held(seq, t) > q:
            return "enforce", seq.op_enforce

        def fn():
            tc["focus"] = t
            try:
                return seq.op_write_merge_tagged(min(2, q - 1), verbatim=True, tags=[t] * min(2, q - 1))
            finally:
                tc["focus"] = None
        return self._done("write_merge_tagged", fn)

    def _cons_within(self, seq):
        m = seq.model
        if m.count == 0 or m._consolidate_plan(TAU, True)[0] == m._consolidate_plan(TAU, False)[0]:
            # nothing held that the two rules treat differently (the copy's original was evicted): write one again
            return "write_merge_tagged", lambda: seq.op_write_merge_tagged(4, verbatim=True)
        return self._done("consolidate", lambda: seq.op_tconsolidate(False, True))

    def _cons_blind(self, seq):
        # (the copies go again: two bit-identical rows of equal strength and age tie in every score, and in a small
        # bank such a pair would sit in most queries' top k + 1 and use up the allowance for the model's near-ties)
        return self._done("consolidate", lambda: seq.op_tconsolidate(False, False))

    def _restore(self, seq):
        self.goals.pop(0)
        return self._quotas(seq, [t for t in self.tc["quota_map"] if t is not None] + [self.tc["mid"]])

    def _tie_a(self, seq):
        t = self.tc["mid"]
        pre = self._quotas(seq, [t])
        if pre:
            return pre
        q = seq.model.quota_of(t)
        if self._held(seq, t) > q:
            return "enforce", seq.op_enforce
        return self._done("write", lambda: seq.op_twrite(q, tags=[t] * q))

    def _tie_b(self, seq):
        t = self.tc["mid"]
        x = max(1, seq.model.quota_of(t) // 3)
        return self._done("write", lambda: seq.op_twrite(x, tags=[t] * x), True)

    def _x(self, seq):
        return max(2, seq.model.quota_of(self.tc["mid"]) // 6)

    def _tie_d(self, seq, copies=False):
        """The write that shows the origin: the mid tag is brought back to its quota and takes ``_x`` tag victims.
        ``copies``: every row of the batch is the same pool row, so the tag victims' slots -- which lie right before
        the new origin -- hold duplicates, and the consolidate that follows removes all but the oldest of them: rows
        that precede the origin leave, and the remap is more than the identity."""
        t = self.tc["mid"]
        n = max(0, seq.model.quota_of(t) - self._held(seq, t)) + self._x(seq)
        feats = (lambda: seq.pool.take(1).repeat(n, 1)) if copies else (lambda: None)
        return self._done("write", lambda: seq.op_twrite(n, tags=[t] * n, feats=feats()), True)

    def _ring(self, seq):
        """(ring position of every held row, of the mid tag's origin, bool: the mid tag's rows)."""
        m, t = seq.model, self.tc["mid"]
        c, start = m.count, m._ring_start()
        return (np.arange(c) - start) % c, (m.origin.get(t, 0) % c - start) % c, m.tags_np() == t

    def _move_origin(self, seq):
        t = self.tc["mid"]
        n = max(0, seq.model.quota_of(t) - self._held(seq, t)) + max(1, seq.model.quota_of(t) // 3)
        return "write", lambda: seq.op_twrite(n, tags=[t] * n), True

    def _tie_copies(self, seq):
        # the victims must not run past the end of the ring: then every one of them precedes the new origin
        ring, at, mine = self._ring(seq)
        self.moved = getattr(self, "moved", 0)
        # (and as many of the tag's rows again stay behind the new origin: what the consolidate merges among them must
        # not leave the origin at the end of the tag's rows, where it is as good as origin 0)
        if int((mine & (ring >= at)).sum()) < 2 * self._x(seq) + 1 and self.moved < 4:
            self.moved += 1
            return self._move_origin(seq)
        self.moved = 0
        return self._tie_d(seq, copies=True)

    def _shows(self, seq):
        """Would the next ``_x`` victims of the mid tag differ from what origin 0 and what the cursor (as it is, and 0
        as a compaction leaves it) would give?  From the model's fp64 keys."""
        m, t = seq.model, self.tc["mid"]
        mine, x, now = m.tags_np() == t, self._x(seq), seq.clock.now
        if int(mine.sum()) <= x:
            return False
        # what ``_before_origin`` takes out must leave a row of the tag before the origin (else origin 0 is as good)
        ring, at, _ = self._ring(seq)
        before_mine, before_other = int((mine & (ring < at)).sum()), int((~mine & (ring < at)).sum())
        if not ((before_other >= 1 and before_mine >= 1) or before_mine >= 4):
            return False
        mine_set = set(m.exact_order(m.count, m.origin.get(t, 0), now, mine, x).tolist())
        return all(mine_set != set(m.exact_order(m.count, c, now, mine, x).tolist()) for c in (0, m.cursor))

    def _compaction(self, seq, op, fn):
        """A planned compaction goes ahead once the mid tag's origin sits where it shows (else the tag is written into
        once more, the clock standing still, which moves its origin on).  After three such writes it goes ahead whether
        or not ``_shows`` holds: nothing here proves that three are enough.  What holds a case to the goal is
        ``tag_events``, which asserts from the log that the write after the compaction took victims that neither
        origin 0 nor the cursor would give; a seed or a size where three moves fall short fails there, by name."""
        self.moved = getattr(self, "moved", 0)
        if not self._shows(seq) and self.moved < 3:
            self.moved += 1
            return self._move_origin(seq)
        self.moved = 0
        return self._done(op, fn, True)

    def _before_origin(self, seq):
        """A few held rows that come before the mid tag's origin in ring order (rows of other tags where there are
        some): taking them out is what makes the remap of the origin more than the identity."""
        m, t = seq.model, self.tc["mid"]
        c, start = m.count, m._ring_start()
        ring = (np.arange(c) - start) % c
        before = ring < (m.origin.get(t, 0) % c - start) % c
        cand = np.nonzero(before & (m.tags_np() != t))[0]
        if cand.size == 0:
            cand = np.nonzero(before)[0] if before.any() else np.arange(1)
        return cand[-3:]

    def _c_forget(self, seq):
        return self._compaction(seq, "forget", lambda: seq.op_forget("rows", rows=self._before_origin(seq)))

    def _c_prune(self, seq):
        return self._compaction(seq, "prune", lambda: seq.op_prune_weak(self._before_origin(seq)))

    def _c_consolidate(self, seq):
        return self._compaction(seq, "consolidate", lambda: seq.op_tconsolidate(False, bool(seq.rng.integers(0, 2))))

    def _c_checkpoint(self, seq):
        return self._compaction(seq, "checkpoint", seq.op_checkpoint)

    def _fill(self, seq):
        room = seq.model.M - seq.model.count
        if room == 0:
            self.goals.pop(0)
            return self._full_both(seq)
        return self._done("bulk", lambda: seq.op_tbulk(room, False, tags=self.tc["free"]))

    def _full_both(self, seq):
        m, t = seq.model, self.tc["small"]
        pre = self._quotas(seq, [t])
        if pre:
            return pre
        q = m.quota_of(t)
        room = m.M - m.count
        if room:
            return "bulk", lambda: seq.op_tbulk(room, False, tags=self.tc["free"])
        if self._held(seq, t) < q:
            return "write", lambda: seq.op_twrite(q, tags=[t] * q)
        k = min(q, 3)
        return self._done("write", lambda: seq.op_twrite(k + 3, tags=[t] * k + [self.tc["free"]] * 3))


def tag_events(seq, live=None):
    """The mandatory events of a tag-aware case, from the op log alone.  ``live``: the row count above which the
    list-sorted image is live (asserted only where the case keeps one)."""
    log, tc = seq.log, seq.tc
    wm = [e for e in log if e["op"] == "write_merge_tagged"]
    ev = {
        "keeps a row that the scope-blind rule would have merged": any(e.get("kept_blind_merges") for e in wm),
        "writes a held row again under its own tag: it merges": any(e.get("verbatim_same") for e in wm),
        "writes a held row again under another tag: it is kept, or merges into its copy there":
            any(e.get("verbatim_other") for e in wm),
        "consolidates within tags with a result the scope-blind pass would not give":
            any(e["op"] == "consolidate" and e.get("within") and e.get("differs_from_other_rule") for e in log),
    }
    if tc["quota"] is None:
        return ev
    ev["takes tag victims while the bank has room"] = any(e.get("room_tag_victims") for e in log)
    ev["takes tag victims and global victims in one run of a full bank"] = any(e.get("full_both") for e in log)
    ev["cuts a batch into runs by a quota"] = any(e.get("quota_cut") for e in log)
    stuck = [e["step"] for e in log if e.get("over_quota_unchanged")]
    ev["writes into a tag over its quota that neither grows nor shrinks, then enforces"] = bool(stuck) and any(
        e["op"] == "enforce" and e.get("removed") and e["step"] > stuck[0] for e in log)
    ev["merges rows of a consolidating write into a tag at its quota: they do not count"] = \
        any(e.get("merged_not_counted") for e in wm)
    mid = tc["mid"]
    for kind in ("forget", "prune", "consolidate", "checkpoint"):
        # a compaction must have taken out a row that precedes the mid tag's origin: its remap is not the identity
        ev[f"{kind} with a non-zero origin{'' if kind == 'checkpoint' else ' that it moves'}, then (the clock standing "
           f"still) tag victims that neither origin 0 nor the global cursor would give"] = any(
            a["op"] == kind and any(a["origins_before"].values())
            and (kind == "checkpoint" or a["origins_after"].get(mid, 0) != a["origins_before"].get(mid, 0))
            and b["still"] and b.get("origin_mattered") for a, b in zip(log, log[1:]))
    if tc["many"]:
        ev["ranks more than 64 limited tags in one run"] = any(any(len(v) > 64 for v in e.get("tag_victims", []))
                                                               for e in log if e["op"] == "write")
    if live:
        ev[f"crosses {live} rows downwards by enforce_tag_quotas or a tagged forget while the image is live"] = any(
            (e["op"] == "enforce" or (e["op"] == "forget" and e.get("kind") == "tags")) and e.get("removed")
            and e["count_before"] >= live > e["count_after"] and e["image_live_before"] for e in log)
    return ev
