"""HippocampalFormation: episodic memory bank with HIP write / recall / centroid kernels.

Drop-in for the reference's ``src/core/hippocampal.py`` on the hot path.  Same constructor,
method names, return types, public attributes and ``state_dict`` buffer names
(``memory_features, memory_locations, memory_metadata, centroids, centroid_counts, ...``,
reference ``hippocampal.py:57-117``), so checkpoints round-trip.

What runs where
  * ``create_episodic_memory`` -> ``aura_bank_write`` (row store + 1/||row|| + metadata, and the
    online nearest-centroid running mean when the index is ready, ref ``:211-232``);
  * ``retrieve_similar_memories`` -> ``aura_knn_search_ex`` (fp32-MFMA scan with the reference's
    combined-score epilogue + exact top-k; optional centroid-candidate mask, ref ``:259-307``);
  * ``rebuild_centroids`` -> ``aura_kmeans_assign`` / ``aura_kmeans_update`` (ref ``:345-377``);
  * ``decay_memories`` -> ``aura_bank_decay`` (ref ``:334``);
  * place / grid / time-cell rate codes stay plain torch ops on the device (SURVEY.md 8a row a6:
    not on the throughput path).

Batch entry points that the reference lacks (its callers loop in Python,
``memory_augmented_layer.py:113-121``): ``create_episodic_memories`` and ``recall_batch``.

Reference defects on this path (SURVEY.md 8a "hazards") and what this class does:
  * full bank -> always slot 0 (``:200-202``): REPRODUCED by default (``overflow='reference'``);
    ``overflow='fifo'`` opts into a real ring buffer, ``overflow='weakest'`` into retention: a full bank
    gives up the rows with the smallest ``strength * exp(-age / 3600)`` (``aura_bank_select_weakest``), and
    ``reinforce`` / ``recall_batch(reinforce=...)`` raise the strength of rows that are used.
  * centroid candidates: ``topk`` positions are looked up as bank rows (``:307-317``) -> right
    scores, wrong ids: FIXED (rows are reported); ``k`` is clamped to the number of candidates
    instead of raising; ``location=`` works with candidates.
  * fp32 timestamps / fp32 ``age`` (``:215,296``): REPRODUCED (deterministic given the clock).
  * ``event_id`` / ``associated_experts`` are accepted and dropped (``:195-243``), metadata column 3 is "reserved":
    REPRODUCED by default.  Build-side: a write may carry an integer ``tag`` (``tags=``), kept in that column, and
    ``recall_batch(tags=..., newer_than=..., older_than=..., min_strength=...)`` recalls exactly within a scope
    (``aura_knn_search_scoped``); a bank that never uses tags is bit for bit what it was.  Consolidation can stay
    within tags (``merge_within_tags``, ``find_repeats(tags=...)``, ``consolidate(within_tags=...)``:
    ``aura_bank_find_repeats`` by tag); off by default, and then scope-blind as before.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from collections.abc import Mapping
from types import MappingProxyType
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import ops


@dataclass
class SpatialLocation:
    coordinates: torch.Tensor
    timestamp: float = field(default_factory=time.time)


@dataclass
class EpisodicMemory:
    memory_id: str
    feature_idx: int
    timestamp: float
    strength: float = 1.0


class _EpisodicView(Mapping):
    """``episodic_memories`` of the reference (``:235-239``: a dict id -> EpisodicMemory) without one
    Python object per write: records are built on access from ``id_to_idx`` and the per-slot write
    times.  Read-only; same keys, ``len`` and iteration order as the reference's dict."""

    def __init__(self, owner: "HippocampalFormation"):
        self._o = owner

    def __getitem__(self, mid: str) -> EpisodicMemory:
        slot = self._o.id_to_idx[mid]
        return EpisodicMemory(memory_id=mid, feature_idx=slot, timestamp=float(self._o._slot_time[slot]))

    def __iter__(self):
        return iter(self._o.id_to_idx)

    def __len__(self) -> int:
        return len(self._o.id_to_idx)

    def __contains__(self, mid) -> bool:
        return mid in self._o.id_to_idx


class _IvfState:
    """Inverted lists of the centroid index in the layout ``aura_knn_search_ivf2`` streams: a
    list-sorted 16-bit image with ``slack`` free entries behind every list, so that writes are
    appended in place (``aura_ivf2_append``) and the lists are re-packed only when the centroids
    are rebuilt or the slack is used up.  The image is IEEE half (``sorted_bf16`` keeps its name): normalised rows
    lie in [-1, 1], so half's 11 significand bits narrow the prefilter's band 5-6 times against bf16's 8 at the same
    size; its residual norms are the bank's ``_rho16``.  The row-ordered shadow stays bf16."""

    def __init__(self, max_rows: int, D: int, slack: int, device):
        self.slack = slack
        self.n_alloc = ops.ivf2_alloc_rows(max_rows, slack)
        self.sorted_bf16 = torch.empty(self.n_alloc, D, dtype=torch.float16, device=device)
        self.sorted_rows = torch.empty(self.n_alloc, dtype=torch.int32, device=device)
        self.pad_off = torch.zeros(257, dtype=torch.int32, device=device)
        self.list_len = torch.zeros(256, dtype=torch.int32, device=device)
        self.pos_of_row = torch.full((max_rows,), -1, dtype=torch.int32, device=device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.n_sorted = 16            # sorted rows in use (host-side bound, a multiple of 16; fixed between re-packs)
        self.appended = 0             # rows appended since the last re-pack
        self.valid = False
        self.lists: Optional[ops.Ivf2Lists] = None     # validated handle of this layout (HippocampalFormation._ivf_lists)
        self.word = ops.CompletionWord(device)         # the recall's flag, polled on the host
        # cached score constants of the sorted rows (aura_ivf2_row_constants): valid for ONE fp32 `now` (the
        # reference's fp32 timestamps give time a 128-second grain) while metadata, rho and layout are unchanged
        self.rowc: Optional[torch.Tensor] = None
        self.rowc_live = False
        self.rowc_now = 0.0           # the fp32 `now` the table was built for
        self.rowc_version = -1        # memory_metadata._version it was built from (catches in-place edits by the user)


OVERFLOW_POLICIES = ('reference', 'fifo', 'weakest')

TAG_LIMIT = 1 << 24                   # tags are integers in [0, 2^24): exact as the fp32 of metadata column 3

_INSTANCE_DEFAULT = object()          # create_episodic_memories(merge_similarity=...): "what the bank was built with"


@dataclass
class ConsolidationReport:
    """What a consolidating write did with its ``n`` rows (host tensors and lists).  ``merged[i]``: row i repeated a
    memory and was not stored; ``ids[i]``: the id of the memory row i became (its own id if it was stored, else the id
    of the memory it repeats); ``rows[i]``: the slot ``s`` that holds that memory when the call returns, with
    ``id_of_row(s) == ids[i]``, or -1 if this same call overwrote it again.  ``n_blended``: how many memories' features
    moved (a blending write: once per chunk for every memory that rows of the chunk repeat; 0 without blending)."""
    merged: torch.Tensor
    rows: torch.Tensor
    ids: List[Optional[str]]
    n_stored: int
    n_merged: int
    n_blended: int = 0


@dataclass
class CompactionReport:
    """What ``forget`` / ``prune`` removed: ``old_to_new`` (host int64, one entry per row held BEFORE the call) is the
    row every memory has now, -1 for a forgotten one."""
    n_removed: int
    old_to_new: np.ndarray


@dataclass
class BankConsolidationReport:
    """What ``consolidate`` did with the ``n_before`` held rows: ``n_kept`` remain, ``n_merged`` repeated a kept memory
    and are gone; ``old_to_new`` (host int64 [n_before]) is the row every memory has now -- for a merged row the row of
    the memory it merged into.  ``n_blended``: how many memories' features moved (``consolidate(blend=...)``: once per
    slab for every memory that rows of the slab repeat; 0 without blending)."""
    n_before: int
    n_kept: int
    n_merged: int
    old_to_new: np.ndarray
    n_blended: int = 0


@dataclass
class ReplaySample:
    """What ``replay`` drew (device tensors; reading none of them is forced by the call): ``rows`` int32 [n], the drawn
    bank rows in draw order, ``-1`` where the scope held fewer than ``n`` eligible memories; ``keys`` fp32 [n], their
    draw keys (descending, ``-inf`` at the padding); ``features`` [n, D], ``memory_features[rows]`` with zeros at the
    padding, or None; ``eligible``, an int64 scalar: how many memories the draw could have taken."""
    rows: torch.Tensor
    keys: torch.Tensor
    features: Optional[torch.Tensor]
    eligible: torch.Tensor


class HippocampalFormation(nn.Module):
    # above this many rows the inverted lists (each probed list read once per batch) beat a masked
    # pass over every row
    MASKED_SCAN_MAX_ROWS = 250_000
    MASKED_SCAN_MAX_QUERIES = 512      # beyond: every 256 queries cost another pass over all rows
    SHADOW_MIN_ROWS = 8192             # below: the all-fp32 scan (no prefilter)

    def __init__(self,
                 spatial_dimensions: int = 2,
                 n_place_cells: int = 2000,
                 n_time_cells: int = 100,
                 n_grid_cells: int = 200,
                 max_memories: int = 100000,
                 feature_dim: int = 768,
                 device: str = 'cuda',
                 use_centroid_index: bool = True,
                 overflow: str = 'reference',
                 bf16_shadow: bool = True,
                 merge_similarity: Optional[float] = None,
                 merge_reinforce: float = 0.1,
                 merge_cap: float = 1.0,
                 merge_within_tags: bool = False,
                 tag_quota=None,
                 replay_seed: int = 0,
                 merge_blend: Optional[float] = None):
        super().__init__()
        # consolidating writes (create_episodic_memories): None = every row is stored, today's behaviour
        self._check_merge(merge_similarity, merge_reinforce, merge_cap)
        self.merge_similarity = merge_similarity
        self.merge_reinforce = merge_reinforce
        self.merge_cap = merge_cap
        # blending merges (consolidating writes and consolidate()): None = the first observation stands, today's behaviour
        self._check_blend(merge_blend, merge_similarity)
        self.merge_blend = merge_blend
        # consolidation within tags (consolidating writes and consolidate()): False = scope-blind, today's behaviour
        self.merge_within_tags = bool(merge_within_tags)
        self.spatial_dims = spatial_dimensions
        self.device = torch.device(device if torch.cuda.is_available() else 'cpu')
        dev = self.device

        # place / grid / time cells (reference :55-82)
        self.register_buffer('place_centers', torch.rand(n_place_cells, spatial_dimensions, device=dev) * 20 - 10)
        self.register_buffer('place_radii', torch.rand(n_place_cells, 1, device=dev) * 1.5 + 0.5)
        self.place_max_rate = 20.0
        spacings = torch.logspace(0, 2, n_grid_cells, base=2.0, device=dev).unsqueeze(1)
        self.register_buffer('grid_spacings', spacings)
        self.register_buffer('grid_orientations', torch.rand(n_grid_cells, 1, device=dev) * (torch.pi / 3))
        self.register_buffer('grid_phases', torch.rand(n_grid_cells, spatial_dimensions, device=dev) * spacings)
        self.grid_max_rate = 25.0
        intervals = torch.logspace(0, 3, n_time_cells, base=10.0, device=dev).unsqueeze(1)
        self.register_buffer('time_intervals', intervals)
        self.register_buffer('time_widths', intervals * 0.3)

        # episodic bank, resident in HBM (reference :84-99)
        self.max_memories = max_memories
        self.memory_count = 0
        self.register_buffer('memory_features', torch.zeros(max_memories, feature_dim, device=dev))
        self.register_buffer('memory_locations', torch.zeros(max_memories, spatial_dimensions, device=dev))
        self.register_buffer('memory_metadata', torch.zeros(max_memories, 4, device=dev))
        # build-side: 1/max(||row||, 1e-12), refreshed by every write (not part of the state_dict)
        self.register_buffer('_inv_norm', torch.zeros(max_memories, device=dev), persistent=False)
        self._norms_valid_upto = 0
        # build-side: bf16 copy of the NORMALISED rows for the exact recall's prefilter (half the bytes
        # to stream; results unchanged) and each row's rounding residual (its part of the prefilter's
        # error bound).  Allocated on the first full-scan recall of >= SHADOW_MIN_ROWS rows.
        self._use_shadow = bool(bf16_shadow) and feature_dim % 8 == 0 and feature_dim <= 768
        self._shadow = None
        self._rho = None
        self._rho16 = None            # residual norms of the list-sorted half image (one per bank row, beside _rho)
        self._shadow_valid_upto = 0

        self.id_to_idx: Dict[str, int] = {}
        self._idx_to_id: List[Optional[str]] = [None] * max_memories  # dense reverse map
        self._slot_time = np.zeros(max_memories, dtype=np.float64)     # host clock of each slot's last write
        self.episodic_memories = _EpisodicView(self)
        # bulk-ingested rows get implicit ids "<prefix><n>" resolved on lookup: (slot0, slot1, prefix, n0)
        self._implicit_ids: List[Tuple[int, int, str, int]] = []

        self.current_location = torch.zeros(spatial_dimensions, device=dev)
        self.last_event_time = time.time()
        self.register_buffer('k_const', 4 * torch.pi / torch.sqrt(torch.tensor(3.0, device=dev)))

        self.use_centroid_index = use_centroid_index
        self.centroids_k = 256
        self.centroids_update_interval = 512
        self.register_buffer('centroids', torch.zeros(self.centroids_k, feature_dim, device=dev))
        self.register_buffer('centroid_counts', torch.zeros(self.centroids_k, device=dev))
        self._index_ready = False
        self._last_flag = None                    # overflow flag of the last candidate-mode recall that read it
        # inverted lists of the centroid index, derived from memory_metadata[:, 2]:
        self._ivf: Optional[_IvfState] = None     # list-sorted bf16 shadow, kept current by the writes
        self._ivf_pending = None                  # (order, seg_off) left by rebuild_centroids for the next re-pack
        self._lists = None                        # fp32 fallback lists (list_rows, list_off, list_len, longest)
        self._lists_dirty = True
        # rows may be held that no inverted list files (centroid id < 0: positioned or bulk writes after the index was
        # built, metadata edited by the user); the next rebuild_centroids assigns every row again
        self._unlisted_rows = False

        if overflow not in OVERFLOW_POLICIES:
            raise ValueError(f"overflow must be 'reference', 'fifo' or 'weakest', got {overflow!r}")
        self._overflow = overflow
        self._write_cursor = 0
        # per-tag quotas (the rule: include/aura_hip.h, "Per-tag quotas"): None = off, today's behaviour
        self._tag_quota_default: Optional[int] = None   # every tag except 0
        self._tag_quota_map: Dict[int, int] = {}        # named tags (0 may be named)
        self._tag_origin: Dict[int, int] = {}           # tie origin c_t per limited tag (missing: 0)
        self._pending_origins: Optional[Dict[int, int]] = None    # left by _plan_slots for the write that follows
        if tag_quota is not None:
            if isinstance(tag_quota, Mapping):
                for t, q in tag_quota.items():
                    self.set_tag_quota(t, q)
            else:
                self.set_tag_quota(None, tag_quota)
        # replay (the rule: include/aura_hip.h, "Replay"): the seed of every draw and how many replay() has numbered
        self.replay_seed = int(replay_seed)
        if not (0 <= self.replay_seed < (1 << 64)):
            raise ValueError(f"replay_seed must be in [0, 2^64), got {replay_seed!r}")
        self._replay_draws = 0
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate_norms())

    # ------------------------------------------------------------------ plumbing
    def _invalidate_norms(self) -> None:
        self._norms_valid_upto = 0
        self._shadow_valid_upto = 0
        self._unlisted_rows = True
        self._invalidate_lists()

    def _invalidate_lists(self) -> None:
        self._lists_dirty = True
        self._ivf_pending = None
        if self._ivf is not None:
            self._ivf.valid = False

    def _ensure_rho(self) -> torch.Tensor:
        dev = self.memory_features.device
        if self._rho is None or self._rho.device != dev:
            self._rho = torch.zeros(self.max_memories, dtype=torch.float32, device=dev)
            self._rho16 = torch.zeros(self.max_memories, dtype=torch.float32, device=dev)
            self._shadow_valid_upto = 0
            if self._ivf is not None:
                self._ivf.valid = False
        return self._rho

    def _shadow_applies(self) -> bool:
        return self._use_shadow and self.memory_count >= self.SHADOW_MIN_ROWS and self.memory_features.is_cuda

    def _ensure_shadow(self):
        """bf16 shadow of rows [0, memory_count) (+ their residual norms), or None when it does not apply."""
        if not self._shadow_applies():
            return None
        self._ensure_norms()
        rho = self._ensure_rho()
        if self._shadow is None or self._shadow.device != self.memory_features.device:
            self._shadow = torch.empty(self.memory_features.shape, dtype=torch.bfloat16,
                                       device=self.memory_features.device)
            self._shadow_valid_upto = 0
        if self._shadow_valid_upto < self.memory_count:
            lo = self._shadow_valid_upto
            ops.bank_shadow_update(self.memory_features, self._inv_norm, self._shadow, rho, lo,
                                   self.memory_count - lo)
            self._shadow_valid_upto = self.memory_count
        return self._shadow

    def _shadow_after_write(self, slot_t: torch.Tensor, lo: int, hi: int, contiguous: bool) -> None:
        """Keep the shadow current for the rows just written.  The watermark ``_shadow_valid_upto`` only
        ever moves over rows that HAVE been converted: a contiguous append that starts at the watermark
        advances it; rows below it are converted in place; anything else is left to ``_ensure_shadow``
        (which converts [watermark, count) before the next recall)."""
        if self._shadow is None:
            return
        upto = self._shadow_valid_upto
        if contiguous and lo == upto:
            ops.bank_shadow_update(self.memory_features, self._inv_norm, self._shadow, self._rho, lo, hi + 1 - lo)
            self._shadow_valid_upto = hi + 1
        elif lo < upto:
            below = slot_t if hi < upto else slot_t[slot_t < upto]
            ops.bank_shadow_update(self.memory_features, self._inv_norm, self._shadow, self._rho, slots=below.contiguous())

    def _ensure_lists(self):
        """fp32 inverted lists (the fallback of the two-stage lists): row ids of [0, memory_count) sorted
        by centroid id (rows with id < 0 first), list starts and lengths -- a stable sort + bincount on
        the device, redone only after a write / rebuild changed the assignments."""
        n = self.memory_count
        if self._lists is None or self._lists_dirty or self._lists[4] != n:
            order, seg_off = ops.group_by_cluster(self.memory_metadata[:n, 2], 256)
            lens = (seg_off[1:] - seg_off[:-1]).contiguous()
            # slots per query: no query can collect more rows than the 8 longest lists hold
            # (one host read per list rebuild, not per recall)
            longest = int(torch.topk(lens, min(8, lens.numel())).values.sum().item())
            self._lists = (order, seg_off, lens, longest, n)
            self._lists_dirty = False
        return self._lists[:4]

    def _ensure_ivf(self) -> Optional[_IvfState]:
        """The list-sorted half image (and ``_rho16``) for the two-stage inverted-list recall (re-packed only after a
        centroid rebuild or when the slack behind the lists is used up); None when it does not apply."""
        if not self._shadow_applies():
            return None
        self._ensure_norms()
        rho = self._ensure_rho()
        slack = ops.ivf2_slack(self.centroids_update_interval)
        st = self._ivf
        D = self.memory_features.shape[1]
        if st is None or st.sorted_bf16.device != self.memory_features.device or st.slack != slack:
            st = self._ivf = _IvfState(self.max_memories, D, slack, self.memory_features.device)
        if not st.valid:
            n = self.memory_count
            if self._ivf_pending is not None and self._ivf_pending[0].numel() == n:
                order, seg_off = self._ivf_pending
            else:
                order, seg_off = ops.group_by_cluster(self.memory_metadata[:n, 2], 256)
            self._ivf_pending = None
            ops.ivf2_layout(order, seg_off, slack, st.sorted_rows, st.pad_off, st.list_len)
            st.n_sorted = min(st.n_alloc, ops.ivf2_alloc_rows(n, slack))
            st.pos_of_row.fill_(-1)
            st.flag.zero_()
            st.rowc_live = False
            ops.bank_shadow_sorted(self.memory_features, self._inv_norm, st.sorted_rows, st.sorted_bf16, rho,
                                   st.pos_of_row, st.n_sorted, rho16=self._rho16)
            st.appended = 0
            st.valid = True
        return st

    def _ivf_row_constants(self, st: _IvfState, now: float) -> torch.Tensor:
        """The sorted rows' score constants for ``now``, rebuilt only when ``now`` (as fp32), the metadata or
        the list layout changed since the last call (31 us per call at 1 M rows otherwise)."""
        nowf = float(np.float32(now))
        if st.rowc is None or st.rowc.device != st.sorted_rows.device:
            st.rowc = torch.empty(st.n_alloc, 4, dtype=torch.float32, device=st.sorted_rows.device)
            st.rowc_live = False
        ver = self.memory_metadata._version
        if not (st.rowc_live and st.rowc_now == nowf and st.rowc_version == ver):
            ops.ivf2_row_constants(self.memory_metadata, self._rho16, st.sorted_rows, st.n_sorted,
                                   self.memory_features.shape[1], nowf, st.rowc, half=True)
            st.rowc_live, st.rowc_now, st.rowc_version = True, nowf, ver
        return st.rowc

    def _ivf_after_write(self, uniq_slots: torch.Tensor, n_rows: int, meta_v0: Optional[int] = None) -> None:
        """Append the rows just written to their lists (their centroid ids are in the metadata).
        ``meta_v0``: ``memory_metadata._version`` before the write touched it (the cached score constants
        follow the write only if nobody else edited the metadata since they were built)."""
        st = self._ivf
        if st is None or not st.valid:
            return
        # Rows spread over the 256 lists, so a list's slack lasts far longer than `slack` appended rows;
        # the append kernel flags a list that does overflow (the row is then missing from the lists) and
        # the next recall sees that flag in the read it does anyway (recall_batch).  Holes (overwritten
        # rows) are scanned like padding: re-pack once they are worth it.
        if self._rho is None or st.appended + n_rows > max(st.slack, self.memory_count // 8):
            st.valid = False
            return
        live = st.rowc is not None and st.rowc_live and meta_v0 is not None and st.rowc_version == meta_v0
        ops.ivf2_append(self.memory_features, self._inv_norm, self.memory_metadata, uniq_slots, st.sorted_bf16,
                        st.sorted_rows, st.pad_off, st.list_len, st.pos_of_row, self._rho, st.flag,
                        row_constants=st.rowc if live else None, row_constants_now=st.rowc_now, rho16=self._rho16)
        st.appended += n_rows
        st.rowc_live = live
        st.rowc_version = self.memory_metadata._version
        # (n_sorted stays what the re-pack set: pad_off is fixed until the next one, so no list reaches beyond it)

    def _apply(self, fn, *a, **k):  # keep self.device / current_location in step with .to()
        out = super()._apply(fn, *a, **k)
        self.device = self.memory_features.device
        self.current_location = fn(self.current_location)
        return out

    def _ensure_norms(self) -> None:
        if self._norms_valid_upto < self.memory_count:
            ops.bank_row_norms(self.memory_features, self._inv_norm, 0, self.memory_count)
            self._norms_valid_upto = self.memory_count

    def refresh_norms(self) -> None:
        """Recompute the cached row norms and drop the bf16 shadows (call after writing
        ``memory_features`` or ``memory_metadata[:, 2]`` directly).  As after ``load_state_dict``, rows may then be
        held that no inverted list files, so until the next ``rebuild_centroids`` ``find_repeats`` (consolidating
        writes) scans the row-ordered bf16 shadow instead of the list-sorted one: on an indexed bank that is a second
        image of the bank (2 bytes per element) and one conversion pass."""
        self._invalidate_norms()
        if self.memory_count:
            self._ensure_norms()

    def _features_to_device(self, features, rows: Optional[int] = None) -> torch.Tensor:
        if (rows is None and isinstance(features, torch.Tensor) and features.dtype == torch.float32 and features.dim() == 2
                and features.device == self.memory_features.device and features.shape[1] == self.memory_features.shape[1]
                and features.is_contiguous() and not features.requires_grad):
            return features                       # already what the kernels take (the common case of batched recall)
        if isinstance(features, np.ndarray):
            features = torch.from_numpy(features)
        f = features.detach().to(device=self.device, dtype=torch.float32)
        D = self.memory_features.shape[1]
        f = f.reshape(-1, D) if rows is None else f.reshape(rows, D)
        return f.contiguous()

    # ------------------------------------------------------------------ spatial / temporal context
    def update_spatial_state(self, new_location: torch.Tensor, dt: float = 0.1) -> None:
        if isinstance(new_location, np.ndarray):
            new_location = torch.from_numpy(new_location).to(self.device, dtype=torch.float32)
        self.current_location = new_location if new_location.dim() == 1 else new_location[0]

    def get_spatial_context(self) -> Dict[str, Any]:
        loc = self.current_location.unsqueeze(0)
        dists = torch.norm(loc - self.place_centers, dim=1, keepdim=True)
        sigmas = self.place_radii / 3.0
        place_rates = self.place_max_rate * torch.exp(-(dists ** 2) / (2 * sigmas ** 2))
        place_rates = place_rates * (dists <= self.place_radii).float()
        cos_o, sin_o = torch.cos(self.grid_orientations), torch.sin(self.grid_orientations)
        x, y = loc[0, 0], loc[0, 1]
        rotated = torch.cat([cos_o * x - sin_o * y, sin_o * x + cos_o * y], dim=1)
        shifted = rotated - self.grid_phases
        k = self.k_const / self.grid_spacings
        u1 = k * shifted[:, 0:1]
        u2 = k * (-0.5 * shifted[:, 0:1] + 0.866 * shifted[:, 1:2])
        u3 = k * (-0.5 * shifted[:, 0:1] - 0.866 * shifted[:, 1:2])
        grid_val = (torch.cos(u1) + torch.cos(u2) + torch.cos(u3)) / 3.0 + 0.5
        grid_rates = self.grid_max_rate * torch.relu(grid_val)
        return {"current_location": self.current_location, "place_cells": place_rates.flatten(),
                "grid_cells": grid_rates.flatten(), "n_memories": self.memory_count}

    def get_temporal_context(self) -> Dict[str, Any]:
        elapsed = time.time() - self.last_event_time
        diff = elapsed - self.time_intervals
        time_rates = 15.0 * torch.exp(-(diff ** 2) / (2 * (self.time_widths / 3) ** 2))
        return {"time_cells": time_rates.flatten(), "elapsed": elapsed}

    # ------------------------------------------------------------------ write
    def _plan_slots(self, n: int, now: Optional[float] = None, tags: Optional[np.ndarray] = None):
        """Slots (int64 ndarray) for the next n writes, how many of them append, and the counters they
        leave behind (nothing is mutated until the kernel launch has been accepted).

        ``overflow='weakest'``: the ``rest`` rows that do not fit overwrite the first ``rest`` rows of the
        eviction order -- ascending ``(strength * exp(-(now - timestamp) / 3600), (row - cursor) mod count)``
        over the rows held BEFORE this write, ``now`` the write's own timestamp.  The batch is the unit: all
        its victims are ranked once, so a batch is NOT the same as n one-row writes (a one-row loop re-ranks
        after every row, and may evict a row it has just written).  In a bank of equal keys the victims are
        exactly the slots ``'fifo'`` takes, in the same order.  The id maps live on the host, so the selected
        slots are copied there: one device-to-host read per OVERFLOWING run; appends and the other two
        policies read nothing back.

        ``tags`` (the run's tags, int [n]) matter only to a bank with ``tag_quota``: a run that carries a limited tag
        is planned by ``_plan_slots_quota``; any other run reads and launches exactly what it did."""
        if tags is not None and (self._tag_quota_map or self._tag_quota_default is not None):
            scopes = self._limited_in(tags)
            if scopes:
                return self._plan_slots_quota(n, time.time() if now is None else now, scopes)
        M, count, cursor = self.max_memories, self.memory_count, self._write_cursor
        n_app = min(n, max(M - count, 0))
        slots = np.empty(n, dtype=np.int64)
        slots[:n_app] = np.arange(count, count + n_app, dtype=np.int64)
        rest = n - n_app
        if rest:
            if self._overflow == 'reference':
                slots[n_app:] = 0                  # count % max_memories with count == max_memories (:200-202)
            elif self._overflow == 'weakest':
                if rest > count:                   # (create_episodic_memories splits such runs)
                    raise ValueError(f"'weakest' cannot evict {rest} rows from a bank that holds {count}")
                rows, _ = ops.bank_select_weakest(self.memory_metadata, count, time.time() if now is None else now,
                                                  cursor % M, rest)
                slots[n_app:] = rows.cpu().numpy()
                cursor += rest
            else:
                slots[n_app:] = (cursor + np.arange(rest, dtype=np.int64)) % M
                cursor += rest
        return slots, n_app, count + n_app, cursor

    # ------------------------------------------------------------------ per-tag quotas
    @staticmethod
    def _check_quota_tag(tag) -> int:
        if isinstance(tag, bool) or not isinstance(tag, (int, np.integer)) or not (0 <= int(tag) < TAG_LIMIT):
            raise ValueError(f"tag_quota: a tag must be an integer in [0, 2^24 = {TAG_LIMIT}), got {tag!r}")
        return int(tag)

    def set_tag_quota(self, tag, quota) -> None:
        """Limit tag ``tag`` to ``quota`` rows (an int >= 1; None removes the limit).  ``tag=None`` sets the quota of
        EVERY tag except 0 that is not named on its own.  Needs ``overflow='weakest'`` (``ValueError`` otherwise): a
        write into a tag at its quota replaces that tag's own weakest memories (the rule: ``include/aura_hip.h``,
        "Per-tag quotas").  Nothing is enforced here: a tag that already holds more keeps its rows -- it neither grows
        nor shrinks on writes -- until ``enforce_tag_quotas()``."""
        if tag is not None:
            tag = self._check_quota_tag(tag)
        if quota is None:
            if tag is None:
                self._tag_quota_default = None
            else:
                self._tag_quota_map.pop(tag, None)
            return
        if isinstance(quota, bool) or not isinstance(quota, (int, np.integer)) or int(quota) < 1:
            raise ValueError(f"tag_quota: a quota must be an integer >= 1, got {quota!r}")
        if self._overflow != 'weakest':
            raise ValueError(f"tag_quota needs overflow='weakest' (a tag at its quota evicts its own weakest rows), "
                             f"this bank has overflow={self._overflow!r}")
        if tag is None:
            self._tag_quota_default = int(quota)
        else:
            self._tag_quota_map[tag] = int(quota)

    @property
    def tag_quotas(self) -> Mapping:
        """Read-only ``{tag: quota}``; the key ``None`` holds the quota of every tag except 0 not named on its own."""
        view = dict(self._tag_quota_map)
        if self._tag_quota_default is not None:
            view[None] = self._tag_quota_default
        return MappingProxyType(view)

    def _quota_of(self, tag: int) -> Optional[int]:
        q = self._tag_quota_map.get(tag)
        if q is None and tag != 0:
            q = self._tag_quota_default
        return q

    def _limited_in(self, tags: np.ndarray) -> List[Tuple[int, int, int]]:
        """``(tag, rows of it, quota)`` for every limited tag among ``tags``, ascending by tag."""
        uniq, n_in = np.unique(np.asarray(tags), return_counts=True)
        out = []
        for t, m in zip(uniq.tolist(), n_in.tolist()):
            q = self._quota_of(int(t))
            if q is not None:
                out.append((int(t), int(m), q))
        return out

    def _quota_run(self, tags: np.ndarray) -> int:
        """The longest prefix of ``tags`` that holds at most q(t) rows of each limited tag t."""
        run = int(tags.size)
        for t, m, q in self._limited_in(tags):
            if m > q:
                run = min(run, int(np.nonzero(tags == t)[0][q]))
        return run

    def _plan_slots_quota(self, n: int, now: float, scopes: List[Tuple[int, int, int]]):
        """``_plan_slots`` for a run that carries limited tags (``scopes``: ``_limited_in`` of its tags): steps 1 - 4 of
        the rule.  One launch sequence and one host read bring held_t, x_t and the tag victims of every scope
        (``ops.bank_select_weakest_scoped``); a second read only when global victims are needed, which are selected
        with the tag victims masked out.  The new tie origins wait in ``_pending_origins`` for the write."""
        M, count, cursor = self.max_memories, self.memory_count, self._write_cursor
        scope_tags = [t for t, _, _ in scopes]
        n_in = [m for _, m, _ in scopes]
        for t, m, q in scopes:
            if m > q:                                      # (_write_batch cuts such runs)
                raise ValueError(f"a run holds at most quota = {q} rows of tag {t}, got {m}")
        tagv = np.zeros(0, dtype=np.int64)
        origins: Dict[int, int] = {}
        bitmap = None
        if count:
            packed, bitmap = ops.bank_select_weakest_scoped(self.memory_metadata, count, now, scope_tags,
                                                            [self._tag_origin.get(t, 0) for t in scope_tags], n_in,
                                                            [q for _, _, q in scopes])
            _, _, victims = ops.scoped_selection_decode(packed.cpu(), n_in)      # THE host read
            for t, v in zip(scope_tags, victims):
                if v.size:
                    origins[t] = int(v[-1]) + 1
            tagv = np.concatenate(victims).astype(np.int64)
        rem = n - int(tagv.size)
        n_app = min(rem, max(M - count, 0))
        g = rem - n_app
        glob = np.zeros(0, dtype=np.int64)
        if g:
            if g > count - tagv.size:
                raise ValueError(f"'weakest' cannot evict {g + tagv.size} rows from a bank that holds {count}")
            if tagv.size:
                rows, _ = ops.bank_select_weakest_masked(self.memory_metadata, count, now, cursor % M, g, bitmap)
            else:
                rows, _ = ops.bank_select_weakest(self.memory_metadata, count, now, cursor % M, g)
            glob = rows.cpu().numpy().astype(np.int64)     # the second read
            cursor += g
        slots = np.concatenate([np.arange(count, count + n_app, dtype=np.int64), tagv, glob])
        self._pending_origins = origins
        return slots, n_app, count + n_app, cursor

    def _limited_tags_held(self) -> List[int]:
        """The limited tags: the named ones, and -- with a quota for every tag -- the tags the bank holds (a read of
        the distinct values of the tag column)."""
        tags = set(self._tag_quota_map)
        if self._tag_quota_default is not None and self.memory_count:
            tags.update(t for t in torch.unique(self.memory_tags).cpu().tolist() if 0 < t < TAG_LIMIT)
        return sorted(tags)

    def tag_counts(self, tags=None) -> Dict[int, int]:
        """``{tag: rows held}`` for ``tags`` (an int or ints; default: the limited tags), counted on the device by one
        pass over the metadata per 64 tags (``ops.bank_tag_counts``) and read back once."""
        if tags is None:
            want = self._limited_tags_held()
        else:
            t = (tags.detach().cpu().numpy() if isinstance(tags, torch.Tensor) else np.asarray(tags)).reshape(-1)
            want = sorted(set(self._check_tags(t, t.size).tolist())) if t.size else []
        if not want:
            return {}
        if self.memory_count == 0:
            return {t: 0 for t in want}
        counts = ops.bank_tag_counts(self.memory_metadata, self.memory_count, want).cpu().tolist()
        return dict(zip(want, counts))

    def enforce_tag_quotas(self, now: Optional[float] = None) -> CompactionReport:
        """Bring every limited tag that holds more than its quota down to it: the first ``held_t - q(t)`` rows of the
        tag's eviction order at ``now`` (default: the clock) are forgotten through ``forget`` (one compaction; the tie
        origins follow).  Two host reads: the counts, then the victims.  Returns ``forget``'s report."""
        count = self.memory_count
        over = [(t, h, self._quota_of(t)) for t, h in self.tag_counts().items() if h > self._quota_of(t)]
        if not over:
            return CompactionReport(0, np.arange(count, dtype=np.int64))
        now = time.time() if now is None else now
        scope_tags = [t for t, _, _ in over]
        n_in = [h - q for _, h, q in over]                  # incoming = the excess: x_t = min(in, held + in - q) = held - q
        packed, _ = ops.bank_select_weakest_scoped(self.memory_metadata, count, now, scope_tags,
                                                   [self._tag_origin.get(t, 0) for t in scope_tags], n_in,
                                                   [q for _, _, q in over])
        _, _, victims = ops.scoped_selection_decode(packed.cpu(), n_in)
        for t, v in zip(scope_tags, victims):
            if v.size:
                self._tag_origin[t] = int(v[-1]) + 1
        return self.forget(rows=np.concatenate(victims))

    @staticmethod
    def _last_occurrences(slots: np.ndarray, n_app: int) -> Optional[np.ndarray]:
        """Indices (ascending) of the last write to every distinct slot, or None if all are distinct."""
        if slots.size - n_app <= 0 or (slots.size - n_app == 1 and n_app == 0):
            return None
        _, first_rev = np.unique(slots[::-1], return_index=True)
        if first_rev.size == slots.size:
            return None
        return np.sort(slots.size - 1 - first_rev)

    def _after_write(self, slot_t: torch.Tensor, uniq_t: torch.Tensor, slots: np.ndarray, c0: int, n_app: int,
                     meta_v0: Optional[int] = None) -> None:
        """Derived state after a write: the appended run [c0, c0 + n_app) and the overwritten slots."""
        if n_app and self._norms_valid_upto >= c0:     # the kernel refreshed 1/||row|| of the written slots
            self._norms_valid_upto = max(self._norms_valid_upto, c0 + n_app)
        if self._shadow is not None:
            if n_app:
                self._shadow_after_write(slot_t[:n_app], c0, c0 + n_app - 1, contiguous=True)
            if slots.size > n_app:
                over = uniq_t[uniq_t < c0] if n_app else uniq_t
                if over.numel():
                    self._shadow_after_write(over, int(slots[n_app:].min()), int(slots[n_app:].max()), contiguous=False)
        self._lists_dirty = True
        self._ivf_pending = None
        self._ivf_after_write(uniq_t, int(uniq_t.numel()), meta_v0)

    def _write_rows(self, ids: Sequence[str], feats: torch.Tensor, now: float,
                    tags: Optional[np.ndarray] = None, plan_tags: Optional[np.ndarray] = None) -> None:
        """Write a run of rows that contains no centroid-rebuild boundary.  ``plan_tags``: the run's tags as the quota
        rule sees them (None: no quota is set, or no row of the run can be limited)."""
        if plan_tags is None:
            slots, n_app, new_count, new_cursor = self._plan_slots(len(ids), now)
        else:
            slots, n_app, new_count, new_cursor = self._plan_slots(len(ids), now, tags=plan_tags)
        origins, self._pending_origins = self._pending_origins, None
        self._store_rows(ids, feats, slots, n_app, new_count, new_cursor, now,
                         online=self.use_centroid_index and self._index_ready, selected=True, tags=tags)
        if origins:                                        # (the write was accepted)
            self._tag_origin.update(origins)

    # ------------------------------------------------------------------ tags
    @staticmethod
    def _check_tags(tags, n: int) -> Optional[np.ndarray]:
        """``tags`` of a write (None, an int for every row, or one int per row) as int32 [n], or None."""
        if tags is None:
            return None
        if isinstance(tags, torch.Tensor):
            tags = tags.detach().cpu().numpy()
        t = np.asarray(tags)
        if t.dtype.kind not in "iu":
            raise ValueError(f"tags must be integers, got dtype {t.dtype}")
        t = t.astype(np.int64)
        if t.ndim == 0:
            t = np.full(n, int(t), dtype=np.int64)
        t = t.reshape(-1)
        if t.size != n:
            raise ValueError(f"{t.size} tags for {n} rows")
        if t.size and (int(t.min()) < 0 or int(t.max()) >= TAG_LIMIT):
            raise ValueError(f"tags must be in [0, 2^24 = {TAG_LIMIT}), got {int(t.min())} .. {int(t.max())}")
        return t.astype(np.int32)

    def _stamp_tags(self, slots: np.ndarray, tags: np.ndarray) -> None:
        """Column 3 of the DISTINCT held rows ``slots`` <- ``tags``, one launch (``aura_bank_set_tags``).  Through the
        library, not an in-place torch op: ``_ivf_after_write`` reads a changed ``memory_metadata._version`` as "the
        cached score constants are stale", and a tag is no part of a score."""
        if slots.size == 0:
            return
        ops.bank_set_tags(self.memory_metadata, self.memory_count,
                          torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).to(self.device),
                          torch.from_numpy(np.ascontiguousarray(tags, dtype=np.int32)).to(self.device))

    @property
    def memory_tags(self) -> torch.Tensor:
        """int32 [memory_count]: the tag of every held row (``memory_metadata[:count, 3]``; 0 = untagged).  Read-only:
        a copy in another dtype, writing to it changes nothing -- use ``retag``."""
        return self.memory_metadata[:self.memory_count, 3].to(torch.int32)

    def retag(self, rows=None, ids: Optional[Sequence[str]] = None, tag=0) -> int:
        """Give the held memories at bank rows ``rows`` (ints of any shape; ``-1``, rows outside the bank and
        duplicates are ignored) and / or with the explicit ids ``ids`` (an unknown id raises ``KeyError`` before
        anything changes) the tag ``tag``: one int for all of them, or -- with ``rows`` alone, when every row is held
        and distinct -- one int per row.  ``tag=0`` removes a tag.  One launch; returns the number of rows stamped."""
        count = self.memory_count
        picked: List[np.ndarray] = []
        if rows is not None:
            r = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
            picked.append(r.reshape(-1).astype(np.int64))
        if ids is not None:
            slots = [self.id_to_idx[mid] for mid in ids]            # KeyError: nothing has changed yet
            picked.append(np.asarray([s for mid, s in zip(ids, slots) if s < count and self._idx_to_id[s] == mid],
                                     dtype=np.int64))
        if not picked:
            raise ValueError("retag needs rows or ids")
        allr = np.concatenate(picked)
        if (tag.dim() if isinstance(tag, torch.Tensor) else np.ndim(tag)) == 0:
            held = np.unique(allr[(allr >= 0) & (allr < count)])
            t = self._check_tags(tag, held.size)
        else:
            t = self._check_tags(tag, allr.size)
            if ids is not None or allr.size != np.unique(allr).size or (allr.size and (allr.min() < 0 or allr.max() >= count)):
                raise ValueError("retag: one tag per row needs rows alone, every one held and distinct")
            held = allr
        self._stamp_tags(held, t)
        return int(held.size)

    def write_at(self, ids: Sequence[str], feats: torch.Tensor, slots: np.ndarray, n_app: int, now: float,
                 cids: Optional[torch.Tensor] = None, tags=None) -> None:
        """Positioned write, the building block of a row-sharded bank (``sharded.ShardedHippocampus``):
        row i goes to local slot ``slots[i]``; the first ``n_app`` slots extend the bank
        (``memory_count .. memory_count + n_app - 1``), the rest overwrite.  No centroid update happens
        here: ``cids`` (fp32 [n], device) are the centroid ids the caller assigned against the
        replicated centroid table (None: -1, "no list").  ``tags``: as ``create_episodic_memories``."""
        feats = self._features_to_device(feats)
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        tags = self._check_tags(tags, len(ids))
        if feats.shape[0] != len(ids) or slots.size != len(ids):
            raise ValueError("write_at: ids, feats and slots disagree")
        if slots.size == 0:
            return
        if n_app and not np.array_equal(slots[:n_app], np.arange(self.memory_count, self.memory_count + n_app)):
            raise ValueError("write_at: the appended slots must continue the bank")
        if slots.min() < 0 or slots.max() >= self.max_memories or slots[n_app:].max(initial=-1) >= self.memory_count + n_app:
            raise ValueError("write_at: slot out of range")
        self._store_rows(ids, feats, slots, n_app, self.memory_count + n_app, self._write_cursor, now,
                         online=False, cids=cids, tags=tags)

    def _store_rows(self, ids, feats, slots: np.ndarray, n_app: int, new_count: int, new_cursor: int, now: float,
                    online: bool, cids: Optional[torch.Tensor] = None, selected: bool = False,
                    tags: Optional[np.ndarray] = None) -> None:
        """``selected``: the slots come from ``_plan_slots`` (not from a caller of ``write_at``).  ``tags`` (int32 [n],
        checked): stamped after the write, by the row that finally owns each slot."""
        c0 = self.memory_count
        meta_v0 = self.memory_metadata._version
        slot_t = torch.from_numpy(slots).to(self.device)
        eff_k = min(self.centroids_k, self.centroids.shape[0])
        if not online:
            self._unlisted_rows = True
        # A batch that overwrites may name a slot more than once, in three ways: a full bank in the reference's
        # mode sends every write to slot 0; a FIFO ring laps itself (more than max_memories overwrites); a FIFO
        # ring wraps onto the slots the SAME batch has just appended (a batch that first fills the bank and then
        # overwrites from the cursor on reaches [c0, c0 + n_app) once cursor + overwrites passes c0).  The last
        # write wins, as in the reference's sequential loop.  The serial centroid kernel walks the rows in order;
        # the parallel kernel orders nothing between rows, so it gets the survivors only.
        # This function decides, and it vouches for distinct slots (``ring_distinct``) only where that follows
        # from the plan: pure appends; a selection of victims held before the write; a ring run that neither laps
        # itself nor reaches the appended run.  Everything else -- and every overwrite whose slots a caller of
        # ``write_at`` chose -- is looked at on the host (``_last_occurrences``).
        rest = slots.size - n_app
        if not selected:
            ring_distinct = False
        elif self._overflow == 'weakest':
            # a selection names every victim once, and victims are rows held before the write (< c0, the
            # appended run starts at c0): distinct as long as no more rows are evicted than were held
            # (_plan_slots refuses more)
            ring_distinct = rest <= c0
        elif self._overflow == 'fifo':
            # the run [cursor, cursor + rest) mod M: distinct from itself up to M rows; with appends in the same
            # batch it also has to end before the first appended slot
            start = self._write_cursor % self.max_memories
            ring_distinct = rest <= self.max_memories and (n_app == 0 or start + rest <= c0)
        else:
            ring_distinct = False
        keep = None if (rest == 0 or ring_distinct) else self._last_occurrences(slots, n_app)
        keep_t = None if keep is None else torch.from_numpy(keep).to(self.device)
        uniq_t = slot_t if keep is None else slot_t[keep_t].contiguous()
        if keep is not None and not online:
            feats_w, slot_w = feats[keep_t].contiguous(), uniq_t
        else:
            feats_w, slot_w = feats, slot_t
        ops.bank_write(self.memory_features, self.memory_locations, self.memory_metadata,
                       self._inv_norm, feats_w, slot_w,
                       self.current_location.to(device=self.device, dtype=torch.float32).contiguous(),
                       now,
                       centroids=self.centroids if online else None,
                       centroid_counts=self.centroid_counts if online else None,
                       eff_k=eff_k if online else 0, distinct_slots=keep is None)
        if cids is not None:
            c = cids.to(device=self.device, dtype=torch.float32)
            self.memory_metadata[uniq_t, 2] = c if keep is None else c[keep_t]
        self.memory_count, self._write_cursor = new_count, new_cursor
        if tags is not None:                           # (the write itself left 0.0, "untagged", in column 3)
            if keep is None:
                self._stamp_tags(slots, tags)
            else:
                self._stamp_tags(slots[keep], tags[keep])
        self._after_write(slot_t, uniq_t, slots, c0, n_app, meta_v0)
        self._slot_time[slots] = time.time()
        slot_list = slots.tolist()
        self.id_to_idx.update(zip(ids, slot_list))
        if n_app:
            self._idx_to_id[c0:c0 + n_app] = list(ids[:n_app])
        if len(slot_list) > n_app:
            over = slot_list[n_app:]
            run = ring_distinct and over[-1] - over[0] == len(over) - 1
            if run and self._overflow == 'weakest':                        # (a selection need not ascend)
                run = bool((np.diff(slots[n_app:]) == 1).all())
            if run:                                                        # one contiguous run of the ring: a slice
                self._idx_to_id[over[0]:over[-1] + 1] = list(ids[n_app:])
            else:
                for mid, slot in zip(ids[n_app:], over):
                    self._idx_to_id[slot] = mid

    def id_of_row(self, row: int) -> Optional[str]:
        """Memory id stored at bank row ``row`` (explicit id, else the implicit bulk id)."""
        mid = self._idx_to_id[row]
        if mid is None:
            for s0, s1, prefix, n0 in reversed(self._implicit_ids):
                if s0 <= row < s1:
                    # (after a compaction took rows out of the range: the surviving original indices, an array)
                    return f"{prefix}{n0 + row - s0}" if isinstance(n0, int) else f"{prefix}{int(n0[row - s0])}"
        return mid

    def bulk_write(self, features: torch.Tensor, id_prefix: str = "bulk-", first_index: int = 0,
                   rebuild: bool = True, tags=None) -> int:
        """Seeding path for very large ingests (BASELINE config 5): rows go to the bank through the
        batched write kernel with NO per-row Python objects (ids are implicit,
        ``f"{id_prefix}{first_index + i}"``, resolved by ``id_of_row``) and NO online centroid
        update; with ``rebuild`` the centroid index is rebuilt once at the end.  This deliberately
        departs from the reference's rebuild-every-512-inserts schedule, which is quadratic in the
        bank size; use ``create_episodic_memories`` for reference-identical semantics.
        ``tags`` (an int, or one int per row of ``features``): as ``create_episodic_memories``.
        Returns the number of rows written (stops at ``max_memories``)."""
        feats = self._features_to_device(features)
        tags = self._check_tags(tags, feats.shape[0])
        n = min(feats.shape[0], self.max_memories - self.memory_count)
        if n <= 0:
            return 0
        s0 = self.memory_count
        meta_v0 = self.memory_metadata._version
        self._unlisted_rows = True
        slot_t = torch.arange(s0, s0 + n, dtype=torch.int64, device=self.device)
        ops.bank_write(self.memory_features, self.memory_locations, self.memory_metadata,
                       self._inv_norm, feats[:n].contiguous(), slot_t,
                       self.current_location.to(device=self.device, dtype=torch.float32).contiguous(),
                       time.time())
        self.memory_count = s0 + n
        if tags is not None:
            self._stamp_tags(np.arange(s0, s0 + n, dtype=np.int64), tags[:n])
        self._after_write(slot_t, slot_t, np.arange(s0, s0 + n, dtype=np.int64), s0, n, meta_v0)
        self._slot_time[s0:s0 + n] = time.time()
        self._implicit_ids.append((s0, s0 + n, id_prefix, first_index))
        if rebuild and self.use_centroid_index and self.memory_count > self.centroids_k:
            self.rebuild_centroids()
        return n

    def create_episodic_memory(self, memory_id: str, event_id: str, features: torch.Tensor,
                               associated_experts: List[str] = None,
                               merge_similarity=_INSTANCE_DEFAULT, tag: Optional[int] = None,
                               merge_within_tags=_INSTANCE_DEFAULT,
                               merge_blend=_INSTANCE_DEFAULT) -> Optional[ConsolidationReport]:
        """Store one memory (reference ``:195-243``).  ``event_id`` / ``associated_experts`` are
        accepted and unused, as in the reference.  ``merge_similarity``, ``tag``, ``merge_within_tags`` and
        ``merge_blend``: as ``create_episodic_memories``."""
        return self.create_episodic_memories([memory_id], self._features_to_device(features, rows=1),
                                             merge_similarity=merge_similarity, tags=tag,
                                             merge_within_tags=merge_within_tags, merge_blend=merge_blend)

    def create_episodic_memories(self, memory_ids: Sequence[str], features: torch.Tensor,
                                 merge_similarity=_INSTANCE_DEFAULT, tags=None,
                                 merge_within_tags=_INSTANCE_DEFAULT,
                                 merge_blend=_INSTANCE_DEFAULT) -> Optional[ConsolidationReport]:
        """Batched one-shot write: identical to calling ``create_episodic_memory`` once per row,
        including the rebuild every ``centroids_update_interval`` inserts (``:242-243``).

        ``merge_similarity`` (default: the value the bank was constructed with; None there: off, nothing changes,
        nothing more is launched and the call returns None): a consolidating write.  A row whose cosine to a held
        memory, or to an earlier row of the batch that is stored, reaches the threshold (in ``(0, 1]``) is NOT stored
        and its id is not registered; the held memory it repeats is reinforced by ``self.merge_reinforce`` up to
        ``self.merge_cap`` and its timestamp refreshed (an in-batch leader has just been written at full strength).
        The batch is cut into chunks of at most ``ops.CONSOLIDATE_MAX_BATCH`` rows; per chunk: ``find_repeats`` (one
        host read), then ``reinforce`` + ``touch`` of the distinct stored targets -- BEFORE the write, so that under
        ``overflow='weakest'`` a memory that has just been repeated is not the one evicted -- then the kept rows go
        through the unchanged write path (every overflow policy applies; the rebuild cadence counts kept rows only).
        Returns a ``ConsolidationReport``.  Without ``merge_blend`` the first observation stands: the repeat's features
        are not blended into the stored row.  ``bulk_write`` and ``write_at`` (the seeding path and the sharded bank's
        building block) do not consolidate, and ``ShardedHippocampus`` has no cross-rank search.

        ``merge_blend`` (default: the value the bank was constructed with; None there: off, nothing more is launched):
        a rate ``beta`` in ``(0, 1]``; needs a merge threshold (``ValueError`` without one).  A memory that rows of a
        chunk repeat moves toward them: ``g = g + beta * (f_i - g)`` over its repeats in ascending batch order, in fp32
        (the rule: ``include/aura_hip.h``, "Blending merges"); an in-batch leader is blended the same way before it is
        stored.  Per chunk the order is search (the one host read), blend (one launch, ``ops.bank_blend``, grouping on
        the device: no further read), reinforce, touch, write: the kept rows written are the blended ones, and the
        caller's tensor is never written.  The launch keeps ``1/||row||``, the bf16 shadow with its residuals and the
        list-sorted image of every moved row current.  All decisions of a chunk are those the search made against the
        bank as it stood BEFORE the chunk's blend: a blended memory that drifts within the threshold of another held
        memory merges with it only at the next ``consolidate()``.  Strength, timestamp, tag, ids and the stored
        centroid id are untouched by the blend; the centroid means follow at the next ``rebuild_centroids``, as after
        ``forget``.

        ``tags`` (default None: nothing changes and nothing more is launched): an int for every row, or a host
        sequence / int array of one int per row, each in ``[0, 2^24)``.  The rows go through the unchanged write path
        (which leaves 0, "untagged", in metadata column 3); one more launch then stamps the column
        (``ops.bank_set_tags``).  Where a run writes a slot more than once (a full bank under ``overflow='reference'``
        rewrites slot 0), the row that finally owns the slot stamps it.  An untagged write over a tagged slot leaves it
        untagged.

        ``merge_within_tags`` (default: the value the bank was constructed with, False there): consolidation within
        tags.  Off, ``tags`` together with a consolidating write raises ``ValueError``: the plain ``find_repeats`` is
        scope-blind, and a near-copy from one scope must not vanish into a memory of another.  On, the two go together:
        a row repeats only a held memory, or a stored earlier row of the batch, that carries ITS tag
        (``find_repeats(tags=...)``, ``aura_bank_find_repeats`` by tag); rows without a tag are tag 0 and merge only
        into untagged memories.  Per chunk the order stays reinforce, touch, write, and the kept rows are written WITH
        their tags before the next chunk searches."""
        tau = self.merge_similarity if merge_similarity is _INSTANCE_DEFAULT else merge_similarity
        within = self.merge_within_tags if merge_within_tags is _INSTANCE_DEFAULT else bool(merge_within_tags)
        if tau is not None:
            self._check_merge(tau, self.merge_reinforce, self.merge_cap)
        if merge_blend is _INSTANCE_DEFAULT:
            beta = self.merge_blend if tau is not None else None      # (a write with merging switched off blends nothing)
        else:
            beta = merge_blend
            self._check_blend(beta, tau)
        feats = self._features_to_device(features)
        n = len(memory_ids)
        if feats.shape[0] != n:
            raise ValueError(f"{n} ids but {feats.shape[0]} feature rows")
        tags = self._check_tags(tags, n)
        if tags is not None and tau is not None and not within:
            raise ValueError("tags cannot go with merge_similarity: a consolidating write searches the whole bank, so a "
                             "near-copy from one scope would merge into a memory of another (write tagged rows with "
                             "merge_similarity=None, or consolidate within tags with merge_within_tags=True)")
        if tau is None:
            self._write_batch(memory_ids, feats, tags)
            return None
        kw = {} if beta is None else dict(blend=float(beta))
        if not within:
            return self._write_consolidated(memory_ids, feats, float(tau), **kw)
        return self._write_consolidated(memory_ids, feats, float(tau), tags=tags, within_tags=True, **kw)

    def _write_batch(self, memory_ids: Sequence[str], feats: torch.Tensor, tags: Optional[np.ndarray] = None) -> None:
        n = len(memory_ids)
        i = 0
        plan_tags = None
        if self._tag_quota_map or self._tag_quota_default is not None:
            # rows without a tag are tag 0, which is limited only when it is named
            plan_tags = tags if tags is not None else (np.zeros(n, dtype=np.int32) if 0 in self._tag_quota_map else None)
        while i < n:
            # run length until the next insert that triggers a rebuild
            run = n - i
            if self._overflow == 'weakest':
                # a run evicts at most the rows held before it: run - room <= count, that is run <= max_memories
                run = min(run, self.max_memories)
            if self.use_centroid_index:
                interval = max(1, int(self.centroids_update_interval))
                if self.memory_count < self.max_memories:
                    to_boundary = interval - (self.memory_count % interval)
                    run = min(run, to_boundary, self.max_memories - self.memory_count)
                elif self.memory_count % interval == 0 and self.memory_count > self.centroids_k:
                    run = 1   # full bank whose size divides the interval: rebuild after every write
            if plan_tags is not None:
                run = self._quota_run(plan_tags[i:i + run])   # at most q(t) rows of a limited tag per run
                self._write_rows(memory_ids[i:i + run], feats[i:i + run], time.time(),
                                 tags=None if tags is None else tags[i:i + run], plan_tags=plan_tags[i:i + run])
            elif tags is None:
                self._write_rows(memory_ids[i:i + run], feats[i:i + run], time.time())
            else:
                self._write_rows(memory_ids[i:i + run], feats[i:i + run], time.time(), tags=tags[i:i + run])
            i += run
            if (self.use_centroid_index and self.memory_count % self.centroids_update_interval == 0
                    and self.memory_count > self.centroids_k):
                self.rebuild_centroids()

    # ------------------------------------------------------------------ consolidating writes
    @staticmethod
    def _check_merge(similarity, reinforce, cap) -> None:
        if similarity is not None:
            try:
                ok = 0.0 < float(similarity) <= 1.0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"merge_similarity must be None or in (0, 1], got {similarity!r}")
        if not (float(reinforce) >= 0.0):
            raise ValueError(f"merge_reinforce must be >= 0, got {reinforce!r}")
        if float(cap) != float(cap):
            raise ValueError("merge_cap must be a number")

    @staticmethod
    def _check_blend(beta, similarity) -> None:
        if beta is None:
            return
        try:
            ok = not isinstance(beta, bool) and 0.0 < float(beta) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"merge_blend must be None or a rate in (0, 1], got {beta!r}")
        if similarity is None:
            raise ValueError("merge_blend needs a merge threshold: blending moves a memory toward the rows that "
                             "merge_similarity decides repeat it")

    def find_repeats(self, features: torch.Tensor, threshold: float, now: Optional[float] = None, *,
                     tags=None, _use_lists: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Which of the (at most ``ops.CONSOLIDATE_MAX_BATCH``) rows ``features`` repeat a held memory or an earlier
        row of the batch at cosine >= ``threshold``: ``(stored_target int32 [n], batch_leader int32 [n], cos fp32
        [n])`` as HOST tensors (the rule: ``include/aura_hip.h``, ``aura_bank_find_repeats``).  Read-only: nothing is
        written to the bank.  The search covers every held row exactly, whether or not the centroid index is on; it
        scans the list-sorted bf16 shadow in candidate mode, the row-ordered shadow otherwise, and the fp32 bank where
        no shadow applies.  One device-to-host read brings the results, the scan's overflow flag and the inverted
        lists' "a row was dropped" flag: stale lists are re-packed and the call repeated once (a dropped row must
        never become a missed duplicate), an overflowing survivor list repeats the call on the fp32 scan.  ``now`` is
        accepted for symmetry with ``recall_batch``; a cosine has no time term.

        ``tags`` (default None: the scope-blind search, exactly as it was): one int for every row, a host sequence of
        one int per row, or an int32 tensor [n] (used where it lives if it is on the bank's device).  The search then
        stays within tags (``ops.find_repeats_scoped``): a held row is a candidate for row i only if it carries
        ``tags[i]``, an earlier row of the batch only if it carries the same tag; 0 is the scope of the untagged rows
        and a tag outside ``[0, 2^24)`` matches nothing.  The same three scans and the same fallbacks; rows of other
        tags never enter a survivor list, so other scopes' near-copies cannot overflow one."""
        if threshold is None:
            raise ValueError("find_repeats needs a threshold in (0, 1]")
        self._check_merge(threshold, 0.0, 1.0)
        packed, _ = self._find_repeats_packed(features, threshold, tags, _use_lists)
        n = (packed.numel() - 2) // 3
        return packed[:n], packed[n:2 * n], packed[2 * n:3 * n].view(torch.float32)

    def _find_repeats_packed(self, features, threshold: float, tags, _use_lists: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        """``find_repeats``' search: ``(packed on the host, the same int32 [3 n + 2] where the library left it)`` --
        stored targets, leaders, cosine bits, the two flags (``ops.find_repeats``).  The device copy is what a blend
        groups by (``ops.bank_blend``)."""
        f = self._features_to_device(features)
        n = f.shape[0]
        if n > ops.CONSOLIDATE_MAX_BATCH:
            raise ValueError(f"find_repeats takes at most {ops.CONSOLIDATE_MAX_BATCH} rows per call, got {n}")
        t_dev = None if tags is None else self._search_tags(tags, n)
        if self.memory_count:
            self._ensure_norms()
        # an image must hold EVERY held row: the inverted lists do unless rows without a list may exist
        # (``_use_lists=False``: ``consolidate``, whose held set is a prefix of the bank that the lists do not describe)
        mode = 'lists' if (_use_lists and self._candidate_mode() and self.centroids.shape[0] == 256 and
                           not self._unlisted_rows) else 'shadow'
        repacked = False
        while True:                                    # lists -> lists (re-packed) -> shadow -> fp32: at most 4 rounds
            kw, ivf = {}, None
            if mode == 'lists':
                ivf = self._ensure_ivf()
                if ivf is None:
                    mode = 'shadow'
                else:
                    kw = dict(image=ivf.sorted_bf16, image_rows=ivf.sorted_rows, n_image=ivf.n_sorted, rho=self._rho,
                              rho16=self._rho16, lists_flag=ivf.flag)
            if mode == 'shadow':
                shadow = self._ensure_shadow()
                if shadow is None:
                    mode = 'fp32'
                else:
                    kw = dict(image=shadow, rho=self._rho)
            if t_dev is None:
                packed_dev = ops.find_repeats(self.memory_features, self._inv_norm, self.memory_count, f,
                                              float(threshold), **kw)[3]
            else:
                packed_dev = ops.find_repeats_scoped(self.memory_features, self._inv_norm, self.memory_metadata,
                                                     self.memory_count, f, t_dev, float(threshold), **kw)[3]
            packed = packed_dev.cpu()                  # THE host read
            overflow, stale = int(packed[3 * n]), int(packed[3 * n + 1])
            if ivf is not None and stale:
                ivf.valid = False                      # a write outgrew a list's slack: re-pack and once more;
                mode = 'shadow' if repacked else 'lists'                  # stale again: the row-ordered shadow
                repacked = True
                continue
            if overflow and mode != 'fp32':
                mode = 'fp32'                          # a survivor list overflowed: the dense scan cannot
                continue
            break
        return packed, packed_dev

    def _blend_groups(self, packed_dev: torch.Tensor, stored: np.ndarray, leader: np.ndarray, beta: float,
                      feats: Optional[torch.Tensor] = None, row0: int = -1) -> Tuple[Optional[torch.Tensor], int]:
        """One blend launch for the batch a search has just decided (``packed_dev``: its device result; ``stored`` /
        ``leader``: the host copies, only counted here).  ``row0 < 0``: the batch is ``feats``; returns the batch as it
        will be stored -- a copy with the blended leaders, ``feats`` itself where no in-batch leader has a repeat -- and
        the number of memories that moved.  ``row0 >= 0``: the batch is bank rows ``[row0, row0 + n)``, blended in
        place.  The derived state the launch keeps current: 1/||row||, the row-ordered shadow below its watermark, the
        list-sorted image while it is valid, rho; the cached score constants are dropped (rho changed)."""
        n = stored.size
        in_batch = (stored < 0) & (leader >= 0)
        n_keys = int(np.unique(stored[stored >= 0]).size + np.unique(leader[in_batch]).size)
        if n_keys == 0:
            return feats, 0
        out = None
        if row0 < 0:
            # the caller's tensor is never written: blended leaders go into a copy (needed only when there are any;
            # the op wants a distinct buffer either way, and a chunk is a few MB at most)
            out = feats.clone()
        kw = {}
        if self._shadow_travels():
            kw.update(shadow=self._shadow, shadow_upto=self._shadow_valid_upto)
        st = self._ivf
        if row0 < 0 and st is not None and st.valid and self._rho is not None and \
                st.sorted_bf16.device == self.memory_features.device:
            kw.update(sorted_bf16=st.sorted_bf16, sorted_rows=st.sorted_rows, pos_of_row=st.pos_of_row,
                      n_sorted=st.n_sorted, rho16=self._rho16)
        if kw:
            kw["rho"] = self._rho
        ops.bank_blend(self.memory_features, self._inv_norm, self.memory_count, packed_dev[:n], packed_dev[n:2 * n],
                       beta, feats=feats if row0 < 0 else None, out=out, feats_row0=row0, **kw)
        if st is not None:
            st.rowc_live = False
        return (out if bool(in_batch.any()) else feats), n_keys

    def _search_tags(self, tags, n: int) -> torch.Tensor:
        """``find_repeats(tags=...)`` as int32 [n] on the bank's device.  Nothing is refused for its value: a tag
        outside ``[0, 2^24)`` matches nothing (host values are clipped to -1 / 2^24 so that they fit int32)."""
        if isinstance(tags, torch.Tensor):
            if tags.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
                raise ValueError(f"tags must be integers, got dtype {tags.dtype}")
            t = tags.detach().reshape(-1)
            if t.dtype != torch.int32:
                t = t.clamp(-1, TAG_LIMIT).to(torch.int32)
            t = t.to(self.memory_features.device).contiguous()
            if t.numel() == 1 and n != 1:
                t = t.expand(n).contiguous()
        else:
            a = np.asarray(tags)
            if a.dtype.kind not in "iu":
                raise ValueError(f"tags must be integers, got dtype {a.dtype}")
            a = np.clip(a.astype(np.int64), -1, TAG_LIMIT).astype(np.int32).reshape(-1)
            if a.size == 1 and n != 1:
                a = np.full(n, a[0], dtype=np.int32)
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self.memory_features.device)
        if t.numel() != n:
            raise ValueError(f"{t.numel()} tags for {n} rows")
        return t

    def touch(self, rows, now: Optional[float] = None) -> None:
        """Refresh the timestamp of the memories at bank rows ``rows`` (int, any shape; ``-1`` and rows outside the
        bank are ignored) to ``now`` (default: the clock), as a write would."""
        if self.memory_count == 0:
            return
        now = time.time() if now is None else now
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(np.asarray(rows))
        if rows.numel() == 0:
            return
        host = rows.detach().cpu().reshape(-1).numpy().astype(np.int64)
        ops.bank_touch(self.memory_metadata, self.memory_count,
                       rows.to(device=self.device, dtype=torch.int32).contiguous(), now)
        host = host[(host >= 0) & (host < self.memory_count)]
        self._slot_time[host] = now
        if self._ivf is not None:
            self._ivf.rowc_live = False                 # timestamps changed under the cached score constants

    def _write_consolidated(self, memory_ids: Sequence[str], feats: torch.Tensor, tau: float,
                            tags: Optional[np.ndarray] = None, within_tags: bool = False,
                            blend: Optional[float] = None) -> ConsolidationReport:
        """``within_tags``: every chunk is searched with its rows' tags (``tags`` int32 [n], checked; None: all 0,
        "untagged") and its kept rows are written with them.  ``blend``: the rate of a blending write (None: off, the
        launches of a plain consolidating write); the blend follows whatever the search decided, tags included."""
        n = len(memory_ids)
        n_blended = 0
        merged = torch.zeros(n, dtype=torch.bool)
        mem_ids: List[Optional[str]] = [None] * n       # the memory every row became
        slot = np.full(n, -1, dtype=np.int64)           # where that memory was when its chunk was done
        step = ops.CONSOLIDATE_MAX_BATCH
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            f = feats[lo:hi]
            now = time.time()
            packed_dev = None
            if blend is not None:
                chunk_tags = None if not within_tags else (0 if tags is None else tags[lo:hi])
                packed, packed_dev = self._find_repeats_packed(f, tau, chunk_tags, True)
                stored, leader = packed[:hi - lo], packed[hi - lo:2 * (hi - lo)]
            elif within_tags:
                stored, leader, _ = self.find_repeats(f, tau, now=now, tags=0 if tags is None else tags[lo:hi])
            else:
                stored, leader, _ = self.find_repeats(f, tau, now=now)
            stored, leader = stored.numpy().astype(np.int64), leader.numpy().astype(np.int64)
            kept = np.nonzero((stored < 0) & (leader < 0))[0]
            if packed_dev is not None:                                   # blend BEFORE reinforce, touch and the write:
                f, moved = self._blend_groups(packed_dev, stored, leader, blend, feats=f)   # f: the rows as stored
                n_blended += moved
            for i in np.nonzero(stored >= 0)[0].tolist():               # ids of the targets as they are held NOW
                mem_ids[lo + i], slot[lo + i] = self.id_of_row(int(stored[i])), stored[i]
            targets = np.unique(stored[stored >= 0])
            if targets.size:
                t = torch.from_numpy(targets)
                self.reinforce(t, amount=self.merge_reinforce, cap=self.merge_cap)
                self.touch(t, now=now)
            if kept.size:
                kept_ids = [memory_ids[lo + i] for i in kept.tolist()]
                kept_f = f if kept.size == hi - lo else f[torch.from_numpy(kept).to(f.device)].contiguous()
                if tags is None:
                    self._write_batch(kept_ids, kept_f)
                else:
                    self._write_batch(kept_ids, kept_f, tags[lo:hi][kept])
                for i, mid in zip(kept.tolist(), kept_ids):
                    mem_ids[lo + i], slot[lo + i] = mid, self.id_to_idx[mid]
            for i in np.nonzero((stored < 0) & (leader >= 0))[0].tolist():
                j = lo + int(leader[i])
                mem_ids[lo + i], slot[lo + i] = mem_ids[j], slot[j]
            merged[lo:hi] = torch.from_numpy((stored >= 0) | (leader >= 0))
        # a memory this same call overwrote again (a full bank) is reported at -1
        live = np.fromiter((s >= 0 and self.id_of_row(int(s)) == m for s, m in zip(slot.tolist(), mem_ids)),
                           dtype=bool, count=n)
        rows = torch.from_numpy(np.where(live, slot, -1))
        n_merged = int(merged.sum())
        return ConsolidationReport(merged=merged, rows=rows, ids=mem_ids, n_stored=n - n_merged, n_merged=n_merged,
                                   n_blended=n_blended)

    # ------------------------------------------------------------------ forgetting, pruning, consolidating held rows
    def _ring_start(self) -> int:
        """Row of the oldest memory of a wrapped ring, 0 where plain row order is the age order."""
        M = self.max_memories
        if self._overflow in ('fifo', 'weakest') and self.memory_count == M:
            return self._write_cursor % M
        return 0

    def _shadow_travels(self) -> bool:
        return self._shadow is not None and self._rho is not None and self._shadow.device == self.memory_features.device

    def _move_rows(self, src: np.ndarray, dst0: int) -> None:
        """Rows ``src`` (ascending) of the bank's row arrays -> rows ``dst0 ..`` (``ops.bank_compact``); the bf16
        shadow and rho travel when they exist."""
        sh = self._shadow_travels()
        ops.bank_compact(self.memory_features, self.memory_locations, self.memory_metadata, self._inv_norm, src, dst0,
                         shadow=self._shadow if sh else None, rho=self._rho if sh else None)

    def _compact(self, kill: np.ndarray) -> np.ndarray:
        """Take the rows ``kill`` (host int64, ascending, distinct, inside the bank) out: the survivors move to rows
        0 .. in ring order, oldest first.  Returns ``old_to_new``."""
        count = self.memory_count
        self._ensure_norms()
        keep = np.ones(count, dtype=bool)
        keep[kill] = False
        gone = None
        if kill.size:                                   # the centroid ids of the rows that leave, before anything moves
            gone = self.memory_metadata[torch.from_numpy(kill).to(self.device), 2]
        full = self._shadow_travels() and self._shadow_valid_upto >= count
        start = self._ring_start()
        if start == 0:
            order = np.nonzero(keep)[0]
            self._move_rows(order, 0)
            shadow_upto = order.size if full else int(keep[:min(self._shadow_valid_upto, count)].sum())
        else:
            # a wrapped ring: the survivors of [start, M) come first.  Those of [0, start) are staged (a temporary
            # of at most `start` rows), the tail moves down in place, the staged head is copied in behind it.
            head = np.nonzero(keep[:start])[0]
            tail = start + np.nonzero(keep[start:])[0]
            arrays = [self.memory_features, self.memory_locations, self.memory_metadata, self._inv_norm]
            if self._shadow_travels():
                arrays += [self._shadow, self._rho]
            head_t = torch.from_numpy(head).to(self.device)
            staged = [a.index_select(0, head_t) for a in arrays] if head.size else []
            self._move_rows(tail, 0)
            for a, t in zip(arrays, staged):
                a[tail.size:tail.size + head.size].copy_(t)
            order = np.concatenate([tail, head])
            shadow_upto = order.size if full else 0
        self._finish_compaction(order, count, gone, shadow_upto)
        old_to_new = np.full(count, -1, dtype=np.int64)
        old_to_new[order] = np.arange(order.size, dtype=np.int64)
        return old_to_new

    def _finish_compaction(self, order: np.ndarray, count: int, gone: Optional[torch.Tensor], shadow_upto: int) -> None:
        """New row i holds what row ``order[i]`` of the ``count`` rows held before: clear the freed tail, bring the
        derived state and the host maps in line.  ``gone``: the centroid ids (metadata column 2) of the rows that left."""
        k = int(order.size)
        if self._tag_origin and count:
            # a tie origin becomes the number of survivors that come before it in ring order (``order`` is in ring
            # order from the ring's start, so the survivors' ring positions ascend)
            start = self._ring_start()
            pos = (order - start) % count
            self._tag_origin = {t: int(np.searchsorted(pos, (c % count - start) % count, side='left'))
                                for t, c in self._tag_origin.items()}
        for a in (self.memory_features, self.memory_locations, self.memory_metadata):
            a[k:count].zero_()                          # what was forgotten does not stay in the state_dict
        if gone is not None and gone.numel():
            ck = self.centroid_counts.shape[0]
            cid = gone[(gone >= 0) & (gone < ck)].long()
            self.centroid_counts.sub_(torch.bincount(cid, minlength=ck).to(self.centroid_counts.dtype)).clamp_(min=0)
        self.memory_count, self._write_cursor = k, 0
        self._norms_valid_upto = k
        self._shadow_valid_upto = min(shadow_upto, k)
        self._invalidate_lists()
        # host maps
        inv = np.full(count, -1, dtype=np.int64)
        inv[order] = np.arange(k, dtype=np.int64)
        times = self._slot_time[order].copy()
        self._slot_time[:count] = 0.0
        self._slot_time[:k] = times
        held = np.empty(count, dtype=object)
        held[:] = self._idx_to_id[:count]
        self._idx_to_id[:count] = held[order].tolist() + [None] * (count - k)
        self.id_to_idx = {mid: int(inv[slot]) for mid, slot in self.id_to_idx.items() if slot < count and inv[slot] >= 0}
        implicit = []
        for s0, s1, prefix, n0 in self._implicit_ids:
            s1 = min(s1, count)
            if s1 <= s0:
                continue
            new_rows = inv[s0:s1]
            alive = new_rows >= 0
            if not alive.any():
                continue
            orig = (n0 + np.arange(s1 - s0, dtype=np.int64)) if isinstance(n0, int) else n0[:s1 - s0]
            new_rows, orig = new_rows[alive], orig[alive]
            # the survivors of a range stay together; a rotated ring cuts a range in two at most
            cuts = (np.nonzero(np.diff(new_rows) != 1)[0] + 1).tolist()
            for a, b in zip([0] + cuts, cuts + [new_rows.size]):
                r0, o = int(new_rows[a]), orig[a:b]
                whole = int(o[-1] - o[0]) == b - a - 1            # (indices ascend: nothing was taken out in between)
                implicit.append((r0, r0 + b - a, prefix, int(o[0]) if whole else o.copy()))
        self._implicit_ids = implicit

    def forget(self, rows=None, ids: Optional[Sequence[str]] = None, tags=None) -> CompactionReport:
        """Take memories out of the bank.  ``rows``: bank rows (int tensor or array of any shape; ``-1``, rows outside
        the bank and duplicates are ignored); ``ids``: explicit memory ids as found in ``id_to_idx`` (an unknown id
        raises ``KeyError`` before anything changes; bulk rows with implicit ids are forgotten by row); ``tags``: an int
        or a sequence of ints -- every held memory that carries one of these tags goes ("forget this session"; 0
        forgets the untagged rows), at the price of one device-to-host read of the tag column.

        The survivors are moved to rows ``0 .. count' - 1`` in place by one kernel (``aura_bank_compact``: features,
        locations, metadata, the cached 1/||row||, and the bf16 shadow with its residuals when they exist -- nothing
        is converted again), in ring order, oldest first: plain row order for a bank that never wrapped, starting at
        ``cursor % max_memories`` for a full bank under ``'fifo'`` / ``'weakest'``.  ``memory_count`` becomes the
        number of survivors and the write cursor 0: later writes append, and once the bank is full again they
        overwrite the oldest first.  The freed tail of features, locations and metadata is zeroed.  The inverted lists
        are rebuilt by the next recall that needs them; ``centroid_counts`` lose the removed rows' counts, the
        centroid MEANS stay as they are (the next ``rebuild_centroids`` recomputes them).  ``id_to_idx``,
        ``episodic_memories`` and ``id_of_row`` follow; forgotten ids disappear.  An empty kill set launches nothing
        and changes nothing.  One host copy of ``rows`` if it lives on the device; nothing else is read back.
        Not available through ``ShardedHippocampus`` (its global rows would shift)."""
        count = self.memory_count
        kill: List[np.ndarray] = []
        if rows is not None:
            r = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
            r = r.reshape(-1).astype(np.int64)
            kill.append(r[(r >= 0) & (r < count)])
        stale = []
        if ids is not None:
            slots = [self.id_to_idx[mid] for mid in ids]            # KeyError: nothing has changed yet
            for mid, slot in zip(ids, slots):
                if slot < count and self._idx_to_id[slot] == mid:
                    kill.append(np.array([slot], dtype=np.int64))
                else:
                    stale.append(mid)                               # its row was overwritten long ago: the id just goes
        for mid in stale:
            self.id_to_idx.pop(mid, None)
        if tags is not None and count:
            t = (tags.detach().cpu().numpy() if isinstance(tags, torch.Tensor) else np.asarray(tags)).reshape(-1)
            want = np.unique(self._check_tags(t, t.size)) if t.size else t
            if want.size:
                held = self.memory_metadata[:count, 3].cpu().numpy().astype(np.int64)    # THE host read
                kill.append(np.nonzero(np.isin(held, want))[0].astype(np.int64))
        k = np.unique(np.concatenate(kill)) if kill else np.zeros(0, dtype=np.int64)
        if k.size == 0:
            return CompactionReport(0, np.arange(count, dtype=np.int64))
        return CompactionReport(int(k.size), self._compact(k))

    def prune(self, min_strength: Optional[float] = None, min_key: Optional[float] = None,
              now: Optional[float] = None) -> CompactionReport:
        """Forget the memories whose strength is below ``min_strength`` or whose ``retention_keys(now)`` (strength
        times ``exp(-age / 3600)``, what ``overflow='weakest'`` evicts by) is below ``min_key`` -- the pruning the
        reference's ``decay_memories`` leaves unfinished (``:336-339``: a free list for weak memories, then ``pass``).
        One comparison on the device and one host read of the rows that go; then ``forget``."""
        if min_strength is None and min_key is None:
            raise ValueError("prune needs min_strength or min_key")
        count = self.memory_count
        if count == 0:
            return CompactionReport(0, np.zeros(0, dtype=np.int64))
        weak = torch.zeros(count, dtype=torch.bool, device=self.memory_metadata.device)
        if min_strength is not None:
            weak |= self.memory_metadata[:count, 0] < float(min_strength)
        if min_key is not None:
            weak |= self.retention_keys(now) < float(min_key)
        return self.forget(rows=torch.nonzero(weak).flatten())

    def consolidate(self, similarity: Optional[float] = None, rebuild: bool = True,
                    within_tags: Optional[bool] = None, blend: Optional[float] = None) -> BankConsolidationReport:
        """Merge the near-copies the bank already holds (rows from ``bulk_write``, ``write_at``, a checkpoint, or
        written before ``merge_similarity`` was set).  The rule: the bank becomes what writing its rows, oldest first,
        into an empty bank with ``create_episodic_memories(merge_similarity=similarity)`` in chunks of
        ``ops.CONSOLIDATE_MAX_BATCH`` would have left -- every row is kept unless its cosine to a row kept before it
        reaches ``similarity`` (default ``self.merge_similarity``; both None: ``ValueError``); rows with a NaN / Inf
        component or of norm 0 are kept.

        In place: a wrapped ring is first put in age order (``forget``'s move with nothing to forget); then, slab by
        slab of 1024 rows, ``find_repeats`` decides the slab (a view of the bank) against the decided prefix -- the
        row-ordered bf16 shadow when it applies, the dense fp32 scan below ``SHADOW_MIN_ROWS`` rows or where no shadow
        is kept; the centroid index is not consulted -- and ``aura_bank_compact`` moves the slab's kept rows down behind
        the prefix.  One host read per slab, as in the write path.  A kept memory takes the largest strength and the
        latest timestamp among itself and the rows merged into it; the distinct STORED targets of a slab are then
        reinforced once by ``merge_reinforce`` up to ``merge_cap``, as a consolidating write does per chunk.  Without
        ``blend`` the kept row's features stand.  With ``rebuild`` the pass ends in ``rebuild_centroids()`` when the
        index is in use and more than ``centroids_k`` rows remain; otherwise the inverted lists are invalidated and
        ``centroid_counts`` corrected as ``forget`` does (the centroid means stay).  If a slab fails, the undecided
        remainder is moved down unchanged and the host maps are committed before the error is raised again: the bank
        stays consistent and nothing undecided is lost.

        ``within_tags`` (None: ``self.merge_within_tags``, False unless the bank was built otherwise).  Off, the pass is
        scope-blind: tags play no part, near-copies merge across tags and the kept (older) row keeps its own tag.  On,
        every slab is searched with the slab rows' own tags -- taken on the device from ``memory_metadata[lo:hi, 3]``,
        nothing more is read back -- so a row merges only into a kept row of ITS tag (0, "untagged", is a scope like any
        other): the bank becomes what writing its rows oldest first, each with its tag, through
        ``create_episodic_memories(..., tags=..., merge_within_tags=True)`` would have left.  Every kept row keeps its
        own tag; strength and timestamp take the maximum as above.

        ``blend`` (None: ``self.merge_blend``, off unless the bank was built otherwise): a rate in ``(0, 1]``.  Per slab,
        after the search and before the metadata maxima, the reinforcement and the move, one launch
        (``ops.bank_blend`` on the slab in place) moves every kept memory toward the slab rows that repeat it,
        ``g = g + beta * (f_i - g)`` in ascending row order (the rule: ``include/aura_hip.h``, "Blending merges").  The
        equivalence above keeps holding, bit for bit in the features: the bank becomes what writing its rows oldest
        first through BLENDED consolidating writes in chunks of 1024 would have left.  As there, a slab's decisions are
        those made before its blend, and a memory that drifts within ``similarity`` of another kept memory merges only
        at the next ``consolidate()``."""
        tau = self.merge_similarity if similarity is None else similarity
        within = self.merge_within_tags if within_tags is None else bool(within_tags)
        if tau is None:
            raise ValueError("consolidate needs a similarity in (0, 1] (none given and the bank has no merge_similarity)")
        self._check_merge(tau, self.merge_reinforce, self.merge_cap)
        tau = float(tau)
        beta = self.merge_blend if blend is None else blend
        self._check_blend(beta, tau)
        n_blended = 0
        n_before = self.memory_count
        first = None
        if self._ring_start():
            first = self._compact(np.zeros(0, dtype=np.int64))
        count = self.memory_count
        if count == 0:
            return BankConsolidationReport(0, 0, 0, np.zeros(0, dtype=np.int64))
        self._ensure_norms()
        dev = self.device
        full = self._shadow_travels() and self._shadow_valid_upto >= count
        order = np.empty(count, dtype=np.int64)             # order[new row] = the row it came from
        old_to_new = np.full(count, -1, dtype=np.int64)
        gone: List[torch.Tensor] = []                       # centroid ids of the merged rows
        n_kept = lo = 0
        strength, stamp = self.memory_metadata[:, 0], self.memory_metadata[:, 1]
        try:
            while lo < count:
                hi = min(count, lo + ops.CONSOLIDATE_MAX_BATCH)   # a slab: what one find_repeats call decides
                self.memory_count = n_kept                  # the held set of this slab: the decided prefix
                packed_dev = None
                if beta is not None:
                    slab_tags = self.memory_metadata[lo:hi, 3].to(torch.int32) if within else None
                    packed, packed_dev = self._find_repeats_packed(self.memory_features[lo:hi], tau, slab_tags, False)
                    stored, leader = packed[:hi - lo], packed[hi - lo:2 * (hi - lo)]
                elif within:
                    stored, leader, _ = self.find_repeats(self.memory_features[lo:hi], tau, _use_lists=False,
                                                          tags=self.memory_metadata[lo:hi, 3].to(torch.int32))
                else:
                    stored, leader, _ = self.find_repeats(self.memory_features[lo:hi], tau, _use_lists=False)
                stored, leader = stored.numpy().astype(np.int64), leader.numpy().astype(np.int64)
                if packed_dev is not None:                  # the slab in place; held targets lie below it
                    n_blended += self._blend_groups(packed_dev, stored, leader, float(beta), row0=lo)[1]
                kept = (stored < 0) & (leader < 0)
                kept_local = np.nonzero(kept)[0]
                merged_local = np.nonzero(~kept)[0]
                if merged_local.size:
                    # where the memory a merged row repeats is NOW (stored targets are in place, leaders still in the slab)
                    target = np.where(stored >= 0, stored, lo + leader)[merged_local]
                    m_t = torch.from_numpy(lo + merged_local).to(dev)
                    t_t = torch.from_numpy(target).to(dev)
                    strength.scatter_reduce_(0, t_t, strength[m_t], 'amax', include_self=True)
                    stamp.scatter_reduce_(0, t_t, stamp[m_t], 'amax', include_self=True)
                    gone.append(self.memory_metadata[m_t, 2])
                    old_target = np.where(stored >= 0, order[np.maximum(stored, 0)], lo + leader)[merged_local]
                    np.maximum.at(self._slot_time, old_target, self._slot_time[lo + merged_local])
                    targets = np.unique(stored[stored >= 0])
                    if targets.size:
                        self.reinforce(torch.from_numpy(targets), amount=self.merge_reinforce, cap=self.merge_cap)
                self._move_rows(lo + kept_local, n_kept)
                new_of_local = np.full(hi - lo, -1, dtype=np.int64)
                new_of_local[kept_local] = n_kept + np.arange(kept_local.size, dtype=np.int64)
                new_of_local[merged_local] = np.where(stored >= 0, stored, new_of_local[np.maximum(leader, 0)])[merged_local]
                old_to_new[lo:hi] = new_of_local
                order[n_kept:n_kept + kept_local.size] = lo + kept_local
                n_kept += kept_local.size
                if not full:                                # rows arrived that the shadow has not converted
                    self._shadow_valid_upto = min(self._shadow_valid_upto, n_kept - kept_local.size)
                lo = hi
        finally:
            rest = np.arange(lo, count, dtype=np.int64)     # undecided rows (none unless a slab failed): kept as they are
            if rest.size:
                self._move_rows(rest, n_kept)
                old_to_new[rest] = n_kept + np.arange(rest.size, dtype=np.int64)
                order[n_kept:n_kept + rest.size] = rest
            shadow_upto = n_kept + rest.size if full else min(self._shadow_valid_upto, n_kept)
            self.memory_count = count
            self._finish_compaction(order[:n_kept + rest.size], count, torch.cat(gone) if gone else None, shadow_upto)
        if self._ivf is not None:
            self._ivf.rowc_live = False
        if rebuild and self.use_centroid_index and self.memory_count > self.centroids_k:
            self.rebuild_centroids()
        if first is not None:
            old_to_new = old_to_new[first]                  # (putting the ring in order removed nothing)
        return BankConsolidationReport(n_before=n_before, n_kept=n_kept, n_merged=count - n_kept, old_to_new=old_to_new,
                                       n_blended=n_blended)

    # ------------------------------------------------------------------ recall
    def _candidate_mode(self) -> bool:
        return bool(self.use_centroid_index and self._index_ready and self.memory_count > self.centroids_k)

    def recall_batch(self, queries: torch.Tensor, k: int = 5,
                     locations: Optional[torch.Tensor] = None, now: Optional[float] = None,
                     use_candidates: Optional[bool] = None, check_overflow: bool = True,
                     fallback_empty: bool = True,
                     probe_ids: Optional[torch.Tensor] = None, _retry: int = 0,
                     bound_exchange=None, reinforce: Optional[float] = None,
                     reinforce_cap: float = 1.0, diversity: Optional[float] = None,
                     max_similarity: Optional[float] = None,
                     fetch_k: Optional[int] = None, tags=None, newer_than: Optional[float] = None,
                     older_than: Optional[float] = None,
                     min_strength: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Batched recall: ``(scores [nq, k'], rows [nq, k'])`` with ``k' = min(k, count)``;
        rows are bank row indices (int32), ``-1`` where a query has fewer than ``k'`` candidates.

        ``check_overflow`` (default) reads one small tensor back per call (a host sync): the
        prefilter's overflow flag (candidate lists that did not fit: the call is re-run on the fp32
        path, same results) and, in candidate mode, whether some query was left without candidates
        (it then falls back to the full scan, reference ``:269-270``).  Pass False only inside
        latency-critical loops whose data is known to be well behaved.  ``fallback_empty=False``
        leaves such queries at ``-1`` (a shard of a row-sharded bank: the query may have candidates
        on another shard, so the fallback is the caller's decision after the merge).  ``probe_ids``:
        ``probe(queries)`` computed earlier for these queries against the current centroid table (the
        inverted-list path then skips its own probe; other paths ignore it).  ``bound_exchange``
        (``sharded.ShardedHippocampus``): ``(fn, parts)`` -- the inverted-list recall runs in stages per pass of
        at most 8192 queries and ``fn(bounds [n, 2]) -> bound [n]`` combines every shard's bounds in between (a
        collective: it is called exactly ``2 ceil(nq / 8192)`` times -- sampled bounds, then the filtered
        candidates' bounds -- whatever path this bank takes).  ``reinforce``: when given, the rows this call
        returns are reinforced by that amount up to ``reinforce_cap`` (``reinforce()``), once, after the results
        are final; None (default) launches nothing.  ``diversity`` / ``max_similarity`` (both None by default:
        nothing changes and nothing more is launched): diverse recall -- the call fetches the top
        ``F = min(fetch_k or max(32, 4 k'), 128, count)`` rows as above and one kernel picks ``k'`` of them greedily
        (``ops.diverse_select``): a candidate whose cosine to an earlier pick reaches ``max_similarity`` (in
        ``(-1, 1]``) is skipped, the others rank by ``(1 - diversity) * score - diversity * (largest cosine to an
        earlier pick)``, ``diversity`` in ``[0, 1]``.  Rows come back in pick order with their recall scores, ``-1`` /
        ``-inf`` where fewer than ``k'`` were eligible; ``reinforce`` then applies to the rows returned.

        Scoped recall -- ``tags``, ``newer_than``, ``older_than``, ``min_strength`` (all None by default: nothing
        changes and nothing more is launched).  Row ``r`` is in query ``i``'s scope iff ``tags[i] < 0 or
        int(memory_metadata[r, 3]) == tags[i]``, ``memory_metadata[r, 1] >= float32(newer_than)``,
        ``memory_metadata[r, 1] <= float32(older_than)`` and ``memory_metadata[r, 0] >= min_strength`` (a condition
        left at None is not applied).  ``tags``: an int for all queries or one per query (host ints); None or a negative
        entry takes any tag, 0 the untagged rows.  The other three are per-call scalars; the time bounds are compared
        with the fp32 timestamps the bank stores, which are 128 s apart at today's epoch values, so a window is no finer
        than that.  The result is the top ``k'`` of the scope by the same combined score (``locations`` included),
        descending, equal scores to the lower row, padded with ``-inf`` / ``-1`` where the scope has fewer than ``k'``
        rows.  It is always exact over the scope and its cost follows the size of the scope, not of the bank
        (``ops.knn_search_scoped``: a per-call scope build, no index to keep current); the centroid index plays no
        part, so ``use_candidates=True`` with a scope raises ``ValueError``.  ``k'`` may be at most
        ``ops.SCOPED_MAX_K`` = 128.  ``reinforce`` and ``diversity`` / ``max_similarity`` compose: the scope goes to the
        inner plain call.  ``check_overflow`` here reads the scoped call's flag back (one host sync)."""
        scope = dict(tags=tags, newer_than=newer_than, older_than=older_than, min_strength=min_strength)
        scoped = any(v is not None for v in scope.values())
        if scoped:
            if use_candidates:
                raise ValueError("a scoped recall (tags / newer_than / older_than / min_strength) is always exact over "
                                 "its scope and does not use the centroid index: not with use_candidates=True")
            if bound_exchange is not None:
                raise ValueError("a scoped recall is not available with bound_exchange (a shard of a row-sharded bank)")
        if diversity is not None or max_similarity is not None:
            return self._recall_diverse(queries, k, diversity, max_similarity, fetch_k, bound_exchange, reinforce,
                                        reinforce_cap, dict(locations=locations, now=now, use_candidates=use_candidates,
                                                            check_overflow=check_overflow, fallback_empty=fallback_empty,
                                                            probe_ids=probe_ids, _retry=_retry, **scope))
        if reinforce is not None:
            # the plain call (with its own retries and fallbacks) first: the rows are final when it returns
            scores, rows = self.recall_batch(queries, k=k, locations=locations, now=now, use_candidates=use_candidates,
                                             check_overflow=check_overflow, fallback_empty=fallback_empty,
                                             probe_ids=probe_ids, _retry=_retry, bound_exchange=bound_exchange, **scope)
            self.reinforce(rows, amount=reinforce, cap=reinforce_cap)
            return scores, rows
        self._last_flag = None                        # set only by a candidate-mode recall that read its flag
        if self.memory_count == 0:
            self._drain_exchanges(queries.shape[0], bound_exchange)
            z = torch.empty(queries.shape[0], 0, device=self.device)
            return z, z.to(torch.int32)
        q = self._features_to_device(queries)
        self._ensure_norms()
        kk = min(int(k), self.memory_count)
        now = time.time() if now is None else now
        q_loc = self._query_locations(locations, q.shape[0])
        if scoped:
            if kk > ops.SCOPED_MAX_K:
                raise ValueError(f"a scoped recall returns at most ops.SCOPED_MAX_K = {ops.SCOPED_MAX_K} rows per "
                                 f"query, got k = {kk}")
            return ops.knn_search_scoped(self.memory_features, self._inv_norm, self.memory_metadata, q, kk, now,
                                         self.memory_count, loc=self.memory_locations if q_loc is not None else None,
                                         q_loc=q_loc, check_flag=check_overflow, **scope)
        cand = self._candidate_mode() if use_candidates is None else (use_candidates and self._candidate_mode())
        kw = dict(count=self.memory_count, loc=self.memory_locations if q_loc is not None else None,
                  q_loc=q_loc, check_overflow=check_overflow)
        if not cand:
            self._drain_exchanges(q.shape[0], bound_exchange)
            shadow = self._ensure_shadow() if q_loc is None else None
            return ops.knn_search(self.memory_features, self._inv_norm, self.memory_metadata, q, kk, now,
                                  shadow=shadow, rho=self._rho if shadow is not None else None, **kw)
        nprobe = min(8, self.centroids_k)
        full_index = self.centroids.shape[0] == 256
        scores = rows = None
        first = None
        if q_loc is None and full_index:
            first = self._recall_two_stage(q, kk, now, nprobe, probe_ids, check_overflow, bound_exchange)
        if first is None:                             # (with an exchange, a two-stage recall is the staged one)
            self._drain_exchanges(q.shape[0], bound_exchange)
        else:
            scores, rows, read_flag = first
        if check_overflow and scores is not None:
            # ONE host read for both conditions: the library's flag carries the overflow bits of the
            # two-stage lists and the "a query has no candidate at all" bit
            f = read_flag()
            if f & ops.KNN_FLAG_LISTS_STALE:          # a write outgrew a list's slack: re-pack, then once more
                self._ivf.valid = False
                if _retry < 2 and bound_exchange is None:   # (an exchanged recall is never repeated: collectives)
                    return self.recall_batch(queries, k=k, locations=locations, now=now, use_candidates=use_candidates,
                                             check_overflow=check_overflow, fallback_empty=fallback_empty,
                                             probe_ids=probe_ids, _retry=_retry + 1)
                f |= 1                                # a fresh re-pack that is stale again: never loop, use the fp32 lists
            if f & ~ops.KNN_FLAG_NO_CANDIDATES:
                scores = rows = None                  # candidate lists too long: the fp32 paths below
            elif not (f & ops.KNN_FLAG_NO_CANDIDATES) or not fallback_empty:
                self._last_flag = f                   # (sharded.ShardedHippocampus: was any query left without candidates?)
                return scores, rows
        if scores is None:
            scores, rows = self._recall_fp32(q, kk, now, nprobe, q_loc is None and full_index, kw)
        if check_overflow and fallback_empty:
            self._fill_empty_queries(q, q_loc, kk, now, scores, rows, kw)
        return scores, rows

    DIVERSE_MIN_FETCH = 32             # candidates fetched per query unless fetch_k says otherwise: max(32, 4 k)

    def _recall_diverse(self, queries, k: int, diversity, max_similarity, fetch_k, bound_exchange, reinforce,
                        reinforce_cap: float, kw) -> Tuple[torch.Tensor, torch.Tensor]:
        """``recall_batch`` with ``diversity`` / ``max_similarity``: one plain recall of F candidates (its retries and
        fallbacks included, whatever path the bank takes), one selection kernel, then the reinforcement."""
        d = 0.0 if diversity is None else float(diversity)
        if not (0.0 <= d <= 1.0):
            raise ValueError(f"diversity must be in [0, 1], got {diversity}")
        if max_similarity is not None and not (-1.0 < float(max_similarity) <= 1.0):
            raise ValueError(f"max_similarity must be in (-1, 1], got {max_similarity}")
        if bound_exchange is not None:
            raise ValueError("diverse recall needs the candidates' rows on this device: not with bound_exchange "
                             "(a shard of a row-sharded bank)")
        if self.memory_count == 0:
            return self.recall_batch(queries, k=k, **kw)
        kk = min(int(k), self.memory_count)
        F = min(int(fetch_k) if fetch_k else max(self.DIVERSE_MIN_FETCH, 4 * kk), ops.DIVERSE_MAX_CANDIDATES,
                self.memory_count)
        if F < kk:
            raise ValueError(f"diverse recall selects k={kk} rows among F={F} fetched candidates: needs k <= fetch_k <= "
                             f"{ops.DIVERSE_MAX_CANDIDATES}")
        cand_s, cand_r = self.recall_batch(queries, k=F, **kw)
        scores, rows = ops.diverse_select(self.memory_features, self._inv_norm, self.memory_count, cand_r.contiguous(),
                                          cand_s.contiguous(), kk, d, max_similarity)
        if reinforce is not None:
            self.reinforce(rows, amount=reinforce, cap=reinforce_cap)
        return scores, rows

    def _query_locations(self, locations, nq: int) -> Optional[torch.Tensor]:
        if locations is None:
            return None
        if isinstance(locations, np.ndarray):
            locations = torch.from_numpy(locations)
        q_loc = locations.to(device=self.device, dtype=torch.float32).reshape(-1, self.spatial_dims)
        if q_loc.shape[0] == 1 and nq > 1:
            q_loc = q_loc.expand(nq, -1)
        return q_loc.contiguous()

    def _drain_exchanges(self, nq: int, bound_exchange) -> None:
        """This bank does not take the staged path: keep the shards' collectives matched with neutral bounds."""
        if bound_exchange is None:
            return
        step = ops.STAGED_MAX_QUERIES
        for lo in range(0, nq, step):
            for _ in range(2):                        # (sampled bounds, then the candidates' bounds)
                bound_exchange[0](torch.full((min(step, nq - lo), 2), -3.0e38, dtype=torch.float32, device=self.device))

    def _recall_two_stage(self, q, kk: int, now: float, nprobe: int, probe_ids, check_overflow: bool, bound_exchange):
        """Candidate mode on the bf16 two-stage scan: ``(scores, rows, read_flag)`` -- ``read_flag()`` returns the
        call's flag -- or None when neither the probe masks nor the inverted lists apply."""
        masked_ok = (self.memory_count <= self.MASKED_SCAN_MAX_ROWS and q.shape[0] <= self.MASKED_SCAN_MAX_QUERIES and
                     bound_exchange is None)
        shadow = self._ensure_shadow() if masked_ok else None
        if shadow is not None:
            # up to a few hundred thousand rows the candidate restriction is cheapest as probe masks
            # inside the two-stage scan (one pass over the bf16 shadow; 0.15 vs 0.20 ms at 100k x 768,
            # 256 queries); same rows and score bits as the inverted lists
            scores, rows, ovf = ops.knn_search(self.memory_features, self._inv_norm, self.memory_metadata,
                                               q, kk, now, centroids=self.centroids, nprobe=nprobe,
                                               shadow=shadow, rho=self._rho, count=self.memory_count,
                                               check_overflow=False, return_flag=True)
            return scores, rows, ovf.item
        if kk > 256:
            return None
        ivf = self._ensure_ivf()
        if ivf is not None and not check_overflow and ivf.appended > ivf.slack:
            ivf.valid = False                         # nobody will read the lists' flag: stay within the proven slack
            ivf = self._ensure_ivf()
        if ivf is None:
            return None
        # large banks / large batches: inverted lists on the two-stage scan (every probed list is streamed once
        # per 2048 queries from the list-sorted bf16 shadow); same rows and score bits.  The flag arrives through
        # the completion word: polled, not synchronised for.
        lists = self._ivf_lists(ivf, now, nprobe)
        if bound_exchange is None:
            scores, rows, _ = lists.search(q, kk, now, probe_ids=probe_ids, word=ivf.word)
            return scores, rows, ivf.word.wait
        scores, rows, ovf = self._recall_staged(lists, q, kk, now, probe_ids, bound_exchange)
        if check_overflow:
            ivf.word.signal(ovf)                      # (the staged chain ends in an entry point without a word)
        return scores, rows, ivf.word.wait

    def _ivf_lists(self, ivf: _IvfState, now: float, nprobe: int) -> "ops.Ivf2Lists":
        """The validated handle of the current lists (rebuilt only when one of its tensors was replaced)."""
        args = (self.memory_features, self._inv_norm, self.memory_metadata, self.centroids, nprobe, ivf.sorted_bf16,
                self._rho, ivf.sorted_rows, ivf.pad_off, ivf.list_len, ivf.n_sorted, ivf.flag,
                self._ivf_row_constants(ivf, now), self._rho16)
        if ivf.lists is None or not ivf.lists.holds(*args):
            ivf.lists = ops.Ivf2Lists(*args)
        return ivf.lists

    def _recall_staged(self, lists: "ops.Ivf2Lists", q, kk: int, now: float, probe_ids, bound_exchange):
        """Inverted-list recall in passes of at most 8192 queries, each in stages with the shards' bounds combined
        in between (``aura_knn_search_ivf2``, staged): ``(scores, rows, overflow flag)``."""
        fn, parts = bound_exchange
        k2 = max(1, -(-kk // max(int(parts), 1)))
        step = ops.STAGED_MAX_QUERIES
        nq = q.shape[0]
        # results land in ONE pair of tensors (each pass writes its slice); the layout is checked once per handle, not
        # once per pass and call: the staged recall of a sharded bank is host-bound otherwise (eight ranks: 2 passes x
        # 5 Python-level steps per call against ~1.1 ms of kernels)
        out_s = torch.empty(nq, kk, dtype=torch.float32, device=q.device)
        out_i = torch.empty(nq, kk, dtype=torch.int32, device=q.device)
        flag = torch.zeros(1, dtype=torch.int32, device=q.device) if nq == 0 else None
        for lo in range(0, nq, step):
            hi = min(nq, lo + step)
            p = lists.staged(q[lo:hi], kk, now, None if probe_ids is None else probe_ids[lo:hi],
                             out=(out_s[lo:hi], out_i[lo:hi]))
            bound = fn(p.stage1(k2))
            # second exchange, on the FILTERED candidates' bounds: the k-th largest lower bound over the shards'
            # candidates (max over shards of each one's k-th, min over shards of each one's ceil(k / S)-th) is close
            # to the global k-th best score itself, so a shard re-scores ~k / S + gap rows per query instead of
            # k + gap -- the refine is half of a shard's share at 8 shards
            bound2 = fn(p.stage2_bounds(bound, k2))
            _, _, f_ = p.stage3(torch.maximum(bound2, bound))
            if hi - lo == nq:
                return out_s, out_i, f_
            flag = f_.clone() if flag is None else flag.bitwise_or_(f_)   # stage 1 of the next pass resets the flag
        return out_s, out_i, flag

    def _recall_fp32(self, q, kk: int, now: float, nprobe: int, use_lists: bool, kw) -> Tuple[torch.Tensor, torch.Tensor]:
        """Candidate mode on the fp32 paths: the fp32 inverted lists (every probed list is streamed once per batch),
        else the fp32 scan with probe masks."""
        if use_lists:
            list_rows, list_off, list_len, longest = self._ensure_lists()
            cap = ops.ivf_capacity(longest, kk)
            if cap is not None:               # else: lists too long for the two-level select
                scores, rows, _ = ops.knn_search_ivf(self.memory_features, self._inv_norm,
                                                     self.memory_metadata, q, kk, now, self.memory_count,
                                                     self.centroids, nprobe, list_rows, list_off,
                                                     list_len, cap)
                return scores, rows
        return ops.knn_search(self.memory_features, self._inv_norm, self.memory_metadata,
                              q, kk, now, centroids=self.centroids, nprobe=nprobe, **kw)

    def _fill_empty_queries(self, q, q_loc, kk: int, now: float, scores, rows, kw) -> None:
        """A query whose probed centroids own no rows falls back to the full scan (ref :269-270), in place."""
        empty = (rows[:, 0] < 0)
        if bool(empty.any()):
            sel = torch.nonzero(empty).squeeze(-1)
            kw2 = dict(kw)
            if q_loc is not None:
                kw2['q_loc'] = q_loc[sel].contiguous()
            s2, r2 = ops.knn_search(self.memory_features, self._inv_norm, self.memory_metadata,
                                    q[sel].contiguous(), kk, now, **kw2)
            scores[sel], rows[sel] = s2, r2

    def probe(self, queries: torch.Tensor) -> Optional[torch.Tensor]:
        """The centroid probes of ``queries`` ([nq, 8] int32, the 8 nearest of the 256 centroid rows in
        distance order, reference ``:261-262``) for ``recall_batch(..., probe_ids=...)``, or None when the
        index is not in use.  Ranks of a sharded bank share one centroid table, so a query is probed once,
        by the rank that brings it."""
        if not self._candidate_mode() or self.centroids.shape[0] != 256 or not self.memory_features.is_cuda:
            return None
        return ops.centroid_probe(self._features_to_device(queries), self.centroids, min(8, self.centroids_k))

    def retrieve_similar_memories(self, query_features: torch.Tensor,
                                  location: Optional[torch.Tensor] = None,
                                  k: int = 5, *, diversity: Optional[float] = None,
                                  max_similarity: Optional[float] = None,
                                  fetch_k: Optional[int] = None, tags=None, newer_than: Optional[float] = None,
                                  older_than: Optional[float] = None,
                                  min_strength: Optional[float] = None) -> List[Tuple[str, float]]:
        """Top-k ``(memory_id, score)`` for one query (reference ``:245-319``).  The keyword arguments are
        ``recall_batch``'s diverse recall and scoped recall (both off by default; ``tags``: one int)."""
        if self.memory_count == 0:
            return []
        q = self._features_to_device(query_features, rows=1)
        scores, rows = self.recall_batch(q, k=k, locations=location, diversity=diversity,
                                         max_similarity=max_similarity, fetch_k=fetch_k, tags=tags,
                                         newer_than=newer_than, older_than=older_than, min_strength=min_strength)
        out = []
        for s, r in zip(scores[0].tolist(), rows[0].tolist()):
            mid = self.id_of_row(r) if r >= 0 else None
            if mid is not None:
                out.append((mid, s))
        return out

    # ------------------------------------------------------------------ persistence
    def bank_state(self) -> Dict[str, Any]:
        """Host-side state the reference forgets to checkpoint (``memory_count``, index flag, id
        maps live outside its ``state_dict``, so a reloaded bank reports 0 memories).  Save this
        beside ``state_dict()``; the tensors themselves stay in the ``state_dict`` unchanged.  An implicit id range
        that a compaction took rows out of carries the surviving original indices (an int64 array) in place of its
        first index; states saved before compaction existed load unchanged."""
        n = self.memory_count
        state = {"memory_count": n, "index_ready": bool(self._index_ready),
                 "write_cursor": self._write_cursor, "centroids_k": self.centroids_k,
                 "centroids_update_interval": self.centroids_update_interval,
                 "ids_by_slot": list(self._idx_to_id[:n]),
                 "id_to_idx": dict(self.id_to_idx),
                 "slot_time": self._slot_time[:n].tobytes(),            # float64 host clock per slot
                 "implicit_ids": list(self._implicit_ids)}
        if self._tag_quota_map or self._tag_quota_default is not None:  # (only then: other states keep their keys)
            state["tag_quota"] = {"default": self._tag_quota_default, "tags": dict(self._tag_quota_map)}
            state["tag_origin"] = dict(self._tag_origin)
        if self._replay_draws:                          # (only then: a bank that never replayed keeps its keys)
            state["replay_draws"] = self._replay_draws
        return state

    def load_bank_state(self, state: Dict[str, Any]) -> None:
        """Inverse of ``bank_state`` (call after ``load_state_dict``)."""
        n = int(state["memory_count"])
        if not (0 <= n <= self.max_memories):
            raise ValueError(f"memory_count {n} does not fit a bank of {self.max_memories}")
        self.memory_count = n
        self._index_ready = bool(state.get("index_ready", False))
        self._write_cursor = int(state.get("write_cursor", 0))
        self.centroids_k = int(state.get("centroids_k", self.centroids_k))
        self.centroids_update_interval = int(state.get("centroids_update_interval",
                                                       self.centroids_update_interval))
        self._idx_to_id = list(state["ids_by_slot"]) + [None] * (self.max_memories - n)
        self.id_to_idx = dict(state.get("id_to_idx") or
                              {mid: i for i, mid in enumerate(state["ids_by_slot"]) if mid is not None})
        self._implicit_ids = [(int(s0), int(s1), prefix, int(n0) if isinstance(n0, (int, np.integer))
                               else np.asarray(n0, dtype=np.int64)) for s0, s1, prefix, n0 in state.get("implicit_ids", [])]
        self._slot_time[:] = 0.0
        st = state.get("slot_time")
        self._slot_time[:n] = np.frombuffer(st, dtype=np.float64)[:n] if st is not None else time.time()
        self._tag_origin = {}
        if "tag_quota" in state:                        # quotas travel with their tie origins; without: this bank's own
            self._tag_quota_default, self._tag_quota_map = None, {}
            self.set_tag_quota(None, state["tag_quota"].get("default"))
            for t, q in state["tag_quota"].get("tags", {}).items():
                self.set_tag_quota(int(t), q)
            self._tag_origin = {int(t): int(c) for t, c in state.get("tag_origin", {}).items()}
        self._replay_draws = int(state.get("replay_draws", 0))
        self._invalidate_norms()

    def gather_features(self, rows: torch.Tensor) -> torch.Tensor:
        """``memory_features[rows]`` for int32 rows of any shape (``-1`` -> zeros): the
        ``[B, k, D]`` gather of ``memory_augmented_layer.py:124-128``."""
        return ops.bank_gather(self.memory_features, rows.to(torch.int32).contiguous())

    # ------------------------------------------------------------------ maintenance
    def decay_memories(self, decay_rate: float = 0.01) -> None:
        if self.memory_count == 0:
            return
        ops.bank_decay(self.memory_metadata, float(decay_rate), self.memory_count)
        if self._ivf is not None:
            self._ivf.rowc_live = False                 # strengths changed under the cached score constants

    def decay(self, rate: float = 0.01) -> None:
        self.decay_memories(decay_rate=rate)

    # ------------------------------------------------------------------ retention
    def reinforce(self, rows, amount: float = 0.1, cap: float = 1.0) -> None:
        """Strengthen the memories at bank rows ``rows`` (int, any shape, e.g. what ``recall_batch`` returned;
        ``-1`` and rows outside the bank are ignored): ``strength = min(strength + amount, cap)`` where it is
        below ``cap``, once per distinct row however often it occurs.  ``cap`` defaults to the strength a write
        gives.  With ``overflow='weakest'`` reinforced rows are the last to be evicted."""
        if self.memory_count == 0:
            return
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(np.asarray(rows))
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        if rows.numel() == 0:
            return
        ops.bank_reinforce(self.memory_metadata, self.memory_count, rows, float(amount), float(cap))
        if self._ivf is not None:
            self._ivf.rowc_live = False                 # strengths changed under the cached score constants

    def retention_keys(self, now: Optional[float] = None) -> torch.Tensor:
        """fp32 [memory_count]: ``strength * exp(-(now - timestamp) / 3600)`` of every held row, the key
        ``overflow='weakest'`` evicts by (read-only)."""
        now = time.time() if now is None else now
        return ops.bank_retention_keys(self.memory_metadata, self.memory_count, now)

    def weakest(self, n: int, now: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(rows int64 [n], keys fp32 [n])``: the ``n`` rows a write at ``now`` would evict first, in that
        order, with the current write cursor (read-only; ``1 <= n <= memory_count``)."""
        now = time.time() if now is None else now
        return ops.bank_select_weakest(self.memory_metadata, self.memory_count, now,
                                       self._write_cursor % self.max_memories, int(n))

    # ------------------------------------------------------------------ replay
    def _replay_scope(self, priority, alpha, tags, newer_than, older_than, min_strength, seed, draw) -> Dict[str, Any]:
        seed = self.replay_seed if seed is None else seed
        draw = self._replay_draws if draw is None else draw
        return dict(priority=priority, alpha=alpha, tags=tags, newer_than=newer_than, older_than=older_than,
                    min_strength=min_strength, seed=seed, draw=draw)

    def replay_keys(self, *, priority: str = 'key', alpha: float = 1.0, tags=None, newer_than: Optional[float] = None,
                    older_than: Optional[float] = None, min_strength: Optional[float] = None,
                    seed: Optional[int] = None, draw: Optional[int] = None,
                    now: Optional[float] = None) -> torch.Tensor:
        """fp32 [memory_count]: the draw key of every held row for ``(seed, draw)``, ``-inf`` for a row ``replay``
        could not take (read-only; ``draw=None``: the number the next ``replay()`` will use).  ``replay`` returns the
        top ``n`` of these by ``(key descending, row ascending)``."""
        now = time.time() if now is None else now
        return ops.bank_replay_keys(self.memory_metadata, self.memory_count, now,
                                    **self._replay_scope(priority, alpha, tags, newer_than, older_than, min_strength,
                                                         seed, draw))

    def replay(self, n: int, *, priority: str = 'key', alpha: float = 1.0, tags=None,
               newer_than: Optional[float] = None, older_than: Optional[float] = None,
               min_strength: Optional[float] = None, seed: Optional[int] = None, draw: Optional[int] = None,
               now: Optional[float] = None, reinforce: Optional[float] = None, reinforce_cap: float = 1.0,
               touch: bool = False, return_features: bool = True) -> ReplaySample:
        """Draw ``n`` held memories nobody asked for, without replacement, seeded: the sample a sleep phase rehearses.
        A memory is the likelier the larger ``p = exp(alpha * lw)``: the first is row ``r`` with probability
        ``p_r / sum p``, each later one is drawn the same way from what is left (the rule: ``include/aura_hip.h``,
        "Replay").  ``priority='key'``: ``p`` = (strength x recency) ^ alpha, the retention key; ``'strength'``;
        ``'uniform'``.  ``alpha`` in [0, 16]: 0 = uniform over the eligible rows, larger = greedier.  The scope is that
        of a scoped recall: ``tags`` (None = any, an int, or up to 64 as a union; 0 = untagged), ``newer_than``,
        ``older_than``, ``min_strength``; under ``'key'`` / ``'strength'`` a memory also needs ``0 < strength < inf``.
        ``n`` beyond ``memory_count`` is clamped; a scope of fewer eligible memories pads with ``-1``.
        ``seed`` defaults to the bank's ``replay_seed``.  ``draw=None`` numbers the call with the bank's counter and
        advances it (successive calls differ; the counter travels in ``bank_state()``); an explicit ``draw`` repeats
        that draw and advances nothing.  The first ``m`` rows of a draw of ``n`` are the draw of ``m``, and the draw of
        a scope is the whole bank's order filtered to it.
        ``reinforce`` (an amount) / ``touch=True`` apply ``reinforce()`` / ``touch()`` to the drawn rows after the draw
        is final.  No host sync (``touch`` reads the rows back for the host's slot clock, as ``touch()`` does)."""
        n = int(n)
        if n < 0:
            raise ValueError(f"replay: n must be >= 0, got {n}")
        now = time.time() if now is None else now
        scope = self._replay_scope(priority, alpha, tags, newer_than, older_than, min_strength, seed, draw)
        dev = self.memory_features.device
        n = min(n, self.memory_count)
        if n == 0:                                      # an empty bank (or n = 0): nothing is drawn or numbered
            feats = self.memory_features.new_zeros(0, self.memory_features.shape[1]) if return_features else None
            return ReplaySample(torch.empty(0, dtype=torch.int32, device=dev),
                                torch.empty(0, dtype=torch.float32, device=dev), feats,
                                torch.zeros((), dtype=torch.int64, device=dev))
        rows, keys, eligible = ops.bank_replay(self.memory_metadata, self.memory_count, now, n, **scope)
        if draw is None:
            self._replay_draws += 1
        feats = ops.bank_gather(self.memory_features, rows) if return_features else None
        if reinforce is not None:
            self.reinforce(rows, amount=reinforce, cap=reinforce_cap)
        if touch:
            self.touch(rows, now=now)
        return ReplaySample(rows, keys, feats, eligible)

    def rebuild_centroids(self, perm: Optional[torch.Tensor] = None) -> None:
        """One Lloyd iteration from a random sample of rows (reference ``:345-377``).

        assign (fp32 matrix cores) -> rows grouped by cluster (device sort) -> means as a segmented
        reduction (the bank is read once) -> second assign -> counts + metadata; the second grouping
        is kept for the next re-pack of the inverted lists."""
        if self.memory_count == 0 or not self.use_centroid_index:
            return
        n = self.memory_count
        k = min(self.centroids_k, n)
        if perm is None:
            # The reference draws randperm(n, device=self.device) (:354).  Up to 2^18 rows the draw comes from
            # torch's CPU generator, so a seeded run reproduces the reference's CPU run (the golden vectors);
            # a full CPU permutation of a 1M-row bank costs ~10 ms per rebuild, so larger banks draw from the
            # device generator, as the reference itself does on a GPU.
            perm = torch.randperm(n) if n <= (1 << 18) else torch.randperm(n, device=self.device)
        init = ops.bank_gather(self.memory_features, perm[:k].to(device=self.device, dtype=torch.int32))
        cent = torch.zeros_like(self.centroids)
        cent[:k] = init
        assign = ops.kmeans_assign(self.memory_features, cent, n, k)
        ops.kmeans_update(self.memory_features, assign, cent, k, update_means=True)
        self.centroids.copy_(cent)          # rows >= k stay zero (ref :366-367)
        assign = ops.kmeans_assign(self.memory_features, self.centroids, n, k)
        counts = torch.zeros(self.centroids_k, device=self.device)
        order, seg_off = ops.kmeans_update(self.memory_features, assign, self.centroids, k, counts=counts,
                                           meta=self.memory_metadata, update_means=False)
        self.centroid_counts = counts
        self._index_ready = True
        self._unlisted_rows = False                   # every held row has just been assigned to a list
        self._invalidate_lists()
        if k == 256 and seg_off.numel() == 257:
            self._ivf_pending = (order, seg_off)
