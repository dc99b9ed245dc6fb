"""HippocampalTransformer: the language model the package's front end, layers and decoding step add up to, with cached
generation on a fused sampler.

API-compatible with the reference's ``src/core/language_zone/hippocampal_transformer.py``: the constructor
``(config, hippocampus)``, the attribute names (``pos_encoder``, ``semantic_encoder``, ``dropout``, ``layer_norm``,
``layers``, ``output_head``), the ``state_dict`` keys, the weight tying (``output_head.weight is
semantic_encoder.token_embedding.weight``), ``set_gradient_checkpointing`` and ``forward(input_ids, prosody=None,
use_memory=True, store_memory=False, memory_ids=None) -> (logits, place_cell_activity)``.  ``forward`` is
``embed_tokens`` (the place code and the theta-gamma add-and-norm kernels), dropout, the layers and the tied head;
gradients flow as they do through the parts.  ``store_memory`` stores the pooled batch through
``create_episodic_memories`` in one call instead of one write per row.

New on this module: ``new_state`` / ``prefill`` / ``step`` / ``generate``.  ``generate`` has the signature users know
from the reference's ``SNNRAGTransformer.generate``; it prefills the layers' K/V caches once, then takes one ``step`` per
token and turns each step's logit row into a token with ``ops.sample_next`` (``csrc/aura_sample.hip``; the rule:
``include/aura_hip.h``, "Next token"), written straight into its column of the preallocated result.  Where it differs
from the reference's loop on purpose:
  * it never truncates the context to ``max_seq_len`` and re-bases the positions: positions simply continue, which the
    theta-gamma table supports (the phase is normalised by ``max_seq_len``, not bounded by it);
  * it stops when every row has finished (each row at its own EOS; a finished row is padded), where the reference stops
    only when every row emits EOS in the same step;
  * top-k keeps exactly ``k`` candidates (equal logits: the lower id), and the random numbers are a function of
    ``(seed, step, stream, token id)``, so a row draws the same tokens alone or in any batch.
Decoding is fp32, runs under ``no_grad`` and has no CPU fallback: CPU tensors raise ``AuraDeviceError``.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from ... import ops
from .decoding import _UNSET, check_seed, decode_loop, start_turn, trim_to_last_finish
from .hippocampal_attention import AttentionCache, row_counts
from .hippocampal_layer import HippocampalTransformerLayer
from .place_cell_encoder import PlaceCellSemanticEncoder
from .theta_gamma_encoding import ThetaGammaPositionalEncoding, embed_tokens


class DecodeState:
    """What a generation carries between steps: one ``AttentionCache`` per layer, all sharing one int32 ``lengths``
    tensor (only the last layer's step advances it; -1 retires a row), the host-side ``position`` (prompt length plus
    steps taken), the ``seen`` mask [B, V] uint8 of the tokens a row holds (the repetition penalty's set),
    ``finished`` uint8 [B], and the sampler's ``seed`` and ``step`` counter.

    ``ragged`` (default False): the rows no longer share one position.  ``step`` and ``extend`` then take the new
    tokens' positions from the device lengths, ``lengths[:, None] + arange(m)``, and ``position`` is only an upper
    bound.  ``pending`` int64 [B] or ``None``: the last token of every row's history, which has not been through the
    model yet (what ``generate(.., return_state=True)`` leaves; the next ``generate(.., state=)`` feeds it first).
    ``stream_ids``: the rows' random streams of the generation that returned the state."""
    __slots__ = ("caches", "lengths", "position", "seen", "finished", "seed", "step", "capacity", "ragged", "pending",
                 "stream_ids")

    def __init__(self, caches: List[AttentionCache], seen: torch.Tensor, finished: torch.Tensor, seed: int):
        self.caches = caches
        self.lengths = caches[0].lengths
        for c in caches[1:]:
            c.lengths = self.lengths
        self.capacity = caches[0].capacity
        self.position = 0
        self.seen = seen
        self.finished = finished
        self.seed = int(seed)
        self.step = 0
        self.ragged = False
        self.pending = None
        self.stream_ids = None

    @property
    def batch(self) -> int:
        return self.seen.shape[0]


class CachedDecodingMixin:
    """``new_state`` / ``step`` / ``extend`` / ``generate`` of a model that has ``config``, ``layers`` (each with ``new_cache``,
    ``prefill``, ``step`` and ``extend``), ``semantic_encoder``, ``pos_encoder``, ``layer_norm``, ``dropout``, ``output_head``
    and its own ``prefill(input_ids, prosody=None, state=None, use_memory=True)``: the cached decoding
    ``HippocampalTransformer`` and ``SNNRAGTransformer`` share, on the loop of ``decoding.py``.  Messages name the class
    that raises."""

    def new_state(self, batch: int, capacity: int, seed: int = 0) -> DecodeState:
        """An empty decoding state for ``batch`` sequences of at most ``capacity`` positions, on the model's device."""
        seed = check_seed(f"{type(self).__name__}.new_state", seed)
        if len(self.layers) < 1:
            raise ValueError(f"{type(self).__name__}.new_state: a model without layers has nothing to cache")
        caches = [layer.new_cache(batch, capacity) for layer in self.layers]
        dev = self.output_head.weight.device
        seen = torch.zeros(batch, self.config.vocab_size, dtype=torch.uint8, device=dev)
        finished = torch.zeros(batch, dtype=torch.uint8, device=dev)
        return DecodeState(caches, seen, finished, seed)

    def _check_state(self, who: str, state, B: int) -> None:
        if not isinstance(state, DecodeState):
            raise TypeError(f"{who}: state must be a DecodeState (new_state), got {type(state)}")
        if state.batch != B or len(state.caches) != len(self.layers):
            raise ValueError(f"{who}: the state holds {state.batch} rows and {len(state.caches)} caches, this call "
                             f"needs {B} rows and {len(self.layers)} caches")

    def _before_fused_steps(self, state: DecodeState) -> None:
        """What ``generate(fused_step=True)`` runs once between the prefill (or a turn's extend) and the first step: a
        model whose fused step needs per-generation constants beyond the caches builds them here.  Nothing here."""

    def _prefill_layer_kwargs(self, who: str, memory) -> Sequence[dict]:
        """What ``_prefill_hidden`` passes to every layer's ``prefill`` beyond the hidden states, the prosody,
        ``use_memory``, the cache and the lengths: one dict per layer.  Nothing here."""
        return [{}] * len(self.layers)

    def _prefill_hidden(self, who, input_ids, prosody, state, use_memory, lengths, memory=None) -> torch.Tensor:
        """``prefill`` up to the head: the last layer's hidden states [B, S, D]."""
        if input_ids.dim() != 2:
            raise ValueError(f"{who}: input_ids is [B, S], got {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        self._check_state(who, state, B)
        extras = self._prefill_layer_kwargs(who, memory)
        if lengths is not None:
            lengths, _ = row_counts(who, "lengths", lengths, B, 1, S, input_ids.device, dtype=torch.int64)
            valid = torch.arange(S, device=input_ids.device)[None, :] < lengths[:, None]
            input_ids = torch.where(valid, input_ids, 0)                   # a valid id where the padding may hold none
        hidden_states, _ = embed_tokens(input_ids, self.semantic_encoder, self.pos_encoder, self.layer_norm)
        hidden_states = self.dropout(hidden_states)
        ragged = {} if lengths is None else dict(lengths=lengths)
        for layer, cache, extra in zip(self.layers, state.caches, extras):
            hidden_states = layer.prefill(hidden_states, prosody=prosody, use_memory=use_memory, cache=cache, **extra,
                                          **ragged)
        with torch.no_grad():
            if lengths is None:
                state.seen.scatter_(1, input_ids.to(torch.int64), 1)
            else:
                self._mark_seen(state.seen, input_ids, valid)
                state.ragged = True
        state.position = S
        return hidden_states

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, prosody: Optional[torch.Tensor] = None, state: Optional[DecodeState] = None,
             use_memory: bool = True, *, fused: bool = False) -> torch.Tensor:
        """One new token per row: tokens [B] (or [B, 1]) at position ``state.position`` -> logits [B, V].  Every
        layer's ``step`` runs on its cache; the last one advances the shared lengths.  ``fused=True`` (B <= 32) takes
        every layer's fused step: six launches a layer instead of fourteen; the front end and the head stay as they
        are.  With ``state.ragged`` every row's position is its device length instead of ``state.position``.  No host
        sync."""
        who = f"{type(self).__name__}.step"
        if tokens.dim() == 1:
            tokens = tokens[:, None]
        if tokens.dim() != 2 or tokens.shape[1] != 1:
            raise ValueError(f"{who}: tokens is [B] or [B, 1], got {tuple(tokens.shape)}")
        self._check_state(who, state, tokens.shape[0])
        if fused and tokens.shape[0] > ops.ROW_LINEAR_MAX_ROWS:
            raise ValueError(f"{who}: the fused step takes at most {ops.ROW_LINEAR_MAX_ROWS} rows, got "
                             f"B={tokens.shape[0]}; use fused=False")
        if state.ragged:
            hidden_states, _ = embed_tokens(tokens, self.semantic_encoder, self.pos_encoder, self.layer_norm,
                                            dense=False, positions=state.lengths[:, None])
        else:
            hidden_states, _ = embed_tokens(tokens, self.semantic_encoder, self.pos_encoder, self.layer_norm,
                                            start=state.position, dense=False)
        hidden_states = self.dropout(hidden_states)[:, 0]
        last = len(self.layers) - 1
        for i, (layer, cache) in enumerate(zip(self.layers, state.caches)):
            hidden_states = layer.step(hidden_states.contiguous() if fused else hidden_states, prosody=prosody,
                                       use_memory=use_memory, cache=cache, advance=i == last, fused=fused)
        state.position += 1
        return self.output_head(hidden_states)

    @torch.no_grad()
    def extend(self, tokens: torch.Tensor, prosody: Optional[torch.Tensor] = None, state: Optional[DecodeState] = None,
               use_memory: bool = True, counts=None) -> torch.Tensor:
        """``m >= 1`` new tokens per row appended to a state that holds a context: tokens [B, m] (prosody [B, m, 4] or
        ``None``) at the positions after each row's context -> logits [B, m, V], what ``m`` calls of ``step`` return.
        The tokens go through the layers' ``extend`` in pieces of at most ``ops.DECODE_EXTEND_MAX``; in each piece the
        last layer advances the shared lengths.  Marks the tokens in ``state.seen``.  No host sync.

        ``counts`` [B] (ints, ``0 <= counts[b] <= m``, on the host or the device): the rows are right-padded and row
        ``b`` appends only its first ``counts[b]`` tokens, at its own positions (the state becomes ``ragged``).  What
        the padding holds is ignored and the logits at the padded places are unspecified.  Only the tokens below the
        count are marked in ``state.seen``.  ``state.position`` advances by ``m``, an upper bound; the capacity check
        uses the largest count where the host knows the counts, ``m`` otherwise."""
        logits = [self.output_head(h) for h in self._extend_hidden(f"{type(self).__name__}.extend", tokens, prosody,
                                                                   state, use_memory, counts)]
        # (one piece without counts is returned as it is; with counts the result has always been a copy)
        return logits[0] if counts is None and len(logits) == 1 else torch.cat(logits, dim=1)

    @staticmethod
    def piece_counts(counts: torch.Tensor, t0: int) -> torch.Tensor:
        """The counts of the piece that starts at token ``t0``: ``clamp(counts - t0, 0, ops.DECODE_EXTEND_MAX)``."""
        return (counts - t0).clamp(0, ops.DECODE_EXTEND_MAX)

    @staticmethod
    def _mark_seen(seen: torch.Tensor, tokens: torch.Tensor, valid: torch.Tensor) -> None:
        """``seen[b, tokens[b, j]] = 1`` where ``valid[b, j]``; the other places mark a column that is cut off."""
        V = seen.shape[1]
        marks = torch.zeros(seen.shape[0], V + 1, dtype=seen.dtype, device=seen.device)
        marks.scatter_(1, torch.where(valid, tokens.to(torch.int64), V), 1)
        seen.bitwise_or_(marks[:, :V])

    @torch.no_grad()
    def _extend_hidden(self, who: str, tokens, prosody, state, use_memory: bool, counts) -> List[torch.Tensor]:
        """``extend`` up to the head: the last layer's hidden states, one [B, n, D] per piece.  Without ``counts`` the
        layers are called without ``counts`` and ``count_bound`` and a state that is not ragged keeps its scalar
        position."""
        if tokens.dim() != 2 or tokens.shape[1] < 1:
            raise ValueError(f"{who}: tokens is [B, m] with m >= 1, got {tuple(tokens.shape)}")
        B, m = tokens.shape
        self._check_state(who, state, B)
        if prosody is not None and tuple(prosody.shape) != (B, m, 4):
            raise ValueError(f"{who}: prosody is [B, m, 4] = ({B}, {m}, 4), got {tuple(prosody.shape)}")
        dev = state.lengths.device
        known = None
        if counts is not None:
            counts, known = row_counts(who, "counts", counts, B, 0, m, dev)
        held = max(cache.max_length for cache in state.caches)
        need = m if known is None else max(known, default=0)
        if held + need > state.capacity:
            raise RuntimeError(f"{who}: {need} more positions do not fit the caches ({held} of {state.capacity} may be "
                               f"held); a sliding cache is not part of this module")
        if counts is not None:
            state.ragged = True                                            # the device lengths are every row's position
            valid = torch.arange(m, dtype=torch.int32, device=dev)[None, :] < counts[:, None]
            tokens = torch.where(valid, tokens.to(dev), 0)                 # a valid id where the padding may hold none
        last = len(self.layers) - 1
        hidden = []
        for t0 in range(0, m, ops.DECODE_EXTEND_MAX):
            piece = tokens[:, t0:t0 + ops.DECODE_EXTEND_MAX]
            n = piece.shape[1]
            at = dict(start=state.position)
            if state.ragged:
                at = dict(positions=state.lengths[:, None] + torch.arange(n, dtype=torch.int32, device=dev))
            hidden_states, _ = embed_tokens(piece, self.semantic_encoder, self.pos_encoder, self.layer_norm,
                                            dense=False, **at)
            hidden_states = self.dropout(hidden_states)
            part = None if prosody is None else prosody[:, t0:t0 + n]
            rows = {}
            if counts is not None:
                bound = n if known is None else max((min(max(c - t0, 0), n) for c in known), default=0)
                rows = dict(counts=self.piece_counts(counts, t0), count_bound=bound)
            for i, (layer, cache) in enumerate(zip(self.layers, state.caches)):
                hidden_states = layer.extend(hidden_states, prosody=part, use_memory=use_memory, cache=cache,
                                             advance=i == last, **rows)
            state.position += n
            hidden.append(hidden_states)
        if counts is None:
            state.seen.scatter_(1, tokens.to(torch.int64), 1)
        else:
            self._mark_seen(state.seen, tokens, valid)
        return hidden

    @staticmethod
    def _assemble(ids: torch.Tensor, lens: torch.Tensor, new: torch.Tensor, pad: int) -> torch.Tensor:
        """[B, S + n]: row ``b`` holds its first ``lens[b]`` of ``ids`` [B, S], then ``new`` [B, n], then ``pad``."""
        S, n = ids.shape[1], new.shape[1]
        col = torch.arange(S + n, device=ids.device)[None, :]
        lens = lens.to(torch.int64)[:, None]
        src = torch.cat([ids.to(torch.int64), new], dim=1)
        # column c of the result is column c of the prompt below the length, column S + (c - len) of the new tokens
        # from there on, and padding past len + n
        take = torch.where(col < lens, col, (col - lens + S).clamp(max=S + n - 1))
        return torch.where(col < lens + n, src.gather(1, take), pad)

    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 50, temperature: float = 0.8, top_k: int = 50,
                 top_p: float = 0.9, use_memory: bool = True, repetition_penalty: float = 1.2, *,
                 repetition_rule: str = "divide", seed: Optional[int] = None, eos_token_id=_UNSET,
                 pad_token_id: Optional[int] = None, sync_every: int = 8, stream_ids=None,
                 fused_step: bool = False, state: Optional[DecodeState] = None, return_state: bool = False,
                 capacity: Optional[int] = None, prompt_lengths=None, new_lengths=None):
        """Generates up to ``max_new_tokens`` tokens after the prompts ``input_ids`` [B, S] (equal lengths, as in the
        reference) -> [B, S + n].  Runs under ``eval()`` and ``no_grad``: one ``prefill``, then per token one ``step``
        and one ``ops.sample_next`` that writes the token into its column of the preallocated result.

        ``temperature=0`` is greedy; ``repetition_penalty`` acts on the tokens a row holds (prompt and generated),
        ``repetition_rule`` ``'divide'`` as the reference's loop or ``'signed'`` as its ``apply_repetition_penalty``.
        ``seed=None`` takes one number from torch's default generator (``torch.manual_seed`` governs it);
        ``stream_ids`` [B] number the rows' random streams (default: the row numbers).  ``eos_token_id`` defaults to the
        config's; with one, a row that draws it is finished: its later tokens are ``pad_token_id`` (default: the EOS
        id) and its cache rows are retired (length -1).  The host looks at the finished flags only every ``sync_every``
        steps, and once at the end to trim the result to the step at which the last row finished.
        ``fused_step=True`` (B <= 32) decodes with the layers' fused step (``step(fused=True)``).

        Differences from the reference's loop, on purpose: the context is never truncated to ``max_seq_len`` and
        re-based, positions simply continue (``S + max_new_tokens`` must fit ``ops.DECODE_MAX_CAP``); generation
        stops when every row has finished, not only when every row emits EOS in the same step; top-k keeps exactly
        ``k`` candidates and the random stream is fixed by ``(seed, step, stream, token id)`` (the rule:
        ``include/aura_hip.h``, "Next token").

        Continuing.  ``return_state=True`` returns ``(tokens, state)``; ``capacity`` (default ``S + max_new_tokens``)
        reserves cache room for later turns.  In the returned state every row stands at the end of its own history
        (the prompt and what it generated up to and including its EOS, or all ``n`` tokens without one): the last
        history token has not been through the model, so ``lengths[b] = len(history_b) - 1`` and ``pending[b]`` is
        that token; ``finished`` is clear and ``ragged`` set.  ``generate(new_ids [B, S2], state=state, ..)`` feeds
        ``[pending, new_ids]`` through ``extend``, samples from the last position and decodes as above -> [B, S2 + n];
        ``state.step`` and ``state.seen`` carry on, the seed and the streams are the state's unless given.  It raises
        on the host, without reading the device, when the turn may not fit the state's capacity.

        Ragged batches.  ``prompt_lengths`` [B] (first turn, ``1 <= prompt_lengths[b] <= S``) and ``new_lengths`` [B] (a
        turn with ``state=``, ``0 <= new_lengths[b] <= S2``), ints on the host or the device: the rows of
        ``input_ids`` are right-padded and what the padding holds is ignored.  Every row is prefilled or extended by
        its own tokens only, its first logits are those at its own last token, and it generates what it generates
        alone.  The result is [B, S + n]: row ``b`` holds its own ``len_b`` tokens, then its generated tokens, then
        ``pad_token_id``.  Lengths the host knows are checked before any launch; no step syncs with the host."""
        who = f"{type(self).__name__}.generate"
        if input_ids.dim() != 2 or input_ids.shape[1] < 1:
            raise ValueError(f"{who}: input_ids is [B, S] with S >= 1, got {tuple(input_ids.shape)}")
        for n, v in (("max_new_tokens", max_new_tokens), ("sync_every", sync_every)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{who}: {n} must be an int >= 1, got {v!r}")
        B, S = input_ids.shape
        width = S + max_new_tokens
        if state is not None:
            self._check_state(who, state, B)
            if state.pending is None or not state.ragged:
                raise ValueError(f"{who}: state must be one that generate(.., return_state=True) returned")
            if capacity is not None:
                raise ValueError(f"{who}: capacity is set where the state is made; this one holds {state.capacity}")
            held = max(cache.max_length for cache in state.caches)
            if held + width > state.capacity:
                raise RuntimeError(f"{who}: this turn needs S + max_new_tokens = {width} more positions, the state "
                                   f"may hold {held} of {state.capacity} (reserve room with capacity= in the first "
                                   f"call; a sliding cache is not part of this module)")
        elif capacity is None:
            capacity = width
        elif isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < width:
            raise ValueError(f"{who}: capacity must be an int >= S + max_new_tokens = {width}, got {capacity!r}")
        if state is None and capacity > ops.DECODE_MAX_CAP:
            raise ValueError(f"{who}: S + max_new_tokens = {capacity} exceeds the cache limit {ops.DECODE_MAX_CAP} (a "
                             f"sliding cache is not part of this module)")
        eos = getattr(self.config, "eos_token_id", None) if eos_token_id is _UNSET else eos_token_id
        pad = pad_token_id if pad_token_id is not None else (eos if eos is not None else 0)
        if seed is None and state is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())
        if fused_step and B > ops.ROW_LINEAR_MAX_ROWS:
            raise ValueError(f"{who}: fused_step takes at most {ops.ROW_LINEAR_MAX_ROWS} rows, got B={B}")
        dev = input_ids.device
        if stream_ids is not None and not isinstance(stream_ids, torch.Tensor):
            stream_ids = torch.as_tensor(list(stream_ids), dtype=torch.int64).to(dev)
        if (prompt_lengths if state is not None else new_lengths) is not None:
            raise ValueError(f"{who}: prompt_lengths goes with a first turn and new_lengths with a turn that has state=")
        first, lens = state is None, None
        if prompt_lengths is not None:
            lens, _ = row_counts(who, "prompt_lengths", prompt_lengths, B, 1, S, dev, dtype=torch.int64)
        elif new_lengths is not None:
            lens, known = row_counts(who, "new_lengths", new_lengths, B, 0, S, dev, dtype=torch.int64)
        if not first and seed is not None:
            seed = check_seed(who, seed)
        sampling = dict(penalty=repetition_penalty, penalty_rule=repetition_rule, temperature=temperature, top_k=top_k,
                        top_p=top_p)
        self.eval()
        with torch.no_grad():
            if lens is None:
                generated = torch.empty(B, width, dtype=torch.int64, device=dev)
                generated[:, :S] = input_ids
                new = generated[:, S:]
            else:
                new = torch.empty(B, max_new_tokens, dtype=torch.int64, device=dev)
            if first:
                state = self.new_state(B, capacity, seed=seed)
                state.stream_ids = stream_ids
            else:
                turn = start_turn(state, input_ids, seed, stream_ids)
            if lens is None:
                logits = (self.prefill(input_ids, state=state, use_memory=use_memory) if first else
                          self.extend(turn, state=state, use_memory=use_memory))[:, -1]
            else:
                if first:
                    fed = lens
                    hidden = self._prefill_hidden(f"{type(self).__name__}.prefill", input_ids, None, state, use_memory,
                                                  lens)
                else:
                    fed = lens + 1                                          # the pending token is always fed
                    hidden = torch.cat(self._extend_hidden(who, turn, None, state, use_memory,
                                                           fed if known is None else [c + 1 for c in known]), dim=1)
                # every row's logits at its own last fed token: the rows are gathered before the head, [B, D] -> [B, V]
                at = (fed - 1).clamp(min=0)[:, None, None].expand(B, 1, hidden.shape[2])
                logits = self.output_head(hidden.gather(1, at)[:, 0])
            if fused_step:
                self._before_fused_steps(state)
            # every row's length with the prompt consumed, before the first retirement: what the returned state counts from
            base = state.lengths.clone() if return_state else None
            n = decode_loop(logits, state, new, sampling, eos, pad, sync_every,
                            lambda column: self.step(column, state=state, use_memory=use_memory, fused=bool(fused_step)),
                            retire=True)
            n = trim_to_last_finish(new[:, :n], eos)
            if return_state:
                self._stand_at_history_end(state, base, new[:, :n], eos)
            generated = generated[:, :S + n] if lens is None else self._assemble(input_ids, lens, new[:, :n], pad)
        return (generated, state) if return_state else generated

    @staticmethod
    def _stand_at_history_end(state: DecodeState, base: torch.Tensor, new: torch.Tensor, eos) -> None:
        """Leaves ``state`` where a next turn starts (see ``generate``): ``new`` [B, n] are the generated columns,
        ``base`` the lengths before the first of them was fed.  A row's history holds ``count`` of them, up to and
        including its first EOS; ``count - 1`` went through the model.  Device ops only."""
        n = new.shape[1]
        count = torch.full((new.shape[0],), n, dtype=torch.int64, device=new.device)
        if eos is not None:
            before = ((new == eos).cumsum(dim=1) == 0).sum(dim=1)         # columns before the row's first EOS; n: none
            count = torch.clamp(before + 1, max=n)
        state.lengths.copy_(base.to(torch.int64) + count - 1)
        state.pending = new.gather(1, (count - 1)[:, None])[:, 0].clone()
        state.finished.zero_()
        state.ragged = True


class HippocampalTransformer(CachedDecodingMixin, nn.Module):
    def __init__(self, config, hippocampus):
        super().__init__()
        self.config = config
        self.hippocampus = hippocampus
        self.use_gradient_checkpointing = getattr(config, 'use_gradient_checkpointing', False)
        self.pos_encoder = ThetaGammaPositionalEncoding(config)
        self.semantic_encoder = PlaceCellSemanticEncoder(config, hippocampus)
        self.dropout = nn.Dropout(config.dropout)
        self.layer_norm = nn.LayerNorm(config.embedding_dim)
        self.layers = nn.ModuleList([HippocampalTransformerLayer(config, hippocampus)
                                     for _ in range(config.num_layers)])
        self.output_head = nn.Linear(config.embedding_dim, config.vocab_size, bias=False)
        self.output_head.weight = self.semantic_encoder.token_embedding.weight      # tied, as upstream

    def set_gradient_checkpointing(self, enable: bool = True):
        self.use_gradient_checkpointing = enable

    def _layer_forward(self, layer, hidden_states, prosody, use_memory):
        return layer(hidden_states, prosody=prosody, use_memory=use_memory)

    # ------------------------------------------------------------------------------------------------ full sequences
    def forward(self, input_ids: torch.Tensor, prosody: Optional[torch.Tensor] = None, use_memory: bool = True,
                store_memory: bool = False, memory_ids: Optional[List[str]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        batch_size = input_ids.shape[0]
        hidden_states, place_cell_activity = embed_tokens(input_ids, self.semantic_encoder, self.pos_encoder,
                                                          self.layer_norm)
        hidden_states = self.dropout(hidden_states)
        for layer in self.layers:
            if self.training and self.use_gradient_checkpointing:
                hidden_states = checkpoint(self._layer_forward, layer, hidden_states, prosody, use_memory,
                                           use_reentrant=False)
            else:
                hidden_states = layer(hidden_states, prosody=prosody, use_memory=use_memory)
        logits = self.output_head(hidden_states)
        if store_memory and self.hippocampus is not None:
            summary = hidden_states.mean(dim=1).detach()
            now = time.time()
            ids = [memory_ids[b] if memory_ids and b < len(memory_ids) else f"step-{int(now)}-b{b}"
                   for b in range(batch_size)]
            self.hippocampus.create_episodic_memories(ids, summary)
        return logits, place_cell_activity

    # ------------------------------------------------------------------------------------------------ cached decoding
    def prefill(self, input_ids: torch.Tensor, prosody: Optional[torch.Tensor] = None,
                state: Optional[DecodeState] = None, use_memory: bool = True, lengths=None) -> torch.Tensor:
        """``forward`` over a prompt [B, S] that also fills every layer's cache and marks the prompt's tokens in
        ``state.seen``.  Returns the logits [B, S, V].  ``lengths`` [B] (ints, ``1 <= lengths[b] <= S``, on the host or
        the device): the rows are right-padded; the caches hold each row's own positions, only its own tokens are
        marked, the state becomes ``ragged`` and the logits at the padded places are unspecified."""
        return self.output_head(self._prefill_hidden("HippocampalTransformer.prefill", input_ids, prosody, state,
                                                     use_memory, lengths))
