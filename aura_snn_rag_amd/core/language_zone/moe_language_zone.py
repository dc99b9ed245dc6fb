"""``MoELanguageZone`` behind the reference's name (``src/core/language_zone/moe_language_zone.py``): embeddings, a GIF
encoder, the spike-to-continuous bridge, the liquid router over ``num_experts`` ``SNNExpert`` modules, the
continuous-to-spike bridge, a GIF decoder and the output projection.  The reference's constructor, attribute names and
``state_dict`` keys; ``forward(input_ids, attention_mask=None) -> (logits, {'probs': ...})``.

The reference runs every expert that any token selected over all ``B S`` tokens, about ten launches per expert, and
masks the result.  Here, when autograd is not recording, ``route_experts`` is five launches in all (``ops.moe_route``,
``ops.moe_experts``; the rule: ``include/aura_hip.h``, "MoE zone"): each expert runs on its own tokens only, with the
activations in LDS.  When autograd is recording, ``route_experts`` is ``route_experts_composed``: the same modules from
torch ops and the differentiable ``GIFNeuron``, each expert on its gathered tokens, so training works.

Decoding.  The zone has no attention: what it remembers of the past is the ``(v, theta)`` state of ``encoder`` and
``decoder``, whose membrane loops run over the sequence axis; everything between them is per token.  So a token costs
O(1) time and O(hidden) state, with no K/V cache and no capacity.  What stood in the way was the bridge's
``torch.rand``: ``forward(.., seed=)`` replaces the bridge and the mean over its timesteps by one
``ContinuousToSpikeBridge.rate_code`` launch (``ops.poisson_rate``; the rule: ``include/aura_hip.h``, "Poisson
bridge") whose draw is keyed by (channel, timestep, position, stream) under the seed, so position ``p`` draws the same
in a forward over the sequence and in a one-token ``step``.  ``new_state`` / ``prefill`` / ``step`` / ``generate`` build
on it; ``generate`` has the meanings and defaults of ``CachedDecodingMixin.generate`` and runs the same loop
(``decoding.py``), without the retirement of finished rows: there is no cache to take a row out of.  One seed drives the sampler and the bridge: the sampler's Philox counter is
(token id, stream, step lo, step hi), the bridge's (channel, timestep group, position, stream); the words feed
different decisions.  ``forward(.., seed=None)`` is what it was, launch for launch.

A step is 14 launches, counted from the code: the embedding gather (1), ``ops.row_linear`` and ``ops.gif_run`` for
the encoder (2), ``row_linear`` for ``spike_to_continuous.proj`` (1), ``route_experts`` (5), ``rate_code`` (1),
``row_linear`` and ``gif_run`` for the decoder (2), the head (1) and the position counter (1).

Not here: ``T > 1`` or carried state in the fused experts, bf16, a fused backward; ragged prompts (``lengths=`` raises:
``gif_run`` has no per-row step counts, so a padded row's state would advance over its padding); a carried-state GIF
epilogue for ``row_linear``; ``FullLanguageZone`` (its prosody gains are a whole-sequence top-k, which is not causal);
``BanditGating``."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ..liquid_moe import LiquidMoERouter, _recording
from .decoding import _UNSET, check_seed, decode_loop, start_turn, trim_to_last_finish
from .gif_neuron import GIFNeuron
from .snn_expert import SNNExpert
from .spike_bridge import ContinuousToSpikeBridge, SpikeToContinuousBridge


class ZoneState:
    """What ``MoELanguageZone`` carries between tokens: ``encoder`` and ``decoder``, each ``(v, theta)`` of [B, width]
    fp32 (fresh: 0 and the neuron's ``threshold``); ``position`` int32 [B] on the device, the position of every row's
    next token (``length`` is the same number on the host: the rows have equal lengths); ``seen`` uint8 [B, V] the
    tokens a row holds (the repetition penalty's set), ``finished`` uint8 [B]; ``seed`` and the sampler's ``step``
    counter; ``stream_ids`` int64 [B] or ``None`` (the row numbers) for the sampler and ``streams`` int32 [B], the same
    numbers for the bridge; ``pending`` int64 [B] or ``None``: the last token of every row's history, which has not been
    through the model yet (what ``generate(.., return_state=True)`` leaves).  It has no capacity."""
    __slots__ = ("encoder", "decoder", "position", "length", "seen", "finished", "seed", "step", "stream_ids",
                 "streams", "pending")

    def __init__(self, encoder, decoder, position, seen, finished, seed, stream_ids, streams):
        self.encoder, self.decoder = encoder, decoder
        self.position, self.length = position, 0
        self.seen, self.finished = seen, finished
        self.seed, self.step = int(seed), 0
        self.stream_ids, self.streams = stream_ids, streams
        self.pending = None

    @property
    def batch(self) -> int:
        return self.seen.shape[0]


def _zone_streams(who: str, stream_ids, B: int, dev):
    """``(stream_ids int64 [B] or None, streams int32 [B])`` on ``dev``: the rows' random streams for the sampler and
    the same numbers as 32-bit words for the bridge.  Host integers are checked; a tensor is taken as it is."""
    if stream_ids is None:
        return None, torch.arange(B, dtype=torch.int32, device=dev)
    if not isinstance(stream_ids, torch.Tensor):
        ids = np.asarray(list(stream_ids))
        if ids.dtype.kind not in "iu" or ids.shape != (B,) or (ids.astype(np.int64) < 0).any() \
                or (ids.astype(np.int64) >= (1 << 32)).any():
            raise ValueError(f"{who}: stream_ids is [B] = ({B},) integers in [0, 2^32), got {stream_ids!r}")
        stream_ids = torch.as_tensor(ids.astype(np.int64)).to(dev)
    if stream_ids.dtype != torch.int64 or tuple(stream_ids.shape) != (B,):
        raise ValueError(f"{who}: stream_ids is int64 [B] = ({B},), got {stream_ids.dtype} {tuple(stream_ids.shape)}")
    stream_ids = stream_ids.to(dev).contiguous()
    return stream_ids, stream_ids.to(torch.int32)


class MoEOutput(NamedTuple):
    """``expert_outputs`` [N, Dm] the weighted sum; ``indices`` int64 [N, k]; ``weights`` [N, k]; ``probs`` [N, E];
    ``trace`` (``return_trace``) [N, k, layers, Hh] every layer's spikes of every (token, slot) pair, else ``None``;
    ``pair_outputs`` [N, k, Dm] every pair's expert output (fused path) or ``None``."""
    expert_outputs: torch.Tensor
    indices: torch.Tensor
    weights: torch.Tensor
    probs: torch.Tensor
    trace: Optional[torch.Tensor] = None
    pair_outputs: Optional[torch.Tensor] = None


class MoELanguageZone(nn.Module):
    def __init__(self, vocab_size: int, embed_dim: int, hidden_dim: int, num_experts: int = 8, top_k: int = 2,
                 moe_hidden_dim: int = 64):
        super().__init__()
        self.vocab_size = vocab_size
        self.embed_dim = embed_dim
        self.hidden_dim = hidden_dim
        self.moe_hidden_dim = moe_hidden_dim
        self.top_k = top_k
        self.num_experts = num_experts
        self.embeddings = nn.Embedding(vocab_size, embed_dim)
        self.encoder = GIFNeuron(embed_dim, hidden_dim, L=16)
        self.spike_to_continuous = SpikeToContinuousBridge(spike_dim=hidden_dim, output_dim=moe_hidden_dim,
                                                           encoding='rate', time_window=10)
        self.experts = nn.ModuleDict({
            f'expert_{i}': SNNExpert(input_dim=moe_hidden_dim, hidden_dim=hidden_dim // 2, output_dim=moe_hidden_dim)
            for i in range(num_experts)})
        self.moe_router = LiquidMoERouter(in_dim=moe_hidden_dim, hidden_dim=64, num_experts=num_experts, top_k=top_k)
        self.continuous_to_spike = ContinuousToSpikeBridge(input_dim=moe_hidden_dim, spike_dim=hidden_dim,
                                                           encoding='poisson')
        self.decoder = GIFNeuron(hidden_dim, embed_dim, L=16)
        self.output_proj = nn.Linear(embed_dim, vocab_size)
        self._table = None
        self._table_key = None

    # ---- the experts' pointer table --------------------------------------------------------------------------------
    def expert_table(self) -> "ops.MoeExpertTable":
        """The device table of the experts' parameter pointers, kept between calls and rebuilt when a parameter was
        written in place (``_version``), re-allocated or moved, or a neuron's setting changed."""
        tensors, gif = [], []
        for i in range(self.num_experts):
            t, g = self.experts[f'expert_{i}'].fused_parameters()
            tensors.append(t)
            gif.append(g)
        key = (tuple((p._version, p.data_ptr(), p.device) for ts in tensors for p in ts), tuple(map(tuple, gif)))
        if self._table is None or key != self._table_key:
            self._table = ops.moe_expert_table([[p.detach() for p in ts] for ts in tensors], gif)
            self._table_key = key
        return self._table

    # ---- routing and experts ---------------------------------------------------------------------------------------
    def route_experts(self, continuous: torch.Tensor, attn_gain: Optional[torch.Tensor] = None,
                      return_trace: bool = False) -> MoEOutput:
        """Router, selected experts and weighted sum on ``continuous`` [N, moe_hidden_dim]."""
        if _recording(self, continuous, attn_gain):
            if return_trace:
                raise ValueError("MoELanguageZone.route_experts: the trace is written by the fused launch; call it "
                                 "under torch.no_grad()")
            return self.route_experts_composed(continuous, attn_gain)
        with torch.no_grad():
            x = continuous.detach().contiguous()
            routing = self.moe_router.route(x, attn_gain)
            out, y, trace = ops.moe_experts(x, routing, self.expert_table(), return_trace=return_trace)
        return MoEOutput(out, routing.indices.long(), routing.weights, routing.probs, trace, y)

    def route_experts_composed(self, continuous: torch.Tensor, attn_gain: Optional[torch.Tensor] = None,
                               routing: Optional[Dict[str, torch.Tensor]] = None) -> MoEOutput:
        """The same from torch ops and this package's modules (differentiable): every selected expert's ``predict`` on
        its gathered tokens, added in ascending expert id.  ``routing``: a router's dict to use instead of routing."""
        route = routing if routing is not None else self.moe_router.compose(continuous, attn_gain)
        idx, w = route['indices'], route['weights']
        out = torch.zeros(continuous.shape[0], self.moe_hidden_dim, device=continuous.device, dtype=continuous.dtype)
        for i in range(self.num_experts):
            chosen = idx == i
            rows = torch.nonzero(chosen.any(dim=1)).flatten()
            if rows.numel() == 0:
                continue
            y = self.experts[f'expert_{i}'].predict(continuous.index_select(0, rows))
            wi = (w * chosen.to(w.dtype)).sum(dim=1).index_select(0, rows)
            out = out.index_add(0, rows, y * wi.unsqueeze(1))
        return MoEOutput(out, idx, w, route['probs'])

    # ---- the model -------------------------------------------------------------------------------------------------
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                keep_on_device: bool = False, *, seed: Optional[int] = None, stream_ids=None, start: int = 0,
                state: Optional[ZoneState] = None) -> Tuple[torch.Tensor, Dict]:
        """``seed=None``: the reference's forward, the bridge's draw from ``torch.rand``.  With a seed the bridge and
        the mean over its timesteps are one ``rate_code`` launch: row ``b`` draws from stream ``stream_ids[b]`` (default
        ``b``) at the positions ``start, start + 1, ..``, and ``encoder`` / ``decoder`` start from ``state``'s ``(v,
        theta)`` when one is given (the state is read, not written: ``prefill`` writes it).  The dict then also holds
        ``encoder_spikes`` [B, S, hidden], ``decoder_spikes`` [B, S, embed] and ``encoder_state``, ``decoder_state``,
        the ``(v, theta)`` after the last token."""
        if seed is None:
            if stream_ids is not None or state is not None or start != 0:
                raise ValueError("MoELanguageZone.forward: stream_ids, start and state go with a seed")
            return self._forward_unseeded(input_ids, keep_on_device)
        who = "MoELanguageZone.forward"
        seed = check_seed(who, seed)
        B, S = input_ids.shape
        if state is not None and (not isinstance(state, ZoneState) or state.batch != B):
            raise ValueError(f"{who}: state must be a ZoneState (new_state) of {B} rows")
        _, streams = _zone_streams(who, stream_ids, B, input_ids.device)
        spikes, enc = self.encoder(self.embeddings(input_ids), None if state is None else state.encoder)
        continuous = self.spike_to_continuous(spikes.reshape(B * S, 1, self.hidden_dim))
        moe = self.route_experts(continuous)
        rate = self.continuous_to_spike.rate_code(moe.expert_outputs, seed=seed, streams=streams, rows_per_stream=S,
                                                  start=start)
        decoded, dec = self.decoder(rate.view(B, S, self.hidden_dim), None if state is None else state.decoder)
        logits = self.output_proj(decoded)
        probs = moe.probs.view(B, S, -1).detach()
        return logits, {'probs': probs if keep_on_device else probs.cpu(), 'encoder_spikes': spikes.detach(),
                        'decoder_spikes': decoded.detach(), 'encoder_state': enc, 'decoder_state': dec}

    def _forward_unseeded(self, input_ids: torch.Tensor, keep_on_device: bool) -> Tuple[torch.Tensor, Dict]:
        B, S = input_ids.shape
        spikes, _ = self.encoder(self.embeddings(input_ids))
        continuous = self.spike_to_continuous(spikes.reshape(B * S, 1, self.hidden_dim))
        moe = self.route_experts(continuous)
        spikes_moe = self.continuous_to_spike(moe.expert_outputs)
        steps = spikes_moe.shape[1]
        decoded, _ = self.decoder(spikes_moe.view(B, S, steps, self.hidden_dim).mean(dim=2))
        logits = self.output_proj(decoded)
        probs = moe.probs.view(B, S, -1).detach()
        return logits, {'probs': probs if keep_on_device else probs.cpu()}

    # ---- decoding --------------------------------------------------------------------------------------------------
    def new_state(self, batch: int, seed: int = 0, stream_ids=None) -> ZoneState:
        """A fresh state for ``batch`` sequences on the model's device: ``v = 0``, ``theta = threshold``, position 0.
        ``stream_ids`` [B] number the rows' random streams (default: the row numbers)."""
        who = "MoELanguageZone.new_state"
        seed = check_seed(who, seed)
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"{who}: batch must be an int >= 1, got {batch!r}")
        dev = self.output_proj.weight.device
        pairs = []
        for neuron, width in ((self.encoder, self.hidden_dim), (self.decoder, self.embed_dim)):
            pairs.append((torch.zeros(batch, width, dtype=torch.float32, device=dev),
                          torch.full((batch, width), float(neuron.threshold), dtype=torch.float32, device=dev)))
        stream_ids, streams = _zone_streams(who, stream_ids, batch, dev)
        return ZoneState(pairs[0], pairs[1], torch.zeros(batch, dtype=torch.int32, device=dev),
                         torch.zeros(batch, self.vocab_size, dtype=torch.uint8, device=dev),
                         torch.zeros(batch, dtype=torch.uint8, device=dev), seed, stream_ids, streams)

    def _check_state(self, who: str, state, B: int) -> None:
        if not isinstance(state, ZoneState):
            raise TypeError(f"{who}: state must be a ZoneState (new_state), got {type(state)}")
        if state.batch != B:
            raise ValueError(f"{who}: the state holds {state.batch} rows, this call needs {B}")

    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor, state: Optional[ZoneState] = None, lengths=None) -> torch.Tensor:
        """The seeded ``forward`` over ``input_ids`` [B, S] (equal lengths) from the state's position, under the
        state's seed and streams -> logits [B, S, V].  Leaves the state after the last token and marks the tokens in
        ``state.seen``.  On a state that already holds history it continues that history."""
        who = "MoELanguageZone.prefill"
        if lengths is not None:
            raise NotImplementedError(f"{who}: ragged prompts are not built: the GIF loop has no per-row step counts, "
                                      f"so a padded row's state would advance over its padding")
        if input_ids.dim() != 2 or input_ids.shape[1] < 1:
            raise ValueError(f"{who}: input_ids is [B, S] with S >= 1, got {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        self._check_state(who, state, B)
        logits, info = self.forward(input_ids, keep_on_device=True, seed=state.seed, stream_ids=state.stream_ids,
                                    start=state.length, state=state)
        state.encoder, state.decoder = info['encoder_state'], info['decoder_state']
        state.position += S
        state.length += S
        state.seen.scatter_(1, input_ids.to(torch.int64), 1)
        return logits

    def _check_steppable(self, who: str) -> None:
        for name in ("encoder", "decoder"):
            if type(getattr(self, name)) is not GIFNeuron:
                raise NotImplementedError(f"{who}: {name} is a {type(getattr(self, name)).__name__}; the step computes "
                                          f"GIFNeuron's currents (one linear) only")
        if self.spike_to_continuous.encoding != 'rate':
            raise NotImplementedError(f"{who}: spike_to_continuous.encoding={self.spike_to_continuous.encoding!r}; the "
                                      f"step takes 'rate' (a window over one step is the step itself)")
        if self.continuous_to_spike.encoding != 'poisson':
            raise NotImplementedError(f"{who}: continuous_to_spike.encoding={self.continuous_to_spike.encoding!r}; the "
                                      f"seeded draw is the 'poisson' bridge's")
        if self.moe_router.training:
            raise RuntimeError(f"{who}: the router is in training mode, where it updates expert_usage; call eval()")

    @staticmethod
    def _gif_step(neuron: GIFNeuron, x: torch.Tensor, pair) -> torch.Tensor:
        """One GIF step of ``neuron`` on ``x`` [B, in] from the carried ``pair`` = (v, theta), updated in place."""
        h = ops.row_linear(x, neuron.linear.weight, neuron.linear.bias)
        out = torch.empty_like(h)
        ops.gif_run(h.view(h.shape[0], 1, -1), out.view(h.shape[0], 1, -1), pair[0], pair[1], float(neuron.decay),
                    int(neuron.L), float(neuron.alpha), float(neuron.threshold), 1)
        return out

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, state: Optional[ZoneState] = None) -> torch.Tensor:
        """One new token per row: ``tokens`` [B] (or [B, 1]), B <= 32, at the state's position -> logits [B, V]: what
        ``prefill`` of one token computes, with the two currents from ``ops.row_linear`` instead of a library GEMM.
        14 launches (the module's docstring counts them), no host sync."""
        who = "MoELanguageZone.step"
        if tokens.dim() == 2 and tokens.shape[1] == 1:
            tokens = tokens[:, 0]
        if tokens.dim() != 1:
            raise ValueError(f"{who}: tokens is [B] or [B, 1], got {tuple(tokens.shape)}")
        B = tokens.shape[0]
        self._check_state(who, state, B)
        if B > ops.ROW_LINEAR_MAX_ROWS:
            raise ValueError(f"{who}: a step takes at most {ops.ROW_LINEAR_MAX_ROWS} rows, got B={B}")
        self._check_steppable(who)
        if state.length + 1 > (1 << 31):
            raise ValueError(f"{who}: positions stay below 2^31")
        spikes = self._gif_step(self.encoder, self.embeddings(tokens), state.encoder)
        proj = self.spike_to_continuous.proj
        continuous = ops.row_linear(spikes, proj.weight, proj.bias) if isinstance(proj, nn.Linear) else spikes
        moe = self.route_experts(continuous)
        rate = self.continuous_to_spike.rate_code(moe.expert_outputs, seed=state.seed, streams=state.streams,
                                                  rows_per_stream=1, start=state.position)
        decoded = self._gif_step(self.decoder, rate, state.decoder)
        state.position += 1
        state.length += 1
        return self.output_proj(decoded)

    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 50, temperature: float = 0.8, top_k: int = 50,
                 top_p: float = 0.9, repetition_penalty: float = 1.2, *, repetition_rule: str = "divide",
                 seed: Optional[int] = None, eos_token_id=_UNSET, pad_token_id: Optional[int] = None,
                 sync_every: int = 8, stream_ids=None, state: Optional[ZoneState] = None, return_state: bool = False,
                 lengths=None):
        """Generates up to ``max_new_tokens`` tokens after the prompts ``input_ids`` [B, S] (equal lengths, B <= 32)
        -> [B, S + n].  Runs under ``eval()`` and ``no_grad``: one ``prefill``, then per token one ``ops.sample_next``
        that writes the token into its column of the preallocated result and one ``step``.  The arguments have the
        meanings and defaults of ``CachedDecodingMixin.generate``: ``temperature=0`` is greedy; ``seed=None`` takes one
        number from torch's default generator; ``stream_ids`` [B] number the rows' random streams (default: the row
        numbers); ``eos_token_id`` defaults to the module's ``eos_token_id`` attribute if it has one, else none; a row
        that draws it is finished and its later tokens are ``pad_token_id`` (default: the EOS id).  The host looks at
        the finished flags every ``sync_every`` steps, and once at the end to trim the result to the step at which the
        last row finished.  The one seed also drives the bridge's draw (the module's docstring says which words go
        where), so a row generates the same tokens alone and in any batch.

        ``return_state=True`` returns ``(tokens, state)``: the state has been through every returned token but the last
        column, which is ``pending``; ``finished`` is clear.  The zone cannot retire a row (its state advances with
        every step), so a row's history is its whole returned row, padding included, and the result is then not
        trimmed.  ``generate(new_ids [B, S2], state=state, ..)`` feeds ``[pending, new_ids]`` through ``prefill`` and
        decodes on; the seed and the streams are the state's unless given.  ``lengths`` raises: ragged prompts are not
        built."""
        who = "MoELanguageZone.generate"
        if lengths is not None:
            raise NotImplementedError(f"{who}: ragged prompts are not built: the GIF loop has no per-row step counts, "
                                      f"so a padded row's state would advance over its padding")
        if input_ids.dim() != 2 or input_ids.shape[1] < 1:
            raise ValueError(f"{who}: input_ids is [B, S] with S >= 1, got {tuple(input_ids.shape)}")
        for n, v in (("max_new_tokens", max_new_tokens), ("sync_every", sync_every)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{who}: {n} must be an int >= 1, got {v!r}")
        B, S = input_ids.shape
        if B > ops.ROW_LINEAR_MAX_ROWS:
            raise ValueError(f"{who}: a step takes at most {ops.ROW_LINEAR_MAX_ROWS} rows, got B={B}")
        if state is not None:
            self._check_state(who, state, B)
            if state.pending is None:
                raise ValueError(f"{who}: state must be one that generate(.., return_state=True) returned")
        if seed is not None:
            seed = check_seed(who, seed)
        eos = getattr(self, "eos_token_id", None) if eos_token_id is _UNSET else eos_token_id
        pad = pad_token_id if pad_token_id is not None else (eos if eos is not None else 0)
        if isinstance(pad, bool) or not isinstance(pad, int) or not 0 <= pad < self.vocab_size:
            raise ValueError(f"{who}: pad_token_id={pad!r} must be a token of the vocabulary, [0, {self.vocab_size}): a "
                             f"finished row's padding goes through the model like any token")
        dev = input_ids.device
        self.eval()
        self._check_steppable(who)
        with torch.no_grad():
            if state is None:
                if seed is None:
                    seed = int(torch.randint(0, 1 << 62, (1,)).item())
                state = self.new_state(B, seed=seed, stream_ids=stream_ids)
                turn = input_ids
            else:
                if stream_ids is not None:
                    stream_ids, state.streams = _zone_streams(who, stream_ids, B, dev)
                turn = start_turn(state, input_ids, seed, stream_ids)
            generated = torch.empty(B, S + max_new_tokens, dtype=torch.int64, device=dev)
            generated[:, :S] = input_ids
            new = generated[:, S:]
            sampling = dict(penalty=repetition_penalty, penalty_rule=repetition_rule, temperature=temperature,
                            top_k=top_k, top_p=top_p)
            n = decode_loop(self.prefill(turn, state)[:, -1], state, new, sampling, eos, pad, sync_every,
                            lambda column: self.step(column, state), retire=False)
            if return_state:
                state.pending = new[:, n - 1].clone()
                state.finished.zero_()
                return generated[:, :S + n], state
            return generated[:, :S + trim_to_last_finish(new[:, :n], eos)]

    def setup_moe_router(self, *args, **kwargs):
        pass

    def forward_async(self, *args, **kwargs):
        raise DeprecationWarning("MoELanguageZone.forward_async is gone: forward() runs on the GPU")
