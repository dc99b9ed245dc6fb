"""``MoELanguageZone`` decoding on the GPU: the seeded ``forward`` against the composition of its public parts, a row's
``step`` alone and in the batch, determinism, ``prefill`` + ``step`` (through ``generate``) against the loop that
recomputes the seeded ``forward`` over the growing context -- greedy and sampled, also across a ``return_state`` /
``state=`` second turn --, EOS handling and the absence of a host sync in ``step``.

The zone: vocab 97, embed 32, hidden 64, moe_hidden 16, 4 experts, k = 2; B = 3, prompts of 7, 12 new tokens; the second
turn feeds 4 more tokens and generates 6.

The step's currents come from ``ops.row_linear`` and the forward's from a library GEMM: two orders of the same sum, and a
spike is a ``floor``.  So the comparison first ASSERTS, on the recompute side's own intermediates at the committed seeds,
that no decision is open:
  * no encoder or decoder neuron's ``n = v / (theta + 1e-6)`` lies within its tolerance of a deciding integer 1 .. L.  The
    tolerance: two orders of the current's sum differ by at most ``dh = 2 (K + 8) 2^-24 (sum_k |x_k W_k| + |b|)`` ("Row
    linear"'s bound, once per side); the potential carries it on as ``dv_t = decay dv_{t-1} + dh_t`` (equal spikes
    subtract equal amounts), plus ``8 2^-24 (|v| + |h|)`` for the roundings of the step's own ops on slightly different
    operands; ``tol = dv_t / (theta + 1e-6)``.  ``n`` comes from an fp64 run of the GIF rule on the side's fp32
    currents, whose spikes must be the kernel's;
  * no bridge ``q`` lies within twice its derived bound (tests/poisson_bridge_rule.py: once per side) of its uniform;
  * no sampler decision lies within the margin tests/test_gpu_generate.py uses, ``1e-4 max|logit|``: greedy the top-2
    gap; sampled the gap of the two best draw keys, of the k-th and (k + 1)-th logit and the nucleus boundary.
Then it demands equal tokens AND equal encoder / decoder spikes at every position.  The seeds were picked so that the
recompute side passes the precondition by itself; they and the smallest margins found are in
``profiles/zone_generate_parity_counts.json``."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import poisson_bridge_rule as RULE

pytestmark = pytest.mark.gpu

V, EMBED, HIDDEN, MOE_HIDDEN, EXPERTS, TOP_K = 97, 32, 64, 16, 4, 2
B, S, NEW, TURN, NEW2 = 3, 7, 12, 4, 6
OPEN = 1e-4
E24 = 2.0 ** -24
MODEL_SEED, PROMPT_SEED = 0, 7
GEN_SEEDS = {"greedy": 21, "sampled": 117}
SAMPLING = {"greedy": dict(temperature=0.0, repetition_penalty=1.2),
            "sampled": dict(temperature=0.8, top_k=20, top_p=0.9, repetition_penalty=1.2)}

_ZONES = {}


def _zone(dev, seed=MODEL_SEED):
    """One zone per seed, built once and left unchanged."""
    if seed not in _ZONES:
        from aura_snn_rag_amd import MoELanguageZone
        torch.manual_seed(seed)
        zone = MoELanguageZone(V, EMBED, HIDDEN, num_experts=EXPERTS, top_k=TOP_K, moe_hidden_dim=MOE_HIDDEN)
        with torch.no_grad():
            zone.moe_router.gate_proj.weight.mul_(100.0)          # routing decisions far from ties
            zone.encoder.linear.weight.mul_(4.0)                  # both populations spike
            zone.decoder.linear.weight.mul_(4.0)
            zone.output_proj.weight.mul_(2.0)
        _ZONES[seed] = zone.to(dev).eval()
    return _ZONES[seed]


def _prompts(dev, seed=PROMPT_SEED, width=S):
    return torch.randint(0, V, (B, width), generator=torch.Generator().manual_seed(seed)).to(dev)


def _parts(zone, ctx, seed, stream_ids=None, start=0, state=None):
    """The seeded forward from its public parts, with every intermediate the margins need."""
    from aura_snn_rag_amd import ops
    Bc, Sc = ctx.shape
    emb = zone.embeddings(ctx)
    spikes, _ = zone.encoder(emb, None if state is None else state.encoder)
    moe = zone.route_experts(zone.spike_to_continuous(spikes.reshape(Bc * Sc, 1, HIDDEN)))
    proj = zone.continuous_to_spike.proj
    streams = list(range(Bc)) if stream_ids is None else stream_ids
    rate, q = ops.poisson_rate(moe.expert_outputs, proj.weight.detach(), proj.bias.detach(), T=10, seed=seed,
                               streams=streams, rows_per_stream=Sc, start=start, return_probs=True)
    rate = rate.view(Bc, Sc, HIDDEN)
    decoded, _ = zone.decoder(rate, None if state is None else state.decoder)
    return dict(emb=emb, enc_spikes=spikes, x=moe.expert_outputs, q=q, rate=rate, dec_spikes=decoded,
                logits=zone.output_proj(decoded), streams=streams)


def _gif_margin(neuron, x, spikes):
    """The smallest ``|n - deciding integer| - tol`` over every neuron and position of one population, from an fp64 run
    of the GIF rule on the fp32 currents of ``x`` [B, S, K]; asserts that the run's spikes are ``spikes``."""
    W, b = neuron.linear.weight.detach().double(), neuron.linear.bias.detach().double()
    h = neuron.currents(x).double()                                  # the side's own fp32 currents
    K = x.shape[-1]
    dh = 2.0 * (K + 8) * E24 * (x.double().abs() @ W.abs().T + b.abs())
    decay, L, alpha, thr = float(neuron.decay), int(neuron.L), float(neuron.alpha), float(neuron.threshold)
    v = torch.zeros_like(h[:, 0])
    theta = torch.full_like(v, thr)
    dv = torch.zeros_like(v)
    ints = torch.arange(1, L + 1, dtype=torch.float64, device=h.device)
    worst = float("inf")
    for t in range(h.shape[1]):
        v = v * decay + h[:, t]
        cl = L * theta * 2.0
        v = torch.minimum(torch.maximum(v, -cl), cl)
        dv = decay * dv + dh[:, t] + 8.0 * E24 * (v.abs() + h[:, t].abs())
        n = v / (theta + 1e-6)
        s = torch.clamp(torch.floor(n), 0, L)
        assert torch.equal(s.float(), spikes[:, t]), f"the fp64 rule's spikes are not the kernel's at position {t}"
        dist = (n[..., None] - ints).abs().min(dim=-1).values
        worst = min(worst, float((dist - dv / (theta + 1e-6)).min()))
        v = v - s * theta
        if alpha > 0:
            theta = theta + alpha * s - alpha * (theta - thr)
    return worst


def _bridge_margin(zone, p, seed, start=0):
    """The smallest ``|q - u| - 2 bound`` over every (row, timestep, channel)."""
    proj = zone.continuous_to_spike.proj
    x = p["x"].cpu().numpy()
    _, bound = RULE.probability64(x, proj.weight.detach().cpu().numpy(), proj.bias.detach().cpu().numpy())
    N = x.shape[0]
    s, pos = RULE.row_addresses(N, p["streams"], N // len(p["streams"]), start)
    u = RULE.uniforms(HIDDEN, 10, s, pos, seed).astype(np.float64)
    q = p["q"].cpu().numpy().astype(np.float64)
    return float((np.abs(q[:, None, :] - u) - 2.0 * bound[:, None, :]).min())


def _sampler_margin(lg, seen, seed, step, sampling):
    """``(tokens, the smallest relative gap of the row's decisions)`` of the recompute side at one step."""
    from aura_snn_rag_amd import ops
    scale = float(lg.abs().max())
    if sampling["temperature"] == 0.0:
        tok = ops.sample_next(lg, seen=seen.clone(), penalty=sampling["repetition_penalty"], temperature=0.0, seed=seed,
                              step=step)
        z = torch.where(seen.bool(), lg / sampling["repetition_penalty"], lg)
        top2 = torch.topk(z, 2, dim=-1).values
        return tok, float(((top2[:, 0] - top2[:, 1]) / scale).min())
    K, P = sampling["top_k"], sampling["top_p"]
    kw = dict(penalty=sampling["repetition_penalty"], temperature=sampling["temperature"], top_p=P, seed=seed, step=step,
              return_candidates=True)
    tok, c = ops.sample_next(lg, seen=seen.clone(), top_k=K, **kw)
    _, c1 = ops.sample_next(lg, seen=seen.clone(), top_k=K + 1, **kw)
    d2 = torch.topk(c["d"], 2, dim=-1).values
    total = c["cum"][:, -1:]
    gaps = torch.stack([(d2[:, 0] - d2[:, 1]) / scale, (c1["z"][:, K - 1] - c1["z"][:, K]) / scale,
                        ((c["cum"][:, :-1] - P * total).abs() / total).min(dim=-1).values])
    return tok, float(gaps.min())


def _recompute(zone, ctx, n, seed, sampling, step0=0):
    """The loop without a state: ``n`` tokens after ``ctx`` from the seeded forward over the growing context.  Returns
    the tokens, the smallest sampler gap and the parts of the last, longest forward."""
    gap = float("inf")
    for t in range(n):
        logits, _ = zone(ctx, seed=seed)
        seen = torch.zeros(B, V, dtype=torch.uint8, device=ctx.device).scatter_(1, ctx, 1)
        tok, g = _sampler_margin(logits[:, -1], seen, seed, step0 + t, sampling)
        gap = min(gap, g)
        ctx = torch.cat([ctx, tok[:, None]], dim=1)
    return ctx, gap


class _Spikes:
    """Records what the stepped side computes: the prefill's populations and every step's."""

    def __init__(self, zone, monkeypatch):
        self.enc, self.dec = [], []
        forward, gif_step = zone.forward, type(zone)._gif_step

        def seeded_forward(*a, **k):
            logits, info = forward(*a, **k)
            self.enc.append(info["encoder_spikes"])
            self.dec.append(info["decoder_spikes"])
            return logits, info

        def step(neuron, x, pair):
            out = gif_step(neuron, x, pair)
            (self.enc if neuron is zone.encoder else self.dec).append(out[:, None])
            return out

        monkeypatch.setattr(zone, "forward", seeded_forward)
        monkeypatch.setattr(zone, "_gif_step", step)

    def take(self):
        enc, dec = torch.cat(self.enc, dim=1), torch.cat(self.dec, dim=1)
        self.enc, self.dec = [], []
        return enc, dec


def run_case(dev, monkeypatch, kind, model_seed=MODEL_SEED, prompt_seed=PROMPT_SEED, gen_seed=None):
    """Both sides of one comparison and every margin; asserts nothing about them (the seed search calls this too)."""
    zone = _zone(dev, model_seed)
    sampling = SAMPLING[kind]
    seed = GEN_SEEDS[kind] if gen_seed is None else gen_seed
    ids, turn = _prompts(dev, prompt_seed), _prompts(dev, prompt_seed + 1, TURN)
    with torch.no_grad():
        # the recompute side: two turns, then its own intermediates over the whole history
        first, gap1 = _recompute(zone, ids, NEW, seed, sampling)
        history = torch.cat([first, turn], dim=1)
        second, gap2 = _recompute(zone, history, NEW2, seed, sampling, step0=NEW)
        p = _parts(zone, second, seed)
        margins = dict(encoder=_gif_margin(zone.encoder, p["emb"], p["enc_spikes"]),
                       decoder=_gif_margin(zone.decoder, p["rate"], p["dec_spikes"]),
                       bridge=_bridge_margin(zone, p, seed), sampler=min(gap1, gap2))
        # the stepped side
        rec = _Spikes(zone, monkeypatch)
        got1, state = zone.generate(ids, max_new_tokens=NEW, seed=seed, return_state=True, **sampling)
        got2 = zone.generate(turn, max_new_tokens=NEW2, state=state, **sampling)
        enc, dec = rec.take()
        monkeypatch.undo()
    fed = second.shape[1] - 1                                        # the last token never goes through the model
    return dict(margins=margins, seed=seed,
                tokens=torch.equal(got1, first) and torch.equal(got2, second[:, first.shape[1]:]),
                encoder=enc.shape[1] == fed and torch.equal(enc, p["enc_spikes"][:, :fed]),
                decoder=dec.shape[1] == fed and torch.equal(dec, p["dec_spikes"][:, :fed]),
                spikes=(float(p["enc_spikes"].mean()), float(p["dec_spikes"].mean())), got=(got1, got2))


# ------------------------------------------------------------------------------------------------ the tests
def test_the_seeded_forward_is_the_composition_of_its_parts(dev):
    zone = _zone(dev)
    ids = _prompts(dev, 3, 19)
    with torch.no_grad():
        logits, info = zone(ids, seed=5, stream_ids=[4, 9, 2], start=3, keep_on_device=True)
        p = _parts(zone, ids, 5, stream_ids=[4, 9, 2], start=3)
        again, _ = zone(ids, seed=5, stream_ids=torch.tensor([4, 9, 2], device=dev), start=3)
        other, _ = zone(ids, seed=6, stream_ids=[4, 9, 2], start=3)
    assert logits.shape == (B, 19, V) and torch.equal(logits, p["logits"]) and torch.equal(again, logits)
    assert torch.equal(info["encoder_spikes"], p["enc_spikes"]) and torch.equal(info["decoder_spikes"], p["dec_spikes"])
    assert not torch.equal(other, logits)
    assert float(p["enc_spikes"].mean()) > 0.01 and float(p["dec_spikes"].mean()) > 0.01, "both populations spike"
    # the bridge's part alone: rate_code is the mean of the module's seeded train
    c2s = zone.continuous_to_spike
    train = c2s(p["x"], seed=5, streams=[4, 9, 2], rows_per_stream=19, start=3)
    assert torch.equal(train.mean(dim=1).view(B, 19, HIDDEN), p["rate"])
    # the unseeded forward still draws from torch's generator
    with torch.no_grad():
        torch.manual_seed(1)
        a, extra = zone(ids)
        torch.manual_seed(1)
        b, _ = zone(ids)
        c, _ = zone(ids)
    assert torch.equal(a, b) and not torch.equal(a, c) and set(extra) == {"probs"}


def test_a_rows_step_is_the_same_alone_and_in_the_batch(dev):
    zone = _zone(dev)
    ids = _prompts(dev, 5, 9)
    state = zone.new_state(B, seed=3, stream_ids=[6, 1, 8])
    zone.prefill(ids[:, :6], state)
    # the rows start from the batch's own prefill (a library GEMM, whose last bits may depend on the batch)
    rows = []
    for b in range(B):
        alone = zone.new_state(1, seed=3, stream_ids=[[6, 1, 8][b]])
        alone.encoder = tuple(t[b:b + 1].clone() for t in state.encoder)
        alone.decoder = tuple(t[b:b + 1].clone() for t in state.decoder)
        alone.position.copy_(state.position[b:b + 1])
        alone.length = state.length
        rows.append(alone)
    together = [zone.step(ids[:, t], state) for t in range(6, 9)]
    for b, alone in enumerate(rows):
        for t in range(6, 9):
            got = zone.step(ids[b:b + 1, t], alone)
            assert torch.equal(got.view(torch.int32), together[t - 6][b:b + 1].view(torch.int32)), (b, t)
        for x, y in zip(alone.encoder + alone.decoder, state.encoder + state.decoder):
            assert torch.equal(x, y[b:b + 1])
    assert state.position.tolist() == [9, 9, 9] and state.length == 9


def test_one_seed_one_generation(dev):
    zone = _zone(dev)
    ids = _prompts(dev)
    kw = dict(max_new_tokens=NEW, **SAMPLING["sampled"])
    a, b, c = zone.generate(ids, seed=7, **kw), zone.generate(ids, seed=7, **kw), zone.generate(ids, seed=8, **kw)
    assert a.shape == (B, S + NEW) and a.dtype == torch.int64 and torch.equal(a[:, :S], ids)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # a row alone with its stream generates what it generates in the batch
    alone = zone.generate(ids[1:2], seed=7, stream_ids=[1], **kw)
    assert torch.equal(alone, a[1:2])
    torch.manual_seed(5)
    d = zone.generate(ids, **kw)
    torch.manual_seed(5)
    assert torch.equal(d, zone.generate(ids, **kw))


@pytest.mark.parametrize("kind", ["greedy", "sampled"])
def test_prefill_and_steps_equal_the_recompute_loop_over_two_turns(dev, monkeypatch, kind):
    r = run_case(dev, monkeypatch, kind)
    m = r["margins"]
    print(f"{kind} seed={r['seed']}: margins {m}; mean spikes (encoder, decoder) {r['spikes']}; tokens {r['tokens']}, "
          f"encoder {r['encoder']}, decoder {r['decoder']}")
    helpers.record_parity(f"zone generate {kind}", int(r["tokens"]), 1, model_seed=MODEL_SEED, prompt_seed=PROMPT_SEED,
                          seed=r["seed"], encoder_margin=m["encoder"], decoder_margin=m["decoder"],
                          bridge_margin=m["bridge"], sampler_gap=m["sampler"])
    assert r["spikes"][0] > 0.01 and r["spikes"][1] > 0.01, "both populations spike"
    assert m["encoder"] > 0 and m["decoder"] > 0, "a neuron of the recompute side is within its tolerance of an integer"
    assert m["bridge"] > 0, "a q of the recompute side is within its tolerance of its uniform"
    assert m["sampler"] >= OPEN, "a sampler decision of the recompute side is open"
    assert r["tokens"] and r["encoder"] and r["decoder"]


def test_eos_pads_trims_and_stops(dev):
    zone = _zone(dev)
    ids = _prompts(dev)
    kw = dict(max_new_tokens=NEW, seed=GEN_SEEDS["sampled"], **SAMPLING["sampled"])
    free = zone.generate(ids, **kw)
    new = free[:, S:].tolist()
    eos = new[0][2]                                                 # row 0's third token
    firsts = [row.index(eos) if eos in row else None for row in new]
    got = zone.generate(ids, eos_token_id=eos, pad_token_id=96, sync_every=2, **kw)
    last = NEW if None in firsts else max(firsts) + 1
    assert got.shape == (B, S + last)
    for b, f in enumerate(firsts):
        keep = last if f is None else f + 1
        assert got[b, S:S + keep].tolist() == new[b][:keep], b
        assert (got[b, S + keep:] == 96).all(), b
    alone = zone.generate(ids[:1], eos_token_id=eos, sync_every=1, **kw)
    assert alone.shape == (1, S + firsts[0] + 1) and int(alone[0, -1]) == eos
    # with return_state the result is not trimmed and the state has been through every column but the last
    kept, state = zone.generate(ids[:1], eos_token_id=eos, sync_every=1, return_state=True, **kw)
    assert torch.equal(kept, alone) and state.length == kept.shape[1] - 1 and int(state.finished.sum()) == 0


def test_a_step_does_not_sync_with_the_host(dev):
    zone = _zone(dev)
    ids = _prompts(dev)
    state = zone.new_state(B, seed=1)
    zone.prefill(ids, state)
    zone.step(ids[:, 0], state)                                      # the expert table is built (one copy) before
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = zone.step(ids[:, 1], state)
        tok = torch.empty(B, dtype=torch.int64, device=dev)
        from aura_snn_rag_amd import ops
        ops.sample_next(logits, seen=state.seen, finished=state.finished, seed=1, step=0, out=tok)
        logits = zone.step(tok, state)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert logits.shape == (B, V) and state.position.tolist() == [S + 3] * B
