"""The Poisson bridge and the zone's decoding on the CPU: the generator's known answers and counter layout, the
distribution the rule draws (tests/poisson_bridge_rule.py), the host-side refusals of ``ops.poisson_rate``, and the
plumbing of ``ContinuousToSpikeBridge`` and ``MoELanguageZone`` (seeded forward, state, prefill, step, generate) on CPU
stand-ins of the ops (tests/cpu_stub_bridge.py, cpu_stub_moe.py, cpu_stub_row_linear.py, cpu_stub_sampling.py)."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import cpu_stub_bridge as BRIDGE
from tests import cpu_stub_moe as MOE
from tests import cpu_stub_row_linear as ROWLIN
from tests import cpu_stub_sampling as SAMPLING
from tests import poisson_bridge_rule as RULE

F32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the generator
def test_all_four_philox_words_against_known_answers():
    """the Random123 vectors of Philox4x32-10, with the seed as the key"""
    for counter, seed, want in (
            ((0, 0, 0, 0), 0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((F32, F32, F32, F32), (1 << 64) - 1, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), 0x299f31d0a4093822,
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in RULE.words(*counter, seed)) == want


def test_the_counter_layout_every_field_reaches_the_words():
    base = dict(c=3, j=1, p=7, s=2, seed=11)
    w0 = [int(w) for w in RULE.words(**base)]
    assert [int(w) for w in RULE.words(**base)] == w0
    for name, other in (("c", 4), ("j", 0), ("p", 8), ("s", 3), ("seed", 12), ("seed", 11 + (1 << 32))):
        w1 = [int(w) for w in RULE.words(**dict(base, **{name: other}))]
        assert all(a != b for a, b in zip(w0, w1)), name
    # uniforms(): timestep t of row (s, p), channel c is word t % 4 of counter (c, t // 4, p, s)
    u = RULE.uniforms(H=5, T=7, stream=np.array([2, 9]), position=np.array([7, 0]), seed=11)
    assert u.shape == (2, 7, 5) and u.dtype == np.float32
    for (n, t, c), (s, p) in (((0, 5, 3), (2, 7)), ((1, 0, 4), (9, 0)), ((1, 6, 0), (9, 0))):
        assert u[n, t, c] == RULE.uniform_of(RULE.words(c, t // 4, p, s, 11)[t % 4])
    assert u.min() > 0.0 and u.max() < 1.0
    # row addressing: (S, start) and (1, start[b] = position) over renumbered streams name the same (s, p)
    s1, p1 = RULE.row_addresses(6, streams=[4, 8], rows_per_stream=3, start=10)
    s2, p2 = RULE.row_addresses(6, streams=[4, 4, 4, 8, 8, 8], rows_per_stream=1, start=[10, 11, 12, 10, 11, 12])
    assert s1.tolist() == s2.tolist() == [4, 4, 4, 8, 8, 8] and p1.tolist() == p2.tolist() == [10, 11, 12] * 2
    s3, p3 = RULE.row_addresses(3)
    assert s3.tolist() == [0, 1, 2] and p3.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ the distribution
CHI2_999 = {8: 26.12}                                           # the 99.9 % quantile, as tests/test_host_replay.py uses


@pytest.mark.parametrize("seed", [1, 20240607, (1 << 63) + 5])
def test_spike_counts_follow_the_binomial(seed):
    """8 rows x 4096 channels at T = 10, q = 0.3: the counts against Binomial(10, q') with q' the exact probability of
    ``u < q`` on the uniforms' grid.  Cells 0 .. 7 and 8+ (expected 52): 8 degrees of freedom."""
    T, H, N = 10, 4096, 8
    q = np.float32(0.3)
    u = RULE.uniforms(H, T, stream=np.arange(N), position=np.arange(N) * 3, seed=seed)
    counts = RULE.spikes_of(np.full((N, H), q), u).sum(axis=1).astype(np.int64).ravel()
    exact = math.ceil((float(q) * 2.0 ** 24 - 1.0) / 2.0) / 2.0 ** 23          # #{k: (2k + 1) / 2^24 < q} / 2^23
    assert abs(exact - 0.3) < 1e-6
    pk = np.array([math.comb(T, k) * exact ** k * (1 - exact) ** (T - k) for k in range(T + 1)])
    expect = np.concatenate([pk[:8], [pk[8:].sum()]]) * counts.size
    seen = np.bincount(np.minimum(counts, 8), minlength=9)
    assert expect.min() > 5
    chi2 = float(np.sum((seen - expect) ** 2 / expect))
    print(f"seed={seed}: chi2={chi2:.2f}")
    assert chi2 < CHI2_999[8]


@pytest.mark.parametrize("seed", [1, 20240607, (1 << 63) + 5])
def test_neighbouring_draws_are_uncorrelated(seed):
    """Lag-1 correlation of the centred uniforms across t, across c and across p: for n independent pairs it is normal
    with deviation 1 / sqrt(n); the bar is the two-sided 99.9 % quantile, 3.29 / sqrt(n)."""
    T, H, P = 64, 512, 32
    u = RULE.uniforms(H, T, stream=np.full(P, 5), position=np.arange(P), seed=seed).astype(np.float64) - 0.5
    for name, a, b in (("t", u[:, :-1], u[:, 1:]), ("c", u[:, :, :-1], u[:, :, 1:]), ("p", u[:-1], u[1:])):
        r = float(np.mean(a * b) * 12.0)
        print(f"seed={seed} lag-1 across {name}: r={r:.5f} n={a.size}")
        assert abs(r) < 3.29 / math.sqrt(a.size), name
    assert abs(float(u.mean())) < 3.29 / math.sqrt(12.0 * u.size)


def test_the_rate_is_the_device_means_product_and_a_nan_never_spikes():
    q = np.array([[np.nan, 0.0, 1.0, 0.5]], dtype=np.float32)
    u = RULE.uniforms(4, 10, np.array([0]), np.array([0]), 3)
    s = RULE.spikes_of(q, u)
    assert s[0, :, 0].sum() == 0 and s[0, :, 1].sum() == 0 and s[0, :, 2].sum() == 10
    assert RULE.rate_of(s)[0, 2] == 1.0 and RULE.rate_of(s).dtype == np.float32
    nine = np.ones((1, 10, 1), dtype=np.float32)
    nine[0, 0, 0] = 0
    # count * fl(1 / T), not count / T: 9 of 10 is one of the places where the two differ
    assert RULE.rate_of(nine)[0, 0] == np.float32(9.0) * (np.float32(1.0) / np.float32(10.0)) != np.float32(0.9)
    assert RULE.dot_order(12) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 9, 10, 11]
    # the restatement lies within half the derived bound of the fp64 probability
    g = np.random.default_rng(0)
    x, W, b = (g.standard_normal(s).astype(np.float32) for s in ((9, 100), (7, 100), (7,)))
    q64, bound = RULE.probability64(x, W, b)
    assert (np.abs(RULE.probability32(x, W, b).astype(np.float64) - q64) <= 0.5 * bound).all()


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_bad_arguments_are_refused_before_the_library_is_loaded(monkeypatch):
    from aura_snn_rag_amd import _lib, ops
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    x, W, b = torch.zeros(6, 8), torch.zeros(5, 8), torch.zeros(5)
    ok = dict(T=10, seed=0)
    with pytest.raises(ops.AuraDeviceError):
        ops.poisson_rate(x, W, b, **ok)
    shifted = torch.zeros(6 * 8 + 1)[1:].view(6, 8)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16
    for bad in (lambda: ops.poisson_rate(torch.zeros(6, 6), torch.zeros(5, 6), b, **ok),              # K % 4
                lambda: ops.poisson_rate(torch.zeros(6, 260), torch.zeros(5, 260), b, **ok),          # K > 256
                lambda: ops.poisson_rate(x, W, b, T=0, seed=0),
                lambda: ops.poisson_rate(x, W, b, T=65, seed=0),
                lambda: ops.poisson_rate(x, torch.zeros(0, 8), torch.zeros(0), **ok),                  # H = 0
                lambda: ops.poisson_rate(x, torch.zeros(4097, 8), torch.zeros(4097), **ok),            # H > 4096
                lambda: ops.poisson_rate(x, torch.zeros(5, 12), b, **ok),                              # W's width
                lambda: ops.poisson_rate(x, W, torch.zeros(4), **ok),                                  # the bias
                lambda: ops.poisson_rate(shifted, W, b, **ok),                                         # misaligned x
                lambda: ops.poisson_rate(x, W, b, start=-1, **ok),
                lambda: ops.poisson_rate(x, W, b, start=1 << 31, **ok),
                lambda: ops.poisson_rate(x, W, b, streams=[0, 1], rows_per_stream=3, start=(1 << 31) - 2, **ok),
                lambda: ops.poisson_rate(x, W, b, streams=[0, 1], **ok),                               # no rows_per_stream
                lambda: ops.poisson_rate(x, W, b, streams=[0, 1], rows_per_stream=4, **ok),            # N % S
                lambda: ops.poisson_rate(x, W, b, streams=[0, 1, 2], rows_per_stream=3, **ok),         # B streams
                lambda: ops.poisson_rate(x, W, b, streams=[0, 1 << 32], rows_per_stream=3, **ok),
                lambda: ops.poisson_rate(x, W, b, start=torch.zeros(5, dtype=torch.int32), **ok),      # [B] = [6]
                lambda: ops.poisson_rate(x, W, b, start=torch.zeros(6, dtype=torch.int64), **ok),
                lambda: ops.poisson_rate(x, W, b, T=10, seed=-1),
                lambda: ops.poisson_rate(x, W, b, T=10, seed=1 << 64),
                lambda: ops.poisson_rate(x, W, b, out=torch.zeros(6, 4), **ok),
                lambda: ops.poisson_rate(x.t().contiguous().t(), torch.zeros(5, 6), b, **ok)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.poisson_rate(x.double(), W, b, **ok), lambda: ops.poisson_rate(x.bfloat16(), W, b, **ok),
                lambda: ops.poisson_rate(x, W, b, T=10.0, seed=0), lambda: ops.poisson_rate(x, W, b, start=0.0, **ok)):
        with pytest.raises(TypeError):
            bad()
    # the last allowed start passes the host checks and reaches the device check
    with pytest.raises(ops.AuraDeviceError):
        ops.poisson_rate(x, W, b, streams=[0, 1], rows_per_stream=3, start=(1 << 31) - 3, **ok)


# ------------------------------------------------------------------------------------------------ the bridge on the stub
def _bridge(encoding="poisson", dims=(8, 20), seed=0):
    from aura_snn_rag_amd.core.language_zone.spike_bridge import ContinuousToSpikeBridge
    torch.manual_seed(seed)
    return ContinuousToSpikeBridge(dims[0], dims[1], encoding=encoding)


def test_the_unseeded_bridge_is_the_torch_rand_path_bit_for_bit(monkeypatch):
    BRIDGE.install(monkeypatch)
    bridge = _bridge()
    x = torch.randn(7, 8)
    torch.manual_seed(5)
    got = bridge(x)
    torch.manual_seed(5)
    feat = bridge.proj(x)
    draw = torch.rand(7, 10, 20)
    assert torch.equal(got, (draw < torch.sigmoid(feat).unsqueeze(1)).to(x.dtype))
    assert BRIDGE.CALLS["poisson_rate"] == 0
    with pytest.raises(ValueError):
        bridge(x, start=3)


def test_rate_code_is_the_mean_of_the_seeded_train_and_both_are_reproducible(monkeypatch):
    BRIDGE.install(monkeypatch)
    bridge = _bridge()
    x = torch.randn(6, 8)
    kw = dict(seed=9, streams=[3, 5], rows_per_stream=3, start=4)
    train = bridge(x, **kw)
    assert train.shape == (6, 10, 20) and set(train.unique().tolist()) <= {0.0, 1.0}
    rate = bridge.rate_code(x, **kw)
    assert torch.equal(rate, train.mean(1))
    assert torch.equal(train, bridge(x, **kw)) and not torch.equal(train, bridge(x, **dict(kw, seed=10)))
    assert not rate.requires_grad
    # a row alone, with its own stream and position, draws what it draws in the batch
    alone = bridge(x[4:5], seed=9, streams=[5], rows_per_stream=1, start=5)
    assert torch.equal(alone[0], train[4])
    for other in (_bridge("temporal"), _bridge("rate"), _bridge(dims=(8, 8))):
        with pytest.raises(ValueError):
            other(x, seed=1)
        with pytest.raises(ValueError):
            other.rate_code(x, seed=1)


# ------------------------------------------------------------------------------------------------ the zone on the stubs
def _cpu_gif(monkeypatch):
    """The GIF loop of the encoder and the decoder in torch on the CPU (the rule of ``ops.gif_run`` in fp32)."""
    from aura_snn_rag_amd import ops
    from aura_snn_rag_amd.core.language_zone import gif_neuron

    def gif_run(h, out, v, theta, decay, L, alpha, threshold, T, time_invariant=False, mean_out=False):
        assert not time_invariant and not mean_out
        for t in range(T):
            v.mul_(decay).add_(h[:, t])
            cl = L * theta * 2.0
            v.copy_(torch.minimum(torch.maximum(v, -cl), cl))
            s = torch.clamp(torch.floor(v / (theta + 1e-6)), 0, L)
            v.sub_(s * theta)
            if alpha > 0:
                theta.copy_(theta + alpha * s - alpha * (theta - threshold))
            out[:, t] = s

    monkeypatch.setattr(ops, "gif_run", gif_run)
    monkeypatch.setattr(gif_neuron, "_check_input", lambda x, who: None)


def _install(monkeypatch):
    for stub in (MOE, BRIDGE, ROWLIN, SAMPLING):
        stub.install(monkeypatch)
    _cpu_gif(monkeypatch)


def _zone(seed=0, **kw):
    from aura_snn_rag_amd.core.language_zone.moe_language_zone import MoELanguageZone
    torch.manual_seed(seed)
    args = dict(vocab_size=50, embed_dim=12, hidden_dim=16, num_experts=4, top_k=2, moe_hidden_dim=8)
    args.update(kw)
    zone = MoELanguageZone(**args)
    with torch.no_grad():
        zone.moe_router.gate_proj.weight.mul_(100.0)
        zone.encoder.linear.weight.mul_(4.0)                   # currents large enough for both populations to spike
        zone.decoder.linear.weight.mul_(4.0)
    return zone.eval()


def test_the_unseeded_forward_is_what_it_was(monkeypatch):
    _install(monkeypatch)
    zone = _zone()
    ids = torch.randint(0, 50, (2, 5))
    with torch.no_grad():
        torch.manual_seed(3)
        logits, extra = zone(ids)
        torch.manual_seed(3)
        spikes, _ = zone.encoder(zone.embeddings(ids))
        moe = zone.route_experts(zone.spike_to_continuous(spikes.reshape(10, 1, 16)))
        train = zone.continuous_to_spike(moe.expert_outputs)
        decoded, _ = zone.decoder(train.view(2, 5, 10, 16).mean(dim=2))
        want = zone.output_proj(decoded)
    assert torch.equal(logits, want) and set(extra) == {"probs"}
    assert BRIDGE.CALLS["poisson_rate"] == 0
    with pytest.raises(ValueError):
        zone(ids, start=2)


def test_the_seeded_forward_is_the_composition_of_its_parts(monkeypatch):
    _install(monkeypatch)
    zone = _zone()
    ids = torch.randint(0, 50, (2, 5))
    with torch.no_grad():
        logits, extra = zone(ids, seed=7, stream_ids=[4, 9], start=3)
        spikes, _ = zone.encoder(zone.embeddings(ids))
        moe = zone.route_experts(zone.spike_to_continuous(spikes.reshape(10, 1, 16)))
        train = zone.continuous_to_spike(moe.expert_outputs, seed=7, streams=[4, 9], rows_per_stream=5, start=3)
        decoded, _ = zone.decoder(train.view(2, 5, 10, 16).mean(dim=2))
    assert torch.equal(logits, zone.output_proj(decoded))
    assert torch.equal(extra["encoder_spikes"], spikes) and torch.equal(extra["decoder_spikes"], decoded)
    assert spikes.sum() > 0 and decoded.sum() > 0, "the fixture's populations spike"
    assert BRIDGE.LAST["S"] == 5 and BRIDGE.LAST["T"] == 10
    with torch.no_grad():
        again, _ = zone(ids, seed=7, stream_ids=[4, 9], start=3)
        other, _ = zone(ids, seed=8, stream_ids=[4, 9], start=3)
    assert torch.equal(again, logits) and not torch.equal(other, logits)


def test_prefill_in_two_pieces_is_prefill_of_the_whole(monkeypatch):
    """The state plumbing: (v, theta) of both populations, the position and the seen mask carry over."""
    _install(monkeypatch)
    zone = _zone()
    ids = torch.randint(0, 50, (3, 9))
    whole = zone.new_state(3, seed=21, stream_ids=[7, 8, 2])
    want = zone.prefill(ids, whole)
    parts = zone.new_state(3, seed=21, stream_ids=[7, 8, 2])
    assert parts.encoder[1].unique().tolist() == [1.0] and parts.position.dtype == torch.int32
    got = torch.cat([zone.prefill(ids[:, :4], parts), zone.prefill(ids[:, 4:], parts)], dim=1)
    assert torch.equal(got, want)
    for a, b in zip(whole.encoder + whole.decoder, parts.encoder + parts.decoder):
        assert torch.equal(a, b)
    assert parts.position.tolist() == [9, 9, 9] and parts.length == 9
    assert torch.equal(parts.seen, whole.seen) and int(parts.seen.sum()) == sum(len(set(r)) for r in ids.tolist())
    # one-token steps continue the same history: their positions, streams and state are the prefill's
    more = torch.randint(0, 50, (3, 2))
    want2 = zone.prefill(more, whole)
    calls = BRIDGE.CALLS["poisson_rate"]
    got2 = torch.stack([zone.step(more[:, i], parts) for i in range(2)], dim=1)
    assert BRIDGE.CALLS["poisson_rate"] == calls + 2 and BRIDGE.LAST["device_start"] and BRIDGE.LAST["S"] == 1
    assert parts.position.tolist() == [11, 11, 11]
    assert torch.allclose(got2, want2, atol=1e-5), "row_linear's stand-in sums as F.linear does, up to the GEMM's order"
    for a, b in zip(whole.encoder + whole.decoder, parts.encoder + parts.decoder):
        assert torch.allclose(a, b, atol=1e-5)


def _recompute(zone, ids, n, seed, step0=0, seen=None, **sampling):
    """The loop without a state: the seeded forward over the growing context, then the sampler."""
    from aura_snn_rag_amd import ops
    B = ids.shape[0]
    if seen is None:
        seen = torch.zeros(B, zone.vocab_size, dtype=torch.uint8)
        seen.scatter_(1, ids, 1)
    for i in range(n):
        with torch.no_grad():
            logits, _ = zone(ids, seed=seed)
        tok = ops.sample_next(logits[:, -1].contiguous(), seen=seen, seed=seed, step=step0 + i, **sampling)
        ids = torch.cat([ids, tok[:, None]], dim=1)
    return ids, seen


@pytest.mark.parametrize("sampling", [dict(temperature=0.0), dict(temperature=0.8, top_k=10, top_p=0.9)])
def test_generate_on_the_stubs_is_the_recompute_loop_also_over_a_second_turn(monkeypatch, sampling):
    _install(monkeypatch)
    zone = _zone()
    ids = torch.randint(0, 50, (2, 6))
    kw = dict(repetition_penalty=1.2, **sampling)
    out = zone.generate(ids, max_new_tokens=5, seed=13, **kw)
    want, _ = _recompute(zone, ids, 5, 13, penalty=1.2, **sampling)
    assert out.shape == (2, 11) and torch.equal(out, want)
    assert torch.equal(out, zone.generate(ids, max_new_tokens=5, seed=13, **kw))
    # a second turn from the returned state against the recompute loop over the whole history
    first, state = zone.generate(ids, max_new_tokens=3, seed=13, return_state=True, **kw)
    assert torch.equal(first, want[:, :9]) and torch.equal(state.pending, first[:, -1]) and state.length == 8
    turn = torch.randint(0, 50, (2, 4))
    second = zone.generate(turn, max_new_tokens=4, state=state, **kw)
    history = torch.cat([first, turn], dim=1)
    seen = torch.zeros(2, 50, dtype=torch.uint8).scatter_(1, history, 1)
    want2, _ = _recompute(zone, history, 4, 13, step0=3, seen=seen, penalty=1.2, **sampling)
    assert torch.equal(second, want2[:, 9:])


def test_generate_pads_trims_and_stops_at_eos(monkeypatch):
    _install(monkeypatch)
    zone = _zone()
    ids = torch.randint(0, 50, (2, 6))
    free = zone.generate(ids, max_new_tokens=8, temperature=0.0, seed=1)
    eos = int(free[0, 7])                                       # row 0's second new token
    at = free[0, 6:].tolist().index(eos)                        # (its first, should the two be equal)
    out = zone.generate(ids, max_new_tokens=8, temperature=0.0, seed=1, eos_token_id=eos, pad_token_id=49,
                        sync_every=1)
    new = out[:, 6:]
    assert torch.equal(new[0, :at + 1], free[0, 6:7 + at]) and (new[0, at + 1:] == 49).all()
    if eos not in free[1, 6:].tolist():
        assert out.shape == (2, 14) and torch.equal(new[1], free[1, 6:])
    alone = zone.generate(ids[:1], max_new_tokens=8, temperature=0.0, seed=1, eos_token_id=eos, sync_every=1)
    assert alone.shape == (1, 7 + at) and int(alone[0, -1]) == eos, "stops and trims at the row's EOS"
    late = zone.generate(ids[:1], max_new_tokens=8, temperature=0.0, seed=1, eos_token_id=eos, sync_every=5)
    assert torch.equal(late, alone), "the host's look every sync_every steps changes no token"


def test_the_generate_defaults_are_the_mixins():
    from aura_snn_rag_amd.core.language_zone.hippocampal_transformer import CachedDecodingMixin
    from aura_snn_rag_amd.core.language_zone.moe_language_zone import MoELanguageZone
    ours = inspect.signature(MoELanguageZone.generate).parameters
    theirs = inspect.signature(CachedDecodingMixin.generate).parameters
    shared = ("input_ids", "max_new_tokens", "temperature", "top_k", "top_p", "repetition_penalty", "repetition_rule",
              "seed", "eos_token_id", "pad_token_id", "sync_every", "stream_ids", "state", "return_state")
    for name in shared:
        assert ours[name].default is theirs[name].default or ours[name].default == theirs[name].default, name
        assert ours[name].kind == theirs[name].kind, name
    assert not {"capacity", "use_memory", "fused_step"} & set(ours)


def test_step_and_generate_refuse_what_they_do_not_compute(monkeypatch):
    from aura_snn_rag_amd.core.language_zone.gif_neuron import BalancedGIFNeuron
    _install(monkeypatch)
    zone = _zone()
    ids = torch.randint(0, 50, (2, 4))
    state = zone.new_state(2, seed=1)
    zone.prefill(ids, state)
    calls = dict(BRIDGE.CALLS)
    with pytest.raises(ValueError):
        zone.step(ids[:1, 0], state)                            # the state holds two rows
    with pytest.raises(TypeError):
        zone.step(ids[:, 0], None)
    with pytest.raises(ValueError):
        zone.step(torch.zeros(33, dtype=torch.int64), zone.new_state(33))
    with pytest.raises(ValueError):
        zone.generate(torch.zeros(33, 4, dtype=torch.int64), max_new_tokens=2)
    with pytest.raises(NotImplementedError):
        zone.generate(ids, max_new_tokens=2, lengths=[4, 3])
    with pytest.raises(NotImplementedError):
        zone.prefill(ids, state, lengths=[4, 3])
    with pytest.raises(ValueError):
        zone.generate(ids, max_new_tokens=2, state=state)       # not a state generate returned
    for bad in (dict(max_new_tokens=0), dict(sync_every=0), dict(seed=-1)):
        with pytest.raises(ValueError):
            zone.generate(ids, **bad)
    zone.train()
    with pytest.raises(RuntimeError):
        zone.step(ids[:, 0], state)
    zone.eval()
    balanced = _zone()
    balanced.encoder = BalancedGIFNeuron(12, 16)
    temporal = _zone()
    temporal.spike_to_continuous.encoding = "temporal"
    silent = _zone()
    silent.continuous_to_spike.encoding = "temporal"
    for other in (balanced, temporal, silent):
        with pytest.raises(NotImplementedError):
            other.step(ids[:, 0], other.new_state(2))
        with pytest.raises(NotImplementedError):
            other.generate(ids, max_new_tokens=2, seed=0)
    assert BRIDGE.CALLS == calls, "a refused call launches nothing"
    assert torch.equal(zone.moe_router.expert_usage, torch.zeros(4)), "eval leaves expert_usage alone"
