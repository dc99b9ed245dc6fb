"""Prosody attention on the build machine: known answers of the rule, the rule against the reference modules and the
golden fixture ``tests/golden/prosody_attention.pt`` against the reference that wrote it, the exhaustive id range that the
GPU test's exact boundary channel rests on, every host-side refusal of the two ops, and the modules on a CPU stand-in."""
import os

import numpy as np
import pytest
import torch

from tests import cpu_stub_prosody_attention as STUB
from tests import prosody_attention_rule as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prosody_attention.pt")
F32 = np.float32
DEFAULTS = dict(decay=[0.7, 0.7, 0.7], weights=[1.0, 1.0, 1.0])
# the three argument sets of the golden fixture: the defaults, the reference's 'analytical_balanced', and a centred window
GOLDEN_SETS = [
    dict(),
    dict(k_winners=5, w_amp=0.8, w_pitch=1.2, w_bound=1.0, smoothing=2, normalize_salience=True, gain_up=1.5,
         gain_down=0.7),
    dict(k_winners=7, decay_amp=0.5, decay_pitch=0.9, decay_bound=0.6, w_amp=1.5, w_pitch=0.5, w_bound=2.0, smoothing=3,
         normalize_salience=False, gain_up=0.9, min_gain=0.25, max_gain=3.0),
]


def _rule_kwargs(att):
    """The rule's arguments of a (reference or package) attention module."""
    return dict(decay=att.decay.numpy(), weights=att.weights.numpy(), k=att.k_winners, m=max(1, att.smoothing),
                normalize_salience=att.normalize_salience, gain_up=att.gain_up, min_gain=att.min_gain,
                max_gain=att.max_gain)


def _forward(amp, pitch, bound, **kw):
    args = dict(DEFAULTS, k=1)
    args.update(kw)
    return R.forward(np.asarray(amp, F32), np.asarray(pitch, F32), np.asarray(bound, F32), **args)


# ------------------------------------------------------------------------------------- known answers
def test_constant_half_input_follows_the_hand_recursion():
    S = 24
    x = np.full((1, S), 0.5, F32)
    z = np.zeros((1, S), F32)
    assert not _forward(x, z, z, decay=[0.0, 0.0, 0.0])["spikes"].any(), "decay 0: v stays 0.5 and never fires"
    d, v, want = F32(0.7), F32(0.0), []
    for _ in range(S):                                                   # the recursion, one scalar at a time
        v = F32(F32(d * v) + F32(0.5))
        s = F32(1.0) if v >= F32(1.0) else F32(0.0)
        v = F32(v - s)
        want.append(s)
    f = _forward(x, z, z)
    assert f["spikes"][0, 0].tolist() == want and 0 < sum(want) < S
    assert f["v_out"][0, 0] == v and f["v_out"][0, 1] == 0.0


def test_an_all_zero_row_gives_zero_salience_min_gain_and_the_first_k_positions():
    z = np.zeros((2, 9), F32)
    f = _forward(z, z, z, k=4)
    assert not f["salience"].any() and np.array_equal(f["mu"], np.full(2, 0.5, F32))
    assert np.array_equal(f["winners"], np.tile(np.arange(4, dtype=np.int32), (2, 1)))
    assert np.array_equal(f["gains"], np.full((2, 9), 0.5, F32))


def test_a_large_input_spikes_once_per_step():
    x = np.full((1, 12), 3.5, F32)
    f = _forward(x, x, x, k=3)
    assert f["spikes"].min() == 1.0 and f["spikes"].max() == 1.0          # one spike, not three, per step
    assert f["v_out"][0, 0] > 2.0                                        # the membrane keeps what one spike leaves
    assert np.array_equal(f["raw"], np.full((1, 12), 3.0, F32))
    assert np.array_equal(f["winners"][0], [0, 1, 2])                    # all equal: the lower positions


def test_k_equal_to_s_and_s_equal_to_one():
    rng = np.random.default_rng(3)
    x = rng.random((3, 2, 6)).astype(F32) * 2
    f = _forward(*x, k=6)
    for b in range(2):
        w = f["winners"][b]
        assert sorted(w.tolist()) == list(range(6))
        vals = f["salience"][b, w]
        assert np.all(vals[:-1] >= vals[1:])
        assert all(w[i] < w[i + 1] for i in range(5) if vals[i] == vals[i + 1]), "ties go to the lower position"
    one = _forward(*(np.full((1, 1), 1.5, F32),) * 3, k=1)
    assert one["winners"].tolist() == [[0]] and one["salience"][0, 0] == F32(3.0) / (F32(3.0) + F32(1e-6))


def test_an_empty_row_has_no_winner_and_gains_of_min_gain():
    x = np.full((2, 5), 3.5, F32)
    v0 = np.array([[0.25, 0.5, 0.75], [0, 0, 0]], F32)
    f = _forward(x, x, x, k=2, lengths=np.array([0, 3]), v0=v0)
    assert f["winners"][0].tolist() == [-1, -1] and f["mu"][0] == 0.5 and f["avg"][0] == 0.0
    assert not f["spikes"][:, 0].any() and not f["salience"][0].any()
    assert np.array_equal(f["gains"][0], np.full(5, 0.5, F32))
    assert np.array_equal(f["v_out"][0], v0[0]), "no step was taken"
    assert f["spikes"][0, 1].tolist() == [1, 1, 1, 0, 0] and f["salience"][1, 3:].tolist() == [0, 0]
    assert np.array_equal(f["gains"][1, 3:], np.full(2, f["mu"][1]))


def test_smoothing_taps_are_the_window_of_the_reference():
    raw = np.arange(1, 7, dtype=F32)[None, :]
    two = R.smooth(raw, 2)[0]
    assert two.tolist() == [0.5, 1.5, 2.5, 3.5, 4.5, 5.5]                # (sal[t-1] + sal[t]) / 2
    three = R.smooth(raw, 3)[0].astype(np.float64)
    want = np.array([1 + 2, 1 + 2 + 3, 2 + 3 + 4, 3 + 4 + 5, 4 + 5 + 6, 5 + 6]) / 3.0
    assert np.all(np.abs(three - want) <= 3 * R.U24 * 6)
    short = R.smooth(raw, 3, lengths=np.array([4]))[0].astype(np.float64)
    assert np.all(np.abs(short - np.array([3, 6, 9, 7, 0, 0]) / 3.0) <= 3 * R.U24 * 6)


# ------------------------------------------------------------------------------------- the rule against the reference
def _reference():
    from oracle import _ref_loader
    if not _ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    return _ref_loader.load("core.language_zone.multi_channel_attention")


def _against_reference(ref_mod, ids, kwargs):
    """``(reference dict, rule dict on the reference's channels)`` and the assertions every argument set shares."""
    att = ref_mod.MultiChannelSpikingAttention(**kwargs)
    amp, pitch, bound = ref_mod.prosody_channels_from_text(ids)
    with torch.no_grad():
        ref = att(amp, pitch, bound)
    kw = _rule_kwargs(att)
    f = R.forward(amp.numpy(), pitch.numpy(), bound.numpy(), **kw)
    sal_ref = ref["salience"].numpy()
    m, k = kw["m"], kw["k"]
    if m <= 2:
        assert np.array_equal(sal_ref, f["salience"]), "salience differs from the reference's bits"
    else:
        e = R.smooth_bound(f["raw"], m)
        bound_s = R.normalized_bound(f["smoothed"], e) if kw["normalize_salience"] else e + 0 * f["smoothed"]
        frac = float(np.max(np.abs(sal_ref.astype(np.float64) - f["salience"]) / np.maximum(bound_s, 1e-300)))
        print(f"smoothing {m}: {frac:.3f} of the bound")
        assert frac <= 1.0
    # winners are admissible: the reference's winner values are the top k values under the rule's order
    ref_vals = np.sort(np.take_along_axis(sal_ref, ref["winners"].numpy(), 1), axis=1)
    win, avg = R.winners(sal_ref, k)
    assert np.array_equal(ref_vals, np.sort(np.take_along_axis(sal_ref, win.astype(np.int64), 1), axis=1))
    # mu: the reference's mean has its own order (k u max|sal|), its tanh its own error
    mx = float(np.abs(sal_ref).max())
    m64, mb = R.mu64(avg, kw["gain_up"], kw["min_gain"], kw["max_gain"])
    rng = abs(float(F32(kw["max_gain"]) - F32(kw["min_gain"])))
    mb = mb + rng * (abs(kw["gain_up"]) * R.avg_bound(k, mx) + R.T)
    frac = float(np.max(np.abs(ref["mu_scalar"].numpy().astype(np.float64) - m64) / mb))
    print(f"mu: {frac:.3f} of the bound")
    assert frac <= 1.0
    return ref, f, (amp, pitch, bound)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_rule_matches_the_reference_modules(which):
    ref_mod = _reference()
    torch.manual_seed(11 + which)
    ids = torch.randint(0, 50257, (16, 512))
    _against_reference(ref_mod, ids, GOLDEN_SETS[which])


def test_the_rule_channels_are_within_their_bound_of_the_reference():
    ref_mod = _reference()
    ids = torch.arange(0, 65536).reshape(64, 1024)
    amp, pitch, bound = (c.numpy() for c in ref_mod.prosody_channels_from_text(ids))
    a64, p64, b, _ = R.channels(ids.numpy())
    assert np.abs(amp - a64).max() <= R.E and np.abs(pitch - p64).max() <= R.E
    assert np.array_equal(bound, b)


def test_no_id_of_the_vocabulary_range_sits_on_the_boundary_threshold():
    """The condition the GPU test's exact boundary channel rests on: over all ids in [0, 65536) the fp64 sine of the
    fp32 phase is further than 1e-6 (> E = 2^-21, the bound of a device sine) from 0.8f, so every accurate sinf decides
    the comparison alike.  (That the rule's boundary channel is the reference's over the same range is the test above.)"""
    _, _, b, margin = R.channels(np.arange(65536))
    assert R.E < 1e-6 and 0 < b.sum() < 65536
    assert int((margin < 1e-6).sum()) == 0, f"{int((margin < 1e-6).sum())} ids within 1e-6 of the threshold"


def _golden_from_reference(ref_mod):
    torch.manual_seed(47)
    ids = torch.randint(0, 50257, (3, 64))
    amp, pitch, bound = ref_mod.prosody_channels_from_text(ids)
    out = dict(ids=ids, amp=amp, pitch=pitch, boundary=bound, sets=[])
    for kwargs in GOLDEN_SETS:
        att = ref_mod.MultiChannelSpikingAttention(**kwargs)
        with torch.no_grad():
            r = att(amp, pitch, bound)
        out["sets"].append(dict(kwargs=dict(kwargs), salience=r["salience"].clone(), mu=r["mu_scalar"].clone(),
                                winner_values=torch.gather(r["salience"], 1, r["winners"]).clone()))
    return out


def test_the_golden_fixture_is_what_the_reference_computes():
    want = _golden_from_reference(_reference())
    have = torch.load(GOLDEN)
    assert set(have) == set(want) and os.path.getsize(GOLDEN) < 32 * 1024
    for n in ("ids", "amp", "pitch", "boundary"):
        assert torch.equal(have[n], want[n]), n
    assert len(have["sets"]) == len(want["sets"]) == 3
    for h, w in zip(have["sets"], want["sets"]):
        assert h["kwargs"] == w["kwargs"]
        for n in ("salience", "mu", "winner_values"):
            assert torch.equal(h[n], w[n]), n


def golden_cases():
    """``(kwargs of the attention module, channels, set)`` of the fixture, for this file and the GPU file."""
    g = torch.load(GOLDEN)
    return [(s["kwargs"], (g["amp"], g["pitch"], g["boundary"]), s) for s in g["sets"]], g


def test_the_golden_fixture_is_the_rule():
    from aura_snn_rag_amd.core.language_zone.prosody_attention import MultiChannelSpikingAttention
    cases, g = golden_cases()
    a64, p64, b, _ = R.channels(g["ids"].numpy())
    assert np.abs(g["amp"].numpy() - a64).max() <= R.E and np.array_equal(g["boundary"].numpy(), b)
    for kwargs, ch, s in cases:
        kw = _rule_kwargs(MultiChannelSpikingAttention(**kwargs))
        f = R.forward(*(c.numpy() for c in ch), **kw)
        if kw["m"] <= 2:
            assert np.array_equal(s["salience"].numpy(), f["salience"])
            assert np.array_equal(np.sort(s["winner_values"].numpy(), 1),
                                  np.sort(np.take_along_axis(f["salience"], f["winners"].astype(np.int64), 1), 1))
        else:
            assert np.all(np.abs(s["salience"].numpy().astype(np.float64) - f["salience"])
                          <= R.smooth_bound(f["raw"], kw["m"]))


# ------------------------------------------------------------------------------------- ops: argument checks
def _args(B=2, S=8, **kw):
    a = dict(ids=torch.zeros(B, S, dtype=torch.int64), k=2, decay=torch.full((3,), 0.7), weights=torch.ones(3))
    a.update(kw)
    return a


def test_ops_refuse_cpu_tensors():
    from aura_snn_rag_amd import ops
    with pytest.raises(ops.AuraDeviceError):
        ops.prosody_attention(**_args())
    with pytest.raises(ops.AuraDeviceError):
        ops.prosody_attention(**_args(ids=None, channels=(torch.zeros(2, 8),) * 3))
    with pytest.raises(ops.AuraDeviceError):
        ops.prosody_channels(torch.zeros(2, 8, dtype=torch.int32))


def test_ops_raise_before_loading_anything(monkeypatch):
    from aura_snn_rag_amd import ops

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", no_lib)
    assert (ops.PROSODY_MAX_S, ops.PROSODY_MAX_K, ops.PROSODY_MAX_SMOOTHING) == (8192, 256, 64)
    z = torch.zeros(2, 8)
    bad = [
        (dict(ids=None), ValueError, "neither ids nor channels"),
        (dict(channels=(z, z, z)), ValueError, "ids and channels"),
        (dict(ids=torch.zeros(2, 8)), TypeError, "float ids"),
        (dict(ids=torch.zeros(2, 8, dtype=torch.int16)), TypeError, "int16 ids"),
        (dict(ids=torch.zeros(8, dtype=torch.int64)), ValueError, "ids rank"),
        (dict(ids=torch.zeros(2, 16, dtype=torch.int64)[:, ::2]), ValueError, "non-contiguous ids"),
        (dict(ids=torch.zeros(2, 0, dtype=torch.int64)), ValueError, "S < 1"),
        (dict(ids=torch.zeros(1, 8193, dtype=torch.int64)), ValueError, "S > 8192"),
        (dict(ids=torch.full((2, 8), 1 << 24)), ValueError, "id out of range"),
        (dict(ids=torch.full((2, 8), -1)), ValueError, "negative id"),
        (dict(ids=None, channels=(z, z)), TypeError, "two channels"),
        (dict(ids=None, channels=(z, z, z.double())), TypeError, "fp64 channel"),
        (dict(ids=None, channels=(z, z, z.bfloat16())), TypeError, "bf16 channel"),
        (dict(ids=None, channels=(z, z, torch.zeros(2, 9))), ValueError, "channel shapes"),
        (dict(ids=None, channels=(z, z, torch.zeros(2, 16)[:, ::2])), ValueError, "non-contiguous channel"),
        (dict(ids=None, channels=(z, z, None)), ValueError, "missing channel"),
        (dict(k=0), ValueError, "k < 1"),
        (dict(k=9), ValueError, "k > S"),
        (dict(k=2.0), TypeError, "float k"),
        (dict(ids=torch.zeros(1, 512, dtype=torch.int64), k=257), ValueError, "k > 256"),
        (dict(smoothing=65), ValueError, "smoothing > 64"),
        (dict(smoothing=-1), ValueError, "smoothing < 0"),
        (dict(smoothing=2.0), TypeError, "float smoothing"),
        (dict(decay=torch.zeros(2)), ValueError, "decay shape"),
        (dict(weights=torch.ones(3).double()), TypeError, "fp64 weights"),
        (dict(decay=None), ValueError, "missing decay"),
        (dict(gain_up=float("nan")), ValueError, "NaN gain_up"),
        (dict(max_gain=float("inf")), ValueError, "infinite max_gain"),
        (dict(lengths=torch.tensor([1, 9], dtype=torch.int32)), ValueError, "lengths > S"),
        (dict(lengths=torch.tensor([-1, 2], dtype=torch.int32)), ValueError, "negative length"),
        (dict(lengths=torch.tensor([1, 2])), TypeError, "int64 lengths"),
        (dict(lengths=torch.tensor([1, 2, 3], dtype=torch.int32)), ValueError, "lengths shape"),
        (dict(state=torch.zeros(2, 4)), ValueError, "state shape"),
        (dict(state=torch.zeros(3, 2).t()), ValueError, "non-contiguous state"),
        (dict(state=torch.zeros(2, 3).half()), TypeError, "fp16 state"),
    ]
    for change, exc, why in bad:
        with pytest.raises(exc):
            ops.prosody_attention(**_args(**change))
            pytest.fail(f"accepted: {why}")
    for ids, exc in ((torch.zeros(2, 8), TypeError), (torch.full((2, 8), 1 << 24), ValueError),
                     (torch.zeros(8, dtype=torch.int64), ValueError)):
        with pytest.raises(exc):
            ops.prosody_channels(ids)
    # the value checks can be switched off; the device check still comes before the library
    with pytest.raises(ops.AuraDeviceError):
        ops.prosody_attention(**_args(ids=torch.full((2, 8), 1 << 24), validate=False))


def test_the_library_table_knows_the_entry():
    from aura_snn_rag_amd import _lib
    res, args = _lib.SIGNATURES["aura_prosody_attention"]
    assert res is _lib.I and len(args) == 25


# ------------------------------------------------------------------------------------- the modules on the stand-in
def test_the_modules_keep_the_reference_surface():
    import aura_snn_rag_amd as pkg
    from aura_snn_rag_amd.core.language_zone import prosody_attention as M
    assert pkg.ProsodyAttentionBridge is M.ProsodyAttentionBridge
    assert pkg.MultiChannelSpikingAttention is M.MultiChannelSpikingAttention
    assert pkg.prosody_channels_from_text is M.prosody_channels_from_text
    att = M.MultiChannelSpikingAttention(k_winners=3, decay_pitch=0.5, w_bound=2.0, gain_down=0.4)
    assert sorted(att.state_dict()) == ["decay", "weights"]
    assert att.decay.tolist() == [F32(0.7), 0.5, F32(0.7)] and att.weights.tolist() == [1.0, 1.0, 2.0]
    assert att.decay.dtype == torch.float32 and att.gain_down == 0.4 and att.k_winners == 3
    bridge = M.ProsodyAttentionBridge(k_winners=4, smoothing=3)
    assert sorted(bridge.state_dict()) == ["attention.decay", "attention.weights"]
    assert bridge.attention.k_winners == 4 and bridge.attention.smoothing == 3
    preset = M.ProsodyAttentionBridge(attention_preset="analytical_balanced").attention
    assert (preset.k_winners, preset.smoothing, preset.gain_up, preset.gain_down) == (5, 2, 1.5, 0.7)
    assert preset.weights.tolist() == [F32(0.8), F32(1.2), 1.0] and preset.normalize_salience is True
    with pytest.raises(ValueError):
        M.ProsodyAttentionBridge(attention_preset="unknown")
    with pytest.raises(ValueError):
        M.ProsodyAttentionBridge(attention_preset="analytical_balanced", smoothing=3)


def test_the_reference_checkpoint_loads():
    from aura_snn_rag_amd.core.language_zone import prosody_attention as M
    ref_mod = _reference()
    kw = dict(k_winners=3, decay_pitch=0.5, w_bound=2.0, gain_down=0.4)
    ref, att = ref_mod.MultiChannelSpikingAttention(**kw), M.MultiChannelSpikingAttention()
    assert sorted(ref.state_dict()) == sorted(att.state_dict())
    att.load_state_dict(ref.state_dict())
    assert torch.equal(att.decay, ref.decay) and torch.equal(att.weights, ref.weights)


def test_the_bridge_on_the_stand_in(monkeypatch):
    STUB.install(monkeypatch)
    from aura_snn_rag_amd.core.language_zone import prosody_attention as M
    torch.manual_seed(5)
    ids = torch.randint(0, 50257, (3, 40))
    bridge = M.ProsodyAttentionBridge(k_winners=5)
    gains, result = bridge(ids, token_strings=["ignored"])
    assert STUB.CALLS == {"attention": 1, "channels": 0} and STUB.LAST["from_ids"]
    assert gains.shape == (3, 40) and gains is result["gains"]
    assert set(result) == {"mu_scalar", "salience", "winners", "gains", "state"}
    assert result["winners"].dtype == torch.int64 and result["winners"].shape == (3, 5)
    assert torch.equal(gains, result["mu_scalar"][:, None] * (1.0 + result["salience"]))
    # the attention module on the channels the ids give is the same computation
    amp, pitch, bound = M.prosody_channels_from_text(ids)
    again = bridge.attention(amp, pitch, bound, return_spikes=True)
    assert STUB.CALLS == {"attention": 2, "channels": 1} and not STUB.LAST["from_ids"]
    for n in ("mu_scalar", "salience", "winners", "gains", "state"):
        assert torch.equal(again[n], result[n]), n
    assert again["spikes"].shape == (3, 3, 40)


def test_the_bridge_on_the_stand_in_against_the_reference_bridge(monkeypatch):
    _reference()
    STUB.install(monkeypatch)
    from aura_snn_rag_amd.core.language_zone import prosody_attention as M
    from oracle import _ref_loader
    torch.manual_seed(5)
    ids = torch.randint(0, 50257, (3, 40))
    gains, result = M.ProsodyAttentionBridge(k_winners=5)(ids)
    ref_bridge = _ref_loader.load("core.language_zone.prosody_attention").ProsodyAttentionBridge(k_winners=5)
    with torch.no_grad():
        ref_gains, ref_result = ref_bridge(ids)
    assert torch.equal(ref_result["salience"], result["salience"])
    assert torch.allclose(ref_gains, gains, atol=1e-5, rtol=0)


def test_chunked_calls_with_state_give_the_spikes_of_the_whole_run(monkeypatch):
    STUB.install(monkeypatch)
    from aura_snn_rag_amd.core.language_zone import prosody_attention as M
    torch.manual_seed(9)
    ids = torch.randint(0, 50257, (2, 50))
    bridge = M.ProsodyAttentionBridge(k_winners=1)           # k <= S holds for the one-step piece too
    _, whole = bridge(ids, return_spikes=True)
    state, parts = None, []
    for lo, hi in ((0, 7), (7, 8), (8, 33), (33, 50)):
        _, r = bridge(ids[:, lo:hi].contiguous(), state=state, return_spikes=True)
        state = r["state"]
        parts.append(r["spikes"])
    assert torch.equal(torch.cat(parts, dim=2), whole["spikes"]) and torch.equal(state, whole["state"])
    assert whole["spikes"].sum() > 0
