"""GPU tests of ``aura_prosody_attention`` and everything above it against the rule restated in NumPy
(tests/prosody_attention_rule.py).

Asserted (tolerances derived from the formats in the rule file's docstring, not from a run):
  spikes, v_out   bit-equal to the rule on the channels the kernel was given (or emitted, from ids).
  salience        bit-equal without smoothing; with a window m within ``m u max|raw|`` (0 for m = 2, where every order gives
                  the same bits), carried through the division (``R.normalized_bound``).
  winners         equal position for position to the rule's selection on the kernel's own salience.
  mu              within ``|range| T + 3u M`` of fp64 on the fp32 mean of the kernel's own winners.
  gains           ``fl(mu fl(1 + sal))`` of the kernel's own mu and salience: bit-equal (inside any bound on them).
  from ids        the boundary channel exact (tests/test_host_prosody_attention.py shows that no id below 65 536 sits
                  within 1e-6 > E of the threshold), amp and pitch within E = 2^-21 of fp64 on the fp32 phase.
A measured maximum above half its bound is flagged in the recorded profile (``over_half_bound``).

Shapes ``(B, S, k, m)``: one element; k = S; a ragged block of 63 / 64 / 65; more rows than a workgroup's four waves and
more than one chunk of 256 (129, 512, 1000); the one-wave-per-workgroup instance with the limits S = 8192, k = 256,
m = 64."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import helpers
from tests import prosody_attention_rule as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 5, 5, 1), (3, 63, 5, 1), (2, 64, 2, 2), (3, 65, 5, 3), (70, 129, 5, 1), (4, 512, 5, 2),
          (2, 1000, 60, 1), (1, 8192, 256, 64)]
KINDS = ["random", "edge", "ids", "lengths", "v0"]
CASES = [(s, kind) for s in SHAPES for kind in KINDS]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prosody_attention.pt")
F32 = np.float32


def _id(case):
    (B, S, k, m), kind = case
    return f"B{B}-S{S}-k{k}-m{m}-{kind}"


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs of one case, computed once and never modified."""
    (B, S, k, m), kind = case
    rng = np.random.default_rng(sum(map(ord, _id(case))))
    c = dict(B=B, S=S, k=k, m=m, ids=None, channels=None, lengths=None, v0=None, decay=np.array([0.7, 0.7, 0.7], F32),
             weights=np.array([1.0, 1.0, 1.0], F32), normalize=True, gain_up=1.8, min_gain=0.5, max_gain=2.5)
    if kind in ("ids", "lengths"):
        c["ids"] = rng.integers(0, 65536, (B, S)).astype(np.int64)
    else:
        ch = rng.random((3, B, S)).astype(F32)
        ch[2] = (ch[2] > 0.8).astype(F32)
        if kind == "edge":
            c["weights"] = np.array([0.8, 1.2, 1.0], F32)
            t = np.arange(S)
            for b in range(B):
                what = (b + 3) % 5
                if what == 0:
                    ch[:, b] = 0.0
                elif what == 1:
                    ch[:, b] = 3.5
                elif what == 2:
                    ch[:, b] = (2.0 * rng.random((3, S)) - 1.0).astype(F32)
                elif what == 3:                         # NaN and both infinities, in different channels at different times
                    ch[0, b, t % 7 == 3] = np.nan
                    ch[1, b, t % 11 == 5] = np.inf
                    ch[2, b, t % 13 == 6] = -np.inf
                    ch[1, b, t % 17 == 9] = -np.inf
        c["channels"] = ch
    if kind == "lengths":
        pool = [0, 1, S, S // 2, max(S - 1, 0)] + rng.integers(0, S + 1, B).tolist()
        shift = SHAPES.index(case[0])
        c["lengths"] = np.array([pool[(b + shift) % len(pool)] for b in range(B)], np.int32)
        c["decay"] = np.array([0.5, 0.9, 0.6], F32)
    if kind == "v0":
        c["v0"] = (2.0 * rng.random((B, 3)) - 0.5).astype(F32)
        c.update(normalize=False, gain_up=0.9, min_gain=0.25, max_gain=3.0, weights=np.array([1.5, 0.5, 2.0], F32))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _call(c, dev, rows=slice(None), **over):
    from aura_snn_rag_amd import ops
    pick = lambda a: None if a is None else _dev(np.ascontiguousarray(a[rows]), dev)
    ch = None if c["channels"] is None else tuple(_dev(np.ascontiguousarray(x[rows]), dev) for x in c["channels"])
    args = dict(k=c["k"], decay=_dev(c["decay"], dev), weights=_dev(c["weights"], dev), gain_up=c["gain_up"],
                min_gain=c["min_gain"], max_gain=c["max_gain"], smoothing=c["m"], normalize=c["normalize"],
                lengths=pick(c["lengths"]), state=pick(c["v0"]), want_spikes=True, want_channels=True)
    args.update(over)
    return ops.prosody_attention(pick(c["ids"]), ch, **args)


@functools.lru_cache(maxsize=None)
def _run(case, dev):
    """The op of one case on the device, once, and the rule on the channels it emitted: shared by the tests."""
    c = _case(case)
    r = _call(c, dev)
    torch.cuda.synchronize()
    ch = _np(r.channels)
    f = R.forward(ch[0], ch[1], ch[2], c["decay"], c["weights"], c["k"], c["m"], c["normalize"], c["gain_up"],
                  c["min_gain"], c["max_gain"], c["lengths"], c["v0"])
    return r, f


def _flag(frac):
    return dict(max_frac_of_bound=round(float(frac), 4), over_half_bound=bool(frac > 0.5))


def _within(name, got, want, bound):
    """Record and assert ``|got - want| <= bound`` elementwise; returns the largest fraction of the bound."""
    got = np.asarray(got, np.float64)
    want, bound = np.broadcast_arrays(np.asarray(want, np.float64), np.asarray(bound, np.float64))
    assert got.shape == want.shape, f"{name}: shape {got.shape} against {want.shape}"
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), f"{name}: not finite"
    err = np.abs(got - want)
    ok = err <= bound
    frac = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0
    print(f"prosody {name}: at {frac:.4f} of its bound")
    helpers.record_parity(f"prosody {name}", int(ok.sum()), err.size, **_flag(frac))
    assert bool(ok.all()), f"{name}: max fraction of the bound {frac}"
    return frac


def _same(name, got, want):
    """Bit-for-bit (NaN equal to NaN), recorded."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} against {want.shape}"
    ok = (got == want) | ((got != got) & (want != want))
    helpers.record_parity(f"prosody {name}", int(ok.sum()), ok.size)
    assert bool(ok.all()), f"{name}: {int((~ok).sum())} of {ok.size} differ"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_against_the_rule(dev, case):
    c = _case(case)
    r, f = _run(case, dev)
    B, S, k, m, tag = c["B"], c["S"], c["k"], c["m"], _id(case)
    assert r.gains.shape == (B, S) and r.salience.shape == (B, S) and r.mu.shape == (B,)
    assert r.winners.shape == (B, k) and r.winners.dtype == torch.int32 and r.state.shape == (B, 3)
    assert r.spikes.shape == (3, B, S) and r.channels.shape == (3, B, S)
    ch = _np(r.channels)
    if c["ids"] is not None:
        a64, p64, b, margin = R.channels(c["ids"])
        assert margin.min() > 1e-6
        _same(f"boundary {tag}", ch[2], b)
        _within(f"amp {tag}", ch[0], a64, R.E)
        _within(f"pitch {tag}", ch[1], p64, R.E)
    else:
        for got, want in zip(ch, c["channels"]):
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), "given channels come back as they went in"
    _same(f"spikes {tag}", _np(r.spikes), f["spikes"])
    _same(f"v_out {tag}", _np(r.state), f["v_out"])
    sal = _np(r.salience)
    assert np.all(np.isfinite(sal))
    if m <= 1:
        _same(f"salience {tag}", sal, f["salience"])
    else:
        e = R.smooth_bound(f["raw"], m)
        bound = R.normalized_bound(f["smoothed"], e) if c["normalize"] else e + 0.0 * f["smoothed"]
        _within(f"salience {tag}", sal, f["salience"], bound)
    lens = np.full(B, S) if c["lengths"] is None else c["lengths"]
    win, avg = R.winners(sal, k, lens)
    _same(f"winners {tag}", _np(r.winners), win)
    m64, mb = R.mu64(avg, c["gain_up"], c["min_gain"], c["max_gain"])
    mu = _np(r.mu)
    _within(f"mu {tag}", mu, m64, mb)
    _same(f"gains {tag}", _np(r.gains), R.gains32(mu, sal))
    beyond = np.arange(S)[None, :] >= np.asarray(lens)[:, None]
    assert not _np(r.spikes)[:, beyond].any() and not sal[beyond].any()
    assert np.array_equal(_np(r.gains)[beyond], np.broadcast_to(mu[:, None], (B, S))[beyond])
    assert np.all(_np(r.winners)[np.arange(k)[None, :] >= np.minimum(k, lens)[:, None]] == -1)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_row_alone_has_the_bits_it_has_in_the_batch(dev, case):
    c = _case(case)
    r, _ = _run(case, dev)
    again = _call(c, dev)
    names = ("gains", "salience", "mu", "winners", "state", "spikes", "channels")
    for n in names:
        assert torch.equal(_bits(getattr(again, n)), _bits(getattr(r, n))), f"the same call gave other bits in {n}"
    for b in sorted({0, c["B"] // 2, c["B"] - 1}):
        alone = _call(c, dev, rows=slice(b, b + 1))
        for n in names:
            whole = getattr(r, n)
            part = whole[:, b:b + 1] if n in ("spikes", "channels") else whole[b:b + 1]
            assert torch.equal(_bits(getattr(alone, n)), _bits(part)), f"row {b} alone differs in {n}"


def test_the_channels_alone_and_int32_ids_give_the_same_bits(dev):
    from aura_snn_rag_amd import ops
    case = ((3, 65, 5, 3), "ids")
    c = _case(case)
    r, _ = _run(case, dev)
    ids = _dev(c["ids"], dev)
    assert torch.equal(_bits(ops.prosody_channels(ids)), _bits(r.channels))
    assert torch.equal(_bits(ops.prosody_channels(ids.int())), _bits(r.channels))
    r32 = _call(dict(c, ids=c["ids"].astype(np.int32)), dev)
    for n in ("gains", "salience", "mu", "winners", "state", "spikes"):
        assert torch.equal(_bits(getattr(r32, n)), _bits(getattr(r, n))), n
    plain = _call(c, dev, want_spikes=False, want_channels=False)
    assert plain.spikes is None and plain.channels is None and torch.equal(_bits(plain.gains), _bits(r.gains))


@pytest.mark.parametrize("shape", [(3, 65, 1, 1), (2, 1000, 1, 2)], ids=str)
def test_chunked_calls_with_state_give_the_spikes_of_the_whole_run(dev, shape):
    from aura_snn_rag_amd.core.language_zone.prosody_attention import ProsodyAttentionBridge
    B, S, k, m = shape
    rng = np.random.default_rng(S)
    ids = torch.from_numpy(rng.integers(0, 65536, (B, S))).to(dev)
    bridge = ProsodyAttentionBridge(k_winners=k, smoothing=m).to(dev)
    _, whole = bridge(ids, return_spikes=True)
    cuts = sorted({0, 1, 7, 64, S // 2 + 3, S})            # a one-step piece, a ragged one, one that ends a block
    state, parts = None, []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _, part = bridge(ids[:, lo:hi].contiguous(), state=state, return_spikes=True)
        state = part["state"]
        parts.append(part["spikes"])
    assert torch.equal(_bits(torch.cat(parts, dim=2)), _bits(whole["spikes"]))
    assert torch.equal(_bits(state), _bits(whole["state"])) and float(whole["spikes"].sum()) > 0


def test_the_golden_channels_give_the_golden_salience(dev):
    from aura_snn_rag_amd.core.language_zone.prosody_attention import MultiChannelSpikingAttention
    g = torch.load(GOLDEN)
    ch = tuple(g[n].to(dev) for n in ("amp", "pitch", "boundary"))
    exact = 0
    for s in g["sets"]:
        att = MultiChannelSpikingAttention(**s["kwargs"]).to(dev)
        out = att(*ch)
        sal, want = _np(out["salience"]), s["salience"].numpy()
        if att.smoothing <= 2:
            _same(f"golden salience smoothing {att.smoothing}", sal, want)
            vals = np.take_along_axis(sal, _np(out["winners"]), 1)
            assert np.array_equal(np.sort(vals, 1), np.sort(s["winner_values"].numpy(), 1))
            exact += 1
        else:
            raw = np.full((want.shape[0], 1), float(np.abs(att.weights.cpu().numpy()).sum()))
            _within(f"golden salience smoothing {att.smoothing}", sal, want, R.smooth_bound(raw, att.smoothing))
        rng = abs(att.max_gain - att.min_gain)
        k = att.k_winners
        bound = rng * (abs(att.gain_up) * 2 * R.avg_bound(k, float(np.abs(want).max())) + 2 * R.T) + 6 * R.U24 * (
            abs(att.min_gain) + rng)
        _within(f"golden mu smoothing {att.smoothing}", _np(out["mu_scalar"]), s["mu"].numpy(), bound)
    assert exact == 2


def test_bridge_gains_drive_the_prosody_gif_like_the_rule_gains(dev):
    from aura_snn_rag_amd.core.language_zone.prosody_attention import ProsodyAttentionBridge
    from aura_snn_rag_amd.core.language_zone.prosody_gif import ProsodyModulatedGIF
    torch.manual_seed(3)
    B, T = 3, 40
    ids = torch.randint(0, 50257, (B, T), device=dev)
    bridge = ProsodyAttentionBridge(attention_preset="analytical_balanced").to(dev)
    gains, result = bridge(ids)
    assert gains.shape == (B, T) and gains.dtype == torch.float32 and result["winners"].dtype == torch.int64
    rule_gains = torch.from_numpy(R.gains32(_np(result["mu_scalar"]), _np(result["salience"]))).to(dev)
    assert torch.equal(_bits(gains), _bits(rule_gains))
    gif = ProsodyModulatedGIF(16, 24).to(dev)
    x = 4.0 * torch.randn(B, T, 16, device=dev)
    with torch.no_grad():
        s1, (v1, th1) = gif(x, attention_gains=gains)
        s2, (v2, th2) = gif(x, attention_gains=rule_gains)
        s0, _ = gif(x)
    assert torch.equal(s1, s2) and torch.equal(v1, v2) and torch.equal(th1, th2)
    assert s1.shape[:2] == (B, T) and not torch.equal(s1, s0), "the gains must reach the neuron"
