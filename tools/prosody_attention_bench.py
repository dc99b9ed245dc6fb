"""Measurements of the prosody-attention launch -> profiles/prosody_attention_bench.json.

    python tools/prosody_attention_bench.py [--batch 8 32 256] [--seq 128 512 2048] [--out ...]

Needs a GPU (no fallback).  One process.  Token ids [B, S] to attention gains [B, S], k = 5, with the module's defaults
(no smoothing) and with the 'analytical_balanced' preset (smoothing 2):
  fused   ``ProsodyAttentionBridge.forward`` with the range check of the ids switched off (``validate = False``: the check
          reads the ids' minimum and maximum on the host, two small launches and a wait that are no part of the kernel).
  torch   the reference's op sequence restated with torch ops here and run on the same GPU: the three channels, the LIF
          as a Python loop over the sequence for each of the three channels (about five small launches per step and
          channel, which is what makes it launch-bound), the weighted sum, conv1d, the division by the row maximum,
          topk, mean, tanh, and the gain line.
Both sides are first checked against each other when their boundary channels agree (torch's device sine is not the
kernel's, so an id may fall on the other side of 0.8 there; such a run is reported, not compared): salience, mu and
gains within 1e-5, and whether the salience has the same bits is recorded.
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), device
events, after a warm-up of every candidate, the candidates taken in alternating order inside each round
(tools/diverse_bench.py's scheme).  The inputs are a few hundred KB: everything is cache-resident on both sides, and
neither side is near any bandwidth.
Floor: the membrane chain is S dependent steps of multiply, add, compare, select, CHAIN_CYCLES = 16 cycles at the 4-cycle
dependent issue of one wave (MI355X microarchitecture notes), at 2.4 GHz, plus one launch; ``chain_floor_ms`` is the
first part, ``share_of_chain_floor`` = floor / measured.
Bar: the fused median must lie below the composition's median by more than both window spreads (max - min) together.
Exit status 1 when a bar is missed; the figures are written either way."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

CHAIN_CYCLES, CLOCK_HZ = 16, 2.4e9


def torch_lif(x, decay):
    v = torch.zeros(x.shape[0], device=x.device)
    out = []
    for t in range(x.shape[1]):
        v = decay * v + x[:, t]
        fired = (v >= 1.0).float()
        v = v - fired
        out.append(fired)
    return torch.stack(out, dim=1)


def torch_gains(ids, att):
    """Ids to gains as a caller without the kernel would compute them."""
    f = ids.float()
    amp, pitch, bound = torch.sin(f * 0.1).abs(), torch.cos(f * 0.05).abs(), (torch.sin(f * 0.3) > 0.8).float()
    spikes = [torch_lif(x, att.decay[c]) for c, x in enumerate((amp, pitch, bound))]
    sal = att.weights[0] * spikes[0] + att.weights[1] * spikes[1] + att.weights[2] * spikes[2]
    m = att.smoothing
    if m > 1:
        kernel = torch.ones(1, 1, m, device=sal.device) / m
        sal = F.conv1d(sal.unsqueeze(1), kernel, padding=m // 2).squeeze(1)[:, :ids.shape[1]]
    if att.normalize_salience:
        sal = sal / (sal.max(dim=1, keepdim=True)[0] + 1e-6)
    top = torch.topk(sal, k=att.k_winners, dim=-1)[0].mean(dim=1)
    mu = att.min_gain + (att.max_gain - att.min_gain) * torch.tanh(att.gain_up * top)
    return mu.unsqueeze(1) * (1.0 + sal), sal, mu, bound


def one(B, S, preset, dev, out, missed):
    from aura_snn_rag_amd import ProsodyAttentionBridge, ops
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + S)
    ids = torch.randint(0, 50257, (B, S), generator=gen, device=dev)
    bridge = ProsodyAttentionBridge(k_winners=5, attention_preset=preset).to(dev)
    att = bridge.attention
    att.validate = False

    # ---- the two sides against each other first
    gains, res = bridge(ids)
    t_gains, t_sal, t_mu, t_bound = torch_gains(ids, att)
    same_boundary = bool(torch.equal(ops.prosody_channels(ids)[2], t_bound))
    check = dict(boundary_channels_agree=same_boundary)
    if same_boundary:
        check.update(salience_bit_equal=bool(torch.equal(res["salience"], t_sal)),
                     salience_max_diff=float((res["salience"] - t_sal).abs().max()),
                     mu_max_diff=float((res["mu_scalar"] - t_mu).abs().max()),
                     gains_max_diff=float((gains - t_gains).abs().max()))
        assert max(check["salience_max_diff"], check["mu_max_diff"], check["gains_max_diff"]) <= 1e-5, check
    del t_gains, t_sal, t_mu

    ms, iters = alternated({"fused": lambda: bridge(ids), "torch": lambda: torch_gains(ids, att)}, events_window)
    f, t = summary(ms["fused"]), summary(ms["torch"])
    spreads = (f["max_ms"] - f["min_ms"]) + (t["max_ms"] - t["min_ms"])
    met = f["median_ms"] < t["median_ms"] - spreads
    floor_ms = 1e3 * S * CHAIN_CYCLES / CLOCK_HZ
    name = f"B{B}_S{S}_{'preset' if preset else 'default'}"
    out[name] = dict(B=B, S=S, k=att.k_winners, smoothing=att.smoothing, fused=f, torch=t, iters=iters,
                     both_spreads_ms=spreads, ratio_fused_over_torch=f["median_ms"] / t["median_ms"],
                     chain_floor_ms=floor_ms, share_of_chain_floor=floor_ms / f["median_ms"],
                     torch_launches_about=S * 3 * 5, check=check, bar_met=bool(met))
    print(f"{name}: fused {f['median_ms']:.4f} ms, torch {t['median_ms']:.3f} ms (spreads {spreads:.4f}); chain floor "
          f"{floor_ms:.4f} ms (share {out[name]['share_of_chain_floor']:.2f})", flush=True)
    if not met:
        missed.append(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 32, 256])
    ap.add_argument("--seq", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_attention_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prosody_attention_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for S in a.seq:
        for B in a.batch:
            for preset in (None, "analytical_balanced"):
                one(B, S, preset, dev, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
