"""Measurements of the theta-gamma kernels -> profiles/theta_gamma_bench.json.

    python tools/theta_gamma_bench.py [--batch 8 32] [--seq 512] [--dim 768] [--out ...]

Needs a GPU (no fallback).  One process.  ``hidden`` [B, S, D] is given (the place code's output in the models); the
positions are ``0 .. S - 1`` with ``max_seq_len = S``, shared by the batch.
  forward   ``ops.theta_gamma_norm`` on a table built once ("cached": what the module does under ``no_grad``) and with
            the table rebuilt in every call ("rebuilt": what it does in training), next to the composition to beat: the
            same formula written with torch ops, ``x + pe``, ``F.layer_norm``, all on the same GPU.
  backward  the derivative-table launch, the main and the finish launch together, next to the composition's autograd
            backward for all six inputs.  Autograd cannot run a backward without its forward, so the composition's
            backward is (forward and backward) minus (forward), and its spread the sum of the two spreads.
Both sides are first checked against each other (outputs and gradients within a relative 1e-4 of the largest entry).
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), device
events, after a warm-up of every candidate, the candidates taken in alternating order inside each round
(tools/diverse_bench.py's scheme).
CACHE-RESIDENT: the largest shape's activation is 50 MB, so x, g_y and the outputs of either side stay in the 256 MiB
Infinity Cache from call to call.  The buffers are not rotated: the figures are cache-resident rates on both sides, and
the floors below, taken at the HBM rate, are floors for a cold activation, not for this loop.
Floors from the shapes: forward ``2 N D 4`` bytes (read x, write y) against ``4 N D 4`` for the composition; backward
``3 N D 4`` (read g_y and x, write g_x) against ``4 N D 4``; at 6.3 TB/s.  The share reported is floor / measured.
Bar: each fused median must lie below the composition's median by more than the composition's own window spread
(max - min).  Exit status 1 when a bar is missed; the figures are written either way."""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
EPS = 1e-5


def torch_table(S, th, ga, amp, max_seq_len, ratio):
    """The reference's formula (src/core/language_zone/theta_gamma_encoding.py) from torch ops."""
    pos = torch.arange(S, device=th.device)
    phi = ((pos.float() / float(max(max_seq_len - 1, 1))) * (2.0 * math.pi)).unsqueeze(-1)
    a = phi + th
    g = phi * ratio + ga
    return (torch.sin(a) + 0.5 * (((torch.cos(a) + 1.0) * 0.5) * torch.sin(g))) * amp


def torch_forward(x, S, th, ga, amp, w, b, max_seq_len, ratio):
    pe = torch_table(S, th, ga, amp, max_seq_len, ratio)
    return F.layer_norm(x + pe, (x.shape[-1],), w, b, EPS)


def one(B, S, D, dev, out, missed):
    from aura_snn_rag_amd import ops
    N = B * S
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)
    x3, g3 = rnd(B, S, D), rnd(B, S, D)
    x, g_y = x3.reshape(N, D), g3.reshape(N, D)
    th, ga, amp = 0.1 * rnd(D), 0.1 * rnd(D), 1.0 + 0.2 * rnd(D)
    w, b = 1.0 + 0.3 * rnd(D), 0.3 * rnd(D)
    ratio = ops.theta_gamma_ratio(8.0, 40.0)

    def table():
        return ops.theta_gamma_table(th, ga, amp, S, ratio, start=0, rows=S)

    def fused_backward(pe, mean, rstd):
        d = ops.theta_gamma_table(th, ga, amp, S, ratio, start=0, rows=S, derivatives=True, pe=False)[1:]
        return ops.theta_gamma_norm_backward(g_y, x, pe, d, mean, rstd, w, S)

    def torch_both():
        leaves = [t.detach().requires_grad_(True) for t in (x3, th, ga, amp, w, b)]
        y = torch_forward(leaves[0], S, *leaves[1:], S, ratio)
        return torch.autograd.grad(y, leaves, g3)

    # ---- the two sides against each other first
    pe = table()
    y, mean, rstd = ops.theta_gamma_norm(x, pe, w, b, S, EPS)
    g_x, grads = fused_backward(pe, mean, rstd)
    y_t = torch_forward(x3, S, th, ga, amp, w, b, S, ratio).reshape(N, D)
    t_grads = torch_both()
    rel = lambda a, c: float((a - c).abs().max() / c.abs().max())
    diffs = dict(y=rel(y, y_t), g_x=rel(g_x, t_grads[0].reshape(N, D)), g_theta=rel(grads[2], t_grads[1]),
                 g_gamma=rel(grads[3], t_grads[2]), g_amp=rel(grads[4], t_grads[3]), g_w=rel(grads[0], t_grads[4]),
                 g_b=rel(grads[1], t_grads[5]))
    assert max(diffs.values()) <= 1e-4, diffs
    del y_t, t_grads, y, g_x, grads

    # ---- forward
    ms, iters = alternated({"fused_cached": lambda: ops.theta_gamma_norm(x, pe, w, b, S, EPS),
                            "fused_rebuilt": lambda: ops.theta_gamma_norm(x, table(), w, b, S, EPS),
                            "torch": lambda: torch_forward(x3, S, th, ga, amp, w, b, S, ratio)}, events_window)
    fc, fr, t = summary(ms["fused_cached"]), summary(ms["fused_rebuilt"]), summary(ms["torch"])
    t_spread = t["max_ms"] - t["min_ms"]
    floor_f, floor_t = 2 * N * D * 4, 4 * N * D * 4
    met_c, met_r = fc["median_ms"] < t["median_ms"] - t_spread, fr["median_ms"] < t["median_ms"] - t_spread
    fwd = dict(fused_cached=fc, fused_rebuilt=fr, torch=t, torch_spread_ms=t_spread, iters=iters,
               ratio_cached_over_torch=fc["median_ms"] / t["median_ms"],
               ratio_rebuilt_over_torch=fr["median_ms"] / t["median_ms"], floor_bytes=floor_f, torch_floor_bytes=floor_t,
               floor_ms=1e3 * floor_f / HBM_BYTES_PER_S, share_of_floor_cached=1e3 * floor_f / HBM_BYTES_PER_S / fc["median_ms"],
               share_of_floor_rebuilt=1e3 * floor_f / HBM_BYTES_PER_S / fr["median_ms"],
               torch_share_of_its_floor=1e3 * floor_t / HBM_BYTES_PER_S / t["median_ms"],
               bar_met_cached=bool(met_c), bar_met_rebuilt=bool(met_r))

    # ---- backward
    ms, iters = alternated({"fused": lambda: fused_backward(pe, mean, rstd), "torch_forward_and_backward": torch_both,
                            "torch_forward": lambda: torch_forward(x3, S, th, ga, amp, w, b, S, ratio)}, events_window)
    fb, tfb, tf = summary(ms["fused"]), summary(ms["torch_forward_and_backward"]), summary(ms["torch_forward"])
    t_bwd = tfb["median_ms"] - tf["median_ms"]
    spread = (tfb["max_ms"] - tfb["min_ms"]) + (tf["max_ms"] - tf["min_ms"])
    floor_b = 3 * N * D * 4
    met_b = fb["median_ms"] < t_bwd - spread
    bwd = dict(fused=fb, torch_forward_and_backward=tfb, torch_forward=tf, torch_backward_ms=t_bwd,
               torch_spread_ms=spread, iters=iters, ratio_fused_over_torch=fb["median_ms"] / max(t_bwd, 1e-9),
               floor_bytes=floor_b, torch_floor_bytes=floor_t, floor_ms=1e3 * floor_b / HBM_BYTES_PER_S,
               share_of_floor=1e3 * floor_b / HBM_BYTES_PER_S / fb["median_ms"],
               torch_share_of_its_floor=1e3 * floor_t / HBM_BYTES_PER_S / max(t_bwd, 1e-9), bar_met=bool(met_b))
    name = f"N{N}"
    out[name] = dict(B=B, S=S, D=D, N=N, max_seq_len=S, forward=fwd, backward=bwd, max_rel_diff_vs_torch=diffs,
                     cache_resident=True)
    print(f"{name} forward: fused {fc['median_ms']:.4f} ms cached, {fr['median_ms']:.4f} ms rebuilt, torch "
          f"{t['median_ms']:.4f} ms (spread {t_spread:.4f}); floor {fwd['floor_ms']:.4f} ms (share "
          f"{fwd['share_of_floor_cached']:.2f} cached)", flush=True)
    print(f"{name} backward: fused {fb['median_ms']:.4f} ms, torch {t_bwd:.4f} ms (spread {spread:.4f}); floor "
          f"{bwd['floor_ms']:.4f} ms (share {bwd['share_of_floor']:.2f})", flush=True)
    for met, what in ((met_c, "forward cached"), (met_r, "forward rebuilt"), (met_b, "backward")):
        if not met:
            missed.append(f"{name} {what}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "theta_gamma_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("theta_gamma_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for B in a.batch:
        one(B, a.seq, a.dim, dev, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
