"""Measurements of the place code -> profiles/place_code_bench.json.

    python tools/place_code_bench.py [--rows 4096 16384] [--dim 768] [--cells 2000] [--k 60] [--out ...]

Needs a GPU (no fallback).  One process.  The logits ``z`` [N, P] and embeddings ``e`` [N, D] are given (the embedding
lookup and the first Linear stay torch in the module and are not part of either side).
  forward   ``ops.place_code`` with the dense code and without it, next to the reference's op sequence composed from
            torch ops on the same GPU: ``topk``, ``sigmoid``, ``zeros_like``, ``scatter``, ``F.linear`` over the dense
            code, residual.  Both are first checked against each other (same winner sets on tie-free logits, the
            outputs within the rule's bound of the composition evaluated in fp64).
  backward  ``ops.place_code_backward`` (g_z from g_out and g_dense) next to the composition's autograd backward for the
            logits alone (``torch.autograd.grad(..., z)``: the parameter gradients are library calls on both sides).
Every figure is the median over WINDOWS windows of at least WINDOW_S of work each (min and max beside it), device
events, after a warm-up, the candidates taken in alternating order inside each round (tools/diverse_bench.py's scheme).
Floors: HBM bytes ``N (2 P + 2 D) 4`` with the dense code (``N (P + 2 D) 4`` without) at 6.3 TB/s, and the gathered
``N k D 4`` table bytes at the 34.5 TB/s aggregate L2 rate; the share reported is floor / measured.
Bars: the fused forward (with the dense code) must beat the composition's FASTEST window; the backward's median must be
no longer than the composition's median plus the composition's own window-to-window spread.  Exit status 1 when a bar is
missed; the figures are written either way."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
L2_BYTES_PER_S = 34.5e12


def torch_forward(z, e, weight, bias, k):
    """The reference's op sequence (src/core/language_zone/place_cell_encoder.py, steps 3 to 7)."""
    v, i = torch.topk(z, k, dim=-1)
    dense = torch.zeros_like(z).scatter(-1, i, torch.sigmoid(v))
    return e + 0.1 * F.linear(dense, weight, bias), dense


def one(N, P, D, k, dev, out, missed):
    from aura_snn_rag_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    z = 2.0 * torch.randn(N, P, generator=g, device=dev)
    e = torch.randn(N, D, generator=g, device=dev)
    weight = torch.randn(D, P, generator=g, device=dev) / k ** 0.5          # place_to_semantic.weight
    bias = 0.1 * torch.randn(D, generator=g, device=dev)
    w2t = weight.t().contiguous()
    # ---- the two sides against each other first
    o_k, idx, act, dense_k = ops.place_code(z, e, w2t, bias, k)
    o_t, dense_t = torch_forward(z, e, weight, bias, k)
    same_sets = bool(torch.equal(dense_k != 0, dense_t != 0))
    o64 = e.double() + float(torch.tensor(0.1, dtype=torch.float32)) * (dense_k.double() @ w2t.double() + bias.double())
    mag = dense_k.double().abs() @ w2t.double().abs() + bias.double().abs()
    bound = 0.1 * (k + 2) * 2.0 ** -24 * mag + 2.0 ** -23 * o64.abs() + 0.1 * 2.0 ** -22 * w2t.double().abs().sum(0)
    frac_k = float(((o_k.double() - o64).abs() / bound).max())
    frac_t = float(((o_t.double() - o64).abs() / bound).max())
    assert same_sets and frac_k <= 1.0 and frac_t <= 1.0, (same_sets, frac_k, frac_t)
    g_out = torch.randn(N, D, generator=g, device=dev)
    g_dense = torch.randn(N, P, generator=g, device=dev) / (N * P)
    zr = z.clone().requires_grad_(True)
    o_r, d_r = torch_forward(zr, e, weight, bias, k)
    gz_t, = torch.autograd.grad([o_r, d_r], zr, [g_out, g_dense])
    gz_k = ops.place_code_backward(g_out, g_dense, idx, act, w2t)
    scale = float(gz_t.abs().max())
    gz_diff = float((gz_k - gz_t).abs().max()) / scale
    assert gz_diff <= 1e-4, gz_diff
    del o64, mag, bound, o_r, d_r, gz_t, gz_k, o_t, dense_t, o_k, dense_k

    # ---- forward
    ms, iters = alternated({"fused": lambda: ops.place_code(z, e, w2t, bias, k),
                            "fused_sparse": lambda: ops.place_code(z, e, w2t, bias, k, dense=False),
                            "torch": lambda: torch_forward(z, e, weight, bias, k)}, events_window)
    f, fs, t = summary(ms["fused"]), summary(ms["fused_sparse"]), summary(ms["torch"])
    hbm_dense, hbm_sparse = N * (2 * P + 2 * D) * 4, N * (P + 2 * D) * 4
    l2 = N * k * D * 4
    fwd_met = f["median_ms"] < t["min_ms"]
    fwd = dict(fused=f, fused_sparse=fs, torch=t, iters=iters, ratio_fused_over_torch=f["median_ms"] / t["median_ms"],
               hbm_bytes=hbm_dense, hbm_bytes_sparse=hbm_sparse, l2_gather_bytes=l2,
               hbm_floor_ms=1e3 * hbm_dense / HBM_BYTES_PER_S, hbm_floor_sparse_ms=1e3 * hbm_sparse / HBM_BYTES_PER_S,
               l2_floor_ms=1e3 * l2 / L2_BYTES_PER_S,
               share_of_hbm_floor=1e3 * hbm_dense / HBM_BYTES_PER_S / f["median_ms"],
               share_of_hbm_floor_sparse=1e3 * hbm_sparse / HBM_BYTES_PER_S / fs["median_ms"],
               share_of_l2_floor=1e3 * l2 / L2_BYTES_PER_S / f["median_ms"], bar_met=bool(fwd_met))

    # ---- backward (the logit gradient)
    def torch_backward():
        zz = z.detach().requires_grad_(True)
        o, d = torch_forward(zz, e, weight, bias, k)
        return torch.autograd.grad([o, d], zz, [g_out, g_dense])

    ms, iters = alternated({"fused": lambda: ops.place_code_backward(g_out, g_dense, idx, act, w2t),
                            "torch_forward_and_backward": torch_backward,
                            "torch_forward": lambda: torch_forward(z, e, weight, bias, k)}, events_window)
    b, tfb, tf = summary(ms["fused"]), summary(ms["torch_forward_and_backward"]), summary(ms["torch_forward"])
    # autograd cannot run a backward without its forward: the composition's backward is the difference of the two
    t_bwd = tfb["median_ms"] - tf["median_ms"]
    spread = (tfb["max_ms"] - tfb["min_ms"]) + (tf["max_ms"] - tf["min_ms"])
    bwd_met = b["median_ms"] <= t_bwd + spread
    hbm_b = N * (2 * P + D) * 4 + 2 * N * k * 4
    bwd = dict(fused=b, torch_forward_and_backward=tfb, torch_forward=tf, torch_backward_ms=t_bwd,
               torch_spread_ms=spread, iters=iters, ratio_fused_over_torch=b["median_ms"] / max(t_bwd, 1e-9),
               hbm_bytes=hbm_b, l2_gather_bytes=l2, hbm_floor_ms=1e3 * hbm_b / HBM_BYTES_PER_S,
               l2_floor_ms=1e3 * l2 / L2_BYTES_PER_S, share_of_hbm_floor=1e3 * hbm_b / HBM_BYTES_PER_S / b["median_ms"],
               share_of_l2_floor=1e3 * l2 / L2_BYTES_PER_S / b["median_ms"], bar_met=bool(bwd_met))
    name = f"N{N}"
    out[name] = dict(N=N, P=P, D=D, k=k, forward=fwd, backward=bwd, same_winner_sets=same_sets,
                     max_frac_of_out_bound=dict(fused=frac_k, torch=frac_t), g_z_max_rel_diff_vs_torch=gz_diff)
    print(f"{name} forward: fused {f['median_ms']:.4f} ms, without dense {fs['median_ms']:.4f} ms, torch "
          f"{t['median_ms']:.4f} ms (fastest window {t['min_ms']:.4f}); HBM floor {fwd['hbm_floor_ms']:.4f} ms (share "
          f"{fwd['share_of_hbm_floor']:.2f}), L2 floor {fwd['l2_floor_ms']:.4f} ms (share {fwd['share_of_l2_floor']:.2f})",
          flush=True)
    print(f"{name} backward: fused {b['median_ms']:.4f} ms, torch {t_bwd:.4f} ms (spread {spread:.4f}); HBM share "
          f"{bwd['share_of_hbm_floor']:.2f}, L2 share {bwd['share_of_l2_floor']:.2f}", flush=True)
    if not fwd_met:
        missed.append(f"{name} forward")
    if not bwd_met:
        missed.append(f"{name} backward")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--cells", type=int, default=2000)
    ap.add_argument("--k", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_code_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("place_code_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for N in a.rows:
        one(N, a.cells, a.dim, a.k, dev, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
