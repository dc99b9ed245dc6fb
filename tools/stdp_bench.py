"""Measurements of timestep STDP -> profiles/stdp_bench.json.

    python tools/stdp_bench.py [--rows 512] [--steps 16] [--dim 768] [--hidden 3072] [--out profiles/stdp_bench.json]

Needs a GPU (no fallback).  One process.  Config 3's two synapses, each with fp32 and with bf16 spikes:
  syn2   B = rows, T = steps, I = hidden, O = dim; levels 0..8 at densities 0.3 / 0.2
  syn1   I = dim, O = hidden, a time-invariant Gaussian ``pre``
``ops.stdp_update`` (applying, in place) against the same update composed from torch ops -- a T-step trace loop, two fp32
``matmul``s (the depression term of a time-invariant ``pre`` sums the post trace over T first, as a careful caller would)
and a clamp -- on the same inputs.  Both are first checked against the rule evaluated in fp64 on the device from the
fp32 traces, within the bound of ``include/aura_hip.h``.  Every figure is the median over WINDOWS windows of at least
WINDOW_S of work each (min and max beside it), device events, after a warm-up, the two taken in alternating order inside
each round (tools/diverse_bench.py's scheme).
The floor: 2 (2 B T) I O FLOP at the 157.3 TFLOP/s fp32 matrix peak (the bytes take a twentieth of that: matrix-bound).
The bar: the kernel's median is no longer than the torch composition's; the margin is the composition's own
window-to-window spread (max - min).  Exit status 1 when a bar is missed; the figures are written either way."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
HBM_BYTES_PER_S = 6.3e12
LAM_PRE, LAM_POST, A_PLUS, A_MINUS, LR, W_MIN, W_MAX = 0.95, 0.9, 0.01, 0.012, 0.5, -1.0, 1.0
KW = dict(lambda_pre=LAM_PRE, lambda_post=LAM_POST, a_plus=A_PLUS, a_minus=A_MINUS, lr=LR, w_min=W_MIN, w_max=W_MAX)


def torch_traces(pre, post, x0, y0, invariant):
    """xs [B, T, I], y_before [B, T, O] in fp32 by the two-rounding recursion (eager torch never fuses mul and add)."""
    B, T, O = post.shape
    post = post.float()
    pre = pre.float()
    xs = torch.empty(B, T, pre.shape[-1], device=post.device)
    yb = torch.empty(B, T, O, device=post.device)
    x, y = x0, y0
    for t in range(T):
        x = LAM_PRE * x + (pre if invariant else pre[:, t])
        yb[:, t] = LAM_POST * y
        y = yb[:, t] + post[:, t]
        xs[:, t] = x
    return pre, post, xs, yb, x, y


def torch_update(pre, post, x0, y0, w, invariant):
    """The update a caller without the kernel would write."""
    B, T, O = post.shape
    pre, post, xs, yb, x, y = torch_traces(pre, post, x0, y0, invariant)
    ltp = post.reshape(B * T, O).t() @ xs.reshape(B * T, -1)
    ltd = yb.sum(dim=1).t() @ pre if invariant else yb.reshape(B * T, O).t() @ pre.reshape(B * T, -1)
    dw = (A_PLUS * ltp - A_MINUS * ltd) / B
    w.add_(LR * dw).clamp_(W_MIN, W_MAX)
    return dw, x, y


def rule64(pre, post, x0, y0, invariant):
    """dW and S in fp64 on the device from the fp32 traces."""
    B, T, O = post.shape
    pre, post, xs, yb, x, y = torch_traces(pre, post, x0, y0, invariant)
    if invariant:
        pre = pre[:, None, :].expand(B, T, pre.shape[-1])
    a = [t.reshape(B * T, -1).double() for t in (post, xs, yb, pre)]
    ap, am = float(torch.tensor(A_PLUS, dtype=torch.float32)), float(torch.tensor(A_MINUS, dtype=torch.float32))
    dw = (ap * (a[0].t() @ a[1]) - am * (a[2].t() @ a[3])) / B
    s = (ap * (a[0].abs().t() @ a[1].abs()) + am * (a[2].abs().t() @ a[3].abs())) / B
    return dw, s, x, y


def spikes(shape, density, g, dev):
    on = torch.rand(shape, generator=g, device=dev) < density
    return (on * torch.randint(1, 9, shape, generator=g, device=dev)).float()


def one(name, B, T, I, O, dtype, invariant, dev, out, missed):
    from aura_snn_rag_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    pre = (torch.randn(B, I, generator=g, device=dev) if invariant else spikes((B, T, I), 0.3, g, dev)).to(dtype)
    post = spikes((B, T, O), 0.2, g, dev).to(dtype)
    x0 = torch.rand(B, I, generator=g, device=dev)
    y0 = torch.rand(B, O, generator=g, device=dev)
    w0 = 0.5 * torch.randn(O, I, generator=g, device=dev)
    kw = dict(KW, pre_time_invariant=invariant)
    # both against the rule first
    dw64, s, xf, yf = rule64(pre, post, x0, y0, invariant)
    bound = (2 * B * T + 8) * 2.0 ** -24 * s
    dw_k = torch.empty(O, I, device=dev)
    xk, yk = ops.stdp_update(pre, post, x0, y0, None, dw_k, **kw)
    dw_t, xt, yt = torch_update(pre, post, x0, y0, w0.clone(), invariant)
    frac_k = float(((dw_k.double() - dw64).abs() / bound.clamp_min(1e-300)).max())
    frac_t = float(((dw_t.double() - dw64).abs() / bound.clamp_min(1e-300)).max())
    assert torch.equal(xk, xf) and torch.equal(yk, yf) and torch.equal(xt, xf), "trace bits"
    assert frac_k <= 1.0 and frac_t <= 1.0, (frac_k, frac_t)
    del dw64, s, bound, dw_t
    w_k, w_t = w0.clone(), w0.clone()
    ms, iters = alternated({"kernel": lambda: ops.stdp_update(pre, post, x0, y0, w_k, None, **kw),
                            "torch": lambda: torch_update(pre, post, x0, y0, w_t, invariant)}, events_window)
    k, t = summary(ms["kernel"]), summary(ms["torch"])
    flop = 2.0 * (2 * B * T) * I * O
    elt = 2 if dtype == torch.bfloat16 else 4
    nbytes = elt * (B * T * O + (B * I if invariant else B * T * I)) + 2 * 4 * O * I + 2 * 4 * B * (I + O)
    floor_ms = 1e3 * max(flop / F32_MATRIX_PEAK, nbytes / HBM_BYTES_PER_S)
    spread = t["max_ms"] - t["min_ms"]
    met = k["median_ms"] <= t["median_ms"] + spread
    out[name] = dict(B=B, T=T, I=I, O=O, dtype=str(dtype).replace("torch.", ""), pre_time_invariant=invariant,
                     kernel=k, torch=t, torch_spread_ms=spread, ratio_kernel_over_torch=k["median_ms"] / t["median_ms"],
                     flop=flop, bytes=nbytes, floor_ms=floor_ms, bound_by="matrix" if flop / F32_MATRIX_PEAK >
                     nbytes / HBM_BYTES_PER_S else "bytes", share_of_floor=floor_ms / k["median_ms"],
                     achieved_tflops=flop / k["median_ms"] / 1e9, max_frac_of_bound=dict(kernel=frac_k, torch=frac_t),
                     iters=iters, bar_met=bool(met))
    print(f"{name}: kernel {k['median_ms']:.3f} ms, torch {t['median_ms']:.3f} ms (spread {spread:.3f}), floor "
          f"{floor_ms:.3f} ms, share {floor_ms / k['median_ms']:.2f}, bound fractions {frac_k:.4f} / {frac_t:.4f}",
          flush=True)
    if not met:
        missed.append(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--hidden", type=int, default=3072)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stdp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stdp_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    for dtype in (torch.float32, torch.bfloat16):
        tag = "fp32" if dtype == torch.float32 else "bf16"
        one(f"syn2 {tag}", a.rows, a.steps, a.hidden, a.dim, dtype, False, dev, out, missed)
        one(f"syn1 {tag} time-invariant", a.rows, a.steps, a.dim, a.hidden, dtype, True, dev, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
