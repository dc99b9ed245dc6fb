"""Measurements of the row linear kernel and of the fused decoding step
-> profiles/fused_step_bench.json.

    python tools/fused_step_bench.py [--rows 1 8 32] [--batch 1 8 32] [--prompt 16 512] [--only kernel|generate] [--out ...]

Needs a GPU (no fallback).  One process.
  kernel    ``ops.row_linear`` at D = 768 for R = 1, 8, 32 rows, the four launches of a layer's fused step -- LayerNorm +
            Q/K/V (three 768 x 768 matrices), ``o_proj`` + residual, LayerNorm + 768 -> 3072 + GELU, 3072 -> 768 +
            residual -- each next to the same result composed from ``F.layer_norm``, ``F.linear``, ``F.gelu`` and an add
            on the same GPU.  Both sides are first checked against each other (within a relative 1e-4 of the largest
            entry).  The weight loads' two cache policies (default and non-temporal) are both timed; ``fused`` is the
            policy the package ships (``ops.ROW_LINEAR_NONTEMPORAL``), ``fused_other`` the other one.  Device events,
            windows alternated in one process (tools/diverse_bench.py's scheme): the figure is the time per call of a
            stream of back-to-back calls, host launch cost included where the host is the slower side.
            Floor: the weights read once, ``4 sum N K`` bytes, at the 6.3 TB/s of DESIGN 4.15.  It is context, not a
            bar: a layer's 28 MB of weights stay in the 256 MiB Infinity Cache between calls, on both sides.
  generate  ``HippocampalTransformer.generate`` with ``fused_step=True`` and ``False``, the recorded configuration of
            tools/generate_bench.py (D 256, H 4, 4 layers, V 32 000, 48 sampled tokens, prompts of 16 and 512, B = 1, 8,
            32): host clock around a device synchronisation, median of five runs after a warm-up, the two alternated.
            The launch counts per token are counted from the code (``launches_per_token``), not measured.
Bars: the fused kernel's median below the composition's, outside both spreads (fused max < composition min), at all
twelve points; the fused ``generate``'s median per token below the unfused minimum at all six points.  Exit status 1
when a bar is missed; the figures are written either way."""
import argparse
import json
import os
import sys
import time
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.diverse_bench import alternated, events_window, summary  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
D, FF = 768, 3072

# launches of one generated token, read off the code: the front end (embedding gather, semantic projection, place code,
# phase table of the new position, add + LayerNorm), per layer the step, the tied head and the sampler
FRONT, HEAD, SAMPLER = 5, 1, 1
LAYER_UNFUSED = 14          # attention_norm, q, k, v, decode x 2, o_proj, add, ffn_norm, ffn.0, GELU, ffn.2, add
LAYER_FUSED = 6             # LN + QKV, decode x 2, o_proj + residual, LN + ffn.0 + GELU, ffn.2 + residual


def launches_per_token(layers: int, fused: bool) -> int:
    return FRONT + layers * (LAYER_FUSED if fused else LAYER_UNFUSED) + HEAD + SAMPLER


def kernel_points(R, dev):
    """name -> (fused callable, composition callable, weight bytes)."""
    from aura_snn_rag_amd import ops
    gen = torch.Generator(device=dev).manual_seed(R)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)
    x, ctx, mid, res = rnd(R, D), rnd(R, D), rnd(R, FF), rnd(R, D)
    g, b = 1.0 + 0.1 * rnd(D), 0.1 * rnd(D)
    Wq, Wk, Wv, Wo = (rnd(D, D) / D ** 0.5 for _ in range(4))
    bq, bk, bv, bo = (rnd(D) for _ in range(4))
    W0, b0, W2, b2 = rnd(FF, D) / D ** 0.5, rnd(FF), rnd(D, FF) / FF ** 0.5, rnd(D)

    def qkv_torch():
        xh = F.layer_norm(x, (D,), g, b, 1e-5)
        return F.linear(xh, Wq, bq), F.linear(xh, Wk, bk), F.linear(xh, Wv, bv), xh

    def qkv_fused():
        (q, k, v), xh = ops.row_linear(x, (Wq, Wk, Wv), (bq, bk, bv), norm=(g, b), return_normed=True)
        return q, k, v, xh

    return {
        "ln_qkv": (qkv_fused, qkv_torch, 4 * 3 * D * D),
        "o_proj_residual": (lambda: (ops.row_linear(ctx, Wo, bo, residual=res),),
                            lambda: (F.linear(ctx, Wo, bo) + res,), 4 * D * D),
        "ln_ffn0_gelu": (lambda: (ops.row_linear(x, W0, b0, norm=(g, b), activation="gelu"),),
                         lambda: (F.gelu(F.linear(F.layer_norm(x, (D,), g, b, 1e-5), W0, b0)),), 4 * FF * D),
        "ffn2_residual": (lambda: (ops.row_linear(mid, W2, b2, residual=res),),
                          lambda: (F.linear(mid, W2, b2) + res,), 4 * D * FF),
    }


def kernel_part(rows, dev, out, missed):
    from aura_snn_rag_amd import ops
    shipped = bool(ops.ROW_LINEAR_NONTEMPORAL)

    def with_policy(fn, nt):
        def run():
            ops.ROW_LINEAR_NONTEMPORAL = nt
            try:
                return fn()
            finally:
                ops.ROW_LINEAR_NONTEMPORAL = shipped
        return run

    for R in rows:
        for name, (fused, comp, wbytes) in kernel_points(R, dev).items():
            diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fused(), comp()))
            assert diff <= 1e-4, (name, R, diff)
            ms, iters = alternated({"fused": with_policy(fused, shipped), "fused_other": with_policy(fused, not shipped),
                                    "torch": comp}, events_window)
            f, o, t = summary(ms["fused"]), summary(ms["fused_other"]), summary(ms["torch"])
            floor_ms = 1e3 * wbytes / HBM_BYTES_PER_S
            met = f["max_ms"] < t["min_ms"]
            key = f"kernel_{name}_R{R}"
            out[key] = dict(R=R, D=D, fused=f, fused_other=o, torch=t, iters=iters,
                            fused_policy="nontemporal" if shipped else "default",
                            other_policy="default" if shipped else "nontemporal",
                            ratio_fused_over_torch=f["median_ms"] / t["median_ms"], weight_bytes=wbytes,
                            floor_ms=floor_ms, share_of_hbm_floor=floor_ms / f["median_ms"],
                            max_rel_diff_vs_torch=diff, bar_met=bool(met))
            print(f"{key}: fused {f['median_ms']:.4f} ms [{f['min_ms']:.4f}, {f['max_ms']:.4f}], other policy "
                  f"{o['median_ms']:.4f} ms, torch {t['median_ms']:.4f} ms [{t['min_ms']:.4f}, {t['max_ms']:.4f}]; floor "
                  f"{floor_ms:.5f} ms (share {floor_ms / f['median_ms']:.3f})", flush=True)
            if not met:
                missed.append(key)


def generate_point(B, S, dev, out, missed):
    from aura_snn_rag_amd import HippocampalTransformer
    V, N, LAYERS = 32000, 48, 4
    cfg = types.SimpleNamespace(vocab_size=V, embedding_dim=256, num_heads=4, num_layers=LAYERS, intermediate_size=1024,
                                n_place_cells=2000, max_seq_len=1024, dropout=0.0, theta_frequency=8.0,
                                gamma_frequency=40.0)
    torch.manual_seed(0)
    m = HippocampalTransformer(cfg, None).to(dev).eval()
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(1)).to(dev)
    run = lambda fused: m.generate(ids, max_new_tokens=N, use_memory=False, temperature=0.8, top_k=50, top_p=0.9,
                                   seed=5, fused_step=fused)
    agree = float((run(True) == run(False)).float().mean())             # the warm-up of both
    times = {True: [], False: []}
    for rnd in range(5):
        for fused in ((True, False) if rnd % 2 == 0 else (False, True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fused)
            torch.cuda.synchronize()
            times[fused].append(1e3 * (time.perf_counter() - t0) / N)
    res = {}
    for fused, name in ((True, "fused"), (False, "unfused")):
        ts = sorted(times[fused])
        res[name] = dict(median_ms_per_token=ts[2], min_ms_per_token=ts[0], max_ms_per_token=ts[-1],
                         launches_per_token=launches_per_token(LAYERS, fused))
    met = res["fused"]["median_ms_per_token"] < res["unfused"]["min_ms_per_token"]
    key = f"generate_B{B}_S{S}"
    out[key] = dict(B=B, V=V, prompt=S, new_tokens=N, layers=LAYERS, D=256, share_of_equal_tokens=agree,
                    ratio_fused_over_unfused=res["fused"]["median_ms_per_token"] / res["unfused"]["median_ms_per_token"],
                    bar_met=bool(met), **res)
    print(f"{key}: fused {res['fused']['median_ms_per_token']:.3f} ms/token ({res['fused']['launches_per_token']} "
          f"launches), unfused {res['unfused']['median_ms_per_token']:.3f} ms/token [min "
          f"{res['unfused']['min_ms_per_token']:.3f}] ({res['unfused']['launches_per_token']} launches); {agree:.3f} of "
          f"the tokens equal", flush=True)
    if not met:
        missed.append(key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prompt", type=int, nargs="+", default=[16, 512])
    ap.add_argument("--only", choices=["kernel", "generate"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_step_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fused_step_bench.py measures on the GPU; none found (nothing is measured on the CPU)")
    dev = torch.device("cuda", 0)
    out, missed = {}, []
    if a.only != "generate":
        kernel_part(a.rows, dev, out, missed)
    if a.only != "kernel":
        for B in a.batch:
            for S in a.prompt:
                generate_point(B, S, dev, out, missed)
    out["device"] = torch.cuda.get_device_name(0)
    out["bars_missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"wrote {a.out}; bars missed: {missed or 'none'}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
