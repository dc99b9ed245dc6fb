#!/usr/bin/env python3
"""The training neuron ops (csrc/aura_train.hip and aura_lif_run) under two builds of libaura_hip.so: the parent of the
"dtype as argument" change, whose C ABI has the ``_bf16`` twins, and this tree's.

    train_dtype_ab.py --parent PARENT.so [--branch BRANCH.so] [--pairs N] [-o outputs.json] [--bench-out bench.json]

Outputs.  Each of the nine ops, fp32 and bf16, on seeded tensors in two child processes, one per library (selected
through ``AURA_HIP_LIB``), one after the other, each under its own time limit; the saved outputs are compared on the
host.  Shapes: H = 8 and 24 (the 16-byte instances), H = 5 (the scalar ones), T in {1, 3}, alpha in {0, 0.01}, L in
{1, 8}, gains present and absent; 4100 rows x H 129 / 516 / 1032 at T = 1 for the second grid pass of the scalar, VEC 4
and VEC 8 instance.  Everything must be byte-identical, except ``g_gains`` where more than one work item adds into an
element (H above the vector width): the float atomics' order is free there, and each side is held to the rule bound
of tests/surrogate_rule.py instead.

Timing (``--pairs N``, N >= 7).  Every kernel instance on one streaming shape (8192 x 16 x 3072, bench.py's GIF shape,
H 3073 for the scalar instances; the LIF steps, which have no row in bench.py, take the same elements as
131072 x 3072): N parent / branch pairs of child processes, alternating, device events around 10 launches after 3
warm-up launches.  A kernel passes when the branch's median does not exceed the parent's by more than the parent's own
spread in the series, (max - min) / median.
"""
import argparse
import ctypes
import hashlib
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECAY, THR0, STRENGTH = 0.9048374180359595, 1.0, 0.3
CHILD_LIMIT_S = 240


# ---- one library, either ABI ---------------------------------------------------------------------------------------
class Lib:
    def __init__(self, path):
        import torch  # noqa: F401  (its HIP runtime first, as aura_snn_rag_amd._lib.load does)
        from aura_snn_rag_amd import _lib
        self.sig = _lib.SIGNATURES
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        self.twins = hasattr(self.lib, "aura_gif_backward_bf16")          # the parent's ABI

    def __call__(self, op, dtype, *args):
        """args: the op's arguments up to the sizes, tensors or None for pointers; dtype and stream are added here."""
        import torch
        res, argt = self.sig["aura_" + op]
        bf16 = dtype == torch.bfloat16
        fn = getattr(self.lib, "aura_" + op + ("_bf16" if self.twins and bf16 else ""))
        fn.restype, fn.argtypes = res, (argt[:-2] + argt[-1:] if self.twins else argt)
        ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
        rc = fn(*[ptr(a) for a in args], *(() if self.twins else (int(bf16),)), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"aura_{op} ({dtype}) returned {rc}"


def run_ops(lib, dev, dtype, rows, T, H, L, alpha, use_gains, seed, keep):
    """All nine ops on one seeded case; ``keep(name, tensor)`` receives every output."""
    import torch
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    mk = lambda t: t.to(dtype).to(dev)
    nan = lambda *s, dt=dtype: torch.full(s, float("nan"), dtype=dt, device=dev)
    h, v0, t0 = mk(2 * rnd(rows, T, H)), mk(0.4 * rnd(rows, H)), mk(1.0 + 0.3 * torch.rand(rows, H, generator=g))
    gains = mk(0.2 + 3.0 * torch.rand(rows, T, generator=g)) if use_gains else None
    ws, wv, wt = mk(rnd(rows, T, H)), mk(rnd(rows, H)), mk(rnd(rows, H))
    gif = (DECAY, L, alpha, THR0)
    # GIF: recording forward, backward from its own saves
    sp, sa, st, v, th = nan(rows, T, H), nan(rows, T, H), nan(rows, T, H), v0.clone(), t0.clone()
    lib("gif_train_forward", dtype, h, sp, v, th, sa, st, *gif, rows, T, H)
    gh, gv, gt = nan(rows, T, H), wv.clone(), wt.clone()
    lib("gif_backward", dtype, sa, st, ws, gh, gv, gt, *gif, rows, T, H)
    for n, t in (("spikes", sp), ("save_a", sa), ("save_theta", st), ("v", v), ("theta", th), ("g_h", gh), ("g_v", gv),
                 ("g_theta", gt)):
        keep("gif." + n, t)
    # prosody GIF: plain loop, recording forward, backward
    sp0, v, th = nan(rows, T, H), v0.clone(), t0.clone()
    lib("gif_prosody_run", dtype, h, gains, sp0, v, th, *gif, STRENGTH, rows, T, H)
    for n, t in (("spikes", sp0), ("v", v), ("theta", th)):
        keep("prosody_run." + n, t)
    sp, sa, st, v, th = nan(rows, T, H), nan(rows, T, H), nan(rows, T, H), v0.clone(), t0.clone()
    lib("gif_prosody_train_forward", dtype, h, gains, sp, v, th, sa, st, *gif, STRENGTH, rows, T, H)
    gh, gv, gt = nan(rows, T, H), wv.clone(), wt.clone()
    gg = torch.zeros(rows, T, device=dev) if use_gains else None
    lib("gif_prosody_backward", dtype, sa, st, h, gains, ws, gh, gg, gv, gt, *gif, STRENGTH, rows, T, H)
    for n, t in (("spikes", sp), ("save_a", sa), ("save_theta", st), ("v", v), ("theta", th), ("g_h", gh), ("g_v", gv),
                 ("g_theta", gt)):
        keep("prosody." + n, t)
    if use_gains:
        keep("prosody.g_gains", gg, rule=dict(save_a=sa, save_theta=st, h=h, gains=gains, ws=ws, wv=wv, wt=wt, L=L,
                                              alpha=alpha))
    # LIF: the T-step loop, the recording step, its backward
    beta, thr, slope = mk(0.8 + 0.19 * torch.rand(H, generator=g)), mk(0.5 + torch.rand(H, generator=g)), \
        mk(5.0 + 20.0 * torch.rand(H, generator=g))
    sp, mem = nan(rows, T, H), v0.clone()
    lib("lif_run", dtype, h, sp, mem, beta, thr, rows, T, H)
    keep("lif_run.spikes", sp); keep("lif_run.mem", mem)
    x, sp, mo, pre = h[:, 0].contiguous(), nan(rows, H), nan(rows, H), nan(rows, H)
    lib("lif_train_forward", dtype, x, v0, beta, thr, sp, mo, pre, rows, H)
    gx, gp, rs = nan(rows, H), nan(rows, H), nan(rows, H, dt=torch.float32)
    lib("lif_backward", dtype, pre, wv, wt, beta, thr, slope, gx, gp, rs, rows, H)
    for n, t in (("spikes", sp), ("mem_out", mo), ("pre", pre), ("g_x", gx), ("g_mem_prev", gp), ("raw_slope", rs)):
        keep("lif." + n, t)


def cases():
    import torch
    for dtype in (torch.float32, torch.bfloat16):
        for H, T, alpha, L, gains in itertools.product((8, 24, 5), (1, 3), (0.0, 0.01), (1, 8), (False, True)):
            yield dtype, 6, T, H, L, alpha, gains
        for H in (129, 516, 1032):
            yield dtype, 4100, 1, H, 8, 0.01, True


def child_outputs(path, out):
    import torch
    from tests import surrogate_rule as R
    lib, dev, saved = Lib(path), torch.device("cuda:0"), {}
    for i, (dtype, rows, T, H, L, alpha, gains) in enumerate(cases()):
        tag = f"{str(dtype)[6:]} {rows}x{T}x{H} L{L} a{alpha} {'gains' if gains else 'plain'}"
        vec = (4 if dtype == torch.float32 else 8)
        vec = vec if H % vec == 0 else 1

        def keep(name, t, rule=None):
            raw = t.detach().cpu().contiguous()
            bits = raw.view(torch.int16 if raw.dtype == torch.bfloat16 else torch.int32)
            e = dict(numel=bits.numel(), sha256=hashlib.sha256(bits.numpy().tobytes()).hexdigest())
            if rule is not None and H > vec:            # order-free float atomics: the rule's bound instead of the bits
                c = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in rule.items()}
                bwd = R.gif_backward(c["save_a"], c["save_theta"], c["ws"], c["wv"], c["wt"], DECAY, c["L"], c["alpha"],
                                     THR0, h=c["h"], gains=c["gains"], strength=STRENGTH, prosody=True)
                e = dict(numel=bits.numel(), err_over_bound=R.worst_ratio(raw, bwd["g_gains"], out_dtype=torch.float32))
            saved[f"{tag}: {name}"] = e
        run_ops(lib, dev, dtype, rows, T, H, L, alpha, gains, 1000 + i, keep)
    torch.cuda.synchronize()
    json.dump(saved, open(out, "w"))


# ---- timing --------------------------------------------------------------------------------------------------------
def child_time(path, out):
    import torch
    lib, dev, ms = Lib(path), torch.device("cuda:0"), {}
    rows, T = 8192, 16

    def timed(name, fn):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(10):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms[name] = a.elapsed_time(b) / 10

    for dtype, H in itertools.product((torch.float32, torch.bfloat16), (3072, 3073)):
        who = f"{str(dtype)[6:]} {'vec' if H == 3072 else 'scalar'}"
        z = lambda *s, dt=dtype: torch.zeros(*s, dtype=dt, device=dev)
        h = (2 * torch.randn(rows, T, H, device=dev)).to(dtype)
        ws = torch.randn(rows, T, H, device=dev).to(dtype)
        gains = (0.2 + 3.0 * torch.rand(rows, T, device=dev)).to(dtype)
        sp, sa, st, gh = z(rows, T, H), z(rows, T, H), z(rows, T, H), z(rows, T, H)
        v, th, gv, gt, gg = z(rows, H), z(rows, H) + 1, z(rows, H), z(rows, H), z(rows, T, dt=torch.float32)
        gif = (DECAY, 8, 0.01, THR0)
        timed(f"gif_train_forward {who}", lambda: lib("gif_train_forward", dtype, h, sp, v, th, sa, st, *gif, rows, T, H))
        timed(f"gif_backward {who}", lambda: lib("gif_backward", dtype, sa, st, ws, gh, gv, gt, *gif, rows, T, H))
        timed(f"gif_prosody_run {who}", lambda: lib("gif_prosody_run", dtype, h, gains, sp, v, th, *gif, STRENGTH, rows, T, H))
        timed(f"gif_prosody_train_forward {who}", lambda: lib("gif_prosody_train_forward", dtype, h, gains, sp, v, th, sa, st,
                                                           *gif, STRENGTH, rows, T, H))
        timed(f"gif_prosody_backward {who}", lambda: lib("gif_prosody_backward", dtype, sa, st, h, gains, ws, gh, gg, gv, gt,
                                                      *gif, STRENGTH, rows, T, H))
        beta, thr, slope = z(H) + 0.9, z(H) + 1, z(H) + 25
        if dtype == torch.bfloat16:
            timed(f"lif_run {who}", lambda: lib("lif_run", dtype, h, sp, v, beta, thr, rows, T, H))
        B = rows * T                                                                  # the same elements as one step
        x, mem, s2, mo, pre, gx = (t.view(B, H) for t in (h, ws, sp, sa, st, gh))
        timed(f"lif_train_forward {who}", lambda: lib("lif_train_forward", dtype, x, mem, beta, thr, s2, mo, pre, B, H))
        rs = z(B, H, dt=torch.float32)
        timed(f"lif_backward {who}", lambda: lib("lif_backward", dtype, pre, x, mem, beta, thr, slope, gx, mo, rs, B, H))
        del h, ws, sp, sa, st, gh, rs, x, mem, s2, mo, pre, gx
    json.dump(ms, open(out, "w"))


# ---- driver --------------------------------------------------------------------------------------------------------
def spawn(mode, lib_path, out):
    env = dict(os.environ, AURA_HIP_LIB=lib_path)
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", mode, "--out", out]
    print(f"[{mode}] {lib_path}", flush=True)
    r = subprocess.run(cmd, env=env, cwd=ROOT)
    if r.returncode != 0:
        sys.exit(f"{mode} child for {lib_path} ended with status {r.returncode}: nothing further is started")
    return json.load(open(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--branch", default=os.path.join(ROOT, "aura_snn_rag_amd", "lib", "libaura_hip.so"))
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("-o", "--out", default="train_dtype_outputs.json")
    ap.add_argument("--bench-out", default="train_dtype_bench.json")
    ap.add_argument("--child", choices=("outputs", "time"))
    a = ap.parse_args()
    if a.child:
        return (child_outputs if a.child == "outputs" else child_time)(os.environ["AURA_HIP_LIB"], a.out)
    tmp = os.path.dirname(os.path.abspath(a.out))
    before = spawn("outputs", a.parent, os.path.join(tmp, "ab_parent.json"))
    after = spawn("outputs", a.branch, os.path.join(tmp, "ab_branch.json"))
    assert set(before) == set(after)
    rep = dict(tensors=len(before), elements=0, byte_identical_elements=0, bounded_elements=0, differing=[])
    for k in sorted(before):
        b, c = before[k], after[k]
        rep["elements"] += b["numel"]
        if "err_over_bound" in b:
            ok = b["err_over_bound"] <= 1.0 and c["err_over_bound"] <= 1.0
            rep["bounded_elements"] += b["numel"]
            rep["worst_err_over_bound"] = max(rep.get("worst_err_over_bound", 0.0), b["err_over_bound"], c["err_over_bound"])
        else:
            ok = b == c
            rep["byte_identical_elements"] += b["numel"] if ok else 0
        if not ok:
            rep["differing"].append({k: [b, c]})
    json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in rep.items() if k != "differing"}), "differing:", len(rep["differing"]))
    for d in rep["differing"][:20]:
        print("  ", d)
    if rep["differing"]:
        return 1
    if a.pairs:
        runs = dict(parent=[], branch=[])
        for i in range(a.pairs):
            runs["parent"].append(spawn("time", a.parent, os.path.join(tmp, "time_parent.json")))
            runs["branch"].append(spawn("time", a.branch, os.path.join(tmp, "time_branch.json")))
        verdict = {}
        for k in runs["parent"][0]:
            p, c = [r[k] for r in runs["parent"]], [r[k] for r in runs["branch"]]
            pm, cm = statistics.median(p), statistics.median(c)
            spread = (max(p) - min(p)) / pm
            verdict[k] = dict(parent_median_ms=pm, branch_median_ms=cm, parent_spread=spread,
                              branch_over_parent=cm / pm, within_bar=bool(cm <= pm * (1 + spread)))
            print(f"{k:44s} parent {pm:8.4f} ms  branch {cm:8.4f} ms  ratio {cm / pm:.4f}  spread {spread:.4f}  "
                  f"{'ok' if verdict[k]['within_bar'] else 'MISSES THE BAR'}")
        json.dump(dict(shape="8192 x 16 x 3072 (vec) / 3073 (scalar); LIF steps 131072 x H", pairs=a.pairs,
                       launches_per_run=10, warm_up=3, runs_ms=runs, verdict=verdict), open(a.bench_out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
