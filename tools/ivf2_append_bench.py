"""Time of ``aura_ivf2_append`` (the inverted lists' upkeep after a write, csrc/aura_bank.hip) -> one JSON line.

    python tools/ivf2_append_bench.py

Needs a GPU (no fallback).  65536 distinct rows of a 131072 x 768 bank are appended to 256 empty lists of 1024 slots,
with a live table of row constants; the lists are emptied before every call, outside the timed span.  The figure is
the median over 7 windows of 20 calls, device events around each call (min and max of the windows beside it).  Compare
two builds of the library with ``AURA_HIP_LIB=<path>``, one fresh process each."""
import json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aura_snn_rag_amd import ops, _lib  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    M, D, CAP, n = 131072, 768, 1024, 65536
    g = torch.Generator(device=dev).manual_seed(3)
    bank = torch.randn(M, D, generator=g, device=dev)
    inv = torch.empty(M, device=dev)
    ops.bank_row_norms(bank, inv, 0, M)
    meta = torch.zeros(M, 4, device=dev)
    meta[:, 0] = 0.25 + 0.75 * torch.rand(M, generator=g, device=dev)
    meta[:, 1] = 1.7e9
    meta[:, 2] = torch.randint(0, 256, (M,), generator=g, device=dev).float()
    n_alloc = 256 * CAP
    image = torch.zeros(n_alloc, D, dtype=torch.bfloat16, device=dev)
    sorted_rows = torch.full((n_alloc,), -1, dtype=torch.int32, device=dev)
    pad_off = (torch.arange(257, dtype=torch.int32) * CAP).to(dev)
    list_len = torch.zeros(256, dtype=torch.int32, device=dev)
    pos = torch.full((M,), -1, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rowc = torch.zeros(n_alloc, 4, device=dev)
    rho = torch.zeros(M, device=dev)
    slots = torch.randperm(M, generator=g, device=dev)[:n].contiguous()
    nowf = float(np.float32(1.7e9 + 777.0))

    def window(iters):
        ms = 0.0
        for _ in range(iters):
            list_len.zero_(); pos.fill_(-1); sorted_rows.fill_(-1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.ivf2_append(bank, inv, meta, slots, image, sorted_rows, pad_off, list_len, pos, rho, flag,
                            row_constants=rowc, row_constants_now=nowf)
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
        return ms / iters

    window(5)
    w = [window(20) for _ in range(7)]
    assert int(flag.item()) == 0 and int(list_len.sum()) == n
    print(json.dumps({"lib": _lib.loaded_path(), "append_65536_ms": statistics.median(w), "min": min(w), "max": max(w)}))


if __name__ == "__main__":
    main()
