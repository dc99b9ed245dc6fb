"""Child of tests/test_gpu_neuron_paths.py::test_time_contiguous_environment_switches.

The AURA_NT_* switches of csrc/aura_neuron.hip are read once per process, so the parent starts this script in a
fresh process with exactly one of them set.  It runs the Izhikevich loop at (130, 100) -- two whole tiles and a
partial one -- and (64, 100) -- one whole tile -- twice each (the second call carries the state), compares
spikes, v and u with the CPU oracle bit for bit, and exits non-zero on any difference.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from aura_snn_rag_amd import ops
from oracle import aura_oracle as O

IZH = (0.02, 0.2, -65.0, 8.0, 0.2)


def main() -> int:
    set_ = [k for k in ("AURA_NT_LEGACY", "AURA_NT_NO_DMA", "AURA_NT_STORE_NT") if os.environ.get(k)]
    if len(set_) != 1:
        print(f"expected exactly one AURA_NT_* switch, got {set_}")
        return 2
    dev = torch.device("cuda:0")
    for N, T in ((130, 100), (64, 100)):
        I = 20 * torch.rand(N, T, generator=torch.Generator().manual_seed(N))
        state = O.izh_initial_state(N, 0.2)
        v, u = (s.to(dev) for s in state)
        Id, spikes = I.to(dev), torch.empty(N, T, device=dev)
        for call in range(2):
            rs, rv, ru = O.izh_run(I, *state, *IZH)
            ops.izh_run_nt(Id, spikes, v, u, *IZH)
            if not (torch.equal(spikes.cpu(), rs) and torch.equal(v.cpu(), rv) and torch.equal(u.cpu(), ru)):
                print(f"{set_[0]}: ({N}, {T}) call {call}: {int((spikes.cpu() != rs).sum())} spikes differ, "
                      f"v equal {torch.equal(v.cpu(), rv)}, u equal {torch.equal(u.cpu(), ru)}")
                return 1
            state = (rv, ru)
        if int(rs.sum()) == 0:
            print(f"({N}, {T}): the oracle never spiked")
            return 1
    print(f"{set_[0]} OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
