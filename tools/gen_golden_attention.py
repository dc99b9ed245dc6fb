"""Writes tests/golden/hippocampal_attention.pt from the reference's HippocampalProsodyAttention, on the CPU.

    python tools/gen_golden_attention.py [--out tests/golden/hippocampal_attention.pt]

Runs on the build machine only, where the reference checkout is present (oracle/_ref_loader.py loads its module by path;
nothing of it is copied).  The file holds data alone: for each case the module's ``state_dict``, the inputs ``hidden``
[B, S, D] and ``prosody`` [B, S, 4] and the recorded outputs of ``forward`` in eval mode with prosody, without prosody,
and with prosody but ``use_memory=False``.  Cases (B, S, D, H): (3, 13, 96, 2) and (2, 9, 128, 4).  About 0.4 MB,
nearly all of it the four D x D projection matrices of the two cases."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((3, 13, 96, 2), (2, 9, 128, 4))


def build(ref_mod):
    out = {"cases": []}
    for n, (B, S, D, H) in enumerate(CASES):
        torch.manual_seed(100 + n)
        cfg = types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0)
        mod = ref_mod.HippocampalProsodyAttention(cfg, hippocampus=object()).eval()
        hidden = torch.randn(B, S, D)
        prosody = 1.5 * torch.randn(B, S, 4)
        with torch.no_grad():
            outs = {"prosody": mod(hidden, prosody=prosody, use_memory=True)[0],
                    "no_prosody": mod(hidden, prosody=None, use_memory=True)[0],
                    "no_memory": mod(hidden, prosody=prosody, use_memory=False)[0]}
        out["cases"].append({"shape": (B, S, D, H), "state_dict": {k: v.clone() for k, v in mod.state_dict().items()},
                             "hidden": hidden, "prosody": prosody, "outputs": outs})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hippocampal_attention.pt"))
    a = ap.parse_args()
    from oracle import _ref_loader
    if not _ref_loader.available():
        raise SystemExit("gen_golden_attention.py needs the reference checkout (oracle/_ref_loader.py); not found")
    data = build(_ref_loader.load("core.language_zone.hippocampal_attention"))
    torch.save(data, a.out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(data['cases'])} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
