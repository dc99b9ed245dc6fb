"""Writes the two fixtures of the memory-augmented model from the reference's classes, on the CPU.

    python tools/gen_golden_snn_rag.py [--dir tests/golden]

Runs on the build machine only, where the reference checkout is present (oracle/_ref_loader.py loads its modules by
path; nothing of it is copied).  Both files hold data alone.
  * ``snn_rag_transformer_keys.json``: the ``state_dict`` key names and shapes of the reference's ``SNNRAGTransformer``
    for the three injections (two layers, the default ``snn_layers``: layer 0 is a HybridFFN layer), and of one
    ``MemoryAugmentedLayer`` per injection and FFN kind, with the config they were built from.
  * ``memory_augmented_layer.pt``: MLP layers only, one case per injection, (B, S, D, H, k) = (3, 9, 48, 4, 5): the
    ``state_dict``, the inputs ``hidden`` and ``prosody``, the memory ``features`` [B, k, D] and ``scores`` [B, k] that a
    duck-typed stand-in bank served the reference's per-row retrieval loop, and the recorded outputs of ``forward`` in
    eval mode with and without memory.  About 0.2 MB."""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INJECTIONS = ("cross_attention", "concat", "gate")
MODEL_CONFIG = dict(vocab_size=257, embedding_dim=96, num_heads=4, num_layers=2, intermediate_size=192,
                    n_place_cells=200, max_seq_len=32, dropout=0.0, theta_frequency=8.0, gamma_frequency=40.0)
B, S, D, H, K = 3, 9, 48, 4, 5


class StandInBank:
    """Serves fixed memories to the reference layer's retrieval loop: call number b (one per batch row, in order)
    gets row b of ``features`` / ``scores``.  Only the four attributes that loop touches."""

    def __init__(self, features, scores):
        self.features, self.scores = features, scores
        n, k, d = features.shape
        self.memory_features = features.reshape(n * k, d)
        self.id_to_idx = {f"r{b}-{i}": b * k + i for b in range(n) for i in range(k)}
        self.memory_count = n * k
        self.calls = 0

    def retrieve_similar_memories(self, query_features, k):
        b = self.calls % self.features.shape[0]
        self.calls += 1
        return [(f"r{b}-{i}", float(self.scores[b, i])) for i in range(k)]


def _keys(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def build_keys(model_mod, layer_mod):
    cfg = types.SimpleNamespace(**MODEL_CONFIG)
    out = {"config": MODEL_CONFIG, "models": {}, "layers": {}}
    for inj in INJECTIONS:
        out["models"][inj] = _keys(model_mod.SNNRAGTransformer(cfg, None, memory_injection=inj))
        for snn in (False, True):
            layer = layer_mod.MemoryAugmentedLayer(cfg, None, use_snn_ffn=snn, memory_injection=inj)
            out["layers"][f"{inj}-{'snn' if snn else 'mlp'}"] = _keys(layer)
    return out


def build_layers(layer_mod):
    out = {"shape": (B, S, D, H, K), "cases": {}}
    for n, inj in enumerate(INJECTIONS):
        torch.manual_seed(300 + n)
        cfg = types.SimpleNamespace(embedding_dim=D, num_heads=H, dropout=0.0, intermediate_size=2 * D)
        bank = StandInBank(torch.randn(B, K, D), torch.rand(B, K))
        layer = layer_mod.MemoryAugmentedLayer(cfg, bank, use_snn_ffn=False, memory_injection=inj,
                                               num_retrieved=K).eval()
        with torch.no_grad():
            for norm in (layer.attention_norm, layer.ffn_norm):             # norms that are not the identity
                norm.weight.add_(0.3 * torch.randn(D))
                norm.bias.add_(0.3 * torch.randn(D))
        hidden, prosody = torch.randn(B, S, D), 1.5 * torch.randn(B, S, 4)
        with torch.no_grad():
            outs = {"memory": layer(hidden, prosody=prosody, use_memory=True),
                    "no_memory": layer(hidden, prosody=prosody, use_memory=False)}
        assert bank.calls == B, "one retrieval per batch row"
        out["cases"][inj] = {"state_dict": {k: v.clone() for k, v in layer.state_dict().items()}, "hidden": hidden,
                             "prosody": prosody, "features": bank.features, "scores": bank.scores, "outputs": outs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    from oracle import _ref_loader
    if not _ref_loader.available():
        raise SystemExit("gen_golden_snn_rag.py needs the reference checkout (oracle/_ref_loader.py); not found")
    layer_mod = _ref_loader.load("src.core.language_zone.memory_augmented_layer")
    model_mod = _ref_loader.load("src.core.language_zone.snn_rag_transformer")
    keys = build_keys(model_mod, layer_mod)
    path = os.path.join(a.dir, "snn_rag_transformer_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path)} bytes; keys per model "
          f"{ {k: len(v) for k, v in keys['models'].items()} }")
    data = build_layers(layer_mod)
    path = os.path.join(a.dir, "memory_augmented_layer.pt")
    torch.save(data, path)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(data['cases'])} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
