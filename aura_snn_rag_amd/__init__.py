"""aura_snn_rag_amd -- MI355X-native (gfx950) implementation of Aura's SNN-timestep +
episodic-retrieval hot path, behind the reference's own module API.

    from aura_snn_rag_amd.core.hippocampal import HippocampalFormation
    from aura_snn_rag_amd.base.neuron import IzhikevichNeuron, AdExNeuron, VectorizedLIFNeuron
    from aura_snn_rag_amd.core.language_zone.gif_neuron import GIFNeuron
    from aura_snn_rag_amd.core.language_zone.snn_ffn import SNNFFN, HybridFFN
    from aura_snn_rag_amd import PlaceCellSemanticEncoder, PlaceCode
    from aura_snn_rag_amd import ThetaGammaPositionalEncoding, embed_tokens
    from aura_snn_rag_amd import ProsodyAttentionBridge, MultiChannelSpikingAttention, prosody_channels_from_text
    from aura_snn_rag_amd import HippocampalProsodyAttention, HippocampalTransformerLayer, AttentionCache
    from aura_snn_rag_amd import HippocampalTransformer, DecodeState      # forward, prefill / step, generate
    from aura_snn_rag_amd import SNNRAGTransformer, MemoryAugmentedLayer, MemoryContext     # generation with memory
    from aura_snn_rag_amd import MoELanguageZone, LiquidMoERouter, SNNExpert                # fused routing and experts
    from aura_snn_rag_amd import ZoneState                                 # MoELanguageZone's prefill / step / generate

All arithmetic on the path runs in ``lib/libaura_hip.so`` (hand-written HIP, C ABI in
``include/aura_hip.h``); there is no CPU or eager-PyTorch fallback.
"""
from ._lib import AuraHipError, AuraHipUnavailable, load as load_library  # noqa: F401

__version__ = "0.1.0"

_LAZY = {"PlaceCellSemanticEncoder": "core.language_zone.place_cell_encoder",
         "PlaceCode": "core.language_zone.place_cell_encoder",
         "ThetaGammaPositionalEncoding": "core.language_zone.theta_gamma_encoding",
         "embed_tokens": "core.language_zone.theta_gamma_encoding",
         "MultiChannelSpikingAttention": "core.language_zone.prosody_attention",
         "ProsodyAttentionBridge": "core.language_zone.prosody_attention",
         "prosody_channels_from_text": "core.language_zone.prosody_attention",
         "HippocampalProsodyAttention": "core.language_zone.hippocampal_attention",
         "AttentionCache": "core.language_zone.hippocampal_attention",
         "HippocampalTransformerLayer": "core.language_zone.hippocampal_layer",
         "HippocampalTransformer": "core.language_zone.hippocampal_transformer",
         "DecodeState": "core.language_zone.hippocampal_transformer",
         "CachedDecodingMixin": "core.language_zone.hippocampal_transformer",
         "MemoryAugmentedLayer": "core.language_zone.memory_augmented_layer",
         "MemoryContext": "core.language_zone.memory_augmented_layer",
         "MemoryLayerCache": "core.language_zone.memory_augmented_layer",
         "FoldedMemory": "core.language_zone.memory_augmented_layer",
         "SNNRAGTransformer": "core.language_zone.snn_rag_transformer",
         "MoELanguageZone": "core.language_zone.moe_language_zone",
         "MoEOutput": "core.language_zone.moe_language_zone",
         "ZoneState": "core.language_zone.moe_language_zone",
         "SNNExpert": "core.language_zone.snn_expert",
         "LiquidMoERouter": "core.liquid_moe"}


def __getattr__(name):
    # the modules import torch; the package itself (and the ctypes loader) does not
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
