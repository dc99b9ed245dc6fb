"""The language zone's modules behind the reference's names: ``gif_neuron``, ``snn_ffn``, ``synapsis``, ``prosody_gif``,
``place_cell_encoder``, ``theta_gamma_encoding``, ``prosody_attention``, ``hippocampal_attention``,
``hippocampal_layer``, ``hippocampal_transformer``, ``spike_bridge``, ``snn_expert`` and ``moe_language_zone`` (its
router is ``core.liquid_moe``).  Nothing is imported here: every module imports torch, and the
package root maps the public names lazily (``aura_snn_rag_amd.HippocampalTransformer`` and the others)."""
