"""The language zone's modules behind the reference's names: ``gif_neuron``, ``snn_ffn``, ``synapsis``, ``prosody_gif``,
``place_cell_encoder``, ``theta_gamma_encoding``, ``prosody_attention``, ``hippocampal_attention``,
``hippocampal_layer`` and ``hippocampal_transformer``.  Nothing is imported here: every module imports torch, and the
package root maps the public names lazily (``aura_snn_rag_amd.HippocampalTransformer`` and the others)."""
