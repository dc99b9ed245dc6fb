"""The language zone's modules behind the reference's names: ``gif_neuron``, ``snn_ffn``, ``synapsis``, ``prosody_gif``,
``place_cell_encoder``, ``theta_gamma_encoding``, ``prosody_attention``, ``hippocampal_attention`` and
``hippocampal_layer``.  Nothing is imported here: every module imports torch, and the package root maps the public
names lazily (``aura_snn_rag_amd.HippocampalProsodyAttention`` and the others)."""
