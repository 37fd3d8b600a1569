"""engine._render_layers: the one statement of which linear layers a module's render path reads.  The lists below were written down from
training._param_names as it stood before that function existed (its order is the order of _RenderTrain.apply's tensor arguments and of the
gradients its backward returns), for every way the staged route makes the per-sample features, with and without the second round."""
import pytest

from cross_attention_renderer_amd.engine import _mode, _render_layers
from cross_attention_renderer_amd.models import CrossAttentionRenderer
from cross_attention_renderer_amd.training import _param_names

DECODER = ("phi.lin_in phi.lin_out phi.lin_z.0 phi.blocks.0.fc_0 phi.blocks.0.fc_1 phi.lin_z.1 phi.blocks.1.fc_0 phi.blocks.1.fc_1 "
           "phi.lin_z.2 phi.blocks.2.fc_0 phi.blocks.2.fc_1")
PARENT = {
    ("concat2", True): "query_encode_latent query_encode_latent_2 latent_value key_map key_map_2 query_embed query_embed_2 "
                       "query_repeat_embed query_repeat_embed_2 encode_latent " + DECODER,
    ("concat2", False): "query_encode_latent query_encode_latent_2 latent_value key_map key_map_2 query_embed query_embed_2 " + DECODER,
    ("concat3", True): "query_encode_latent query_encode_latent_2 latent_value key_map key_map_2 query_embed query_embed_2 "
                       "query_repeat_embed query_repeat_embed_2 encode_latent " + DECODER,
    ("concat3", False): "query_encode_latent query_encode_latent_2 latent_value key_map key_map_2 query_embed query_embed_2 " + DECODER,
    ("single", True): "update_val_merge latent_value key_map key_map_2 query_embed query_embed_2 "
                      "query_repeat_embed query_repeat_embed_2 encode_latent " + DECODER,
    ("single", False): "update_val_merge latent_value key_map key_map_2 query_embed query_embed_2 " + DECODER,
    ("plain", True): "latent_value key_map key_map_2 query_embed query_embed_2 query_repeat_embed query_repeat_embed_2 encode_latent " + DECODER,
    ("plain", False): "latent_value key_map key_map_2 query_embed query_embed_2 " + DECODER,
}
CONSTRUCTOR = {"concat2": dict(n_view=2), "concat3": dict(n_view=3), "single": dict(n_view=1), "plain": dict(n_view=2, no_latent_concat=True)}


@pytest.mark.parametrize("mode,repeat", sorted(PARENT))
def test_the_shared_layer_list_yields_the_parameters_of_the_training_step_in_their_order(mode, repeat):
    m = CrossAttentionRenderer(model="tiny", repeat_attention=repeat, with_encoder=False, **CONSTRUCTOR[mode])
    assert _mode(m) == mode
    want = [n + k for n in PARENT[(mode, repeat)].split() for k in (".weight", ".bias")]
    layers = _render_layers(m)
    got = layers.head + layers.attention + (layers.round2 if repeat else []) + layers.decoder
    assert [n + k for n in got for k in (".weight", ".bias")] == want
    assert _param_names(m) == want
    named = dict(m.named_parameters())
    # every part names parameters of the module: the second round's layers exist whether or not the path reads them
    for n in layers.head + layers.attention + layers.round2 + layers.decoder:
        assert n + ".weight" in named and n + ".bias" in named, n
