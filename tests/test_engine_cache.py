"""``-m gpu``: the render engine's caches (engine._Cached) never serve what was built from other parameter values or another plan.  A
module whose parameters changed between forwards renders exactly what a module built afresh from the same state dict renders."""
import pytest
import torch

import cases as C
from golden_util import load_case
from hip_harness import build_module, to_device

pytestmark = pytest.mark.gpu

KEYS = ("rgb", "depth_ray", "at_wt", "valid_mask", "at_wt_max", "pixel_val")
# one parameter of each cached family that the case has: packed layers and plan (phi.lin_out), projected levels (query_encode_latent),
# the three-view exchange's pack (query_encode_latent_2), key / query pack (key_map_2), round-2 pack (query_repeat_embed_2), the
# single-view merge (update_val_merge)
FAMILIES = ("phi.lin_out.weight", "query_encode_latent.weight", "query_encode_latent_2.bias", "key_map_2.weight",
            "query_repeat_embed_2.weight", "update_val_merge.weight")
STAGED = ("t1_nview1", "t1_nview3", "t1_no_latent_concat")


def _setup(name, precision, dev):
    c, inp, z, sd, _ = load_case(name)
    m = build_module(c, sd, dev)
    m.render_precision = precision
    return c, m, to_device(inp, dev, cameras_on_host=True), [t.to(dev) for t in z]


def _render(m, inp, z):
    with torch.no_grad():
        out = m(inp, z=z)
    return {k: out[k].clone() for k in KEYS}


def _assert_fresh_module_agrees(c, m, precision, inp, z, got):
    fresh = build_module(c, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, z[0].device)
    fresh.render_precision = precision
    want = _render(fresh, inp, z)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("name,precision", [("t1_c1", "fp32"), ("t1_c1", "fp16")] + [(n, "fp32") for n in STAGED])
def test_in_place_update_between_forwards(name, precision):
    dev = torch.device("cuda:0")
    c, m, inp, z = _setup(name, precision, dev)
    first = _render(m, inp, z)
    assert (m._engine._pair is not None) == (name == "t1_c1")         # the one-call route, or the staged one
    params = dict(m.named_parameters())
    with torch.no_grad():
        for n in FAMILIES:
            if n in params:
                params[n].mul_(1.5)
    got = _render(m, inp, z)
    assert not torch.equal(got["rgb"], first["rgb"])
    _assert_fresh_module_agrees(c, m, precision, inp, z, got)


@pytest.mark.parametrize("name", ["t1_c1", *STAGED])
def test_parameter_replaced_at_a_recycled_address(name):
    """``p.data = new`` keeps the Parameter's _version: a cache keyed on (data pointer, _version) alone matches the new values when the
    allocator hands the freed block back.  Whether it did is printed; either way the new values must be rendered."""
    dev = torch.device("cuda:0")
    c, m, inp, z = _setup(name, "fp32", dev)
    first = _render(m, inp, z)
    p = m.query_repeat_embed.weight                                    # packed by _weights, the round-2 pack and the plan
    old, new = p.data_ptr(), p.detach().cpu() * 1.5                    # the new values made on the host: no device block of that size freed
    p.data = torch.empty(0, device=dev)
    p.data = new.to(dev)
    print(f"{name}: address reused: {p.data_ptr() == old}")
    got = _render(m, inp, z)
    assert not torch.equal(got["rgb"], first["rgb"])
    _assert_fresh_module_agrees(c, m, "fp32", inp, z, got)


def test_prefetched_pair_across_a_weight_change():
    """A pair announced with one plan and rendered after the parameters changed: the announced entry keeps the plan its side-stream
    projection read (its block is not handed to the rebuilt plan), and the forward re-projects with the new plan."""
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    dev = torch.device("cuda:0")
    H, P, R, b = 64, 16, 120, 2

    def module():
        f = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=P, with_encoder=False).eval()
        f.H = f.W = H
        return f

    torch.manual_seed(0)
    m = module()
    S.perturb_parameters(m, seed=3)
    m = m.to(dev)
    inp = to_device(S.stereo_scene(H, b=b, uv=C.select_rays(H, R), seed=4, alpha=0.4), dev, cameras_on_host=True)
    za, zb = ([t.to(dev) for t in S.feature_maps(b, 2, H, seed=sd)] for sd in (1, 2))
    with torch.no_grad():
        m(inp, z=za)
        eng = m._engine
        read = eng._plan_for(eng._dims(b, R, zb), dev)                 # the plan in place
        assert m.prefetch_pair(zb)
        (entry,) = eng._pf.values()
        m.phi.lin_out.weight.mul_(1.5)
        rebuilt = eng._plan_for(eng._dims(b, R, zb), dev)
        assert rebuilt is not read and entry["plan"] is read and rebuilt.data_ptr() != read.data_ptr()
        got = _render(m, inp, zb)
        assert not eng._pf, "the forward did not take the announced pair over"
    fresh = module()
    fresh.load_state_dict(m.state_dict())
    want = _render(fresh.to(dev), inp, zb)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
