"""The encoder's transformer stage without a GPU: tests/vit_reference.py (the float64 restatement the GPU tests of test_vit_hip.py are judged
against) held to the package's own encoder.Block / encoder.Attention, the ctypes table of include/car_encoder.h held to the header, and the
renderer's encoder_route switch."""
import ctypes
import os
import re

import pytest
import torch

import vit_reference as VR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F64 = torch.float64


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("dim,heads,b,S", [(128, 2, 2, 37), (768, 12, 1, 70)])
def test_restatement_is_the_encoders_block(dim, heads, b, S):
    """One block and its attention, float64, from the module's own parameters in PARAM_ORDER: 1e-12 relative."""
    from cross_attention_renderer_amd import encoder
    torch.manual_seed(dim)
    blk = encoder.Block(dim, heads).double()
    with torch.no_grad():
        for p in blk.parameters():                                     # nothing at an initial value (the biases start at zero)
            p.add_(0.1 * torch.randn_like(p))
        P = VR.block_params(blk)
        tok = torch.randn(b, S, dim, dtype=F64)
        want = blk(tok).reshape(b * S, dim)
        got, bound = VR.block(tok.reshape(b * S, dim), P, b, S, heads, F64)
        assert _rel(got, want) < 1e-12
        assert bound.shape == (b * S, 1) and bool((bound >= got.abs().amax(dim=1, keepdim=True) * (1 - 1e-15)).all())
        x = torch.randn(b, S, dim, dtype=F64)
        want_a = blk.attn(x).reshape(b * S, dim)
        qkv, _ = VR.linear(x.reshape(b * S, dim), P[2], P[3], F64)
        a, Ba = VR.attention(qkv, b, S, heads, F64)
        got_a, _ = VR.linear(a, P[4], P[5], F64)
        assert _rel(got_a, want_a) < 1e-12
        assert bool((Ba >= a.abs() * (1 - 1e-12)).all())                  # sum p |v| bounds |sum p v|
        n, Bn = VR.layernorm(x.reshape(b * S, dim), P[0], P[1])
        assert _rel(n, blk.norm1(x).reshape(b * S, dim)) < 1e-12 and bool((Bn >= n.abs() * (1 - 1e-12)).all())
        g, Bg = VR.gelu(x)
        assert _rel(g, torch.nn.functional.gelu(x)) < 1e-12 and torch.equal(Bg, x.abs())


def test_stage_is_the_blocks_in_sequence_with_taps():
    from cross_attention_renderer_amd import encoder
    torch.manual_seed(5)
    dim, heads, b, S, depth = 128, 2, 2, 9, 3
    blocks = [encoder.Block(dim, heads).double() for _ in range(depth)]
    with torch.no_grad():
        for blk in blocks:
            for p in blk.parameters():
                p.add_(0.1 * torch.randn_like(p))
        params = [t for blk in blocks for t in VR.block_params(blk)]
        tok = torch.randn(b, S, dim, dtype=F64)
        x, want = tok, {}
        for i, blk in enumerate(blocks):
            x = blk(x)
            want[i] = x.reshape(b * S, dim)
        got, bound, tapped = VR.stage(tok.reshape(b * S, dim), params, b, S, heads, taps=(1, 2))
    assert _rel(got, want[2]) < 1e-12 and len(tapped) == 2
    assert _rel(tapped[0][0], want[1]) < 1e-12 and _rel(tapped[1][0], want[2]) < 1e-12
    assert torch.equal(bound, got.abs().amax(dim=1, keepdim=True))


def test_a_scene_attends_to_its_own_rows_only():
    """The restatement's own reading of `b`: scene 1's rows do not reach scene 0's result, and the yardstick is the same formula in float32."""
    qkv = VR.mha_input("gauss", 2, 5, 2)
    both, _ = VR.attention(qkv, 2, 5, 2)
    other = qkv.clone()
    other[5:] = torch.randn(5, qkv.shape[1])
    assert torch.equal(VR.attention(other, 2, 5, 2)[0][:5], both[:5])
    ref, B, y32 = VR.mha_reference("gauss", 2, 5, 2)
    assert y32.dtype == torch.float32 and ref.dtype == F64 and float(((y32.double() - ref).abs() / B).max()) < 1e-5
    dom = VR.mha_input("dominant", 2, 5, 2)
    ref, _ = VR.attention(dom, 2, 5, 2)
    assert float((ref - VR.dominant_rows(dom, 2, 5, 2).double()).abs().max()) < 1e-12      # weight 1 - S e^-80
    uni = VR.mha_input("uniform", 1, 32, 1)
    ref, _ = VR.attention(uni, 1, 32, 1)
    assert torch.equal(ref, uni[:, 128:].double().mean(dim=0, keepdim=True).expand(32, 64))


def test_encoder_signatures_mirror_their_header_type_by_type():
    """include/car_encoder.h against _lib.ENCODER_SIGNATURES, by test_abi's own comparison: names, return types, arity, each parameter's kind.
    The header is included by car_hip.h, inside its extern "C" block, and holds nothing but the encoder's entries; the source hash and the
    build's unit table know the new files."""
    import test_abi as T
    from cross_attention_renderer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "car_encoder.h")).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(car_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in " ".join(params.split()).split(",")]
        params = [] if params == ["void"] else ["*" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const") for p in params]
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    assert len(protos) == 9 == len(_lib.ENCODER_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.MATCH_SIGNATURES))
    assert T._abi_disagreements(protos, _lib.ENCODER_SIGNATURES) == []
    assert all(n.startswith(("car_layernorm", "car_gelu", "car_mha", "car_vit_")) for n in protos)
    hip_h = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    assert '#include "car_encoder.h"' in hip_h and hip_h.index('#include "car_encoder.h"') < hip_h.index("#ifdef __cplusplus\n}")
    assert "#define CAR_VERSION 300" in hip_h                                                  # additive entries: the number stays
    import __graft_entry__ as G
    assert "car_vit.hip" in G.UNITS
    src = open(os.path.join(ROOT, "cross_attention_renderer_amd", "_lib.py")).read()
    assert '"car_encoder.h"' in src[src.index("def source_hash"):src.index("def _rebuild_stale")]


def test_encoder_entries_are_exported_bound_and_refuse_without_a_device():
    """Every entry on both handles, the checked one raising; the sizes and the refusals need no GPU (a refused call launches nothing)."""
    from cross_attention_renderer_amd import _lib
    lib, api = _lib.load(), _lib.api()
    for name, (res, _) in _lib.ENCODER_SIGNATURES.items():
        assert hasattr(lib, name), name
        assert (getattr(api, name).errcheck is _lib._errcheck) == (res is ctypes.c_int), name
    _lib.check_exports()
    assert lib.car_version() == 300
    with pytest.raises(_lib.CarError, match="null pointer"):
        api.car_mha(None, 0, 1, 1, 1, None, 0, None, 0, None)
    # sizes: one tile record is 16 KB (k and v as hi / lo halves); a refused shape gives 0 with a message
    one = lib.car_mha_workspace_bytes(1, 32, 1)
    assert lib.car_mha_workspace_bytes(1, 33, 1) - one == 16384 and lib.car_mha_workspace_bytes(1, 1, 1) == one
    for bad in ((1, 0, 1), (1, 1025, 1), (1, 5, 0), (1, 5, 17), (0, 5, 1)):
        assert lib.car_mha_workspace_bytes(*bad) == 0 and b"outside" in lib.car_last_error(), bad
    for dim in (0, 32, 96, 1088):
        assert lib.car_vit_packed_floats(dim, 1) == 0 and b"multiple of 64" in lib.car_last_error()
        assert lib.car_vit_workspace_bytes(1, 5, dim) == 0
    assert lib.car_vit_packed_floats(128, 0) == 0 and lib.car_vit_packed_floats(128, 33) == 0 and b"depth" in lib.car_last_error()
    per = lib.car_vit_packed_offset(768, 12)
    assert lib.car_vit_packed_floats(768, 12) == 12 * per
    sizes = [768, 768, lib.car_linear_x3_packed_floats(768, 2304), 2304, lib.car_linear_x3_packed_floats(768, 768), 768, 768, 768,
             lib.car_linear_x3_packed_floats(768, 3072), 3072, lib.car_linear_x3_packed_floats(3072, 768), 768]
    off = 0
    for i, n in enumerate(sizes):
        assert lib.car_vit_packed_offset(768, i) == off and off % 4 == 0
        off += (n + 3) & ~3
    assert off == per
    assert lib.car_vit_workspace_bytes(1, 514, 768) >= 514 * 768 * 4 * 6 + lib.car_mha_workspace_bytes(1, 514, 12)


def test_encoder_route_switch():
    from cross_attention_renderer_amd.encoder import MultiViewDPTEncoder
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    bare = CrossAttentionRenderer(model="midas_vit", n_view=2, with_encoder=False)
    assert bare.encoder_route == "torch"
    bare.encoder_route = "torch"
    with pytest.raises(ValueError, match="EncoderNotBuilt has no vit_route"):
        bare.encoder_route = "device"
    with pytest.raises(ValueError, match="must be 'torch' or 'device'"):
        bare.encoder_route = "hip"
    own = CrossAttentionRenderer(model="midas_vit", n_view=2, encoder=torch.nn.Identity())
    with pytest.raises(ValueError, match="Identity has no vit_route"):
        own.encoder_route = "device"
    enc = MultiViewDPTEncoder()
    assert enc.vit_route == "torch"
    with pytest.raises(ValueError, match="vit_route must be"):
        enc.vit_route = "cuda"
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, encoder=enc)
    assert m.encoder_route == "torch"
    m.encoder_route = "device"
    assert enc.vit_route == "device" and m.encoder_route == "device"
    assert not any("vit" in k and "route" in k for k in m.state_dict())
    # the device route refuses CPU tensors instead of falling back (the check comes before anything touches the library)
    with torch.no_grad(), pytest.raises(ValueError, match="CPU tensors run on vit_route = 'torch'"):
        enc(torch.zeros(2, 3, 256, 256), torch.zeros(2, 16), 2)
    m.encoder_route = "torch"
    assert enc.vit_route == "torch"
    assert len(enc._vit_parameters()) == 144
    assert all(a is b for a, b in zip(enc._vit_parameters()[:12], VR.block_params(enc.pretrained.model.blocks[0])))


def test_encoder_route_flag_parses_and_reaches_the_model():
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("car_scripts_common", os.path.join(ROOT, "experiment_scripts", "common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    p = common.parser("t")
    assert p.parse_args(["--experiment_name", "x"]).encoder_route == "torch"
    opt = p.parse_args(["--experiment_name", "x", "--encoder_route", "device", "--synthetic"])
    assert opt.encoder_route == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--experiment_name", "x", "--encoder_route", "hip"])
    # a renderer-only model (no checkpoint, no --with_encoder: what eval --synthetic builds) never calls get_z and ignores the flag
    model = common.build_model(opt, torch.device("cpu"))
    assert model.encoder_route == "torch" and type(model.encoder).__name__ == "EncoderNotBuilt"
