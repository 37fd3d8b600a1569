"""CPU checks for the encoder's back half: the restatement of tests/decoder_reference.py (what the GPU suite compares the kernels against)
held to encoder.py's own modules run in float64 and to F.interpolate, the normalisation held to get_z's lines bit for bit, the ctypes table
of include/car_decoder.h held to the header, the sizes and refusals that need no device, and the renderer's fourth encoder_route value."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import decoder_reference as DR
from cross_attention_renderer_amd import encoder as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
REL = 1e-12                       # of the bound that goes with the value


def _close(got, want, bound, what):
    err = (got.double() - want.double()).abs()
    assert bool((err <= REL * bound).all()), (what, float((err / bound).max()))
    assert bool((bound >= got.abs() * (1 - 1e-12)).all()), what


def _cl(t):                       # NCHW -> channel-last rows
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


def _load(params, values):
    with torch.no_grad():
        for p, v in zip(params, values, strict=True):
            p.copy_(v.to(p.dtype))


def _rand(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=DR.gen(seed), dtype=F64)


# ---- the pieces against encoder.py -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,P", [(64, 1), (64, 6), (768, 4)])
def test_readout_in_its_split_form_is_project_readout(dim, P):
    mod = E.ProjectReadout(dim).double()
    w, b = _rand((dim, 2 * dim), dim, dim ** -0.5), _rand((dim,), P, 0.1)
    _load(mod.parameters(), [w, b])
    tok = _rand((3, 1 + P, dim), dim + P)
    tok[:, 0] *= 1e2                                                    # the class row dominates: the split form must not lose the patch term
    with torch.no_grad():
        want = mod(tok)
    got, bound, _ = DR.readout(tok, w, b)
    _close(got, want, 1.2 * bound, "readout")                          # GELU's slope stays below 1.13


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4)])
def test_residual_unit_and_strided_layer(H, W):
    C = 16
    mod = E.ResidualConvUnit(C).double()
    p = [_rand((C, C, 3, 3), 1, 0.1), _rand((C,), 2, 0.1), _rand((C, C, 3, 3), 3, 0.1), _rand((C,), 4, 0.1)]
    _load(mod.parameters(), p)
    x = _rand((2, C, H, W), H * 10 + W)
    with torch.no_grad():
        want = mod(x)
        strided = F.conv2d(x, p[0], p[1], stride=2, padding=1)
    got, bound = DR.rcu(_cl(x), H, W, p)
    _close(got, _cl(want), bound, "rcu")
    got, bound = DR.conv3x3_pad1(_cl(x), H, W, p[0], stride=2, bias=p[1])
    assert strided.shape[-2:] == (DR.pad1_out(H, 2), DR.pad1_out(W, 2))
    _close(got, _cl(strided), bound, "stride 2")
    # the epilogue's order: act_out((conv + bias) + add) + y
    add, y = _rand(got.shape, 5), _rand(got.shape, 6)
    full, _ = DR.conv3x3_pad1(_cl(x), H, W, p[0], stride=2, bias=p[1], add=add, flags=DR.RELU_IN | DR.RELU_OUT | DR.ACCUM, y=y)
    with torch.no_grad():
        want = torch.relu(_cl(F.conv2d(torch.relu(x), p[0], p[1], stride=2, padding=1)) + add) + y
    assert float((full - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("skip", [False, True])
def test_fusion_block(skip):
    mod = E.FeatureFusionBlock(DR.FUSE).double()
    shapes = [tuple(p.shape) for p in mod.parameters()]
    p = [_rand(s, i, 0.1 if len(s) == 1 else (s[1] * s[2] * s[3]) ** -0.5) for i, s in enumerate(shapes)]
    _load(mod.parameters(), p)
    assert [n for n, _ in mod.named_parameters()][:4] == ["out_conv.weight", "out_conv.bias", "resConfUnit1.conv1.weight", "resConfUnit1.conv1.bias"]
    h, w = 3, 2
    x, s = _rand((2, DR.FUSE, h, w), 7), _rand((2, DR.FUSE, h, w), 8)
    with torch.no_grad():
        want = mod(x, s) if skip else mod(x)
    got, bound = DR.fusion(_cl(x), h, w, p, skip=_cl(s)) if skip else DR.fusion(_cl(x), h, w, p[:2] + p[6:])
    assert want.shape[-2:] == (2 * h, 2 * w)
    _close(got, _cl(want), bound, "fusion")


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 2), (3, 7), (16, 16), (2, 3)])
def test_upsampling_is_interpolate_with_aligned_corners(H, W):
    x = _rand((2, 4, H, W), H * 17 + W)
    want = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    got, bound = DR.upsample2x(_cl(x), H, W)
    _close(got, _cl(want), bound, "upsample2x")
    got = got.reshape(2, 2 * H, 2 * W, 4)
    for oy, iy in ((0, 0), (2 * H - 1, H - 1)):
        for ox, ix in ((0, 0), (2 * W - 1, W - 1)):
            assert torch.equal(got[:, oy, ox], x[:, :, iy, ix]), "a corner is the input's corner"
    const = torch.full((1, H * W, 4), 0.3, dtype=F32)
    assert torch.equal(DR.upsample2x(const, H, W, F32)[0], torch.full((1, 4 * H * W, 4), 0.3, dtype=F32))


def test_conv7x7_is_conv_map():
    w, b = _rand((64, 3, 7, 7), 1, 0.1), _rand((64,), 2, 0.1)
    for H, W in ((1, 1), (3, 5), (8, 8)):
        x = _rand((2, 3, H, W), H)
        got, bound = DR.conv7x7(x, w, b)
        _close(got, _cl(F.conv2d(x, w, b, padding=3)), bound, "conv7x7")


def test_normalize_is_get_zs_lines_bit_for_bit():
    rgb = torch.rand(2, 9, 7, 3, generator=DR.gen(3)) * 2 - 1
    rgb[0, 0, 0] = torch.tensor([-1.0, 1.0, 0.0])
    x = rgb.permute(0, -1, 1, 2)                                       # models.get_z, lines 213-216
    x = (x + 1) / 2.0
    mean = x.new_tensor([0.485, 0.456, 0.406])[None, :, None, None]
    std = x.new_tensor([0.229, 0.224, 0.225])[None, :, None, None]
    x = (x - mean) / std
    assert torch.equal(DR.normalize(rgb).view(torch.int32), x.contiguous().view(torch.int32))


def test_decoder_is_the_tail_of_the_encoders_forward():
    """MultiViewDPTEncoder.forward from the tapped states on, in float64 at the one size it takes (a 16 x 16 grid): the trunk and the blocks
    are replaced by seeded values through the two device hooks, so what runs is forward's own read-out, re-assembly and fusion."""
    enc = E.MultiViewDPTEncoder()
    params = enc._decoder_parameters()
    assert [tuple(p.shape) for p in params] == DR.decoder_shapes() and len(params) == 50
    names = {id(p): n for n, p in enc.named_parameters()}
    order = [n for n in enc.state_dict() if ("act_postprocess" in n or n.startswith("scratch.")) and "output_conv" not in n and "refinenet4.resConfUnit1" not in n]
    assert [names[id(p)] for p in params] == order                     # state_dict order of what is evaluated
    enc.scratch.double(); enc.pretrained.act_postprocess3.double(); enc.pretrained.act_postprocess4.double()
    _load(params, DR.seeded_decoder())
    BV, gh, gw = 1, 16, 16
    tap3, tap4 = _rand((BV, 257, 768), 1), _rand((BV, 257, 768), 2)
    l1, l2 = torch.relu(_rand((BV, 256, 64, 64), 3)), torch.relu(_rand((BV, 512, 32, 32), 4))
    enc.trunk_route = enc.vit_route = "device"
    enc._front_on_device = lambda x, pose, gh_, gw_: (l1, l2, torch.zeros(BV, 257, 768, dtype=F64))
    enc._blocks_on_device = lambda tok, x, BV_, T: {8: tap3, 11: tap4}
    with torch.no_grad():
        want = enc(torch.zeros(BV, 3, 256, 256), torch.zeros(BV, 16), 1)
    got = DR.decoder(tap3, tap4, _cl(l1), _cl(l2), gh, gw, DR.seeded_decoder())
    for (g, b), w_, name in zip(got, want, ("path_2", "path_1")):
        assert g.shape[1] == w_.shape[-1] * w_.shape[-2]
        _close(g, _cl(w_), b, name)


# ---- the C ABI's table, sizes and refusals (no device) ---------------------------------------------------------------------------------------
def test_decoder_signatures_mirror_their_header_type_by_type():
    import test_abi as T
    from cross_attention_renderer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "car_decoder.h")).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(car_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in " ".join(params.split()).split(",")]
        params = [] if params == ["void"] else ["*" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const") for p in params]
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    assert len(protos) == 16 == len(_lib.DECODER_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.MATCH_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.TRUNK_SIGNATURES))
    assert T._abi_disagreements(protos, _lib.DECODER_SIGNATURES) == []
    hip_h = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    assert hip_h.index('#include "car_trunk.h"') < hip_h.index('#include "car_decoder.h"') < hip_h.index("#ifdef __cplusplus\n}")
    assert "#define CAR_VERSION 300" in hip_h                                                  # additive entries: the number stays
    import __graft_entry__ as G
    assert G.UNITS["car_decoder.hip"] == []                                                    # the sweep's arithmetic: the flags of the other units that include it
    src = open(os.path.join(ROOT, "cross_attention_renderer_amd", "_lib.py")).read()
    assert '"car_decoder.h"' in src[src.index("def source_hash"):src.index("def _rebuild_stale")]
    assert "DECODER_SIGNATURES" in src[src.index("def check_exports"):src.index("def check(")]
    for flag, value in (("CAR_LIN_RELU_IN", DR.RELU_IN), ("CAR_LIN_RELU_OUT", DR.RELU_OUT), ("CAR_LIN_ACCUM", DR.ACCUM)):
        assert re.search(rf"#define {flag}\s+{value}\b", hip_h), flag


def test_decoder_entries_are_exported_bound_and_refuse_without_a_device():
    import __graft_entry__ as G
    G.build()
    from cross_attention_renderer_amd import _lib
    lib, api = _lib.load(), _lib.api()
    for name, (res, _) in _lib.DECODER_SIGNATURES.items():
        assert hasattr(lib, name), name
        assert (getattr(api, name).errcheck is _lib._errcheck) == (res is ctypes.c_int), name
    with pytest.raises(_lib.CarError, match="null pointer"):
        api.car_conv3x3_pad1(None, 1, 1, 1, 256, 256, 1, None, None, None, 0, None, None)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    msg = lambda: lib.car_last_error().decode()
    # sizes: the 3x3 layer is car_conv3x3_same_pack's tiles and 64 floats of scale
    for K in (256, 512, 768):
        for N in (256, 768):
            assert lib.car_conv3x3_pad1_packed_floats(K, N) == 9 * K * N + 64
    for bad in ((64, 256), (256, 512), (768, 64), (1024, 256)):
        assert lib.car_conv3x3_pad1_packed_floats(*bad) == 0 and msg().startswith("car_conv3x3_pad1_packed_floats"), bad
    lin = lib.car_linear_x3_packed_floats
    assert lib.car_readout_packed_floats(768) >= 2 * lin(768, 768) + 768 and lib.car_readout_packed_floats(64) >= 2 * lin(64, 64) + 64
    for bad in (0, 32, 100, 2048):
        assert lib.car_readout_packed_floats(bad) == 0 and msg().startswith("car_readout_packed_floats"), bad
    assert lib.car_readout_workspace_bytes(2, 256, 768) == (2 * 257 * 768 + 2 * 768) * 4
    for bad in ((0, 4, 64), (1, 0, 64), (1, 4, 96 + 4), (4097, 4, 64), (1, 4097, 64)):
        assert lib.car_readout_workspace_bytes(*bad) == 0 and msg().startswith("car_readout_workspace_bytes"), bad
    assert lib.car_decoder_packed_floats() >= 2 * lib.car_readout_packed_floats(768) + 2 * lin(768, 768) + 9 * 768 * 768 + 9 * 256 * (256 + 512 + 768 + 768) \
        + 14 * 9 * 256 * 256 + 4 * lin(256, 256)
    small, pair = lib.car_decoder_workspace_bytes(2, 2, 2), lib.car_decoder_workspace_bytes(2, 16, 16)
    assert pair >= 2 * 256 * (3 * 768 + 7 * 16 * 256) * 4 > small > 0
    for bad in ((0, 2, 2), (1, 1, 2), (1, 2, 3), (1, 66, 2), (1, 2, 0), (4097, 2, 2)):
        assert lib.car_decoder_workspace_bytes(*bad) == 0 and msg().startswith("car_decoder_workspace_bytes"), bad
    d = ints(3, 4, 9)
    whole = lib.car_getz_workspace_bytes(2, 256, 256, 16, 16, 2, d, 12)
    assert whole > pair and whole > lib.car_trunk_workspace_bytes(2, 256, 256, d) and whole > lib.car_vit_workspace_bytes(1, 514, 768)
    assert lib.car_getz_workspace_bytes(2, 32, 32, 2, 2, 1, ints(1, 1, 1), 2) > 0
    for bad in ((3, 256, 256, 16, 16, 2, d, 12),        # BV no multiple of nviews
                (2, 256, 256, 16, 14, 2, d, 12),        # the image does not give the grid
                (2, 250, 256, 16, 16, 2, d, 12),        # ceil(250 / 4) = 63, not 64
                (2, 256, 256, 16, 16, 0, d, 12), (2, 256, 256, 16, 16, 2, None, 12), (2, 256, 256, 16, 16, 2, d, 0), (2, 256, 256, 16, 16, 2, d, 33),
                (8, 256, 256, 16, 16, 4, d, 12),        # 4 x 257 rows per scene pass car_mha's 1024
                (2, 256, 256, 16, 16, 2, ints(3, 0, 9), 12), (0, 256, 256, 16, 16, 1, d, 12)):
        assert lib.car_getz_workspace_bytes(*bad) == 0 and msg().startswith("car_"), bad
    assert lib.car_decoder_pack(None, 50, None, None) == -1 and msg().startswith("car_decoder_pack: null pointer")
    some = (ctypes.c_void_p * 50)(*([256] * 50))
    assert lib.car_decoder_pack(some, 49, ctypes.c_void_p(256), None) == -1 and "49 parameter arrays" in msg()
    assert lib.car_decoder_pack(some, 50, ctypes.c_void_p(260), None) == -1 and "16-byte aligned" in msg()
    assert lib.car_conv3x3_pad1(ctypes.c_void_p(256), 1, 4, 4, 256, 256, 3, ctypes.c_void_p(256), None, None, 0, ctypes.c_void_p(256), None) == -1 and "stride" in msg()
    assert lib.car_conv3x3_pad1(ctypes.c_void_p(256), 1, 4, 4, 256, 256, 1, ctypes.c_void_p(256), None, None, 8, ctypes.c_void_p(256), None) == -1 and "flags" in msg()
    assert lib.car_upsample2x_bilinear(ctypes.c_void_p(256), 1, 4, 4, 6, ctypes.c_void_p(256), None) == -1 and "multiple of 4" in msg()


# ---- the switches ----------------------------------------------------------------------------------------------------------------------------
def test_encoder_route_has_a_fourth_value_and_the_decoder_a_switch():
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    enc = E.MultiViewDPTEncoder()
    assert enc.decoder_route == "torch"
    with pytest.raises(ValueError, match="decoder_route must be 'torch' or 'device'"):
        enc.decoder_route = "cuda"
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, encoder=enc)
    routes = lambda: (enc.trunk_route, enc.vit_route, enc.decoder_route, m.encoder_route)
    m.encoder_route = "device_full"
    assert routes() == ("device", "device", "device", "device_full")
    for name, want in (("device_trunk", ("device", "device", "torch")), ("device", ("torch", "device", "torch")), ("torch", ("torch", "torch", "torch"))):
        m.encoder_route = "device_full"
        m.encoder_route = name                                          # the three earlier values put the decoder back on torch
        assert routes() == want + (name,)
    enc.trunk_route, enc.vit_route = "device", "torch"                  # unnamed, decoder on torch: the pair, as before
    assert m.encoder_route == ("device", "torch")
    enc.decoder_route = "device"                                        # unnamed, decoder on the device: the triple
    assert m.encoder_route == ("device", "torch", "device")
    enc.trunk_route = "torch"
    assert m.encoder_route == ("torch", "torch", "device")
    with torch.no_grad(), pytest.raises(ValueError, match="CPU tensors run on decoder_route = 'torch'"):
        enc(torch.zeros(2, 3, 256, 256), torch.zeros(2, 16), 2)         # the torch trunk and blocks ran; the decoder refuses before it touches the library
    m.encoder_route = "device_full"
    cpu_input = {"context": {"rgb": torch.zeros(1, 2, 256, 256, 3), "cam2world": torch.eye(4).expand(1, 2, 4, 4)}}
    with torch.no_grad(), pytest.raises(ValueError, match="CPU tensors run on encoder_route = 'torch'"):
        m.get_z(cpu_input)
    m.encoder_route = "torch"
    assert routes() == ("torch", "torch", "torch", "torch")
    assert not any("route" in k for k in m.state_dict())
    bare = CrossAttentionRenderer(model="midas_vit", n_view=2, with_encoder=False)
    assert bare.encoder_route == "torch"
    with pytest.raises(ValueError, match="EncoderNotBuilt has no vit_route"):
        bare.encoder_route = "device_full"
    with pytest.raises(ValueError, match="'device_trunk' or 'device_full'"):
        bare.encoder_route = "full"
    with pytest.raises(ValueError, match="must be 'torch' or 'device'"):
        bare.encoder_route = "hip"

    class Older(torch.nn.Module):                                       # a caller's module with the two earlier switches only
        vit_route = trunk_route = "torch"
    own = CrossAttentionRenderer(model="midas_vit", n_view=2, encoder=Older())
    own.encoder_route = "device_trunk"
    assert own.encoder_route == "device_trunk"
    with pytest.raises(ValueError, match="Older has no decoder_route"):
        own.encoder_route = "device_full"


def test_drop_device_caches_forgets_the_decoder():
    enc = E.MultiViewDPTEncoder.__new__(E.MultiViewDPTEncoder)
    torch.nn.Module.__init__(enc)

    class Held:
        dropped = False

        def drop(self):
            self.dropped = True
    held = Held()
    enc._vit_packed = enc._trunk_packed = enc._tokens_packed = None
    enc._decoder_packed, enc._decoder_work = held, {"key": 1}
    enc.drop_device_caches()
    assert held.dropped and enc._decoder_work == {}


def test_encoder_route_flag_takes_the_fourth_value():
    import importlib.util
    spec = importlib.util.spec_from_file_location("car_scripts_common", os.path.join(ROOT, "experiment_scripts", "common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    opt = common.parser("t").parse_args(["--experiment_name", "x", "--encoder_route", "device_full", "--synthetic"])
    assert opt.encoder_route == "device_full"
