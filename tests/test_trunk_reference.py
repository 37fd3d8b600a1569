"""CPU checks for the encoder's front half: the restatement of tests/trunk_reference.py (what the GPU suite compares the kernels against)
held to encoder.py's own modules run in float64, the SAME-padding table, the ctypes table of include/car_trunk.h held to the header, the
sizes and refusals that need no device, and the renderer's third encoder_route value."""
import ctypes
import os
import re

import pytest
import torch

import trunk_reference as TR
from cross_attention_renderer_amd import encoder as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
REL = 1e-12                       # the bound tests/test_vit_reference.py holds its restatement to


def _close(got, want, what):
    err = float((got.double() - want.double()).abs().max())
    scale = float(want.double().abs().max()) + 1e-300
    assert err <= REL * scale, (what, err, scale)


def _cl(t):                       # NCHW -> channel-last rows
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


def _nchw(rows, h, w):
    return rows.reshape(rows.shape[0], h, w, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("stride", [1, 2])
def test_same_padding_table(stride):
    """Extents 1..9, windows 1, 3 and 7: the padded extent _same_pad makes, with the odd pixel behind; at stride 2 a 3-wide window pads an
    even extent 0 and 1, an odd one 1 and 1.  (StdConv2dSame pads a stride-1 window statically by (k - 1) / 2 on both sides.)"""
    for k in (1, 3, 7):
        for i in range(1, 10):
            front, behind = TR.same_pad(i, k, stride)
            if stride == 1:
                assert (front, behind) == ((k - 1) // 2, (k - 1) // 2)
            x = torch.arange(1.0, i + 1).reshape(1, 1, i, 1).expand(1, 1, i, i)
            padded = E._same_pad(x, k, stride)
            assert padded.shape[-2] == i + front + behind, (k, i)
            assert float(padded[0, 0, :front, front].abs().sum()) == 0 and float(padded[0, 0, front, front]) == 1.0     # square: the column pads alike
            assert TR.same_out(i, stride) == (padded.shape[-2] - k) // stride + 1
            if stride == 2 and k == 3:
                assert (front, behind) == ((0, 1) if i % 2 == 0 else (1, 1))


@pytest.mark.parametrize("k,stride,cin,cout,eps", [(1, 1, 8, 16, 1e-8), (1, 2, 8, 16, 1e-8), (3, 1, 8, 8, 1e-8), (3, 2, 8, 8, 1e-8), (7, 2, 3, 64, 1e-6)])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (8, 6)])
def test_std_conv_same(k, stride, cin, cout, eps, H, W):
    conv = E.StdConv2dSame(cin, cout, k, stride=stride, eps=eps).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=TR.gen(k + H), dtype=F64) + 0.3)
        x = torch.randn(2, cin, H, W, generator=TR.gen(W), dtype=F64)
        want = conv(x)
    w_std, _ = TR.weight_standardize(conv.weight.detach(), eps)
    if k == 7:
        got, bound = TR.stem(x, w_std)
    elif k == 3:
        got, bound = TR.conv_same(_cl(x), H, W, w_std, stride)
    else:                                                            # the 1x1 layer: at stride 2 the pixel copy, then the linear
        src = TR.pixels_stride2(_cl(x), H, W) if stride == 2 else _cl(x)
        got, bound = TR.linear(src, w_std.reshape(cout, cin))
    _close(got, _cl(want), (k, stride, H, W))
    assert bool((bound >= got.abs() * (1 - 1e-12)).all())


def test_weight_standardize_of_a_constant_filter_is_zero():
    w = torch.full((2, 3, 3, 3), 1e3)
    assert float(TR.weight_standardize(w, 1e-8)[0].abs().max()) == 0.0


@pytest.mark.parametrize("C,relu", [(64, True), (256, False)])
def test_groupnorm_and_pool(C, relu):
    norm = E.GroupNormAct(C, apply_act=relu).double()
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(C, generator=TR.gen(1), dtype=F64))
        norm.bias.copy_(0.2 * torch.randn(C, generator=TR.gen(2), dtype=F64))
        x = torch.randn(2, C, 5, 7, generator=TR.gen(3), dtype=F64) * 3 + 1
        want = norm(x)
    got, bound = TR.groupnorm(_cl(x), 32, norm.weight.detach(), norm.bias.detach(), relu=relu)
    _close(got, _cl(want), "groupnorm")
    assert bool((bound >= got.abs() * (1 - 1e-12)).all())
    for H, W in ((1, 1), (2, 2), (5, 7), (6, 4)):
        x = torch.randn(2, 4, H, W, generator=TR.gen(H), dtype=F64)
        assert torch.equal(TR.maxpool(_cl(x), H, W), _cl(E.MaxPool2dSame()(x))), (H, W)
    x = torch.zeros(1, 1, 3, 3)
    x[0, 0, 1, 1] = float("nan")
    assert bool(torch.isnan(TR.maxpool(_cl(x), 3, 3)).all()) and bool(torch.isnan(E.MaxPool2dSame()(x)).all())


def _load(module, params):
    with torch.no_grad():
        for (_, p), v in zip(module.named_parameters(), params, strict=True):
            p.copy_(v.double())


@pytest.mark.parametrize("cin,cout,stride,project", [(64, 256, 1, True), (256, 256, 1, False), (256, 512, 2, True)])
def test_bottleneck_and_downsample(cin, cout, stride, project):
    blk = E.Bottleneck(cin, cout, stride, project).double()
    shapes = [tuple(p.shape) for p in blk.parameters()]
    params = [torch.randn(s, generator=TR.gen(i + cin)) + (0.3 if len(s) == 4 else 0.0) for i, s in enumerate(shapes)]
    _load(blk, params)
    H, W = 5, 6
    x = torch.randn(2, cin, H, W, generator=TR.gen(9), dtype=F64)
    with torch.no_grad():
        want = blk(x)
    got, bound, ho, wo = TR.bottleneck(_cl(x), H, W, params, (cin, cout // 4, cout, stride, project))
    assert (ho, wo) == tuple(want.shape[-2:])
    _close(got, _cl(want), "bottleneck")
    if project:
        with torch.no_grad():
            want = blk.downsample(x)
        src = TR.pixels_stride2(_cl(x), H, W) if stride == 2 else _cl(x)
        sc, _ = TR.linear(src, TR.weight_standardize(params[0], 1e-8)[0].reshape(cout, cin))
        _close(TR.groupnorm(sc, 32, params[1], params[2])[0], _cl(want), "downsample")


def test_trunk_and_parameter_order():
    """ResNetV2Trunk (depths 3, 4, 9) on a 2 x 3 x 32 x 48 image; trunk_shapes is the module's state_dict order."""
    net = E.ResNetV2Trunk().double()
    depths = (3, 4, 9)
    assert [tuple(p.shape) for p in net.parameters()] == TR.trunk_shapes(depths) and len(TR.trunk_shapes(depths)) == 156
    assert [n for n, _ in net.named_parameters()] == list(net.state_dict())
    params = TR.seeded_trunk(depths)
    _load(net, params)
    x = torch.randn(2, 3, 32, 48, generator=TR.gen(4), dtype=F64)
    with torch.no_grad():
        want = net(x)
    got = TR.trunk(x, params, depths)
    for (g, b), w_ in zip(got, want):
        _close(g, _cl(w_), "trunk")
        assert bool((b >= g.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("grid,gh,gw", [(4, 1, 1), (4, 2, 3), (24, 16, 16), (4, 7, 5)])
def test_token_rows(grid, gh, gw):
    """The token lines of MultiViewDPTEncoder.forward on a small MultiViewViT in float64."""
    vit = E.MultiViewViT(depth=1, grid=grid).double()
    pw, pb, cls, pos, sw, sb = TR.seeded_tokens(grid)
    with torch.no_grad():
        vit.patch_embed.proj.weight.copy_(pw.double().reshape(768, 1024, 1, 1)); vit.patch_embed.proj.bias.copy_(pb.double())
        vit.cls_token.copy_(cls.double().reshape(1, 1, -1)); vit.pos_embed.copy_(pos.double()[None])
        vit.pose_embed.weight.copy_(sw.double()); vit.pose_embed.bias.copy_(sb.double())
        BV = 3
        feat = torch.randn(BV, 1024, gh, gw, generator=TR.gen(gh), dtype=F64)
        pose16 = torch.randn(BV, 16, generator=TR.gen(gw), dtype=F64)
        tok = vit.patch_embed.proj(feat).flatten(2).transpose(1, 2)
        tok = torch.cat((vit.cls_token.expand(BV, -1, -1), tok), dim=1)
        want = tok + vit.resized_pos_embed(gh, gw) + vit.pose_embed(pose16)[:, None, :]
    got, bound = TR.tokens(_cl(feat), pose16, pw, pb, cls, pos, grid, sw, sb, gh, gw)
    _close(got, want, "tokens")
    assert bool((bound >= got.abs() * (1 - 1e-12)).all())


# ---- the C ABI's table, sizes and refusals (no device) ---------------------------------------------------------------------------------------
def test_trunk_signatures_mirror_their_header_type_by_type():
    """include/car_trunk.h against _lib.TRUNK_SIGNATURES, by test_abi's own comparison.  The header is included by car_hip.h, inside its
    extern "C" block; the source hash and the build's unit table know the new files."""
    import test_abi as T
    from cross_attention_renderer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "car_trunk.h")).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(car_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in " ".join(params.split()).split(",")]
        params = [] if params == ["void"] else ["*" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const") for p in params]
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    assert len(protos) == 17 == len(_lib.TRUNK_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.MATCH_SIGNATURES) | set(_lib.ENCODER_SIGNATURES))
    assert T._abi_disagreements(protos, _lib.TRUNK_SIGNATURES) == []
    hip_h = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    assert '#include "car_trunk.h"' in hip_h and hip_h.index('#include "car_encoder.h"') < hip_h.index('#include "car_trunk.h"') < hip_h.index("#ifdef __cplusplus\n}")
    assert "#define CAR_VERSION 300" in hip_h                                                  # additive entries: the number stays
    import __graft_entry__ as G
    assert G.UNITS["car_trunk.hip"] == []                                                      # the sweep's arithmetic: the flags of car_lpips.hip and car_linear16.hip
    src = open(os.path.join(ROOT, "cross_attention_renderer_amd", "_lib.py")).read()
    assert '"car_trunk.h"' in src[src.index("def source_hash"):src.index("def _rebuild_stale")]
    assert f"#define CAR_GN_RELU {_lib.CAR_GN_RELU}" in open(os.path.join(ROOT, "include", "car_trunk.h")).read()


def test_trunk_entries_are_exported_bound_and_refuse_without_a_device():
    import __graft_entry__ as G
    G.build()
    from cross_attention_renderer_amd import _lib
    lib, api = _lib.load(), _lib.api()
    for name, (res, _) in _lib.TRUNK_SIGNATURES.items():
        assert hasattr(lib, name), name
        assert (getattr(api, name).errcheck is _lib._errcheck) == (res is ctypes.c_int), name
    with pytest.raises(_lib.CarError, match="null pointer"):
        api.car_groupnorm(None, 1, 1, 64, 32, None, None, 1e-5, None, 0, None, None, 0, None)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    # sizes: the 3x3 layer is car_conv3x3's tiles and 64 floats of scale; GroupNorm keeps two doubles per (image, group, slab of 8192 / C pixels)
    assert lib.car_conv3x3_same_packed_floats(64, 128) == 9 * 64 * 128 + 64
    for bad in ((32, 64), (64, 512), (64, 96)):
        assert lib.car_conv3x3_same_packed_floats(*bad) == 0 and lib.car_last_error().startswith(b"car_conv3x3_same_packed_floats"), bad
    assert lib.car_groupnorm_workspace_bytes(2, 128, 64, 32) == 2 * 2 * 32 * 8 and lib.car_groupnorm_workspace_bytes(2, 129, 64, 32) == 2 * 2 * 32 * 2 * 8
    for bad in ((1, 5, 64, 3), (1, 5, 64, 64), (1, 5, 96, 32), (1, 5, 2048, 32), (0, 5, 64, 32), (1, 0, 64, 32), (70000, 1, 64, 32)):
        assert lib.car_groupnorm_workspace_bytes(*bad) == 0 and lib.car_last_error().startswith(b"car_groupnorm_workspace_bytes"), bad
    assert lib.car_trunk_packed_floats(ints(3, 4, 9)) > lib.car_trunk_packed_floats(ints(1, 1, 1)) > 9 * 256 * 256
    for bad in ((0, 1, 1), (1, 17, 1), (1, 1, -1)):
        assert lib.car_trunk_packed_floats(ints(*bad)) == 0 and b"outside 1..16" in lib.car_last_error(), bad
        assert lib.car_trunk_workspace_bytes(1, 32, 32, ints(*bad)) == 0
    assert lib.car_trunk_packed_floats(None) == 0
    assert lib.car_trunk_workspace_bytes(2, 256, 256, ints(3, 4, 9)) > 2 * 64 * 64 * 256 * 4 * 3
    assert lib.car_trunk_workspace_bytes(0, 32, 32, ints(1, 1, 1)) == 0 and lib.car_trunk_workspace_bytes(1, 0, 32, ints(1, 1, 1)) == 0
    assert lib.car_vit_tokens_packed_floats(16, 16) >= lib.car_linear_x3_packed_floats(1024, 768) + (3 + 257 + 16) * 768
    assert lib.car_vit_tokens_packed_floats(0, 16) == 0 and lib.car_vit_tokens_packed_floats(16, 65) == 0
    assert lib.car_vit_tokens_workspace_bytes(2, 16, 16) == (2 * 256 * 768 + 2 * 768) * 4
    assert lib.car_vit_tokens_workspace_bytes(0, 16, 16) == 0 and lib.car_vit_tokens_workspace_bytes(1, 16, 0) == 0


# ---- the switches ----------------------------------------------------------------------------------------------------------------------------
def test_encoder_route_has_a_third_value():
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    enc = E.MultiViewDPTEncoder()
    assert enc.trunk_route == "torch"
    with pytest.raises(ValueError, match="trunk_route must be"):
        enc.trunk_route = "cuda"
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, encoder=enc)
    m.encoder_route = "device_trunk"
    assert (enc.trunk_route, enc.vit_route, m.encoder_route) == ("device", "device", "device_trunk")
    m.encoder_route = "device"                                          # the blocks alone, as before: the trunk switch goes back
    assert (enc.trunk_route, enc.vit_route, m.encoder_route) == ("torch", "device", "device")
    enc.trunk_route, enc.vit_route = "device", "torch"                  # the two switches are independent on the encoder
    assert m.encoder_route == ("device", "torch")                       # no name for this pair: the pair itself
    with torch.no_grad(), pytest.raises(ValueError, match="CPU tensors run on trunk_route = 'torch'"):
        enc(torch.zeros(2, 3, 256, 256), torch.zeros(2, 16), 2)         # refused before anything touches the library
    m.encoder_route = "torch"
    assert (enc.trunk_route, enc.vit_route, m.encoder_route) == ("torch", "torch", "torch")
    assert not any("route" in k for k in m.state_dict())
    assert len(enc._trunk_parameters()) == 156 and len(enc._token_parameters()) == 6
    bare = CrossAttentionRenderer(model="midas_vit", n_view=2, with_encoder=False)
    with pytest.raises(ValueError, match="EncoderNotBuilt has no vit_route"):
        bare.encoder_route = "device_trunk"
    with pytest.raises(ValueError, match="'device_trunk'"):
        bare.encoder_route = "trunk"


def test_encoder_route_flag_takes_the_third_value():
    import importlib.util
    spec = importlib.util.spec_from_file_location("car_scripts_common", os.path.join(ROOT, "experiment_scripts", "common.py"))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    opt = common.parser("t").parse_args(["--experiment_name", "x", "--encoder_route", "device_trunk", "--synthetic"])
    assert opt.encoder_route == "device_trunk"
