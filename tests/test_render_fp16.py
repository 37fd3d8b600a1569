"""``-m gpu``: the opt-in fp16 render precision (``CrossAttentionRenderer.render_precision = "fp16"``, car_render_forward_f16).

The fused per-sample kernel's fp16 instance takes one fp16 product per term instead of the three of the split-fp16 default; everything
else of the one-call route is the fp32 route's own.  Contract: geometry outputs bit-identical to the fp32 route, the rest
within bounds about ten times the error of a CPU emulation of the same arithmetic (tests/test_render_fp16_cpu.py)."""
import ctypes
import math

import pytest
import torch

from golden_util import load_case
from hip_harness import build_module, to_device

pytestmark = pytest.mark.gpu

ONE_CALL_CASES = ["t1_c1", "t1_c1_diverging", "t1_no_sample", "t1_no_repeat", "t2_c2", "t2_c3", "t2_c4", "t2_c5"]
EXACT = ("valid_mask", "coords", "pixel_val")
RGB_PSNR_DB, RGB_MAX, DEPTH_MAX, AT_WT_MAX, ARGMAX_AGREE = 60.0, 1e-2, 5e-3, 1e-4, 0.98


def _psnr(a, b):
    mse = torch.mean((a.double() - b.double()) ** 2).item()
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def _check_fp16_against_fp32(got, want, what=""):
    for k in EXACT:
        assert torch.equal(got[k], want[k]), f"{what} {k} is not bit-identical to the fp32 route"
    for k in ("rgb", "depth_ray", "at_wt"):
        assert torch.isfinite(got[k]).all(), f"{what} {k}"
    assert _psnr(got["rgb"], want["rgb"]) >= RGB_PSNR_DB, f"{what} rgb PSNR {_psnr(got['rgb'], want['rgb']):.1f} dB"
    assert (got["rgb"] - want["rgb"]).abs().max().item() <= RGB_MAX, what
    assert (got["depth_ray"] - want["depth_ray"]).abs().max().item() <= DEPTH_MAX, what
    assert (got["at_wt"] - want["at_wt"]).abs().max().item() <= AT_WT_MAX, what
    agree = (got["at_wt_max"] == want["at_wt_max"]).double().mean().item()
    assert agree >= ARGMAX_AGREE, f"{what} at_wt_max agreement {agree:.3f}"


def _module_and_inputs(name, dev, sd_edit=None, z_edit=None):
    c, inp, z, sd, _ = load_case(name)
    if sd_edit is not None:
        sd = sd_edit(dict(sd))
    if z_edit is not None:
        z = z_edit(z)
    m = build_module(c, sd, dev)
    return m, to_device(inp, dev, cameras_on_host=True), [t.to(dev) for t in z]


def _render(m, inp, z, precision, debug=False):
    m.render_precision = precision
    with torch.no_grad():
        out = m(inp, z=z, debug=debug)
    torch.cuda.synchronize()
    return {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


@pytest.mark.parametrize("name", ONE_CALL_CASES)
def test_fp16_forward_against_the_fp32_route(name):
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs(name, dev)
    want = _render(m, inp, z, "fp32")
    assert m._engine.last_precision == "fp32"
    got = _render(m, inp, z, "fp16")
    assert m._engine.last_calls >= 1 and m._engine.last_precision == "fp16"
    _check_fp16_against_fp32(got, want, name)


def test_fp16_full_frame():
    """One whole 256 x 256 frame at 64 samples per ray (the bench frame's shape)."""
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    dev = torch.device("cuda:0")
    H, P = 256, 64
    torch.manual_seed(0)
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=P, with_encoder=False).eval()
    S.perturb_parameters(m, seed=6)
    m.H = m.W = H
    inp = to_device(S.stereo_scene(H, b=1, seed=9), dev, cameras_on_host=True)          # every pixel of the frame
    assert inp["query"]["uv"].shape[2] == H * H
    z = [t.to(dev) for t in S.feature_maps(1, 2, H, seed=3)]
    m = m.to(dev)
    want = _render(m, inp, z, "fp32")
    got = _render(m, inp, z, "fp16")
    assert m._engine.last_precision == "fp16"
    _check_fp16_against_fp32(got, want, "256 x 256 x 64 frame")


def test_default_route_is_untouched_by_an_fp16_render():
    """fp32, fp16, fp32 on one module: both fp32 renders bit-identical to each other and to a fresh module's."""
    dev = torch.device("cuda:0")
    keys = ("rgb", "valid_mask", "depth_ray", "at_wt", "at_wt_max", "coords", "pixel_val")
    m, inp, z = _module_and_inputs("t2_c2", dev)
    a = _render(m, inp, z, "fp32")
    h = _render(m, inp, z, "fp16")
    b = _render(m, inp, z, "fp32")
    assert m._engine.last_precision == "fp32"
    fresh, inp2, z2 = _module_and_inputs("t2_c2", dev)
    f = _render(fresh, inp2, z2, "fp32")
    for k in keys:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], f[k]), k
    assert not torch.equal(a["rgb"], h["rgb"]), "the fp16 render took the fp32 kernel"


@pytest.mark.parametrize("s", [2.0 ** -20, 2.0 ** 20])
def test_fp16_dynamic_range_of_the_feature_maps(s):
    """The pyramid 2^+-20 times larger with the first layer's feature columns scaled back (same function): the powers of two of the
    fp16 operands keep the bounds, and nothing overflows."""
    def sd_edit(sd):
        w = sd["query_encode_latent.weight"].clone()
        w[:, :576] = w[:, :576] / s
        return dict(sd, **{"query_encode_latent.weight": w})
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs("t2_c2", dev, sd_edit=sd_edit, z_edit=lambda z: [t * s for t in z])
    want = _render(m, inp, z, "fp32")
    got = _render(m, inp, z, "fp16")
    _check_fp16_against_fp32(got, want, f"maps x{s:g}")


def test_fp16_debug_stages():
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs("t1_c1", dev)
    want = _render(m, inp, z, "fp32", debug=True)
    got = _render(m, inp, z, "fp16", debug=True)
    assert torch.equal(got["stages"]["g"], want["stages"]["g"]) and torch.equal(got["stages"]["pt"], want["stages"]["pt"])
    e, e0 = got["stages"]["interp_val"], want["stages"]["interp_val"]
    assert (e - e0).abs().max().item() <= 4e-3 * e0.abs().max().item()


@pytest.mark.parametrize("name,ws_mib,level_mib", [("t2_c3", 30, None), ("t2_c3", None, 2600), ("t2_c2", 20, None)])
def test_fp16_split_calls_are_bit_identical(name, ws_mib, level_mib):
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs(name, dev)
    one = _render(m, inp, z, "fp16")
    assert m._engine.last_calls == 1
    m2, inp2, z2 = _module_and_inputs(name, dev)
    m2._engine = None
    m2.render_precision = "fp16"
    from cross_attention_renderer_amd.engine import RenderEngine
    m2._engine = RenderEngine(m2)
    m2._engine.max_workspace_bytes = None if ws_mib is None else ws_mib << 20
    if level_mib is not None:
        m2._engine.max_level_bytes = level_mib << 20
    many = _render(m2, inp2, z2, "fp16")
    assert m2._engine.last_calls > 1 and m2._engine.last_precision == "fp16"
    for k in ("rgb", "valid_mask", "depth_ray", "at_wt", "at_wt_max", "coords", "pixel_val"):
        assert torch.equal(one[k], many[k]), k


# ---- the C entries directly ---------------------------------------------------------------------------------------------------------
def _abi(name="t1_c1"):
    from cross_attention_renderer_amd import _lib
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs(name, dev)
    m.render_precision = "fp16"
    with torch.no_grad():
        ref = m(inp, z=z)
    torch.cuda.synchronize()
    eng, lib = m._engine, _lib.load()
    b, R, P, H = 1, inp["query"]["uv"].shape[2], m.npoints, m.H
    d_all = eng._dims(b, R, z)
    plan = eng._plan_for(d_all, dev)
    plan16 = eng._plan16_for(d_all, dev)
    pair, d_pair = eng._pair_for(plan, z, dev, 0, b, R)
    ctx = dict(m=m, inp=inp, z=z, ref=ref, eng=eng, lib=lib, plan=plan, plan16=plan16, pair=pair, d_pair=d_pair, R=R, P=P, H=H, dev=dev,
               poses=eng._poses(inp, H, 2, dev), uv=inp["query"]["uv"].reshape(1, R, 2).float().contiguous(),
               steps=eng._linspace(0.0, 1.0, P, dev))
    return ctx


def _outputs(rc, P, dev):
    f32 = dict(device=dev, dtype=torch.float32)
    return {"rgb": torch.empty(1, 1, rc, 3, **f32), "valid_mask": torch.empty(1, rc, 1, **f32), "depth_ray": torch.empty(1, rc, 1, **f32),
            "at_wt": torch.empty(2, rc, P, **f32), "at_wt_max": torch.empty(2, rc, 1, device=dev, dtype=torch.int32),
            "coords": torch.empty(2, rc, 9, **f32), "pixel_val": torch.empty(2, rc, P, 2, **f32)}


ORDER = ("rgb", "valid_mask", "depth_ray", "at_wt", "at_wt_max", "coords", "pixel_val")


def _inputs(x, uv):
    from cross_attention_renderer_amd import _lib
    ci = _lib.CarInputs()
    ci.poses, ci.uv, ci.lattice, ci.steps = x["poses"].data_ptr(), uv.data_ptr(), x["pair"].data_ptr(), x["steps"].data_ptr()
    ci.gmeta = x["pair"].data_ptr() + 4 * x["lib"].car_gmeta_offset(ctypes.byref(x["d_pair"]))
    return ci


def test_kernel_level_e_logit_g_pt_against_the_fp32_entry():
    """The per-sample phase alone through both entries: e and the first-round logits within 4e-3 of each tensor's largest magnitude,
    g and pt (geometry) bit-identical."""
    from cross_attention_renderer_amd import _lib
    from cross_attention_renderer_amd.engine import _ptr
    x = _abi("t2_c2")
    lib, R, P, dev = x["lib"], x["R"], x["P"], x["dev"]
    d = x["eng"]._dims(1, R, x["z"])
    need = lib.car_workspace_bytes(ctypes.byref(d))
    ws = {}
    for prec in ("fp32", "fp16"):
        o = _outputs(R, P, dev)
        work = torch.zeros(need // 4, device=dev, dtype=torch.float32)
        ci, co = _inputs(x, x["uv"]), _lib.CarOutputs(*[o[k].data_ptr() for k in ORDER])
        if prec == "fp32":
            rc = lib.car_render_forward_phase(ctypes.byref(d), _ptr(x["plan"]), ctypes.byref(ci), ctypes.byref(co), _ptr(work), need, 1, None)
        else:
            rc = lib.car_render_forward_f16(ctypes.byref(d), _ptr(x["plan"]), _ptr(x["plan16"]), ctypes.byref(ci), ctypes.byref(co), _ptr(work),
                                            need, 1, None)
        _lib.check(rc, prec)
        torch.cuda.synchronize()
        ws[prec] = work.cpu()

    def t(prec, name):
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.car_workspace_find(ctypes.byref(d), name.encode(), ctypes.byref(off), ctypes.byref(cnt)), name)
        return ws[prec][off.value:off.value + cnt.value]
    for name in ("g", "pt"):
        assert torch.equal(t("fp16", name), t("fp32", name)), name
    for name in ("e", "logit"):
        a, b = t("fp16", name), t("fp32", name)
        assert torch.isfinite(a).all()
        assert (a - b).abs().max().item() <= 4e-3 * b.abs().max().item(), name
        assert not torch.equal(a, b), f"{name}: the fp16 entry ran the fp32 kernel"


def test_fp16_two_phases_on_two_streams_equal_one_fp16_call():
    from cross_attention_renderer_amd import _lib
    from cross_attention_renderer_amd.engine import _ptr
    x = _abi("t1_c1")
    lib, R, P, dev, nb = x["lib"], x["R"], x["P"], x["dev"], 2
    rc = R // nb
    d = x["eng"]._dims(1, rc, x["z"])
    need = lib.car_workspace_bytes(ctypes.byref(d))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    keep, outs = [], []
    for c in range(nb):
        o = _outputs(rc, P, dev)
        u = x["uv"][:, c * rc:(c + 1) * rc].contiguous()
        work = torch.empty(need // 4, device=dev, dtype=torch.float32)
        ci, co = _inputs(x, u), _lib.CarOutputs(*[o[k].data_ptr() for k in ORDER])
        ev = torch.cuda.Event()
        for phase, stream in ((1, sa), (2, sb)):
            if phase == 2:
                sb.wait_event(ev)
            _lib.check(lib.car_render_forward_f16(ctypes.byref(d), _ptr(x["plan"]), _ptr(x["plan16"]), ctypes.byref(ci), ctypes.byref(co), _ptr(work),
                                                  need, phase, ctypes.c_void_p(stream.cuda_stream)), "car_render_forward_f16")
            if phase == 1:
                ev.record(sa)
        keep += [u, work, ci, co, ev]
        outs.append(o)
    torch.cuda.synchronize()
    ref = x["ref"]
    assert torch.equal(torch.cat([o["rgb"] for o in outs], dim=2), ref["rgb"])
    for k in ("depth_ray", "at_wt", "valid_mask"):
        assert torch.equal(torch.cat([o[k] for o in outs], dim=1), ref[k]), k
    assert lib.car_render_forward_f16(ctypes.byref(d), _ptr(x["plan"]), _ptr(x["plan16"]), ctypes.byref(ci), ctypes.byref(co), _ptr(work), need, 4,
                                      None) != 0
    assert lib.car_render_forward_f16(ctypes.byref(d), _ptr(x["plan"]), None, ctypes.byref(ci), ctypes.byref(co), _ptr(work), need, 3, None) != 0


def test_fp16_entries_between_nan_margins():
    """car_plan_f16_build and car_render_forward_f16 with every buffer argument between NaN margins (tests/oob_runner.py's Guarded):
    the results equal the plain call's bit for bit and no margin changes."""
    from cross_attention_renderer_amd import _lib
    from oob_runner import Guarded
    x = _abi("t1_c1")
    lib, R, P, dev, eng = x["lib"], x["R"], x["P"], x["dev"], x["eng"]
    d = eng._dims(1, R, x["z"])
    # plan16 into a guarded buffer and into a plain one, both zeroed first (the alignment gaps between its sections are never written)
    gp, p16 = Guarded(torch.zeros_like(x["plan16"])), torch.zeros_like(x["plan16"])
    for ptr in (gp.ptr, p16.data_ptr()):
        _lib.check(lib.car_plan_f16_build(ctypes.byref(d), ctypes.byref(eng._plan_w), ctypes.c_void_p(ptr), None), "car_plan_f16_build")
    torch.cuda.synchronize()
    assert gp.margins_intact()
    assert torch.equal(gp.read().view(torch.int32), p16.view(torch.int32))
    need = lib.car_workspace_bytes(ctypes.byref(d))
    plain = _outputs(R, P, dev)
    work = torch.empty(need // 4, device=dev, dtype=torch.float32)
    ci, co = _inputs(x, x["uv"]), _lib.CarOutputs(*[plain[k].data_ptr() for k in ORDER])
    _lib.check(lib.car_render_forward_f16(ctypes.byref(d), ctypes.c_void_p(x["plan"].data_ptr()), ctypes.c_void_p(x["plan16"].data_ptr()),
                                          ctypes.byref(ci), ctypes.byref(co), ctypes.c_void_p(work.data_ptr()), need, 3, None), "plain")
    guarded = {k: Guarded(torch.zeros_like(v) if v.dtype != torch.int32 else torch.zeros_like(v)) for k, v in _outputs(R, P, dev).items()}
    g_in = {"poses": Guarded(x["poses"]), "uv": Guarded(x["uv"]), "steps": Guarded(x["steps"]), "plan": Guarded(x["plan"]),
            "plan16": Guarded(x["plan16"]), "work": Guarded(torch.zeros(need // 4, device=dev))}
    gl = Guarded(x["pair"])
    ci2 = _lib.CarInputs()
    ci2.poses, ci2.uv, ci2.lattice, ci2.steps = g_in["poses"].ptr, g_in["uv"].ptr, gl.ptr, g_in["steps"].ptr
    ci2.gmeta = gl.ptr + 4 * lib.car_gmeta_offset(ctypes.byref(x["d_pair"]))
    co2 = _lib.CarOutputs(*[guarded[k].ptr for k in ORDER])
    _lib.check(lib.car_render_forward_f16(ctypes.byref(d), ctypes.c_void_p(g_in["plan"].ptr), ctypes.c_void_p(g_in["plan16"].ptr),
                                          ctypes.byref(ci2), ctypes.byref(co2), ctypes.c_void_p(g_in["work"].ptr), need, 3, None), "guarded")
    torch.cuda.synchronize()
    for k in ORDER:
        assert torch.equal(guarded[k].read().view(torch.int32), plain[k].view(torch.int32)), k
        assert guarded[k].margins_intact(), k
    for k, g in list(g_in.items()) + [("lattice", gl)]:
        assert g.margins_intact(), k


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,why", [("t1_nview1", "n_view = 1"), ("t1_nview3", "n_view = 3"), ("t1_no_latent_concat", "no_latent_concat"),
                                      ("t0_default", "widths")])
def test_fp16_refuses_configs_off_the_one_call_route(name, why):
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs(name, dev)
    m.render_precision = "fp16"
    with pytest.raises(ValueError, match=why):
        with torch.no_grad():
            m(inp, z=z)


def test_fp16_refuses_a_pyramid_without_a_common_lattice():
    import torch.nn.functional as F
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs("t1_c1", dev)
    z = [z[0], F.interpolate(z[1], size=(z[1].shape[2] - 2, z[1].shape[3] - 2)), z[2]]
    m.render_precision = "fp16"
    with pytest.raises(ValueError, match="common lattice"):
        with torch.no_grad():
            m(inp, z=z)


def test_fp16_refuses_training_and_unknown_values():
    from cross_attention_renderer_amd.training import render_train
    dev = torch.device("cuda:0")
    m, inp, z = _module_and_inputs("t1_c1", dev)
    m.render_precision = "fp16"
    with pytest.raises(ValueError, match="render_precision"):
        render_train(m, inp, z)
    m.train()
    with pytest.raises(ValueError, match="render_precision"):
        m(inp, z=z)
    with pytest.raises(ValueError):
        m.render_precision = "bf16"
    m._render_precision = "int8"                                      # set behind the validating setter: the engine refuses it too
    m.eval()
    with pytest.raises(ValueError, match="render_precision"):
        with torch.no_grad():
            m(inp, z=z)
