"""CPU side of the opt-in fp16 render precision (``render_precision = "fp16"``).

The error budget of tests/test_render_fp16.py comes from the arithmetic, not from luck: the CPU oracle with its 1x1 layers replaced by
an emulation of the fp16 instance's arithmetic — operands moved into fp16's window by the kernels' powers of two (activations per row to
[2^13, 2^14), weights per layer), rounded to nearest fp16, one product per term, wide accumulation — stays well inside the same bounds
on the real-width fixtures.  (It puts more layers into fp16 than the kernel does, so it errs on the pessimistic side.)"""
import math
import os
import re

import pytest
import torch

from golden_util import load_case
from hip_harness import oracle_cfg
from oracle import car_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_PSNR_DB, RGB_MAX, DEPTH_MAX, AT_WT_MAX, ARGMAX_AGREE = 60.0, 1e-2, 5e-3, 1e-4, 0.98


def _pow2_into_window(m: torch.Tensor) -> torch.Tensor:
    """2^k with m 2^k in [2^13, 2^14) (csrc/car_split.h pow2_scale: the exponent clamped for zeros)."""
    e = torch.floor(torch.log2(m.clamp_min(2.0 ** -126)))
    return torch.exp2((13 - e).clamp(-43, 90))


def _conv1x1_fp16(x, w, bias):
    w2 = w.reshape(w.shape[0], -1)
    px = _pow2_into_window(x.abs().amax(dim=-1, keepdim=True).double())
    pw = _pow2_into_window(w2.abs().max().double())
    xh = (x.double() * px).to(torch.float16).double()
    wh = (w2.double() * pw).to(torch.float16).double()
    y = (xh @ wh.T) / (px * pw)
    return (y + bias.double()).to(torch.float32)


def _psnr(a, b):
    mse = torch.mean((a.double() - b.double()) ** 2).item()
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


@pytest.mark.parametrize("name", ["t1_c1", "t1_c1_diverging", "t1_no_repeat", "t2_c2"])
def test_fp16_emulation_of_the_oracle_keeps_the_bounds(name, monkeypatch):
    c, inp, z, sd, _ = load_case(name)
    cfg = oracle_cfg(c)
    with torch.no_grad():
        want = O.render_forward(sd, inp, z, cfg)
        monkeypatch.setattr(O, "_conv1x1", _conv1x1_fp16)
        got = O.render_forward(sd, inp, z, cfg)
    assert torch.equal(got["valid_mask"], want["valid_mask"])
    assert not torch.equal(got["rgb"], want["rgb"]), "the emulation did not take effect"
    assert _psnr(got["rgb"], want["rgb"]) >= RGB_PSNR_DB
    assert (got["rgb"] - want["rgb"]).abs().max().item() <= RGB_MAX
    assert (got["depth_ray"] - want["depth_ray"]).abs().max().item() <= DEPTH_MAX
    assert (got["at_wt"] - want["at_wt"]).abs().max().item() <= AT_WT_MAX
    assert (got["at_wt_max"] == want["at_wt_max"]).double().mean().item() >= ARGMAX_AGREE


def test_render_precision_validation_on_a_cpu_module():
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=8, with_encoder=False)
    assert m.render_precision == "fp32"
    m.render_precision = "fp16"
    assert m.render_precision == "fp16"
    assert not any("precision" in k for k in m.state_dict()), "a render setting must not enter checkpoints"
    for bad in ("bf16", "FP16", None, 16):
        with pytest.raises(ValueError):
            m.render_precision = bad
    assert m.render_precision == "fp16"
    m.render_precision = "fp32"
    assert m.render_precision == "fp32"


def test_render_train_refuses_fp16_before_touching_a_device():
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    from cross_attention_renderer_amd.training import render_train
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=8, with_encoder=False)
    m.render_precision = "fp16"
    with pytest.raises(ValueError, match="render_precision"):
        render_train(m, {"query": {"uv": torch.zeros(1, 1, 4, 2)}})


def _header_functions():
    src = open(os.path.join(ROOT, "include", "car_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return set(re.findall(r"^\s*(?:[A-Za-z_][\w ]*?[\s*]+)(car_\w+)\s*\(", src, flags=re.M))


def test_fp16_entries_are_declared_and_bound():
    from cross_attention_renderer_amd import _lib
    declared = _header_functions()
    new = {"car_plan_f16_bytes", "car_plan_f16_build", "car_render_forward_f16"}
    assert new <= declared, new - declared
    assert new <= set(_lib.SIGNATURES), new - set(_lib.SIGNATURES)
    missing = sorted(declared - set(_lib.SIGNATURES))
    assert not missing, f"declared in include/car_hip.h but not in _lib.SIGNATURES: {missing}"
