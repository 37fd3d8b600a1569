"""SSIM of the evaluation scripts (car_ssim, harness.ssim): the float64 restatement of scikit-image 0.18.3 (tests/ssim_restatement.py)
against scipy and closed forms, the C entry's argument checks and the wrapper's refusals on the CPU; on the GPU the kernel against the
restatement, its exact cases, its determinism, the reference's protocol on a real render and the eval script's new output lines."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssim_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _smooth(rng, h, w, c, amp=1e-3):
    """Low-variance image (the worst case for uxx - ux**2): a slow gradient of amplitude `amp` around 0.5 plus a little noise."""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = 0.5 + amp * np.sin(3 * xx + 2 * yy)[..., None] * np.ones(c)
    return (base + 0.1 * amp * rng.standard_normal((h, w, c))).astype(np.float32)


def _pair(kind, rng, b, h, w, c):
    if kind == "random":
        x, y = rng.random((b, h, w, c)), rng.random((b, h, w, c))
    elif kind == "smooth":
        x = np.stack([_smooth(rng, h, w, c) for _ in range(b)])
        y = np.stack([_smooth(rng, h, w, c) for _ in range(b)])
    else:                                                            # a noisy copy of the other image
        x = rng.random((b, h, w, c))
        y = np.clip(x + 0.05 * rng.standard_normal(x.shape), 0, 1)
    return x.astype(np.float32), y.astype(np.float32)


# ---- CPU: the restatement -----------------------------------------------------------------------------------------------------------

def test_restatement_filter_is_the_interior_of_scipy_gaussian_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(0).random((40, 37))
    full = ndimage.gaussian_filter(img, sigma=SR.SIGMA, truncate=SR.TRUNCATE)
    assert SR.RADIUS == 5 and SR.WIN == 11
    np.testing.assert_allclose(SR.filter_valid(img), full[5:-5, 5:-5], rtol=0, atol=1e-15)


def test_restatement_weights():
    w = SR.gaussian_weights()
    assert w.shape == (11,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    assert math.isclose(w[6] / w[5], math.exp(-0.5 / 2.25), rel_tol=1e-14)


def test_restatement_identical_images_give_exactly_one():
    rng = np.random.default_rng(1)
    for img in (rng.random((11, 11, 3)), rng.random((40, 33, 1)), _smooth(rng, 30, 30, 3)):
        for r in (1.0, 2.0):
            assert SR.ssim(img, img, r) == 1.0


def test_restatement_constant_pairs_follow_the_closed_form():
    for c1, c2 in ((0.2, 0.7), (0.5, 0.5), (0.0, 1.0), (0.9, 0.1)):
        for r in (1.0, 2.0):
            x, y = np.full((16, 20, 3), c1), np.full((16, 20, 3), c2)
            assert abs(SR.ssim(x, y, r) - SR.constant_pair(c1, c2, r)) < 1e-12


def test_restatement_refuses_images_smaller_than_the_window():
    with pytest.raises(ValueError):
        SR.ssim(np.zeros((10, 20, 3)), np.zeros((10, 20, 3)))


# ---- CPU: the C entry and the wrapper -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    return _lib.load()


def test_car_ssim_scratch_size(lib):
    # 246 x 246 kept pixels in 32 x 16 tiles: 8 x 16 tiles per channel
    assert lib.car_ssim_scratch_doubles(1, 256, 256, 3) == 3 * 8 * 16
    assert lib.car_ssim_scratch_doubles(4, 11, 11, 1) == 4
    for bad in ((0, 64, 64, 3), (1, 10, 64, 3), (1, 64, 10, 3), (1, 64, 64, 0), (1, 64, 64, 5)):
        assert lib.car_ssim_scratch_doubles(*bad) == 0, bad


def test_car_ssim_refuses_bad_arguments(lib):
    """Every refusal happens before the device is touched, so host addresses stand in for the buffers (never dereferenced)."""
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    good = dict(x=p, y=p, B=1, H=64, W=64, C=3, data_range=2.0, mssim=p, scratch=p, n=4096)

    def call(**kw):
        a = dict(good, **kw)
        return lib.car_ssim(a["x"], a["y"], a["B"], a["H"], a["W"], a["C"], a["data_range"], a["mssim"], a["scratch"], a["n"], None)

    cases = [(dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(mssim=None), b"null pointer"),
             (dict(scratch=None), b"null pointer"), (dict(B=0), b"B = 0"), (dict(B=-2), b"B = -2"),
             (dict(H=10), b"H >= 11"), (dict(W=10), b"W >= 11"), (dict(H=3, W=3), b"H >= 11"),
             (dict(C=0), b"C = 0"), (dict(C=5), b"C = 5"),
             (dict(data_range=0.0), b"data_range"), (dict(data_range=-1.0), b"data_range"), (dict(data_range=float("nan")), b"data_range"),
             (dict(n=lib.car_ssim_scratch_doubles(1, 64, 64, 3) - 1), b"scratch"), (dict(B=1 << 20, C=4), b"too large")]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        err = lib.car_last_error()
        assert err.startswith(b"car_ssim:") and msg in err, (kw, err)


def test_harness_ssim_refuses_cpu_tensors_and_bad_shapes():
    from cross_attention_renderer_amd import harness
    x = torch.rand(16, 16, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        harness.ssim(x, x)
    with pytest.raises(ValueError):
        harness.ssim(x, x[:15])
    with pytest.raises(ValueError):
        harness.ssim(x.numpy(), x.numpy())


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------

def _gpu_ssim(x, y, r):
    from cross_attention_renderer_amd import harness
    dev = torch.device("cuda:0")
    return harness.ssim(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), data_range=r).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "smooth", "noisy"])
@pytest.mark.parametrize("hw", [(11, 11), (12, 12), (64, 64), (256, 256), (250, 333), (384, 384)])
def test_ssim_matches_the_restatement(kind, hw):
    rng = np.random.default_rng(["random", "smooth", "noisy"].index(kind) * 1000 + hw[0] * 7 + hw[1])
    for c in (1, 3):
        for b in (1, 4):
            x, y = _pair(kind, rng, b, *hw, c)
            for r in (1.0, 2.0):
                got = _gpu_ssim(x, y, r)
                want = np.array([SR.ssim(x[i], y[i], r) for i in range(b)])
                assert got.shape == (b,) and got.dtype == np.float64
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-7, err_msg=f"{kind} {hw} C={c} B={b} data_range={r}")


@pytest.mark.gpu
def test_ssim_single_pixel_map():
    """11 x 11: one kept pixel, so the mean is that pixel's S."""
    rng = np.random.default_rng(3)
    x, y = _pair("noisy", rng, 1, 11, 11, 1)
    s = SR.ssim_map(x[0, ..., 0], y[0, ..., 0], 2.0)
    assert s.shape == (1, 1)
    assert abs(_gpu_ssim(x, y, 2.0)[0] - s[0, 0]) < 1e-12


@pytest.mark.gpu
def test_ssim_exact_cases():
    rng = np.random.default_rng(4)
    for hw in ((11, 11), (64, 64), (250, 333)):
        for kind in ("random", "smooth"):
            x, _ = _pair(kind, rng, 4, *hw, 3)
            for r in (1.0, 2.0):
                got = _gpu_ssim(x, x, r)
                assert (got == 1.0).all(), (hw, kind, r, got)
    for c1, c2 in ((0.2, 0.7), (0.5, 0.5), (0.0, 1.0), (0.9, 0.1)):
        x, y = np.full((1, 40, 50, 3), c1, np.float32), np.full((1, 40, 50, 3), c2, np.float32)
        for r in (1.0, 2.0):
            want = SR.constant_pair(float(np.float32(c1)), float(np.float32(c2)), r)
            assert abs(_gpu_ssim(x, y, r)[0] - want) < 1e-12


@pytest.mark.gpu
def test_ssim_is_deterministic_and_batch_independent():
    from cross_attention_renderer_amd import harness
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    x, y = (torch.from_numpy(a).to(dev) for a in _pair("noisy", rng, 4, 256, 256, 3))
    a, b = harness.ssim(x, y), harness.ssim(x, y)
    assert a.shape == (4,) and a.dtype == torch.float64 and a.device == x.device
    assert torch.equal(a, b)
    for i in range(4):
        one = harness.ssim(x[i], y[i])
        assert one.shape == () and torch.equal(one, a[i]), i


@pytest.mark.gpu
def test_ssim_refuses_what_car_ssim_refuses():
    from cross_attention_renderer_amd import harness
    dev = torch.device("cuda:0")
    x = torch.rand(16, 16, 3, device=dev)
    for bad in (torch.rand(10, 16, 3, device=dev), torch.rand(16, 16, 5, device=dev), torch.rand(0, 16, 16, 3, device=dev)):
        with pytest.raises(ValueError):
            harness.ssim(bad, bad)
    with pytest.raises(ValueError, match="data_range"):
        harness.ssim(x, x, data_range=0.0)
    with pytest.raises(ValueError):
        harness.ssim(x, x.cpu())


@pytest.mark.gpu
def test_ssim_on_a_rendered_frame_with_the_reference_protocol():
    """A synthetic 64 x 64 render composited over 0.5 grey with its valid mask (eval_realestate10k.py:179-180, as our eval script
    does) against a perturbed copy of the same frame: harness.ssim agrees with the restatement on exactly those images."""
    from cross_attention_renderer_amd import harness, synthetic
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    H = 64
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = CrossAttentionRenderer(model="midas_vit", n_view=2, with_encoder=False).eval()
    synthetic.perturb_parameters(model, seed=0)
    model.H = model.W = H
    model = model.to(dev)
    inp, z = harness.synthetic_pair(H, 2)
    tile = harness.render_frame(model, harness.to_device(inp, dev), [t.to(dev) for t in z])
    valid = tile[0, :, 4:5]
    g = torch.Generator(device="cpu").manual_seed(7)
    target = (tile[0, :, :3] + 0.1 * torch.randn(H * H, 3, generator=g).to(dev)).clamp(-1, 1)

    def composite(img):
        return ((img + 1) * 0.5) * valid + 0.5 * (1 - valid)
    rgb, target = composite(tile[0, :, :3]).reshape(H, H, 3), composite(target).reshape(H, H, 3)
    got = harness.ssim(rgb, target).item()
    want = SR.ssim(rgb.cpu().numpy(), target.cpu().numpy())
    assert 0.0 < want < 1.0 and valid.mean().item() > 0.1
    assert abs(got - want) < 1e-7, (got, want)
    assert abs(harness.ssim(rgb, target, data_range=1.0).item() - SR.ssim(rgb.cpu().numpy(), target.cpu().numpy(), 1.0)) < 1e-7


@pytest.mark.gpu
def test_eval_script_reports_ssim_of_the_chunked_render(tmp_path):
    """The arguments of test_harness.py::test_entry_points_run_on_gpu: the target is the un-chunked render of the same frame."""
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "eval_realestate10k.py"), "--experiment_name", "t", "--views", "2",
           "--synthetic", "--img_sidelength", "64", "--out_dir", str(tmp_path), "--logging_root", str(tmp_path), "--batch_size", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "item 0 ssim" in out.stdout and "mean mse" in out.stdout, out.stdout
    assert float(out.stdout.split("mean ssim")[1].split()[0]) >= 0.999999, out.stdout
    assert float(out.stdout.split("mean mse")[1].split()[0]) < 1e-10, out.stdout


@pytest.mark.gpu
def test_eval_script_reports_ssim_on_the_committed_scene(tmp_path):
    """The arguments of test_harness.py::test_eval_script_reads_the_dataset_and_runs_get_z (tests/golden/dataio_scene_vis)."""
    vis = os.path.join(ROOT, "tests", "golden", "dataio_scene_vis")
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "eval_realestate10k.py"), "--experiment_name", "t", "--views", "2",
           "--data_root", os.path.join(vis, "scenes"), "--pose_root", os.path.join(vis, "poses.mat"), "--logging_root", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    s = float(out.stdout.split("mean ssim")[1].split()[0])
    assert math.isfinite(s) and -1.0 < s <= 1.0, out.stdout
