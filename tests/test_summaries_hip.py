"""``-m gpu``: the summary kernels (csrc/car_summary.hip) against their numpy restatements (tests/summary_restatement.py) and the
reference-made fixture (tests/golden/summary_expected.npz); the host module (summaries.py) — img_summaries, render_full, the guard against
stale packed weights between eval() renders and optimizer steps — and the training script's new flags, run as a child process."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import summary_cases
import summary_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")
TAGS = ["ent", "predictions", "depth_images", "context_images", "query_images", "epipolar_line", "out_min", "out_max", "trgt_min", "trgt_max"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits_equal(got, want) -> bool:
    """Same shape, NaN in the same places, the same bits everywhere else."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])


# ---- entropy ----------------------------------------------------------------------------------------------------------------------------
def _weights(rows, S, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.softmax(3 * torch.randn(rows, S, generator=g), dim=-1)
    if S > 1:
        w[::3, ::2] = 0.0                                             # rows holding exact zeros
    w[rows // 2] = 1.0 / S                                            # the uniform row: entropy ln S
    return w


@pytest.mark.parametrize("S", [1, 7, 64, 65, 128, 192])
def test_entropy_matches_the_float64_restatement(dev, S):
    from cross_attention_renderer_amd import summaries
    tol = R.entropy_tolerance(S)
    assert tol == 8 * 2.0 ** -24 * (math.log(S) + 1)
    for rows in (1, 3, 1000, 4097):
        w = _weights(rows, S, seed=rows + S)
        wd = w.to(dev)
        for flag in (True, False):
            got = summaries.attention_entropy(wd, nan_rows_zero=flag)
            assert got.dim() == 0 and got.dtype == torch.float64 and got.device.type == "cuda"
            again = summaries.attention_entropy(wd, nan_rows_zero=flag)
            assert got.view(torch.int64).item() == again.view(torch.int64).item(), "two runs differ"
            want = R.entropy_mean(w.numpy(), flag)
            ref32 = -(w * torch.log(w + 1e-5)).sum(dim=-1)            # the reference's fp32 expression, on the CPU
            print(f"S {S} rows {rows} flag {flag}: kernel {got.item():.9f} float64 {want:.9f} (diff {abs(got.item() - want):.2e}, bound {tol:.2e})")
            assert abs(got.item() - want) <= tol
            assert abs(got.item() - ref32.double().mean().item()) <= tol
        total, n = summaries.attention_entropy_sum(wd, True)
        assert n == rows and abs(total.item() / rows - want) <= tol


@pytest.mark.parametrize("rows,S", [(1, 7), (3, 64), (1000, 65)])
def test_entropy_nan_row_under_both_flags(dev, rows, S):
    from cross_attention_renderer_amd import summaries
    w = _weights(rows, S, seed=5)
    w[rows // 3, S // 2] = float("nan")
    zeroed = summaries.attention_entropy(w.to(dev), nan_rows_zero=True).item()
    assert abs(zeroed - R.entropy_mean(w.numpy(), True)) <= R.entropy_tolerance(S)          # the row counts in the mean with entropy 0
    if rows > 1:
        clean = np.delete(w.numpy(), rows // 3, axis=0)
        assert abs(zeroed - R.entropy_mean(clean, True) * (rows - 1) / rows) <= R.entropy_tolerance(S)
    assert math.isnan(summaries.attention_entropy(w.to(dev), nan_rows_zero=False).item()) and math.isnan(R.entropy_mean(w.numpy(), False))


def test_entropy_refuses_769_samples(dev):
    from cross_attention_renderer_amd import summaries
    with pytest.raises(ValueError, match="S = 769"):
        summaries.attention_entropy(torch.rand(2, 769, device=dev))
    summaries.attention_entropy(torch.rand(2, 768, device=dev))


# ---- colour map -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", [(2, 48, 48), (3, 37, 53)])
def test_colormap_bit_equal(dev, N, H, W):
    from cross_attention_renderer_amd import harness, summaries
    g = torch.Generator().manual_seed(H)
    x = torch.rand(N, H, W, generator=g) * 14 - 2
    special = torch.tensor([0.0, -0.0, 10.0, 9.999999, 10.000001, -1e-30, 1e30, float("nan"), float("inf"), -float("inf"), 10 / 256, 2550 / 256, 5.0])
    x.view(-1)[:special.numel()] = special
    x.view(-1)[-special.numel():] = special
    got = summaries.colormap(x.to(dev), 10.0)
    want = R.colormap(x.numpy(), 10.0, harness.jet_lut().numpy())
    assert got.shape == (N, H, W, 3) and bits_equal(got.cpu().numpy(), want)
    assert not np.isnan(want).any() and (want[0, 0, 7] == 0).all()    # NaN is the "bad" colour (0, 0, 0)
    lut = torch.rand(256, 3, generator=g)
    assert bits_equal(summaries.colormap(x.to(dev), 3.0, lut.to(dev)).cpu().numpy(), R.colormap(x.numpy(), 3.0, lut.numpy()))


# ---- overlay ----------------------------------------------------------------------------------------------------------------------------
def _overlay_inputs(B, V, H, W, S, rays, probe, seed):
    g = torch.Generator().manual_seed(seed)
    trgt, ctxt = torch.rand(B, H, W, 3, generator=g) * 2 - 1, torch.rand(B * V, H, W, 3, generator=g) * 2 - 1
    pixel_val = torch.rand(B * V, rays, S, 2, generator=g) * 2.6 - 1.3
    best = torch.randint(0, S, (B * V, rays, 1), generator=g)
    uv = torch.stack([torch.randint(0, W, (B, rays), generator=g), torch.randint(0, H, (B, rays), generator=g)], dim=-1).float()[:, None]
    return trgt, ctxt, pixel_val, best, uv


def _overlay_both(dev, args, V, probe):
    from cross_attention_renderer_amd import summaries
    got = summaries.epipolar_overlay(*[t.to(dev) for t in args], V, probe)
    want = R.overlay(*[t.numpy() for t in args], V, probe)
    return got.cpu().numpy(), want


@pytest.mark.parametrize("name", sorted(summary_cases.CASES))
def test_overlay_equals_the_fixture(dev, name):
    from cross_attention_renderer_amd import summaries
    B, V, H, W = summary_cases.CASES[name]
    inp, out, fx = summary_cases.load(name)
    got = summaries.epipolar_overlay(inp["query"]["rgb"].reshape(B, H, W, 3).to(dev), inp["context"]["rgb"].reshape(B * V, H, W, 3).to(dev),
                                     out["pixel_val"].to(dev), out["at_wt_max"].to(dev), out["uv"].to(dev), V)
    assert bits_equal(got.cpu().numpy(), fx["epipolar_line"])


@pytest.mark.parametrize("B,V,H,W,S,probe", [(2, 2, 64, 80, 16, 2065), (1, 3, 48, 48, 7, 100), (3, 1, 130, 70, 64, 0), (1, 2, 200, 136, 192, 9099)])
def test_overlay_bit_equal_on_other_shapes(dev, B, V, H, W, S, probe):
    args = _overlay_inputs(B, V, H, W, S, 9100, probe, seed=H + S)
    got, want = _overlay_both(dev, args, V, probe)
    assert got.shape == (B * (1 + V), H, W, 3) and bits_equal(got, want)
    assert (want[:B] == -1).all(axis=-1).any() and (want[B:] == 0).all(axis=-1).any()


def test_overlay_probe_on_each_border_and_empty_squares(dev):
    B, V, H, W, S, rays = 1, 2, 48, 56, 8, 64
    borders = {"left": ((0.0, 20.0), (-1.0, 0.1)), "right": ((W - 1.0, 20.0), (1.0, 0.1)), "top": ((30.0, 0.0), (0.2, -1.0)),
               "bottom": ((30.0, H - 1.0), (0.2, 1.0)), "corner": ((W - 1.0, H - 1.0), (1.0, 1.0)),
               "off the image": ((W + 5.0, 3.0), (7.0, -7.0)), "negative": ((-0.5, -0.9), (-1.0, -1.0)), "far": ((1e12, -1e12), (1e30, -1e30))}
    for k, (name, (pixel, sample)) in enumerate(borders.items()):
        trgt, ctxt, pixel_val, best, uv = _overlay_inputs(B, V, H, W, S, rays, k, seed=k)
        uv[:, 0, k] = torch.tensor(pixel)
        pixel_val[:, k] = torch.tensor(sample)                        # every sample of the probe ray on the border: squares cut by the edge
        pixel_val[1, k, 3] = torch.tensor([0.0, 0.0])
        got, want = _overlay_both(dev, (trgt, ctxt, pixel_val, best, uv), V, k)
        assert bits_equal(got, want), name
        marked = (want[0] == -1).all(axis=-1).sum()
        if name in ("right", "bottom", "corner", "off the image", "far"):
            # the exclusive upper end: a square centred on the last column or row stops before it
            assert not (want[:, -1] == -1).all(axis=-1).any() and not (want[:, :, -1] == -1).all(axis=-1).any(), name
        if name in ("off the image", "far"):
            assert marked == 0 and np.array_equal(want[0], trgt[0].numpy()), name        # an empty square: the target tile is the input
        else:
            assert marked > 0, name


def test_overlay_refuses_a_frame_with_fewer_rays(dev):
    from cross_attention_renderer_amd import summaries
    args = [t.to(dev) for t in _overlay_inputs(1, 1, 32, 32, 4, 1024, 0, seed=0)]
    with pytest.raises(ValueError, match="probe ray 2065"):
        summaries.epipolar_overlay(*args, 1)


# ---- grid -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (48, 48)])
def test_grid_bit_equal(dev, H, W):
    from cross_attention_renderer_amd import summaries
    for N in (1, 2, 8, 9, 17):
        g = torch.Generator().manual_seed(N * H)
        x = torch.randn(N, H, W, 3, generator=g) * torch.linspace(0.5, 2.0, N)[:, None, None, None]    # images of different range
        for scale_each in (False, True):
            for clamp in (None, (-1.0, 1.0)):
                got = summaries.image_grid(x.to(dev), scale_each=scale_each, clamp=clamp)
                want = R.make_grid(x.numpy(), scale_each=scale_each, clamp=clamp)
                assert tuple(got.shape) == (3, *R.grid_shape(N, H, W)) == want.shape
                assert bits_equal(got.cpu().numpy(), want), (N, scale_each, clamp)
    const = torch.full((3, H, W, 3), 0.25)
    assert (summaries.image_grid(const.to(dev)) == 0).all()


def test_grid_nan_rule(dev):
    from cross_attention_renderer_amd import summaries
    g = torch.Generator().manual_seed(3)
    x = torch.randn(9, 5, 7, 3, generator=g)
    x[4, 2, 3, 1] = float("nan")
    for scale_each in (False, True):
        for clamp in (None, (-1.0, 1.0)):
            got = summaries.image_grid(x.to(dev), scale_each=scale_each, clamp=clamp).cpu().numpy()
            want = R.make_grid(x.numpy(), scale_each=scale_each, clamp=clamp)
            assert bits_equal(got, want)
            cell = got[:, 2:7, 4 * 9 + 2:4 * 9 + 9]
            assert np.isnan(cell).all() and (got[:, :2] == 0).all()
            assert np.isnan(got[:, 2:7, 2:9]).all() == (not scale_each)           # the other images only under the global range
    one = summaries.image_grid(x[4:5].to(dev)).cpu().numpy()
    assert one.shape == (3, 5, 7) and np.isnan(one).all()


# ---- the host module ----------------------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, value, step))

    def add_image(self, tag, img, step):
        self.calls.append((tag, img, step))


@pytest.mark.parametrize("name", sorted(summary_cases.CASES))
def test_img_summaries_on_device_tensors(dev, name, monkeypatch):
    from cross_attention_renderer_amd import summaries
    B, V, H, W = summary_cases.CASES[name]
    inp, out, fx = summary_cases.load(name)
    to = lambda d: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    inp_d, out_d = {k: to(v) for k, v in inp.items()}, to(out)
    grids, real_grid = [], summaries.image_grid

    def recording_grid(x, scale_each=False, clamp=None):
        grids.append((x.detach().cpu().numpy().copy(), scale_each, clamp))
        return real_grid(x, scale_each=scale_each, clamp=clamp)
    monkeypatch.setattr(summaries, "image_grid", recording_grid)
    rec = Recorder()
    summaries.img_summaries(None, inp_d, None, {}, out_d, rec, 40, prefix="val_", img_shape=(H, W), n_view=V)
    assert [c[0] for c in rec.calls] == ["val_" + t for t in TAGS] == list(fx["tags"]) and all(c[2] == 40 for c in rec.calls)
    got = dict((c[0][4:], c[1]) for c in rec.calls)
    pred, depth, _, _, panel = grids
    assert pred[1:] == (False, (-1.0, 1.0)) and depth[1:] == (True, None) and panel[1:] == (False, None)
    assert bits_equal(np.clip(pred[0], -1, 1), fx["predictions"])
    assert bits_equal(depth[0], fx["depth_images"])
    assert bits_equal(panel[0], fx["epipolar_line"])
    for tag, arg in (("predictions", pred), ("depth_images", depth), ("epipolar_line", panel)):
        assert tuple(got[tag].shape) == (3, *R.grid_shape(arg[0].shape[0], H, W)) and got[tag].device.type == "cuda"
        assert bits_equal(got[tag].cpu().numpy(), R.make_grid(*arg))
    assert abs(got["ent"].item() - float(fx["ent"])) <= R.entropy_tolerance(summary_cases.SAMPLES)
    for tag in ("out_min", "out_max", "trgt_min", "trgt_max"):
        assert got[tag].item() == float(fx[tag]), tag
    # the tensors handed in are not painted
    assert torch.equal(inp_d["context"]["rgb"].cpu(), inp["context"]["rgb"]) and torch.equal(inp_d["query"]["rgb"].cpu(), inp["query"]["rgb"])


def _module(H, P, seed, dev=None):
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    torch.manual_seed(0)
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=P, with_encoder=False).eval()
    if seed is not None:
        S.perturb_parameters(m, seed=seed)
    m.H = m.W = H
    return m if dev is None else m.to(dev)


def _scene(H, b, dev, uv=None):
    from cross_attention_renderer_amd import harness, synthetic as S
    inp = harness.to_device(S.stereo_scene(H, b=b, seed=11, uv=uv), dev, "host")
    return inp, [t.to(dev) for t in S.feature_maps(b, 2, H, seed=3)]


def test_render_full_in_chunks_equals_one_call(dev):
    from cross_attention_renderer_amd import summaries
    H, P, b = 64, 16, 2
    m = _module(H, P, 1, dev)
    inp, z = _scene(H, b, dev)
    with torch.no_grad():
        whole = m(inp, z=z)
    ent = R.entropy_mean(whole["at_wt"].cpu().numpy(), False)
    for kw in (dict(chunk_rays=1000), dict(chunk_rays=2048), dict(chunk_rays=4095)):
        out = summaries.render_full(m, inp, z, **kw)
        assert torch.equal(out["rgb"], whole["rgb"]) and torch.equal(out["depth_ray"], whole["depth_ray"]), kw
        assert torch.equal(out["valid_mask"], whole["valid_mask"]) and out["uv"] is inp["query"]["uv"]
        assert out["probe"] == 2065 and out["pixel_val"].shape == (b * 2, 1, P, 2) and out["at_wt_max"].shape == (b * 2, 1, 1)
        assert torch.equal(out["pixel_val"][:, 0], whole["pixel_val"][:, 2065]) and torch.equal(out["at_wt_max"][:, 0], whole["at_wt_max"][:, 2065])
        assert out["ent_rows"] == b * 2 * H * H and out["ent_sum"].device.type == "cuda"
        assert abs(out["ent_sum"].item() / out["ent_rows"] - ent) <= R.entropy_tolerance(P)
        assert "at_wt" not in out
    # the chunked dict draws the same epipolar panel as the one call's
    rec_a, rec_b = Recorder(), Recorder()
    g = torch.Generator().manual_seed(2)
    tiles = {"context": dict(inp["context"], rgb=(torch.rand(b, 2, H, H, 3, generator=g) * 2 - 1).to(dev)),
             "query": dict(inp["query"], rgb=(torch.rand(b, 1, H * H, 3, generator=g) * 2 - 1).to(dev))}
    summaries.img_summaries(m, tiles, None, {}, whole, rec_a, 0, "val_", img_shape=(H, H), n_view=2)
    summaries.img_summaries(m, tiles, None, {}, out, rec_b, 0, "val_", img_shape=(H, H), n_view=2)
    assert [c[0] for c in rec_a.calls] == [c[0] for c in rec_b.calls] == ["val_" + t for t in TAGS]
    for a, b_ in zip(rec_a.calls, rec_b.calls):
        if a[0] != "val_ent":
            assert torch.equal(a[1], b_[1]), a[0]
    with pytest.raises(ValueError, match="probe ray"):
        summaries.render_full(m, inp, z, probe=H * H)


def test_eval_render_after_an_optimizer_step_sees_the_new_weights(dev):
    """Validation alternates eval() renders with optimizer steps on one module: the engine's packed-weight caches must follow the
    in-place parameter updates."""
    from cross_attention_renderer_amd import synthetic as S, training
    H, P, R_ = 64, 16, 96
    m = _module(H, P, 1, dev)
    uv = S.pixel_grid(H, H)[:: (H * H) // R_][:R_].contiguous()
    inp, z = _scene(H, 1, dev, uv=uv)

    def render(module):
        module.eval()
        with torch.no_grad():
            return module(inp, z=z)["rgb"].clone()
    first = render(m)
    m.train()
    opt = training.make_adam([p for p in m.parameters() if p.requires_grad], 1e-3)
    out = m(inp, z=z)                                                 # train() under autograd: render_train
    out["rgb"].abs().mean().backward()
    opt.step()
    second = render(m)
    assert not torch.equal(first, second)
    fresh = _module(H, P, None)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    assert torch.equal(second, render(fresh.to(dev)))


# ---- the training script ------------------------------------------------------------------------------------------------------------------
def _losses(stdout):
    return re.findall(r"^step (\d+): loss (\S+)", stdout, flags=re.M)


def test_training_script_with_summaries(dev, tmp_path):
    base = [sys.executable, TRAIN, "--experiment_name", "t", "--synthetic", "--img_sidelength", "64", "--batch_size", "2", "--query_sparsity", "192",
            "--max_steps", "3", "--steps_til_summary", "2"]
    new = subprocess.run(base + ["--logging_root", str(tmp_path / "new"), "--summaries", "--iters_til_ckpt", "2"], capture_output=True, text=True, timeout=600)
    assert new.returncode == 0, new.stdout + new.stderr
    old = subprocess.run(base + ["--logging_root", str(tmp_path / "old")], capture_output=True, text=True, timeout=600)
    assert old.returncode == 0, old.stdout + old.stderr
    # summaries, validation and the extra checkpoint leave the training itself alone
    assert _losses(new.stdout) == _losses(old.stdout) and [s for s, _ in _losses(old.stdout)] == ["0", "2"]
    assert new.stdout.split("trained 3 steps: loss ")[1].split(";")[0] == old.stdout.split("trained 3 steps: loss ")[1].split(";")[0]
    assert not (tmp_path / "old" / "t" / "summaries").exists()
    assert sorted(os.listdir(tmp_path / "old" / "t" / "checkpoints")) == ["model_current.pth", "model_final.pth"]
    run = tmp_path / "new" / "t"
    assert (run / "checkpoints" / "model_epoch_0000_iter_000002.pth").exists()
    lines = [json.loads(l) for l in open(run / "summaries" / "scalars.jsonl")]
    steps = lambda tag: [l["step"] for l in lines if l["tag"] == tag]
    for tag in ("total_at_entropy", "total_train_loss", "img_loss"):
        assert steps(tag) == [0, 1, 2], tag
    for tag in ("val_img_loss", "val_ent", "val_out_min", "val_trgt_max"):
        assert steps(tag) == [0, 2], tag
    assert all(math.isfinite(l["value"]) for l in lines)
    ent = [l["value"] for l in lines if l["tag"] == "total_at_entropy"]
    assert all(0 < e <= math.log(64) + 1e-3 for e in ent)
    printed = dict(_losses(new.stdout))
    for l in lines:
        if l["tag"] == "total_train_loss" and str(l["step"]) in printed:
            assert f"{l['value']:.5f}" == printed[str(l["step"])]
    sizes = {"val_predictions": 8, "val_depth_images": 8, "val_context_images": 16, "val_query_images": 8, "val_epipolar_line": 24}
    for tag, n in sizes.items():
        for step in (0, 2):
            data = open(run / "summaries" / "images" / tag / f"{step:06d}.png", "rb").read()
            Hg, Wg = R.grid_shape(n, 64, 64)
            assert (int.from_bytes(data[20:24], "big"), int.from_bytes(data[16:20], "big")) == (Hg, Wg), tag
