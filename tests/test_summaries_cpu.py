"""CPU checks of the training summaries: the numpy restatements (tests/summary_restatement.py) against what the reference's own code made
(tests/golden/summary_expected.npz, tests/golden/make_summary_golden.py) and against matplotlib, make_grid's closed forms, the C entries'
argument checks, the built-in writer and the training script's refusals.  The kernels themselves: tests/test_summaries_hip.py."""
import argparse
import ctypes
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import summary_cases
import summary_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["ent", "predictions", "depth_images", "context_images", "query_images", "epipolar_line", "out_min", "out_max", "trgt_min", "trgt_max"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(summary_cases.CASES))
def test_restatements_equal_what_the_reference_made(name):
    from cross_attention_renderer_amd import harness
    B, V, H, W = summary_cases.CASES[name]
    inp, out, fx = summary_cases.load(name)
    assert list(fx["tags"]) == ["val_" + t for t in TAGS]
    trgt = inp["query"]["rgb"].reshape(B, H, W, 3).numpy()
    ctxt = inp["context"]["rgb"].reshape(B * V, H, W, 3).numpy()
    panel = R.overlay(trgt, ctxt, out["pixel_val"].numpy(), out["at_wt_max"].numpy(), out["uv"].numpy(), V)
    assert panel.shape == fx["epipolar_line"].shape and np.array_equal(panel, fx["epipolar_line"])
    assert (panel != np.concatenate([trgt, ctxt.reshape(B, V, H, W, 3).transpose(1, 0, 2, 3, 4).reshape(B * V, H, W, 3)])).any()
    depth = R.colormap(out["depth_ray"].reshape(B, H, W).numpy(), 10.0, harness.jet_lut().numpy())
    assert depth.dtype == np.float32 and np.array_equal(depth, fx["depth_images"])
    pred = np.clip(out["rgb"].reshape(B, H, W, 3).numpy(), -1, 1)
    assert np.array_equal(pred, fx["predictions"])
    assert float(pred.min()) == fx["out_min"] and float(pred.max()) == fx["out_max"]
    assert float(trgt.min()) == fx["trgt_min"] and float(trgt.max()) == fx["trgt_max"]
    # the reference's entropy is an fp32 torch expression: the same bound as the kernel's
    assert abs(R.entropy_mean(out["at_wt"].numpy(), False) - float(fx["ent"])) <= R.entropy_tolerance(summary_cases.SAMPLES)


def test_fixture_cases_exercise_the_edges():
    """The left-edge clip at 48 x 48 (ray 2065 is row 43, column 1), pix = 2 at 64 x 64, samples outside [-1, 1], and an arg-max on a border."""
    for name, (B, V, H, W) in summary_cases.CASES.items():
        _, out, fx = summary_cases.load(name)
        uv = out["uv"][0, 0, summary_cases.PROBE]
        assert (int(uv[0]), int(uv[1])) == (summary_cases.PROBE % W, summary_cases.PROBE // W)
        row = out["pixel_val"][:, summary_cases.PROBE]
        assert (row.abs() > 1).any() and (row.abs() < 1).any()
        panel = fx["epipolar_line"]
        assert (panel[:B] == -1).all(axis=-1).sum() > 0 and (panel[B:] == 0).all(axis=-1).sum() > 0 and (panel[B:] == -1).all(axis=-1).sum() > 0
        assert not (panel[:, -1] == -1).all(axis=-1).any() and not (panel[:, :, -1] == -1).all(axis=-1).any()   # the last row / column is never painted
    assert summary_cases.PROBE % 48 == 1 and 48 // 64 + 1 == 1 and 64 // 64 + 1 == 2


def test_jet_table_and_colormap_equal_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from cross_attention_renderer_amd import harness
    cmap = plt.get_cmap("jet")
    table = cmap(np.arange(256))[:, :3]                               # integer input indexes the table directly
    assert np.array_equal(R.jet_table(), table)
    lut = harness.jet_lut()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (256, 3)
    assert np.array_equal(lut.numpy(), table.astype(np.float32))
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-0.2, 1.2, 4000), [-1.0, -0.0, 0.0, 1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 1.5, np.nan, np.inf, -np.inf,
                                                       1 / 256, 255 / 256]]).astype(np.float32)
    want = torch.Tensor(cmap(x)[..., :3]).numpy()                     # summaries.py:38-41
    assert np.array_equal(R.colormap(x, 1.0, lut.numpy()), want)
    depth = (x * np.float32(10)).astype(np.float32)
    assert np.array_equal(R.colormap(depth, 10.0, lut.numpy()), torch.Tensor(cmap(depth / 10.)[..., :3]).numpy())


def test_grid_closed_forms():
    rng = np.random.default_rng(1)
    for N, want in ((1, (5, 7)), (2, (9, 20)), (8, (9, 74)), (9, (16, 74))):
        x = rng.normal(size=(N, 5, 7, 3)).astype(np.float32)
        g = R.make_grid(x)
        assert g.shape == (3, *want) == (3, *R.grid_shape(N, 5, 7))
        assert g.min() == 0.0 and g.max() == 1.0
        if N > 1:
            xm = min(8, N)
            mask = np.ones(g.shape[1:], bool)
            for k in range(N):
                r, c = (k // xm) * 7 + 2, (k % xm) * 9 + 2
                mask[r:r + 5, c:c + 7] = False
                assert np.array_equal(g[:, r:r + 5, c:c + 7], ((x[k] - x.min()) / np.float32(max(float(x.max()) - float(x.min()), 1e-5))).transpose(2, 0, 1))
            assert (g[:, mask] == 0).all()                           # the padding and the empty cells
    assert (R.make_grid(np.full((3, 5, 7, 3), 0.25, np.float32)) == 0).all()          # a constant image maps to 0
    two = np.stack([rng.uniform(0, 1, (5, 7, 3)), rng.uniform(-4, 4, (5, 7, 3))]).astype(np.float32)
    each, whole = R.make_grid(two, scale_each=True), R.make_grid(two, scale_each=False)
    first = each[:, 2:7, 2:9]
    assert first.min() == 0.0 and first.max() == 1.0                  # its own range
    assert whole[:, 2:7, 2:9].max() < 0.7 and whole[:, 2:7, 11:18].max() == 1.0        # the global range is the second image's
    assert np.array_equal(each[:, 2:7, 11:18], whole[:, 2:7, 11:18])
    clamped = R.make_grid(two, clamp=(-1, 1))
    assert np.array_equal(clamped, R.make_grid(np.clip(two, -1, 1)))
    bad = two.copy()
    bad[1, 2, 3, 1] = np.nan
    each = R.make_grid(bad, scale_each=True)
    assert np.isnan(each[:, 2:7, 11:18]).all() and np.array_equal(each[:, 2:7, 2:9], first) and np.isnan(R.make_grid(bad)[:, 2:7, 2:9]).all()
    assert (R.make_grid(bad)[:, :2] == 0).all()                       # the padding stays 0


def test_entries_refuse_bad_arguments(lib):
    """The four entries and their size queries: CAR_E_ARG (or size 0) with a message, never an abort, and without a GPU."""
    p = ctypes.c_void_p(64)                                           # a non-null pointer that no refused call reads

    def refused(code, word):
        assert code == -1 and word.encode() in lib.car_last_error(), (code, lib.car_last_error())
    assert lib.car_attention_entropy_scratch_doubles(4097, 64) == 1024 and lib.car_attention_entropy_scratch_doubles(3, 7) == 1
    for S in (0, 769):
        assert lib.car_attention_entropy_scratch_doubles(10, S) == 0 and b"S = " in lib.car_last_error()
        refused(lib.car_attention_entropy(p, 10, S, 1, p, p, 1024, None), "S = ")
    assert lib.car_attention_entropy_scratch_doubles(0, 64) == 0
    refused(lib.car_attention_entropy(p, 0, 64, 1, p, p, 1024, None), "rows")
    refused(lib.car_attention_entropy(None, 10, 64, 1, p, p, 1024, None), "null pointer")
    refused(lib.car_attention_entropy(p, 10, 64, 1, None, p, 1024, None), "null pointer")
    refused(lib.car_attention_entropy(p, 4097, 64, 1, p, p, 1023, None), "scratch")
    refused(lib.car_colormap(None, 1, 8, 8, 10.0, p, p, None), "null pointer")
    refused(lib.car_colormap(p, 1, 0, 8, 10.0, p, p, None), "H >= 1")
    refused(lib.car_colormap(p, 1, 8, 8, 0.0, p, p, None), "scale")
    refused(lib.car_epipolar_overlay(p, p, None, p, p, 1, 1, 64, 64, 4096, 2065, 16, p, None), "null pointer")
    refused(lib.car_epipolar_overlay(p, p, p, p, p, 1, 1, 32, 32, 1024, 2065, 16, p, None), "probe ray 2065")
    refused(lib.car_epipolar_overlay(p, p, p, p, p, 1, 1, 32, 32, 1024, -1, 16, p, None), "probe ray")
    refused(lib.car_epipolar_overlay(p, p, p, p, p, 1, 1, 0, 64, 4096, 2065, 16, p, None), "1 <= H")
    for S in (0, 769):
        refused(lib.car_epipolar_overlay(p, p, p, p, p, 1, 1, 64, 64, 4096, 2065, S, p, None), "S = ")
    refused(lib.car_epipolar_overlay(p, p, p, p, p, 0, 1, 64, 64, 4096, 2065, 16, p, None), "scene")
    assert lib.car_image_grid_scratch_floats(9, 48, 48) == 18
    assert lib.car_image_grid_scratch_floats(9, 0, 48) == 0 and b"H >= 1" in lib.car_last_error()
    refused(lib.car_image_grid(None, 2, 8, 8, 0, 0, 0.0, 0.0, p, p, 4, None), "null pointer")
    refused(lib.car_image_grid(p, 2, 0, 8, 0, 0, 0.0, 0.0, p, p, 4, None), "H >= 1")
    refused(lib.car_image_grid(p, 0, 8, 8, 0, 0, 0.0, 0.0, p, p, 4, None), "N >= 1")
    refused(lib.car_image_grid(p, 2, 8, 8, 0, 1, 1.0, -1.0, p, p, 4, None), "clamp")
    refused(lib.car_image_grid(p, 2, 8, 8, 0, 0, 0.0, 0.0, p, p, 3, None), "scratch")


def test_host_module_refuses_cpu_tensors():
    from cross_attention_renderer_amd import summaries
    with pytest.raises(ValueError, match="no CPU fallback"):
        summaries.attention_entropy(torch.rand(4, 8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        summaries.image_grid(torch.rand(2, 5, 7, 3))
    assert summaries.grid_shape(9, 48, 48) == R.grid_shape(9, 48, 48) == (102, 402) and summaries.grid_shape(1, 5, 7) == (5, 7)


def test_summary_log_writes_lines_and_pngs_and_keeps_tensors_until_flush(tmp_path):
    from cross_attention_renderer_amd import summaries
    log = summaries.SummaryLog(str(tmp_path / "s"))
    t = torch.tensor(1.5)
    log.add_scalar("a", t, 0)
    log.add_scalar("b", 0.25, 0)
    log.add_scalar("a", torch.tensor(float("nan"), dtype=torch.float64), 1)
    assert log._pending[0][2] is t or log._pending[0][2].data_ptr() == t.data_ptr()           # the tensor itself is kept, not a number
    assert not os.path.exists(tmp_path / "s" / "scalars.jsonl")
    t.fill_(2.5)                                                      # read at flush(), not at add_scalar()
    log.flush()
    lines = [json.loads(l) for l in open(tmp_path / "s" / "scalars.jsonl")]
    assert lines[:2] == [{"tag": "a", "step": 0, "value": 2.5}, {"tag": "b", "step": 0, "value": 0.25}]
    assert lines[2]["tag"] == "a" and lines[2]["step"] == 1 and math.isnan(lines[2]["value"])
    log.add_scalar("c", 3, 7)
    log.close()
    assert len(open(tmp_path / "s" / "scalars.jsonl").readlines()) == 4                        # appended
    img = torch.rand(3, 9, 20)
    log.add_image("val_predictions", img, 12)
    path = tmp_path / "s" / "images" / "val_predictions" / "000012.png"
    assert str(path) == log.image_path("val_predictions", 12) and path.exists()
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and (int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")) == (20, 9)
    with pytest.raises(ValueError):
        log.add_image("x", torch.rand(9, 20, 3), 0)


def _script():
    spec = importlib.util.spec_from_file_location("train_realestate10k_for_test", os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_refusals_need_no_device():
    mod = _script()
    parse = lambda *a: mod._parser().parse_args(["--experiment_name", "t", *a])
    opt = parse()
    assert not opt.summaries and opt.val_root is None and opt.val_batch_size == 8 and opt.iters_til_ckpt == 10000
    mod._check(opt)
    mod._check(parse("--summaries"))
    with pytest.raises(SystemExit, match="--val_pose_root"):
        mod._check(parse("--data_root", "d", "--pose_root", "p.mat", "--val_root", "v"))
    with pytest.raises(SystemExit, match="synthetic"):
        mod._check(parse("--synthetic", "--val_root", "v", "--val_pose_root", "v.mat"))
    mod._check(parse("--data_root", "d", "--pose_root", "p.mat", "--val_root", "v", "--val_pose_root", "v.mat", "--summaries"))


def test_leaving_train_mode_parks_the_parameter_caches_and_returning_restores_them(lib):
    """The validation pass renders from empty caches and hands the training loop's own caches back untouched (no device needed: the
    engine's caches are host objects)."""
    from cross_attention_renderer_amd.engine import RenderEngine
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=8, with_encoder=False).eval()
    m._engine = eng = RenderEngine(m)
    names = RenderEngine._PARAMETER_CACHES
    m.eval()                                                          # already in eval(): nothing is set aside
    before = {n: getattr(eng, n) for n in names}
    m.train()
    assert all(getattr(eng, n) is before[n] for n in names)
    eng._packed.value, eng._layer_packs["x"].value = "packed while training", "layer pack"
    m.eval()                                                          # the validation pass: empty caches
    assert all(getattr(eng, n) is not before[n] for n in names)
    assert eng._packed.value is None and not eng._layer_packs and eng._plan.value is None
    eng._packed.value = "packed for validation"
    m.eval()                                                          # a second eval() does not set the validation caches aside
    assert eng._packed.value == "packed for validation"
    m.train()                                                         # back to the loop: its caches as they were
    assert all(getattr(eng, n) is before[n] for n in names)
    assert eng._packed.value == "packed while training" and eng._layer_packs["x"].value == "layer pack"
    m.eval()
    assert eng._packed.value is None
