"""Render/eval plumbing (cross_attention_renderer_amd/harness.py, experiment_scripts/): CPU checks of the pieces that
need no GPU, and a GPU run of both entry points on a small synthetic pair."""
import os
import subprocess
import sys
import zlib

import pytest
import torch

from cross_attention_renderer_amd import harness, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trajectory_interpolates_between_context_cameras():
    inp = synthetic.stereo_scene(16, b=2, uv=synthetic.pixel_grid(16, 16)[:4].contiguous())
    frames = harness.trajectory(inp, 5)
    c2w = inp["context"]["cam2world"]
    assert len(frames) == 5
    assert torch.allclose(frames[0]["query"]["cam2world"][:, 0], c2w[:, 0], atol=1e-6)
    assert torch.allclose(frames[-1]["query"]["cam2world"][:, 0], c2w[:, 1], atol=1e-6)
    mid = frames[2]["query"]["cam2world"][0, 0]
    assert torch.allclose(mid[:3, :3] @ mid[:3, :3].T, torch.eye(3), atol=1e-5)          # still a rotation
    assert torch.allclose(mid[:3, 3], (c2w[0, 0, :3, 3] + c2w[0, 1, :3, 3]) / 2, atol=1e-6)


def test_png_writer_and_psnr(tmp_path):
    img = torch.rand(5, 7, 3) * 2 - 1
    p = tmp_path / "x.png"
    harness.write_png(str(p), img)
    data = p.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and b"IHDR" in data and b"IEND" in data
    idat = data[data.index(b"IDAT") + 4: data.index(b"IEND") - 8]
    raw = zlib.decompress(idat)
    assert len(raw) == 5 * (1 + 7 * 3)
    assert harness.psnr(img, img) == float("inf")
    assert abs(harness.psnr(torch.zeros(4), torch.full((4,), 0.1)) - 20.0) < 1e-4


def test_entry_points_parse_reference_flags():
    sys.path.insert(0, os.path.join(ROOT, "experiment_scripts"))
    import common
    opt = common.parser("x").parse_args(["--experiment_name", "e", "--views", "2", "--gpus", "1", "--model", "midas_vit",
                                         "--checkpoint_path", "c.pth", "--no_sample", "--no_latent_concat",
                                         "--no_multiview", "--batch_size", "3"])
    assert opt.views == 2 and opt.no_sample and opt.batch_size == 3


@pytest.mark.gpu
@pytest.mark.parametrize("script,extra", [("render_realestate10k_traj.py", ["--n_frames", "2"]),
                                          ("render_unposed_traj.py", ["--n_frames", "2"]),
                                          ("eval_realestate10k.py", ["--batch_size", "1"]),
                                          ("eval_acid.py", ["--batch_size", "1"])])
def test_entry_points_run_on_gpu(script, extra, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", script), "--experiment_name", "t", "--views", "2",
           "--synthetic", "--img_sidelength", "64", "--out_dir", str(tmp_path), "--logging_root", str(tmp_path)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    if script.startswith("render"):
        assert (tmp_path / "frame_0001.png").exists()
        assert "rays/s" in out.stdout or "rendered 2 frames" in out.stdout
    else:
        psnr = float(out.stdout.split("psnr vs un-chunked render")[1].split("dB")[0])
        assert psnr > 100.0, out.stdout          # chunking must not change the image


@pytest.mark.gpu
def test_render_script_reads_a_scene_directory(tmp_path):
    """--data_root / --pose_root: cameras of every frame come from the RealEstate10K reader (tests/golden/dataio_scene)."""
    scene_root = os.path.join(ROOT, "tests", "golden", "dataio_scene")
    import shutil
    data_root = tmp_path / "scenes"
    shutil.copytree(os.path.join(scene_root, "scene0"), data_root / "scene0")
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "render_realestate10k_traj.py"), "--experiment_name", "t", "--views", "2",
           "--data_root", str(data_root), "--pose_root", os.path.join(scene_root, "poses"), "--img_sidelength", "64", "--n_frames", "2",
           "--out_dir", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "out" / "scene0" / "frame_0001.png").exists() and "rendered 2 frames" in out.stdout


@pytest.mark.gpu
def test_eval_script_reads_the_dataset_and_runs_get_z(tmp_path):
    """eval_realestate10k.py on the committed evaluation scene (tests/golden/dataio_scene_vis: frames at 256 x 455 + .mat poses): the
    item comes from dataio.RealEstate10kVis, get_z runs the multi-view DPT encoder on the two context frames (random weights: no
    checkpoint offline), the 65 536 query rays are rendered in 9 chunks and a PSNR against the ground-truth frame is reported."""
    vis = os.path.join(ROOT, "tests", "golden", "dataio_scene_vis")
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "eval_realestate10k.py"), "--experiment_name", "t", "--views", "2",
           "--data_root", os.path.join(vis, "scenes"), "--pose_root", os.path.join(vis, "poses.mat"), "--logging_root", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "item 0:" in out.stdout and "mean psnr" in out.stdout
    psnr = float(out.stdout.split("mean psnr")[1].split()[0])
    assert 0.0 < psnr < 60.0                      # an untrained model: a finite, unremarkable number


@pytest.mark.gpu
def test_training_entry_point_runs_and_writes_reference_style_checkpoints(tmp_path):
    """experiment_scripts/train_realestate10k.py on synthetic scenes: a few optimizer steps through render_train (HIP forward and
    backward), checkpoints in the reference's {'model', 'optimizer'} format (training.py:82-84, 244-246)."""
    import torch
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py"), "--experiment_name", "t", "--views", "2",
           "--img_sidelength", "64", "--batch_size", "2", "--max_steps", "4", "--steps_til_summary", "2", "--logging_root", str(tmp_path), "--depth",
           "--query_sparsity", "1024"]          # --depth: one 32 x 32 pixel patch per scene (the reference's depth-variance term works on such patches)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "trained 4 steps" in out.stdout
    ck = torch.load(tmp_path / "t" / "checkpoints" / "model_final.pth", map_location="cpu")
    assert set(ck) == {"model", "optimizer"} and "query_encode_latent.weight" in ck["model"] and ck["optimizer"]["state"]
    first, last = [float(x) for x in out.stdout.split("loss ")[-1].split(";")[0].split(" -> ")]
    assert first == first and last == last                      # finite


@pytest.mark.gpu
def test_bench_prints_one_line_with_the_contract_fields():
    """`python bench.py --full` (small K / W, a 256-ray CPU sample): the last stdout line is ONE JSON object with the fields the driver
    reads — metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config —
    plus the `roofline` (bound in {hbm, mfma}, achieved / peak / unit / frac / traffic) and `cpu_baseline` objects, and what the
    restructured path keeps outside the timed region: `pair_setup_ms`, `lattice_bytes`, `workspace_bytes`, `eval_mode`, the gather stage with
    its spread, the rank-share projection and the cost of handing the cameras over on the GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "4", "--warmup", "2", "--cpu-rays", "256"],
                         capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "rendered_rays_per_sec" and d["unit"] == "rays/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 65536 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.0 < r["frac"] < 1.0 and r["traffic"] is not None and set(r["live_fields"]).isdisjoint(r["static_fields"])
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1 and "sample" in c
    assert d["config"]["name"] == "c2" and d["config"]["builder_kept"] is False
    assert d["pair_setup_ms"] > 0 and d["lattice_bytes"] > 2e9 and d["workspace_bytes"] > 1e10
    ev = d["eval_mode"]
    assert ev["unit"] == "rays/s" and ev["ms_per_step"] > 0 and abs(ev["value"] - 65536 / (ev["ms_per_step"] * 1e-3)) < 1e-3 * ev["value"]
    g = d["gather_stage"]
    assert g["pairs"] >= 20 and g["warmup_pairs"] >= 30 and g["ms_min"] <= g["ms"] <= g["ms_max"] and g["frac_min"] <= g["frac"] <= g["frac_max"]
    assert abs(g["spread"] - (g["ms_max"] - g["ms_min"]) / g["ms"]) < 1e-9
    assert d["rank_share"]["rays_per_step"] == 8192 and 1.0 < d["rank_share"]["projected_scaling_8"] <= 8.5
    assert 1.0 < d["rank_share"]["projected_scaling_2"] <= 2.2 and 1.0 < d["rank_share"]["projected_scaling_4"] <= 4.3
    # the A/B blocks: presence and sanity only — which side is faster (and by how much) is a measurement recorded under profiles/, not a
    # property a test on a power-capped, possibly shared GPU can assert
    ab = d["first_round_ab"]
    for side in (ab["rows_of_e"]["stage_ms"], d["stage_ms"]):
        assert side["attend_1"] > 0 and side["fused_samples"] > 0 and all(v == v and v < 1e4 for v in side.values())
    assert 0.0 < r["frac"] < 1.0 and 0.0 < r["frac_without_partial_sums"] < 1.0 and 0.0 < r["frac_executed"] < r["frac"]
    pw = d["power"]                                                    # sampled beside the timed loop; a box without a power interface says so
    assert "available" in pw and (not pw["available"] or (pw["mean_w"] > 50 and pw["samples"] >= 5 and pw["joule_per_frame"] > 0))
    assert ("sclk_mhz_live" in r) and ("socket_w_live" in r)
    assert d["pose_route"]["download_and_sync_ms"] > 0 and d["pose_route"]["cameras_on_gpu_ms_per_step"] > 0


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_last_frame(tmp_path):
    """`python bench.py --dump-outputs DIR` without --full: the contract fields, none of the secondary measurements, and the last timed
    step's frame and attention weights as float32 arrays (at most 64 MB) that two runs with the same arguments reproduce."""
    import json
    import numpy as np
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        runs.append((json.loads(lines[0]), {p.stem: np.load(p) for p in d.glob("*.npy")}))
    line, arrays = runs[0]
    assert line["metric"] == "rendered_rays_per_sec" and line["unit"] == "rays/s" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and "split-f16" in line["dtype"]
    assert abs(line["value"] - 65536 / (line["ms_per_step"] * 1e-3)) < 1e-3 * line["value"]
    for k in ("stage_ms", "roofline", "hbm", "gather_stage", "eval_mode", "rank_share", "first_round_ab", "power", "pose_route", "cpu_baseline"):
        assert line[k] is None, k
    assert set(arrays) == {"rgb", "depth_ray", "valid_mask", "at_wt"}
    assert arrays["rgb"].shape == (1, 65536, 3) and arrays["depth_ray"].shape == arrays["valid_mask"].shape == (1, 65536)
    assert arrays["at_wt"].shape == (2 * 65536, 64) and sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert set(np.unique(arrays["valid_mask"])) <= {0.0, 1.0}
    assert np.allclose(arrays["at_wt"].reshape(2, 65536, 64).sum(axis=(0, 2)), 1.0, atol=1e-4)     # one softmax over both views' samples
    for k, a in arrays.items():
        np.testing.assert_array_equal(a, runs[1][1][k], err_msg=k)


def test_bench_refuses_a_world_size_that_is_not_the_requested_gpu_count():
    """--gpus N with fewer (or more) launched ranks must fail loudly, not print a line that looks like an N-GPU figure."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, cwd=root, env={k: v for k, v in os.environ.items() if k != "WORLD_SIZE"})
    assert out.returncode != 0 and "--gpus 2" in out.stderr and not [l for l in out.stdout.splitlines() if l.startswith("{")]
