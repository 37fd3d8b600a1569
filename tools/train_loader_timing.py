"""Times the training input (dataio.TrainLoader, csrc/car_frames.hip) — profiles/train_loader.md.

At the reference's training shape, 12 scenes x (2 context + 1 query) frames per batch, every scene storing raw 360 x 640 frames:
  1. ms per batch of the host chain (the loader's host path: plan + resize / crop / flip / resize in numpy) with 1 and with N reader
     threads, and of the device path (plan + one upload + the two launches), each loader drained on its own with nothing consuming
     the batches but a final synchronisation;  the reader's share alone (np.load of three frames out of a compressed scene) is timed too,
     since that is what bounds the device path;
  2. the two kernels on one such batch's frames (device events around a window of launches, median of the windows);
  3. the training step at 12 x 192 rays: experiment_scripts/train_realestate10k.py as a child process per run, the routes alternating:
     on the loader, on one cached device batch replayed (--replay_batch: no data wait), and the synthetic step (with and without the
     encoder), the figure being the script's own steady-state line.  Loader minus replay is the data wait.
Prints one JSON line per figure and a markdown table at the end.
Usage (GPU box): python tools/train_loader_timing.py --data_root DIR --pose_root FILE.mat [--workers N] [--sections host,device,kernels,train] [--out FILE]
(CAR_TRAIN_STEPS, default 60, and CAR_TRAIN_RUNS, default 2, in the environment set the length and number of the runs of section 3;
the scenes: e.g. tests/train_scene.py's formula, written beforehand; enough of them for several batches per epoch, since a loader
prepares ahead within an epoch only)."""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cross_attention_renderer_amd import _lib, dataio  # noqa: E402

B, VIEWS, RAYS = 12, 2, 192


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def drain(loader, max_batches, sync):
    """ms per batch over one epoch of `loader` (at most `max_batches` of it), the first batch (thread start, allocations) left out."""
    n, t0 = 0, None
    for _batch in loader:
        if t0 is None:
            sync()
            t0 = time.perf_counter()
        else:
            n += 1
            if n == max_batches:
                break
    sync()
    return (time.perf_counter() - t0) / max(n, 1) * 1e3, n


def kernel_times(ds, dev, windows=5, calls=50):
    """(stage A us, stage B us) on the frames of one batch, laid out as the loader lays them out."""
    lib = _lib.load()
    plans = [ds.plan(i, dataio.PrivateStreams([0, i])) for i in range(B)]
    frames = [f for p in plans for f in p["frames"][:1]] + [f for p in plans for f in p["frames"][1:]]
    records = [r for p in plans for r in p["records"][:1]] + [r for p in plans for r in p["records"][1:]]
    pixels = [x for p in plans for x in p["pixels"]] + [None] * (len(frames) - B)
    offs, at = [], 0
    for f in frames:
        offs.append(at)
        at = dataio._align(at + f.nbytes)
    n_a = sum(r["resize360"] for r in records)
    upload, scratch = at, n_a * 256 * 256 * 3
    recs_a, recs_b, idx = dataio.stage_records([f.shape for f in frames], records, pixels, offs, upload)
    host = np.zeros(upload + scratch, np.uint8)
    for f, o in zip(frames, offs):
        host[o:o + f.nbytes] = f.reshape(-1)
    buf, tables = torch.from_numpy(host).to(dev), torch.from_numpy(dataio.frame_tables()).to(dev)
    ra, rb, ib = (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev) for a in (recs_a, recs_b, idx))
    n_out = int(recs_b["dst_off"][-1]) + 256 * 256 * 3
    out = torch.empty(n_out, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def stage_a():
        _lib.check(lib.car_frames_resize_u8(buf.data_ptr(), upload, recs_a.ctypes.data, ra.data_ptr(), n_a, tables.data_ptr(), buf.data_ptr() + upload, scratch, s))

    def stage_b():
        _lib.check(lib.car_frames_resize_f32(buf.data_ptr(), upload + scratch, recs_b.ctypes.data, rb.data_ptr(), len(frames), idx.ctypes.data, ib.data_ptr(),
                                             len(idx), tables.data_ptr(), out.data_ptr(), n_out, s))
    res = []
    for fn in (stage_a, stage_b):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / calls * 1e3)
        res.append((statistics.median(times), min(times), max(times)))
    return res, {"frames": len(frames), "raw": n_a, "upload_MB": upload / 1e6, "out_MB": n_out * 4 / 1e6}


def train_steps(data_root, pose_root, workers, runs, steps):
    script = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")
    with tempfile.TemporaryDirectory() as tmp:
        base = [sys.executable, script, "--experiment_name", "t", "--views", str(VIEWS), "--batch_size", str(B), "--query_sparsity", str(RAYS),
                "--max_steps", str(steps), "--steps_til_summary", str(10 * steps), "--logging_root", tmp]
        real = ["--data_root", data_root, "--pose_root", pose_root, "--num_workers", str(workers)]
        routes = (("reader + loader", real), ("one cached device batch replayed", real + ["--replay_batch"]),
                  ("synthetic, with the encoder", ["--synthetic", "--with_encoder"]), ("synthetic, pyramid as a leaf (the step as it was)", ["--synthetic"]))
        times = [[] for _ in routes]
        for _ in range(runs):
            for i, (name, extra) in enumerate(routes):
                out = subprocess.run(base + extra, capture_output=True, text=True, timeout=900)
                if out.returncode != 0:                                 # a failed run ends the section: nothing more is started
                    raise RuntimeError(f"{name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
                ms = float(re.search(r"steady state: ([0-9.]+) ms per step", out.stdout).group(1))
                times[i].append(ms)
                print(json.dumps({"train": name, "ms_per_step": ms}), flush=True)
    return [(name, statistics.median(t), min(t), max(t)) for (name, _), t in zip(routes, times)]


def main():
    data_root, pose_root = arg("--data_root"), arg("--pose_root")
    if not data_root or not pose_root:
        raise SystemExit(__doc__)
    workers = int(arg("--workers", "8"))
    sections = arg("--sections", "host,device,kernels,train").split(",")
    gpu = any(x in sections for x in ("device", "kernels", "train"))             # --sections host runs anywhere
    dev = torch.device("cuda:0") if gpu else None
    ds = dataio.RealEstate10k(data_root, pose_root, num_ctxt_views=VIEWS, num_query_views=1, query_sparsity=RAYS, augment=True)
    info = {"device": torch.cuda.get_device_name(0) if gpu else "none (host figures only)", "scenes": len(ds), "batch": B, "views": VIEWS, "rays": RAYS, "workers": workers}
    print(json.dumps(info), flush=True)
    lines = ["| 12 scenes x 3 raw 360 x 640 frames | ms per batch | batches timed |", "|---|---|---|"]
    if "host" in sections:
        t0 = time.perf_counter()
        for i in range(B):
            ds.plan(i, dataio.PrivateStreams([1, i]))
        plan_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"plans of one batch, one thread (np.load of 3 frames per scene + draws) ms": plan_ms}), flush=True)
        lines.append(f"| the plans alone, one thread (np.load of 3 frames per scene, draws, cameras) | {plan_ms:.1f} | 1 |")
    loaders = []
    if "host" in sections:
        loaders += [("host chain, 1 reader thread", dataio.TrainLoader(ds, B, seed=0, num_workers=1), lambda: None, 2),
                    (f"host chain, {workers} reader threads", dataio.TrainLoader(ds, B, seed=0, num_workers=workers), lambda: None, 6)]
    if "device" in sections:
        loaders += [("device path, 1 reader thread", dataio.TrainLoader(ds, B, seed=0, num_workers=1, device=dev), torch.cuda.synchronize, 6),
                    (f"device path, {workers} reader threads", dataio.TrainLoader(ds, B, seed=0, num_workers=workers, device=dev), torch.cuda.synchronize, 100)]
    if loaders:
        for name, loader, sync, most in loaders:
            ms, n = drain(loader, most, sync)
            print(json.dumps({"loader": name, "ms_per_batch": ms, "batches": n}), flush=True)
            lines.append(f"| {name} | {ms:.1f} | {n} |")
    if "kernels" in sections:
        (a, b), shape = kernel_times(ds, dev)
        print(json.dumps({"stage A us": a, "stage B us": b, **shape}), flush=True)
        lines += ["", f"| kernel ({shape['frames']} frames, {shape['raw']} raw; {shape['upload_MB']:.1f} MB uploaded, {shape['out_MB']:.1f} MB written) | us (min .. max) |", "|---|---|",
                  f"| stage A: 360 x 640 -> the 256 x 256 window, uint8 | {a[0]:.1f} ({a[1]:.1f} .. {a[2]:.1f}) |",
                  f"| stage B: flip, crop, 256 x 256, float32 | {b[0]:.1f} ({b[1]:.1f} .. {b[2]:.1f}) |"]
    if "train" in sections:
        torch.cuda.synchronize()
        steps = train_steps(data_root, pose_root, workers, int(os.environ.get("CAR_TRAIN_RUNS", "2")), int(os.environ.get("CAR_TRAIN_STEPS", "60")))
        lines += ["", "| train_realestate10k.py, 12 scenes x 192 rays | ms per step (min .. max) |", "|---|---|"]
        lines += [f"| {name} | {med:.1f} ({lo:.1f} .. {hi:.1f}) |" for name, med, lo, hi in steps]
    table = "\n".join(lines)
    print(table)
    if arg("--out"):
        with open(arg("--out"), "w") as fh:
            fh.write(json.dumps(info) + "\n\n" + table + "\n")


if __name__ == "__main__":
    main()
