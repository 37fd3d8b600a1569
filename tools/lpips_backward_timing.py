"""Times the LPIPS training loss (csrc/car_lpips.hip: car_lpips_forward_train, car_lpips_backward) — profiles/lpips_backward.md.

  1. Each data-gradient layer (car_conv3x3_backward, no act / add and with both) against car_conv3x3 at the SWAPPED shape and the same
     pixel count: the same kernel on the same amount of matrix work, the gradient reading up to two more maps in its epilogue.  Two
     settings: the 12 layers on one 256 x 256 image pair's prediction (n = 1 image) and on a training step's 12 patches of 32 x 32.
  2. The whole loss: car_lpips (forward, two scratch maps), car_lpips_forward_train (13 maps kept) and forward + backward with the
     gradient of the prediction only, as training asks for it, at 12 and 24 patches of 32 x 32 and at 1 and 8 pairs of 256 x 256.
  3. Information only: torch's own autograd of the same chain (F.conv2d / max_pool2d on MIOpen, float32) where it runs.
  4. The training step: experiment_scripts/train_realestate10k.py at 12 scenes x 1024 rays, each run a child process of its own, the
     routes alternating: without --lpips (the step as it was before the loss existed, at that ray count), with --depth (the same
     32 x 32 patch sampler, no LPIPS) and with --lpips on seeded weight files; the figure is the script's own steady-state line
     (wall clock per step after the first two, the last checkpoint write included), median and min .. max over CAR_TRAIN_RUNS runs.

Method: tools/lpips_timing.py's, imported from it (device events around a window of calls; every route is warmed up; the number of
calls per window is calibrated so that a window lasts CAR_WINDOW_S seconds, default 1.0; CAR_WINDOWS windows, default 3, of the routes
alternate in one process; the tables show the median and the spread, min .. max).  Prints one JSON line per row and markdown tables at
the end.
Usage (GPU box): python tools/lpips_backward_timing.py [--sections layers,whole,train] [--out FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cross_attention_renderer_amd import _lib, harness  # noqa: E402
from lpips_timing import alternate, seeded_weights, stream  # noqa: E402  (tools/: the measuring method and the seeded weights)

WIDTHS = harness.LPIPS_WIDTHS
POOL_BEFORE = (2, 4, 7, 10)
TAP_AFTER = (1, 3, 6, 9, 12)


def train_steps(conv_w, conv_b, lin, runs, steps):
    """[(name, median, min, max)] of the training script's steady-state ms per step; weight files in the layout of torchvision's VGG16
    and the lpips package's vgg.pth, seeded."""
    import re
    import subprocess
    import tempfile
    script = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")
    with tempfile.TemporaryDirectory() as tmp:
        vgg = {}
        for i, w, b in zip(harness.LPIPS_FEATURES, conv_w, conv_b):
            vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"] = w, b
        torch.save(vgg, os.path.join(tmp, "vgg16.pth"))
        torch.save({f"lin{k}.model.1.weight": w.reshape(1, -1, 1, 1) for k, w in enumerate(lin)}, os.path.join(tmp, "lin.pth"))
        base = [sys.executable, script, "--experiment_name", "t", "--views", "2", "--synthetic", "--batch_size", "12", "--query_sparsity", "1024",
                "--max_steps", str(steps), "--steps_til_summary", str(10 * steps), "--logging_root", tmp]
        routes = (("without --lpips", []), ("--depth (patch sampler, no LPIPS)", ["--depth"]),
                  ("--lpips", ["--lpips", "--lpips_weights", os.path.join(tmp, "vgg16.pth"), os.path.join(tmp, "lin.pth")]))
        times = [[] for _ in routes]
        for _ in range(runs):
            for i, (name, extra) in enumerate(routes):
                out = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:                                 # a failed run ends the section: nothing more is started
                    raise RuntimeError(f"{name}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
                ms = float(re.search(r"steady state: ([0-9.]+) ms per step", out.stdout).group(1))
                times[i].append(ms)
                print(json.dumps({"train": name, "ms_per_step": ms, "last_line": out.stdout.strip().splitlines()[-1]}), flush=True)
    return [(name, statistics.median(t), min(t), max(t)) for (name, _), t in zip(routes, times)]


def torch_chain(x, y, conv_w, conv_b, lin):
    """LPIPS in torch's own float32 ops, channel-first: the chain autograd differentiates (information only)."""
    shift = torch.tensor(harness.LPIPS_SHIFT, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(harness.LPIPS_SCALE, device=x.device).view(1, 3, 1, 1)
    h = (torch.cat([x, y]).permute(0, 3, 1, 2) - shift) / scale
    b, total, k = x.shape[0], 0.0, 0
    for l in range(13):
        if l in POOL_BEFORE:
            h = F.max_pool2d(h, 2, 2)
        h = F.relu(F.conv2d(h, conv_w[l], conv_b[l], padding=1))
        if l in TAP_AFTER:
            f0, f1 = h[:b], h[b:]
            n0, n1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
            d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)).pow(2)
            total = total + (lin[k].view(1, -1, 1, 1) * d).sum(1).mean(dim=(1, 2))
            k += 1
    return total


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    seconds = float(os.environ.get("CAR_WINDOW_S", "1.0"))
    windows = int(os.environ.get("CAR_WINDOWS", "3"))
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sections = (sys.argv[sys.argv.index("--sections") + 1] if "--sections" in sys.argv else "layers,whole,train").split(",")
    conv_w, conv_b, lin = seeded_weights("cpu")
    weights = harness.LpipsWeights(conv_w, conv_b, lin)
    dw, db, dl = ([t.to(dev) for t in group] for group in (conv_w, conv_b, lin))
    info = {"device": torch.cuda.get_device_name(0), "window_s": seconds, "windows": windows}
    print(json.dumps(info), flush=True)
    rows, g = [], torch.Generator().manual_seed(1)

    # 1. the data gradient of layer l (K -> N forward) against the forward kernel at N -> K, same images and side
    for n, side0, what in ((1, 256, "one 256 x 256 image"), (12, 32, "12 patches of 32 x 32")) if "layers" in sections else ():
        side = side0
        for l in range(1, 13):
            if l in POOL_BEFORE:
                side //= 2
            K, N = WIDTHS[l - 1], WIDTHS[l]
            d = (1e-6 * torch.randn(n, side, side, N, generator=g)).to(dev)
            act = torch.randn(n, side, side, K, generator=g).clamp_min(0).to(dev)
            add = (1e-6 * torch.randn(n, side, side, K, generator=g)).to(dev)
            out = torch.empty(n, side, side, K, device=dev)
            pb = torch.empty(lib.car_conv3x3_backward_packed_floats(K, N), device=dev)
            _lib.check(lib.car_conv3x3_backward_pack(dw[l].data_ptr(), K, N, pb.data_ptr(), stream()), "car_conv3x3_backward_pack")
            wsw = dw[l].permute(1, 0, 2, 3).contiguous()                # any [K][N][3][3] weights: the forward kernel at the swapped shape
            pf = torch.empty(lib.car_conv3x3_packed_floats(N, K), device=dev)
            _lib.check(lib.car_conv3x3_pack(wsw.data_ptr(), db[l - 1].data_ptr(), N, K, pf.data_ptr(), stream()), "car_conv3x3_pack")
            xin = d.abs()

            def fwd():
                _lib.check(lib.car_conv3x3(xin.data_ptr(), n, side, side, N, K, pf.data_ptr(), out.data_ptr(), stream()), "car_conv3x3")

            def bwd_plain():
                _lib.check(lib.car_conv3x3_backward(d.data_ptr(), n, side, side, K, N, pb.data_ptr(), None, None, out.data_ptr(), stream()),
                           "car_conv3x3_backward")

            def bwd_full():
                _lib.check(lib.car_conv3x3_backward(d.data_ptr(), n, side, side, K, N, pb.data_ptr(), act.data_ptr(), add.data_ptr(), out.data_ptr(),
                                                    stream()), "car_conv3x3_backward")
            res = alternate([fwd, bwd_plain, bwd_full], seconds, windows)
            row = {"setting": what, "layer": l, "gradient": f"{N} -> {K} at {side} x {side}", "gmac": n * side * side * 9 * K * N / 1e9}
            for nm, (med, lo, hi) in zip(("car_conv3x3 swapped", "backward", "backward act+add"), res):
                row[nm] = {"us": med * 1e6, "min_us": lo * 1e6, "max_us": hi * 1e6}
            row["ratio_plain"], row["ratio_act_add"] = res[1][0] / res[0][0], res[2][0] / res[0][0]
            rows.append(row)
            print(json.dumps(row), flush=True)

    # 2. the whole loss; 3. torch's autograd of the chain
    whole = []
    for b, side in ((12, 32), (24, 32), (1, 256), (8, 256)) if "whole" in sections else ():
        x = (torch.rand(b, side, side, 3, generator=g) * 2 - 1).to(dev)
        y = (x + 0.1 * torch.randn(x.shape, generator=g).to(dev)).clamp(-1, 1)
        yg = y.clone().requires_grad_(True)
        x01, y01 = x * 0.5 + 0.5, y * 0.5 + 0.5

        def forward_only():
            harness.lpips(x01, y01, weights)

        def forward_train():
            with torch.no_grad():
                harness.lpips_loss(x, y, weights)

        def both():
            yg.grad = None
            harness.lpips_loss(x, yg, weights).mean().backward()
        routes, names = [forward_only, forward_train, both], ["car_lpips", "car_lpips_forward_train", "forward_train + backward (gy)"]
        try:
            def torch_both():
                yg.grad = None
                torch_chain(x, yg, dw, db, dl).mean().backward()
            torch_both()
            torch.cuda.synchronize()
            routes.append(torch_both)
            names.append("torch autograd (MIOpen, fp32)")
        except Exception as e:                                          # information only
            print(json.dumps({"torch": f"does not run: {type(e).__name__}: {e}"}), flush=True)
        res = alternate(routes, seconds, windows)
        row = {"pairs": b, "side": side}
        for nm, (med, lo, hi) in zip(names, res):
            row[nm] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3}
        whole.append(row)
        print(json.dumps(row), flush=True)

    lines = ["| setting | layer | gradient | G MAC | car_conv3x3, swapped shape us (min .. max) | data gradient us (min .. max) | ratio | with act + add us (min .. max) | ratio |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(k):
            return f"{r[k]['us']:.1f} ({r[k]['min_us']:.1f} .. {r[k]['max_us']:.1f})"
        lines.append(f"| {r['setting']} | {r['layer']} | {r['gradient']} | {r['gmac']:.3f} | {cell('car_conv3x3 swapped')} | {cell('backward')} | "
                     f"{r['ratio_plain']:.3f} | {cell('backward act+add')} | {r['ratio_act_add']:.3f} |")
    lines += ["", "| pairs | side | car_lpips ms | car_lpips_forward_train ms | forward_train + backward (gy) ms (min .. max) | torch autograd ms |", "|---|---|---|---|---|---|"]
    for r in whole:
        def cell(k):
            return f"{r[k]['ms']:.3f} ({r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f})" if k in r else "-"
        lines.append(f"| {r['pairs']} | {r['side']} | {cell('car_lpips')} | {cell('car_lpips_forward_train')} | {cell('forward_train + backward (gy)')} | "
                     f"{cell('torch autograd (MIOpen, fp32)')} |")
    if "train" in sections:
        torch.cuda.synchronize()
        steps = train_steps(conv_w, conv_b, lin, int(os.environ.get("CAR_TRAIN_RUNS", "3")), int(os.environ.get("CAR_TRAIN_STEPS", "60")))
        lines += ["", "| train_realestate10k.py, 12 scenes x 1024 rays | ms per step (min .. max) |", "|---|---|"]
        lines += [f"| {name} | {med:.1f} ({lo:.1f} .. {hi:.1f}) |" for name, med, lo, hi in steps]
    table = "\n".join(lines)
    print(table)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(info) + "\n" + "\n".join(json.dumps(r) for r in rows + whole) + "\n\n" + table + "\n")


if __name__ == "__main__":
    main()
