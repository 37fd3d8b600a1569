"""Times car_ssim (csrc/car_metrics.hip) through harness.ssim on 256 x 256 x 3 image pairs: one frame, as the eval loop calls it, and
a batch of 76 frames (one unposed trajectory).  torch.cuda.Event pairs around CAR_LOOP calls (default 20) after 5 warm-up calls;
prints the median of 7 such windows per size, in microseconds per call.
Usage (GPU box): python tools/bench_ssim.py"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cross_attention_renderer_amd import harness  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    loop = int(os.environ.get("CAR_LOOP", "20"))
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {}
    for b in (1, 76):
        x = torch.rand(b, 256, 256, 3, generator=g).to(dev)
        y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).clamp(0, 1)
        for _ in range(5):
            harness.ssim(x, y)
        torch.cuda.synchronize()
        times = []
        for _ in range(7):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(loop):
                out = harness.ssim(x, y)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / loop)
        res[f"batch_{b}_us"] = round(statistics.median(times), 2)
        res[f"batch_{b}_spread_us"] = [round(min(times), 2), round(max(times), 2)]
        res[f"batch_{b}_mean_ssim"] = out.mean().item()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
