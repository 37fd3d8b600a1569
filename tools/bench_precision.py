"""fp32 against the opt-in fp16 render precision (``CrossAttentionRenderer.render_precision``), in one process.

    python tools/bench_precision.py [--config c2 c4 c5] [--steps 20] [--warmup 5] [--power]

Per configuration (bench.py's frames: a camera trajectory between the two context views, one whole query frame per step): the two
precisions' frames alternate (the order flips every step, so neither gets a warmer or cooler clock), each timed with HIP events around
its forward; then a few frames per precision with the engine's stage events on (``engine.stage_times()``), the errors of the fp16 frame
against the fp32 one, and with ``--power`` socket power / shader clock sampled over an fp32-only and an fp16-only loop.  Prints one JSON
line per configuration."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402

PRECISIONS = ("fp32", "fp16")


def _render(model, frame, z, precision):
    model.render_precision = precision
    with torch.no_grad():
        return model(frame, z=z)


def _errors(a, b):
    d = (a["rgb"].double() - b["rgb"].double())
    mse = torch.mean(d * d).item()
    return {"rgb_max_abs": d.abs().max().item(), "rgb_psnr_db": float("inf") if mse == 0 else -10.0 * math.log10(mse),
            "depth_ray_max_abs": (a["depth_ray"] - b["depth_ray"]).abs().max().item(),
            "at_wt_max_abs": (a["at_wt"] - b["at_wt"]).abs().max().item(),
            "at_wt_max_agreement": (a["at_wt_max"] == b["at_wt_max"]).double().mean().item(),
            "exact": {k: bool(torch.equal(a[k], b[k])) for k in ("valid_mask", "coords", "pixel_val")}}


def run_config(name, steps, warmup, power, dev):
    Hc, Pc, nb, R, what = bench.CONFIGS[name]
    if nb != 1:
        raise SystemExit(f"{name}: one scene per step only (c2, c4, c5)")
    bench.H, bench.P = Hc, Pc
    bench.SCENE = "unposed" if name == "c5" else "stereo"
    from cross_attention_renderer_amd import synthetic as S
    model = bench.build_model(dev)
    frames = bench.trajectory(steps + warmup + 1, dev, cameras_on_host=True)
    z = [t.to(dev) for t in S.feature_maps(1, bench.V, Hc, seed=1)]
    ref = {k: v for k, v in _render(model, frames[0], z, "fp32").items() if isinstance(v, torch.Tensor)}
    got = {k: v for k, v in _render(model, frames[0], z, "fp16").items() if isinstance(v, torch.Tensor)}
    eng = model._engine
    assert eng.last_precision == "fp16" and eng.last_calls == 1
    errors = _errors(got, ref)
    del got, ref
    for i in range(warmup):
        for prec in PRECISIONS:
            _render(model, frames[1 + i], z, prec)
    torch.cuda.synchronize()
    ms = {p: [] for p in PRECISIONS}
    for i in range(steps):
        order = PRECISIONS if i % 2 == 0 else PRECISIONS[::-1]
        for prec in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _render(model, frames[1 + warmup + i], z, prec)
            e1.record()
            e1.synchronize()
            ms[prec].append(e0.elapsed_time(e1))
    stages = {}
    for prec in PRECISIONS:
        eng.profile(True)
        eng.stage_times()
        k = max(3, steps // 4)
        acc = {}
        for i in range(k):
            _render(model, frames[1 + warmup + i], z, prec)
            for st, t in eng.stage_times():
                acc[st] = acc.get(st, 0.0) + t
        eng.profile(False)
        stages[prec] = {st: round(t / k, 4) for st, t in acc.items()}
    pw = {}
    if power:
        from power_sampler import PowerSampler
        for prec in PRECISIONS:
            torch.cuda.synchronize()
            with PowerSampler(interval=0.005, skip=0.05) as ps:
                for i in range(steps):
                    _render(model, frames[1 + warmup + i], z, prec)
                torch.cuda.synchronize()
            pw[prec] = ps.summary()
    med = {p: sorted(v)[len(v) // 2] for p, v in ms.items()}
    fused = {p: stages[p].get("fused_samples") for p in PRECISIONS}
    return {"config": name, "what": what, "rays": R, "steps": steps, "warmup": warmup,
            "ms_per_frame": {p: round(med[p], 3) for p in PRECISIONS}, "ms_per_frame_min": {p: round(min(ms[p]), 3) for p in PRECISIONS},
            "rays_per_s": {p: round(R / (med[p] * 1e-3)) for p in PRECISIONS},
            "frame_ratio_fp16_over_fp32": round(med["fp16"] / med["fp32"], 4),
            "fused_ratio_fp16_over_fp32": round(fused["fp16"] / fused["fp32"], 4) if fused["fp16"] and fused["fp32"] else None,
            "stage_ms": stages, "errors_fp16_vs_fp32": errors, "power": pw or None,
            "device": torch.cuda.get_device_name(dev)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", nargs="+", default=["c2"], choices=["c2", "c4", "c5"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--power", action="store_true", help="sample socket power / shader clock over an fp32-only and an fp16-only loop")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda:0")
    for name in args.config:
        print(json.dumps(run_config(name, args.steps, args.warmup, args.power, dev)), flush=True)


if __name__ == "__main__":
    main()
