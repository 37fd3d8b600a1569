"""A/B of the second attention round: one launch (car_attend_round2, engine.second_round_merged = True) against the two launches it
replaces (car_round2_logits_from_g + car_attend, CAR_PHASE_SPLIT_SECOND_ROUND), in ONE process on one device.

The model, the frames and a step are bench.py's own (its builders are imported); the two forms alternate, split first, for `--rounds`
rounds of `--steps` timed steps each, every round with the stage events of the C ABI on.  Printed: per round the ms per step and the tail's
stage times, then per form the median with min and max, and the verdict by the rule the change was accepted under: the forms' per-round
ranges must not overlap and the medians must differ by at least three times the split form's own max - min.

    python tools/ab_second_round.py [--config c2|c3|c4|c5] [--rounds 4] [--steps 20] [--warmup 3] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TAIL = ("attend_1", "ray_layers_1", "round2_logits", "attend_2", "ray_layers_2")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(bench.CONFIGS), default="c2")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the result there")
    args = ap.parse_args()
    if args.rounds < 4 or args.steps < 1:
        sys.exit("ab_second_round.py: at least four rounds of at least one step")
    if not torch.cuda.is_available():
        sys.exit("ab_second_round.py needs a ROCm device")
    from cross_attention_renderer_amd.engine import RenderEngine
    dev = torch.device("cuda", 0)
    Hc, Pc, nb, R, _ = bench.CONFIGS[args.config]
    if args.config == "c5":
        bench.SCENE = "unposed"
    model = bench.build_model(dev, Pc, Hc)
    model._engine = eng = RenderEngine(model)
    _, z = bench.make_frame(0.5, dev, Hc, nb)
    band = ((3 * Hc // 8) * Hc, (3 * Hc // 8) * Hc + R) if nb != 1 else None
    frames = bench.trajectory(args.steps + args.warmup, dev, band, True, Hc, nb)
    tile = torch.empty(nb, R, 5, device=dev)
    chunk = 1 << 30
    rows = {False: [], True: []}
    with torch.no_grad():
        bench.render_frame(model, frames[0], z, tile, chunk)                 # plan, lattice, workspace
        for rnd in range(args.rounds):
            for merged in (False, True):
                eng.second_round_merged = merged
                for i in range(args.warmup):
                    bench.render_frame(model, frames[args.steps + i], z, tile, chunk)
                eng.profile(True)
                sec = bench.timed_loop(model, frames, z, tile, None, args.steps, chunk, None)
                st = {}
                for name, ms in eng.stage_times():
                    st.setdefault(name, []).append(ms)
                eng.profile(False)
                st = {k: sum(v) / args.steps for k, v in st.items()}        # ms per step of every stage
                row = {"round": rnd, "merged": merged, "ms_per_step": sec / args.steps * 1e3, "stage_ms": st,
                       "second_round_ms": st.get("round2_logits", 0.0) + st["attend_2"]}
                rows[merged].append(row)
                print(f"round {rnd} {'merged' if merged else 'split ':6s}: {row['ms_per_step']:7.3f} ms/step   second round {row['second_round_ms']:6.3f} ms   "
                      + "  ".join(f"{k} {st[k]:.3f}" for k in TAIL if k in st) + f"   fused_samples {st.get('fused_samples', float('nan')):.3f}", flush=True)
    eng.second_round_merged = True
    res = {"config": args.config, "rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "rows": rows[False] + rows[True]}
    for key in ("ms_per_step", "second_round_ms"):
        s, m = spread([r[key] for r in rows[False]]), spread([r[key] for r in rows[True]])
        gain = s["median"] - m["median"]
        apart = m["max"] < s["min"]
        clear = apart and gain >= 3.0 * (s["max"] - s["min"])
        res[key] = {"split": s, "merged": m, "gain_ms": gain, "ranges_apart": apart, "clears_the_bar": clear}
        print(f"{key:16s} split {s['median']:.3f} [{s['min']:.3f}, {s['max']:.3f}]   merged {m['median']:.3f} [{m['min']:.3f}, {m['max']:.3f}]   "
              f"gain {gain:+.3f} ms   ranges apart: {apart}   >= 3 x split spread ({3.0 * (s['max'] - s['min']):.3f}): {clear}")
    split_logits = statistics.median([r["stage_ms"].get("round2_logits", 0.0) for r in rows[False]])
    split_attend = statistics.median([r["stage_ms"]["attend_2"] for r in rows[False]])
    print(f"bounds: the gain cannot exceed the split form's round2_logits ({split_logits:.3f} ms); a merged second round below the split "
          f"form's attend_2 alone ({split_attend:.3f} ms) would be a measurement error")
    res["split_round2_logits_ms"], res["split_attend_2_ms"] = split_logits, split_attend
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
