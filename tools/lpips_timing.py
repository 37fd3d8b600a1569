"""Times car_lpips (csrc/car_lpips.hip) on 256 x 256 pairs — one pair, as the eval loop calls it, and a batch of 8 — and each of its 13
convolutions against the composition that exists without it: nine accumulating car_linear_x3 calls (CAR_LIN_ACCUM), one per tap, over a
zero-padded channel-last copy of the layer's input.

The composition works on the padded grid: every one of the (H + 2)(W + 2) padded positions is a row, tap (dy, dx) reads the rows
(dy (W + 2) + dx) further on, and the interior positions of the result are the convolution (the border positions are never read).  It
computes (H + 2)(W + 2) / (H W) as many rows as the one-sweep kernel; making the padded copy is NOT in its time.  The script checks the
composition against car_conv3x3 before it times anything.

Method: device events around a window of calls; every shape is warmed up first; the number of calls per window is calibrated so that
a window lasts CAR_WINDOW_S seconds (default 1.0); CAR_WINDOWS windows (default 3) of the two routes alternate in the same process,
and the table shows the median and the spread (min .. max) of each.  Share of the split-f16 roof: the larger of
2 x MAC / (2500 / 3 TFLOP/s) and bytes / (8 TB/s), over the measured time, with the bound that applies.  torch's own F.conv2d is a
third column where it runs.  Prints one JSON line per row and a markdown table at the end.
Usage (GPU box): python tools/lpips_timing.py [--out FILE]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cross_attention_renderer_amd import _lib, harness  # noqa: E402

WIDTHS = harness.LPIPS_WIDTHS
POOL_BEFORE = (2, 4, 7, 10)
MATRIX_ROOF = 2500e12 / 3          # split fp16: three f16 products per term
HBM_ROOF = 8.0e12
CAR_LIN_RELU_OUT, CAR_LIN_ACCUM = 2, 4


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def calibrate(fn, seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = window(fn, 5)
    return max(5, int(seconds / max(t, 1e-7)))


def alternate(fns, seconds, windows):
    """[(median, min, max) per route], the routes' windows alternating."""
    reps = [calibrate(f, seconds) for f in fns]
    times = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            times[i].append(window(f, reps[i]))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def seeded_weights(dev):
    g = torch.Generator().manual_seed(0)
    conv_w, conv_b, k = [], [], 3
    for n in WIDTHS:
        conv_w.append((torch.randn(n, k, 3, 3, generator=g) * (2.0 / (9 * k)) ** 0.5).to(dev))
        conv_b.append((0.01 * torch.randn(n, generator=g)).to(dev))
        k = n
    lin = [(torch.randn(c, generator=g).abs() / c).to(dev) for c in harness.LPIPS_TAP_WIDTHS]
    return conv_w, conv_b, lin


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    seconds = float(os.environ.get("CAR_WINDOW_S", "1.0"))
    windows = int(os.environ.get("CAR_WINDOWS", "3"))
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    conv_w, conv_b, lin = seeded_weights(dev)
    weights = harness.LpipsWeights([t.cpu() for t in conv_w], [t.cpu() for t in conv_b], [t.cpu() for t in lin])
    rows = []
    info = {"device": torch.cuda.get_device_name(0), "window_s": seconds, "windows": windows}
    try:
        import subprocess
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        info["sclk"] = [l.strip() for l in smi.splitlines() if "sclk" in l][:1]
    except Exception as e:                                              # the clock is information only
        info["sclk"] = f"not read: {e}"
    print(json.dumps(info), flush=True)

    g = torch.Generator().manual_seed(1)
    for pairs in (1, 8):
        n = 2 * pairs
        x = torch.rand(pairs, 256, 256, 3, generator=g).to(dev)
        y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).clamp(0, 1)
        (med, lo, hi), = alternate([lambda: harness.lpips(x, y, weights)], seconds, windows)
        rows.append({"what": f"car_lpips, {pairs} pair(s) of 256 x 256", "ms": med * 1e3, "spread_ms": [lo * 1e3, hi * 1e3],
                     "lpips": harness.lpips(x, y, weights)[0].item()})
        print(json.dumps(rows[-1]), flush=True)

        cur = ((torch.cat([x, y]) - 0.5) * 2).contiguous()
        pool_s = 0.0
        for l in range(13):
            if l in POOL_BEFORE:
                _, H, W, C = cur.shape
                nxt = torch.empty(n, H // 2, W // 2, C, device=dev)
                src = cur

                def run_pool():
                    _lib.check(lib.car_maxpool2x2(src.data_ptr(), n, H, W, C, nxt.data_ptr(), stream()), "car_maxpool2x2")
                (pm, _, _), = alternate([run_pool], seconds / 4, windows)
                pool_s += pm
                cur = nxt
            _, H, W, K = cur.shape
            N = WIDTHS[l]
            packed = torch.empty(lib.car_conv3x3_packed_floats(K, N), device=dev)
            _lib.check(lib.car_conv3x3_pack(conv_w[l].data_ptr(), conv_b[l].data_ptr(), K, N, packed.data_ptr(), stream()), "car_conv3x3_pack")
            out = torch.empty(n, H, W, N, device=dev)
            src = cur

            def run_conv():
                _lib.check(lib.car_conv3x3(src.data_ptr(), n, H, W, K, N, packed.data_ptr(), out.data_ptr(), stream()), "car_conv3x3")
            routes, names = [run_conv], ["conv3x3"]
            if K >= 64:
                # the composition: padded grid, one packed [N, K] matrix per tap
                Wp = W + 2
                margin = Wp + 1
                rows_p = n * (H + 2) * Wp
                big = torch.zeros(margin + rows_p + margin, K, device=dev)
                big[margin:margin + rows_p].view(n, H + 2, Wp, K)[:, 1:-1, 1:-1] = cur
                taps = []
                for t in range(9):
                    wt = conv_w[l][:, :, t // 3, t % 3].contiguous()
                    pk = torch.empty(lib.car_linear_x3_packed_floats(K, N), device=dev)
                    _lib.check(lib.car_linear_x3_pack(wt.data_ptr(), K, K, N, pk.data_ptr(), stream()), "car_linear_x3_pack")
                    taps.append(pk)
                yp = torch.empty(rows_p, N, device=dev)

                def run_composition():
                    for t in range(9):
                        off = (t // 3 - 1) * Wp + (t % 3 - 1)
                        flags = (CAR_LIN_ACCUM if t else 0) | (CAR_LIN_RELU_OUT if t == 8 else 0)
                        _lib.check(lib.car_linear_x3(big.data_ptr() + 4 * K * (margin + off), K, taps[t].data_ptr(),
                                                     conv_b[l].data_ptr() if t == 0 else None, K, N, yp.data_ptr(), N, rows_p, flags, stream()),
                                   "car_linear_x3")
                run_conv()
                run_composition()
                torch.cuda.synchronize()
                inner = yp.view(n, H + 2, Wp, N)[:, 1:-1, 1:-1]
                diff = ((inner - out).abs() / out.abs().clamp_min(1.0)).max().item()
                assert diff <= 1e-4, f"layer {l}: the composition and car_conv3x3 disagree by {diff:.3e}"
                routes.append(run_composition)
                names.append("nine car_linear_x3")
            try:
                xin = cur.permute(0, 3, 1, 2).contiguous()
                F.conv2d(xin, conv_w[l], conv_b[l], padding=1)
                torch.cuda.synchronize()
                routes.append(lambda: F.relu(F.conv2d(xin, conv_w[l], conv_b[l], padding=1)))
                names.append("torch conv2d + relu")
            except Exception as e:                                      # information only
                print(json.dumps({"layer": l, "torch": f"does not run: {type(e).__name__}"}), flush=True)
            res = alternate(routes, seconds, windows)
            mac = n * H * W * 9 * K * N
            bytes_ = 4 * n * H * W * (K + N) + 4 * 9 * K * N
            t_mat, t_hbm = 2 * mac / MATRIX_ROOF, bytes_ / HBM_ROOF
            row = {"pairs": pairs, "layer": l, "shape": f"{K} -> {N} at {H} x {W}", "gmac": mac / 1e9,
                   "bound": "matrix pipe" if t_mat >= t_hbm else "HBM", "roof_us": max(t_mat, t_hbm) * 1e6}
            for nm, (med, lo, hi) in zip(names, res):
                row[nm] = {"us": med * 1e6, "min_us": lo * 1e6, "max_us": hi * 1e6}
            row["share_of_roof"] = max(t_mat, t_hbm) / res[0][0]
            rows.append(row)
            print(json.dumps(row), flush=True)
            cur = out
        rows.append({"pairs": pairs, "what": "the four max-pool launches together", "us": pool_s * 1e6})
        print(json.dumps(rows[-1]), flush=True)

    lines = ["| pairs | layer | shape | G MAC | car_conv3x3 us (min .. max) | nine car_linear_x3 us (min .. max) | torch us | roof us (bound) | share |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "layer" not in r:
            continue

        def cell(k):
            return f"{r[k]['us']:.1f} ({r[k]['min_us']:.1f} .. {r[k]['max_us']:.1f})" if k in r else "-"
        lines.append(f"| {r['pairs']} | {r['layer']} | {r['shape']} | {r['gmac']:.3f} | {cell('conv3x3')} | {cell('nine car_linear_x3')} | "
                     f"{cell('torch conv2d + relu')} | {r['roof_us']:.1f} ({r['bound']}) | {100 * r['share_of_roof']:.1f} % |")
    table = "\n".join(lines)
    print(table)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(info) + "\n" + "\n".join(json.dumps(r) for r in rows) + "\n\n" + table + "\n")


if __name__ == "__main__":
    main()
