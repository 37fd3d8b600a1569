"""Times the relative-pose entries (csrc/car_pose.hip) at N = 1024 matches and H = 1000, 8192, 65536 hypotheses: car_essential_solve,
_score, _select and the one call car_essential_ransac, then the wall time of harness.estimate_pose and, up to 8192 hypotheses, of the
float64 numpy restatement the tests compare against (tests/pose_reference.py, which also supplies the seeded scene: 35 % inliers, 1 px
of noise).  The table of profiles/pose_estimate.md.

Method: device events around each call, 2 warm-up calls, then 10 timed ones; the median and the spread (min .. max) are printed.
Usage (GPU box): python tools/pose_timing.py"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pose_reference as P  # noqa: E402
from cross_attention_renderer_amd import _lib, harness  # noqa: E402

N = 1024
BUDGETS = (1000, 8192, 65536)
RESTATEMENT_UP_TO = 8192


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, reps=10, warmup=2):
    """(median, min, max) in ms of ``reps`` calls, each between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    lib = _lib.load()
    k0, k1, R, t, _ = P.scene(N, 7, noise=1.0, outliers=0.65)
    x0, x1, nt = P.normalise(k0, k1, P.K, P.K, 1.0)
    d0, d1 = torch.from_numpy(x0).cuda(), torch.from_numpy(x1).cuda()
    thresh = ctypes.c_double(nt)
    for H in BUDGETS:
        table = torch.from_numpy(harness.pose_sample_table(N, H, 0)).cuda()
        cand = torch.empty(H, 10, 9, dtype=torch.float64, device="cuda")
        nsol = torch.empty(H, dtype=torch.int32, device="cuda")
        counts = torch.empty(H, 10, dtype=torch.int32, device="cuda")
        hyp_best = torch.empty(H, dtype=torch.int32, device="cuda")
        E = torch.empty(9, dtype=torch.float64, device="cuda")
        best = torch.empty(3, dtype=torch.int32, device="cuda")
        inliers = torch.empty(N, dtype=torch.uint8, device="cuda")
        nbytes = lib.car_essential_workspace_bytes(N, H)
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def solve():
            return lib.car_essential_solve(d0.data_ptr(), d1.data_ptr(), N, table.data_ptr(), H, cand.data_ptr(), nsol.data_ptr(), stream())

        def score():
            return lib.car_essential_score(d0.data_ptr(), d1.data_ptr(), N, cand.data_ptr(), nsol.data_ptr(), H, thresh, counts.data_ptr(),
                                           hyp_best.data_ptr(), stream())

        def select():
            return lib.car_essential_select(d0.data_ptr(), d1.data_ptr(), N, cand.data_ptr(), nsol.data_ptr(), counts.data_ptr(), H, thresh,
                                            E.data_ptr(), best.data_ptr(), inliers.data_ptr(), stream())

        def ransac():
            return lib.car_essential_ransac(d0.data_ptr(), d1.data_ptr(), N, table.data_ptr(), H, thresh, E.data_ptr(), best.data_ptr(),
                                            inliers.data_ptr(), work.data_ptr(), nbytes, stream())

        for name, fn in (("solve", solve), ("score", score), ("select", select), ("ransac", ransac)):
            assert fn() == 0, lib.car_last_error()
            med, lo, hi = timed(fn)
            print(f"H={H:6d} {name:7s} median {med:8.3f} ms  min {lo:8.3f}  max {hi:8.3f}", flush=True)
        print(f"H={H:6d} best {best.cpu().tolist()}, mean candidates per hypothesis {nsol.float().mean().item():.2f}", flush=True)
        t0 = time.time()
        got = harness.estimate_pose(k0, k1, P.K, P.K, 1.0, hypotheses=H)
        wall = time.time() - t0
        print(f"H={H:6d} estimate_pose wall {wall * 1e3:.1f} ms (table, uploads, kernels, downloads, recoverPose): {int(got[2].sum())} inliers, "
              f"R {np.degrees(P.rot_angle(got[0], R)):.3f} deg and t {np.degrees(P.dir_angle(got[1], t)):.3f} deg from the true pose", flush=True)
        if H <= RESTATEMENT_UP_TO:
            t0 = time.time()
            ref = P.estimate(k0, k1, P.K, P.K, 1.0, hypotheses=H)
            print(f"H={H:6d} numpy restatement {time.time() - t0:.2f} s, best {ref[3]['best']}", flush=True)


if __name__ == "__main__":
    main()
