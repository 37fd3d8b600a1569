"""Times the matcher's two stages on the device for profiles/matcher.md: SuperPoint on two 256 x 256 images, SuperGlue at 1024 x 1024
keypoints with 18 layers and 20 Sinkhorn iterations (split per entry), and the same two stages as the float32 torch restatement
(tests/matcher_reference.py) on the same GPU.  Seeded random weights: the arithmetic does not depend on the values.

    python tools/matcher_timing.py [--reps 20]

Every figure is the median over `reps` of a HIP-event pair around the stage, after 3 warm-up runs."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import matcher_cases as C  # noqa: E402
import matcher_reference as R  # noqa: E402
from cross_attention_renderer_amd import _lib, matching as M  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=20)
    opt = p.parse_args()
    dev = torch.device("cuda:0")
    layers = ["self", "cross"] * 9
    sp, sg = C.superpoint_state(), C.superglue_state(layers=18)
    w = M.MatcherWeights(sp, sg, layers)
    g = torch.Generator().manual_seed(0)
    gray = torch.rand(2, 256, 256, generator=g).to(dev)
    print(f"superpoint, two 256 x 256 images (max_keypoints 1024): {timed(lambda: M.superpoint(gray, w), opt.reps):.3f} ms, the count read included")
    N = 1024
    k = (torch.rand(2, N, 2, generator=g) * 255).to(dev)
    s = torch.rand(2, N, generator=g).to(dev)
    d = torch.nn.functional.normalize(torch.randn(2, N, 256, generator=g), dim=-1).to(dev)
    print(f"superglue, 1024 x 1024 keypoints, 18 layers, 20 iterations: "
          f"{timed(lambda: M.superglue(k[0], s[0], d[0], k[1], s[1], d[1], (256, 256), w), opt.reps):.3f} ms")
    lib, st = _lib.api(), _lib.stream()
    packed = w.packed_glue(dev)
    sizes = [lib.car_superglue_workspace_bytes(N, N), lib.car_superglue_transport_workspace_bytes(N, N), lib.car_superglue_matches_workspace_bytes(N, N)]
    work = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
    mdesc = torch.empty(2 * N, 256, device=dev)
    Z = torch.empty(N + 1, N + 1, device=dev)
    cross = (ctypes.c_int * 18)(*[i % 2 for i in range(18)])
    m0, m1 = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    s0, s1 = torch.empty(N, device=dev), torch.empty(N, device=dev)
    qkv = torch.randn(2 * N, 768, generator=g).to(dev)
    att = torch.empty(N, 256, device=dev)
    parts = {
        "car_superglue_descriptors (18 layers, both images)": lambda: lib.car_superglue_descriptors(
            k[0].data_ptr(), s[0].data_ptr(), d[0].data_ptr(), N, 256, 256, k[1].data_ptr(), s[1].data_ptr(), d[1].data_ptr(), N, 256, 256, packed.data_ptr(), 18,
            cross, mdesc.data_ptr(), work.data_ptr(), sizes[0], st),
        "  of which one car_superglue_attention call (1024 x 1024; 36 per forward)": lambda: lib.car_superglue_attention(
            qkv.data_ptr(), 768, qkv.data_ptr() + 1024, 768, qkv.data_ptr() + 2048, 768, N, N, att.data_ptr(), 256, st),
        "car_superglue_transport (20 iterations: 42 launches)": lambda: lib.car_superglue_transport(
            mdesc.data_ptr(), N, mdesc[N:].data_ptr(), N, w.bin_score, 20, Z.data_ptr(), work.data_ptr(), sizes[1], st),
        "car_superglue_matches": lambda: lib.car_superglue_matches(Z.data_ptr(), N, N, 0.2, m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(),
                                                                  work.data_ptr(), sizes[2], st),
    }
    for name, fn in parts.items():
        print(f"{name}: {timed(fn, opt.reps):.3f} ms")
    # the float32 torch restatement on the same GPU
    spd = {k_: v.to(dev) for k_, v in sp.items()}
    sgd = {k_: v.to(dev) for k_, v in sg.items()}
    torch.set_default_device(dev)
    with torch.no_grad():
        print(f"torch restatement, superpoint dense + nms + select + sample, two images: "
              f"{timed(lambda: R.superpoint(spd, gray, 4, 0.005, 1024, 4, dtype=torch.float32), max(opt.reps // 4, 3)):.3f} ms")

        def glue_torch():
            (a, _), (b, _) = R.match_descriptors(sgd, layers, k[0], s[0], d[0], (256, 256), k[1], s[1], d[1], (256, 256), torch.float32)
            return R.matches(R.transport(a, b, C.BIN_SCORE, 20, torch.float32)[0], 0.2)
        print(f"torch restatement, superglue 1024 x 1024, 18 layers, 20 iterations: {timed(glue_torch, max(opt.reps // 4, 3)):.3f} ms (bounds included)")


if __name__ == "__main__":
    main()
