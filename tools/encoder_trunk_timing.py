"""Times the front half of get_z's encoder on its two routes for profiles/encoder_trunk.md: the ResNetV2 trunk plus the token assembly alone
and the whole get_z, torch route against device route (MultiViewDPTEncoder.trunk_route; car_trunk_forward and car_vit_tokens), in the same
process on the same GPU, in alternation; the torch route once more with pre-standardised weights substituted (how much of its time is the
per-forward weight standardisation of StdConv2dSame — a substitution made inside this tool only); then the device route's stage entries at
one layer of each kind, and the two packs.  Random weights: the arithmetic does not depend on the values.

    python tools/encoder_trunk_timing.py [--windows 5] [--reps 50] [--entry-reps 2000] [--shapes 1x2,1x3,8x2]
    rocprofv3 --kernel-trace --stats -d DIR/trace -o trunk -- python tools/encoder_trunk_timing.py --trace-front 20
        (a run of its own: only the device route's front half at b = 1, V = 2, N times; tools/summarize_prof.py DIR prints the kernels' table)

A window is `reps` calls between one pair of HIP events (a quarter as many for the large shape), after a warm-up of every shape and route:
0.15 to 0.5 s for the front half and get_z, and `entry-reps` calls, 10 to 300 ms, for a stage entry; a figure is the per-call time of a
window, reported as min .. max over the windows (median in brackets).  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from cross_attention_renderer_amd import _lib  # noqa: E402
from cross_attention_renderer_amd import encoder as E  # noqa: E402
from cross_attention_renderer_amd.models import CrossAttentionRenderer  # noqa: E402


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, windows, reps):
    """{name: [per-call ms of each window]}, the candidates taking turns window by window."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in fns}
    for _ in range(windows):
        for n, fn in fns.items():
            out[n].append(window(fn, reps))
    return out


def show(ms):
    return f"{min(ms):8.3f} .. {max(ms):8.3f} ms (median {statistics.median(ms):8.3f})"


def context(b, V, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    rgb = (torch.rand(b, V, 256, 256, 3, generator=g) * 2 - 1).to(dev)
    c2w = torch.eye(4).repeat(b, V, 1, 1)
    c2w[:, :, 0, 3] = 0.1 * torch.arange(V, dtype=torch.float32)[None, :]
    return {"context": {"rgb": rgb, "cam2world": c2w.to(dev)}}


class prestandardised:
    """Inside the block, StdConv2dSame.forward convolves with a weight standardised once (kept per module) instead of on every call."""

    def __enter__(self):
        self.saved, cache = E.StdConv2dSame.forward, {}

        def forward(conv, x):
            if conv.dynamic_pad:
                x = E._same_pad(x, conv.kernel_size[0], conv.stride[0])
            if conv not in cache:
                w = conv.weight.reshape(conv.out_channels, -1)
                var, mean = torch.var_mean(w, dim=1, unbiased=False, keepdim=True)
                cache[conv] = ((w - mean) * torch.rsqrt(var + conv.eps)).reshape_as(conv.weight)
            return F.conv2d(x, cache[conv], None, conv.stride, conv.padding)
        E.StdConv2dSame.forward = forward

    def __exit__(self, *exc):
        E.StdConv2dSame.forward = self.saved


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--entry-reps", type=int, default=2000, help="calls per window of one stage entry (5 to 150 us a call)")
    p.add_argument("--shapes", type=str, default="1x2,1x3,8x2", help="comma-separated b x V")
    p.add_argument("--trace-front", type=int, default=0, metavar="N",
                   help="run only the device route's trunk and token assembly at b = 1, V = 2, N times after a warm-up, and exit (for a kernel trace)")
    opt = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_trunk_timing needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = E.MultiViewDPTEncoder().eval()
    with torch.no_grad():
        for q in enc.parameters():
            q.add_(0.02 * torch.randn_like(q))
    enc = enc.to(dev)
    vit = enc.pretrained.model
    lib, st = _lib.api(), _lib.stream()
    print(f"device: {torch.cuda.get_device_name(0)}, {lib.car_device_cu_count()} CUs; windows {opt.windows}, reps {opt.reps}")

    def front_torch(x, pose16):
        BV = x.shape[0]
        layer_1, layer_2, feat = vit.patch_embed.backbone(x)
        tok = vit.patch_embed.proj(feat).flatten(2).transpose(1, 2)
        tok = torch.cat((vit.cls_token.expand(BV, -1, -1), tok), dim=1)
        return layer_1, layer_2, (tok + vit.resized_pos_embed(16, 16) + vit.pose_embed(pose16)[:, None, :]).contiguous()

    if opt.trace_front:
        x, pose16 = torch.randn(2, 3, 256, 256, device=dev), torch.randn(2, 16, device=dev)
        with torch.no_grad():
            for _ in range(3 + opt.trace_front):
                enc._front_on_device(x, pose16, 16, 16)
        torch.cuda.synchronize()
        print(f"ran the device route's front half {3 + opt.trace_front} times (3 of them warm-up, the packs in the first)")
        return

    for shape in opt.shapes.split(","):
        b, V = (int(v) for v in shape.split("x"))
        BV, reps = b * V, max(opt.reps // (4 if b * V > 4 else 1), 2)
        model = CrossAttentionRenderer(model="midas_vit", n_view=V, encoder=enc).eval().to(dev)
        inp = context(b, V, dev)
        x, pose16 = torch.randn(BV, 3, 256, 256, device=dev), torch.randn(BV, 16, device=dev)
        print(f"\n== b = {b}, V = {V}: {BV} images of 256 x 256, {reps} calls per window ==")

        def getz(route):
            def run():
                model.encoder_route = route
                return model.get_z(inp)
            return run
        with torch.no_grad():
            res = alternate({"front  torch ": lambda: front_torch(x, pose16), "front  device": lambda: enc._front_on_device(x, pose16, 16, 16)},
                            opt.windows, reps)
            with prestandardised():
                res.update(alternate({"front  torch, weights standardised once": lambda: front_torch(x, pose16)}, opt.windows, reps))
            res.update(alternate({"get_z  torch ": getz("torch"), "get_z  device (blocks only)": getz("device"), "get_z  device_trunk": getz("device_trunk")},
                                 opt.windows, reps))
            model.encoder_route = "torch"
        for n, ms in res.items():
            print(f"{n}: {show(ms)}")
        med = {n: statistics.median(ms) for n, ms in res.items()}
        verdict = lambda d, t: f"{d / t:.3f}  ({'device route faster' if d < t else 'DEVICE ROUTE SLOWER'})"
        print(f"front  device / torch = {verdict(med['front  device'], med['front  torch '])}")
        print(f"get_z  device_trunk / torch = {verdict(med['get_z  device_trunk'], med['get_z  torch '])}")
        print(f"get_z  device_trunk / device (blocks only) = {med['get_z  device_trunk'] / med['get_z  device (blocks only)']:.3f}")
        once = med["front  torch, weights standardised once"]
        print(f"the torch route's per-forward weight standardisation: {med['front  torch '] - once:.3f} ms of {med['front  torch ']:.3f} ms "
              f"({100 * (1 - once / med['front  torch ']):.1f} %)")

        # the device route's entries at one layer of each kind (stage 3's repeated block is 8 of the trunk's 16 blocks)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        gnw = torch.empty(1 << 20, device=dev)
        g1 = torch.ones(1024, device=dev)

        def gn(HW, C, add=None):
            t = torch.randn(BV * HW, C, device=dev)
            nb = lib.car_groupnorm_workspace_bytes(BV, HW, C, 32)
            return lambda: lib.car_groupnorm(P(t), BV, HW, C, 32, P(g1), P(g1), 1e-5, None if add is None else P(add), 1, P(t), P(gnw), nb, st)

        def lin(rows, K, N):
            w, xin, y = torch.randn(N, K, device=dev), torch.randn(rows, K, device=dev), torch.empty(rows, N, device=dev)
            pk = torch.zeros(lib.car_linear_x3_packed_floats(K, N), device=dev)
            lib.car_linear_x3_pack(P(w), K, K, N, P(pk), st)
            return lambda: lib.car_linear_x3(P(xin), K, P(pk), None, K, N, P(y), N, rows, 0, st)

        def conv(H, C, stride):
            w, xin = torch.randn(C, C, 3, 3, device=dev), torch.randn(BV * H * H, C, device=dev)
            y = torch.empty(BV * (H // stride) ** 2, C, device=dev)
            pk = torch.zeros(lib.car_conv3x3_same_packed_floats(C, C), device=dev)
            lib.car_conv3x3_same_pack(P(w), C, C, P(pk), st)
            return lambda: lib.car_conv3x3_same(P(xin), BV, H, H, C, C, stride, P(pk), P(y), st)
        img, stem_w, stem_y = torch.randn(BV, 3, 256, 256, device=dev), torch.randn(64, 147, device=dev), torch.empty(BV * 128 * 128, 64, device=dev)
        pool_y, res3 = torch.empty(BV * 64 * 64, 64, device=dev), torch.randn(BV * 256, 1024, device=dev)
        entries = {
            "car_stem7x7 256 x 256                      ": lambda: lib.car_stem7x7(P(img), BV, 256, 256, P(stem_w), P(stem_y), st),
            "car_groupnorm stem (16384 px, C 64)        ": gn(128 * 128, 64),
            "car_maxpool3x3s2_same 128 x 128, C 64      ": lambda: lib.car_maxpool3x3s2_same(P(stem_y), BV, 128, 128, 64, P(pool_y), st),
            "car_linear_x3 stage 1 conv1 (256 -> 64)    ": lin(BV * 4096, 256, 64),
            "car_conv3x3_same stage 1 (64, 64 x 64)     ": conv(64, 64, 1),
            "car_linear_x3 stage 1 conv3 (64 -> 256)    ": lin(BV * 4096, 64, 256),
            "car_groupnorm stage 1 out (4096 px, C 256) ": gn(4096, 256),
            "car_conv3x3_same stage 2 (128, 32 x 32)    ": conv(32, 128, 1),
            "car_conv3x3_same stage 3 first (256, s 2)  ": conv(32, 256, 2),
            "car_linear_x3 stage 3 conv1 (1024 -> 256)  ": lin(BV * 256, 1024, 256),
            "car_groupnorm stage 3 mid (256 px, C 256)  ": gn(256, 256),
            "car_conv3x3_same stage 3 (256, 16 x 16)    ": conv(16, 256, 1),
            "car_linear_x3 stage 3 conv3 (256 -> 1024)  ": lin(BV * 256, 256, 1024),
            "car_groupnorm stage 3 out (256 px, C 1024) ": gn(256, 1024, res3),
            "car_linear_x3 token projection (1024->768) ": lin(BV * 256, 1024, 768),
        }
        for n, ms in alternate(entries, opt.windows, opt.entry_reps).items():
            print(f"  {n}: {show(ms)}")

    # the packs: 156 + 6 tensors -> two arrays
    depths = (ctypes.c_int * 3)(*enc.TRUNK_DEPTHS)
    params = enc._trunk_parameters()
    src = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
    packed = torch.empty(lib.car_trunk_packed_floats(depths), device=dev)
    ms = alternate({"pack": lambda: lib.car_trunk_pack(src, len(params), depths, ctypes.c_void_p(packed.data_ptr()), st)}, opt.windows, 5)["pack"]
    print(f"\ncar_trunk_pack, depths (3, 4, 9) ({packed.numel() * 4 / 1e6:.0f} MB packed): {show(ms)}")
    t = [q.detach().contiguous() for q in enc._token_parameters()]
    tp = torch.empty(lib.car_vit_tokens_packed_floats(16, 16), device=dev)
    ms = alternate({"pack": lambda: lib.car_vit_tokens_pack(*[ctypes.c_void_p(q.data_ptr()) for q in t[:4]], 24, ctypes.c_void_p(t[4].data_ptr()),
                                                             ctypes.c_void_p(t[5].data_ptr()), 16, 16, ctypes.c_void_p(tp.data_ptr()), st)}, opt.windows, 5)["pack"]
    print(f"car_vit_tokens_pack, 16 x 16 ({tp.numel() * 4 / 1e6:.1f} MB packed): {show(ms)}")


if __name__ == "__main__":
    main()
