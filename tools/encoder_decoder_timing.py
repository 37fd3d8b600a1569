"""Times the back half of get_z's encoder on its two routes for profiles/encoder_decoder.md: the read-out through path_1 plus conv_map alone
and the whole get_z, torch route against device route (MultiViewDPTEncoder.decoder_route; car_decoder_forward, car_conv7x7_pad3), in the
same process on the same GPU, in alternation; then the device route's stage entries at one layer of each kind, and the pack.  The only
yardsticks are the torch route and "device_trunk" of the same commit on the same box.  Random weights: the arithmetic does not depend on
the values.

    python tools/encoder_decoder_timing.py [--windows 5] [--reps 50] [--entry-reps 1000] [--shapes 1x2,1x3,8x2]
    rocprofv3 --kernel-trace --stats -d DIR/trace -o decoder -- python tools/encoder_decoder_timing.py --trace-back 20
        (a run of its own: only the device route's back half at b = 1, V = 2, N times; tools/summarize_prof.py DIR prints the kernels' table)

A window is `reps` calls between one pair of HIP events (a quarter as many for the large shape), after a warm-up of every shape and route;
a figure is the per-call time of a window, reported as min .. max over the windows (median in brackets).  Needs a GPU: there is no CPU
fallback."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

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


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--entry-reps", type=int, default=1000, help="calls per window of one stage entry")
    p.add_argument("--shapes", type=str, default="1x2,1x3,8x2", help="comma-separated b x V")
    p.add_argument("--trace-back", type=int, default=0, metavar="N",
                   help="run only the device route's back half (car_decoder_forward, car_conv7x7_pad3) at b = 1, V = 2, N times after a warm-up, and exit")
    opt = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_decoder_timing needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = E.MultiViewDPTEncoder().eval()
    with torch.no_grad():
        for q in enc.parameters():
            q.add_(0.02 * torch.randn_like(q))
    enc = enc.to(dev)
    pre, s = enc.pretrained, enc.scratch
    lib, st = _lib.api(), _lib.stream()
    print(f"device: {torch.cuda.get_device_name(0)}, {lib.car_device_cu_count()} CUs; windows {opt.windows}, reps {opt.reps}")

    def back_torch(model, tap3, tap4, layer_1, layer_2, x):
        def reassemble(t, post):
            t = post[0](t).transpose(1, 2).unflatten(2, (16, 16))
            for layer in post[3:]:
                t = layer(t)
            return t
        layer_3, layer_4 = reassemble(tap3, pre.act_postprocess3), reassemble(tap4, pre.act_postprocess4)
        path_4 = s.refinenet4(s.layer4_rn(layer_4))
        path_3 = s.refinenet3(path_4, s.layer3_rn(layer_3))
        path_2 = s.refinenet2(path_3, s.layer2_rn(layer_2))
        return path_2, s.refinenet1(path_2, s.layer1_rn(layer_1)), model.conv_map(x)

    def back_device(model, tap3, tap4, layer_1, layer_2, x):
        return (*enc._back_on_device(tap3, tap4, layer_1, layer_2, x, 16, 16), model._conv_map_on_device(x))

    def inputs(BV):
        tap = lambda: torch.randn(BV, 257, 768, device=dev)
        cl = lambda c, h: torch.relu(torch.randn(BV, h, h, c, device=dev)).permute(0, 3, 1, 2)       # as trunk_route = 'device' hands them over
        return tap(), tap(), cl(256, 64), cl(512, 32), torch.randn(BV, 3, 256, 256, device=dev)

    if opt.trace_back:
        model = CrossAttentionRenderer(model="midas_vit", n_view=2, encoder=enc).eval().to(dev)
        args = inputs(2)
        with torch.no_grad():
            for _ in range(3 + opt.trace_back):
                back_device(model, *args)
        torch.cuda.synchronize()
        print(f"ran the device route's back half {3 + opt.trace_back} times (3 of them warm-up, the pack in the first)")
        return

    for shape in opt.shapes.split(","):
        b, V = (int(v) for v in shape.split("x"))
        BV, reps = b * V, max(opt.reps // (4 if b * V > 4 else 1), 2)
        model = CrossAttentionRenderer(model="midas_vit", n_view=V, encoder=enc).eval().to(dev)
        inp, args = context(b, V, dev), inputs(BV)
        nchw = (args[0], args[1], args[2].contiguous(), args[3].contiguous(), args[4])                   # as the torch trunk hands them over
        print(f"\n== b = {b}, V = {V}: {BV} images of 256 x 256, {reps} calls per window ==")

        def getz(route):
            def run():
                model.encoder_route = route
                return model.get_z(inp)
            return run
        with torch.no_grad():
            res = alternate({"back   torch ": lambda: back_torch(model, *nchw), "back   device": lambda: back_device(model, *args)}, opt.windows, reps)
            res.update(alternate({"get_z  torch ": getz("torch"), "get_z  device_trunk": getz("device_trunk"), "get_z  device_full": getz("device_full")},
                                 opt.windows, reps))
            model.encoder_route = "torch"
        for n, ms in res.items():
            print(f"{n}: {show(ms)}")
        med = {n: statistics.median(ms) for n, ms in res.items()}
        verdict = lambda d, t: f"{d / t:.3f}  ({'device route faster' if d < t else 'DEVICE ROUTE SLOWER'})"
        print(f"back   device / torch = {verdict(med['back   device'], med['back   torch '])}")
        print(f"get_z  device_full / torch = {verdict(med['get_z  device_full'], med['get_z  torch '])}")
        print(f"get_z  device_full / device_trunk = {verdict(med['get_z  device_full'], med['get_z  device_trunk'])}")

        # the device route's entries at one layer of each kind
        P = lambda t: ctypes.c_void_p(t.data_ptr())

        def conv(H, K, N, stride=1, flags=0, residual=False):
            w, xin, bias = torch.randn(N, K, 3, 3, device=dev) / (9 * K) ** 0.5, torch.randn(BV * H * H, K, device=dev), torch.randn(N, device=dev)
            y = torch.zeros(BV * (H // stride) ** 2, N, device=dev)
            add = torch.randn_like(y) if residual else None
            pk = torch.zeros(lib.car_conv3x3_pad1_packed_floats(K, N), device=dev)
            lib.car_conv3x3_pad1_pack(P(w), K, N, P(pk), st)
            return lambda: lib.car_conv3x3_pad1(P(xin), BV, H, H, K, N, stride, P(pk), P(bias), None if add is None else P(add), flags, P(y), st)

        def lin(rows, K, N):
            w, xin, y, bias = torch.randn(N, K, device=dev), torch.randn(rows, K, device=dev), torch.empty(rows, N, device=dev), torch.randn(N, device=dev)
            pk = torch.zeros(lib.car_linear_x3_packed_floats(K, N), device=dev)
            lib.car_linear_x3_pack(P(w), K, K, N, P(pk), st)
            return lambda: lib.car_linear_x3(P(xin), K, P(pk), P(bias), K, N, P(y), N, rows, 0, st)

        def up(H):
            xin, y = torch.randn(BV * H * H, 256, device=dev), torch.empty(BV * 4 * H * H, 256, device=dev)
            return lambda: lib.car_upsample2x_bilinear(P(xin), BV, H, H, 256, P(y), st)
        ro_w, ro_b, tok = torch.randn(768, 1536, device=dev) / 40, torch.randn(768, device=dev), torch.randn(BV, 257, 768, device=dev)
        ro_pk = torch.zeros(lib.car_readout_packed_floats(768), device=dev)
        lib.car_readout_pack(P(ro_w), P(ro_b), 768, P(ro_pk), st)
        ro_work, ro_y = torch.empty(lib.car_readout_workspace_bytes(BV, 256, 768) // 4, device=dev), torch.empty(BV * 256, 768, device=dev)
        img, map_w, map_b, map_y = torch.randn(BV, 3, 256, 256, device=dev), torch.randn(64, 147, device=dev), torch.randn(64, device=dev), torch.empty(BV * 65536, 64, device=dev)
        rgb, norm_y = torch.rand(BV, 256, 256, 3, device=dev), torch.empty(BV, 3, 256, 256, device=dev)
        R = 1                                                            # CAR_LIN_RELU_IN
        entries = {
            "car_readout (256 patches, 768)                  ": lambda: lib.car_readout(P(tok), BV, 256, 768, P(ro_pk), P(ro_y), P(ro_work), ro_work.numel() * 4, st),
            "car_linear_x3 act_postprocess[3] (768 -> 768)   ": lin(BV * 256, 768, 768),
            "car_conv3x3_pad1 act_postprocess4[4] (768, s 2) ": conv(16, 768, 768, stride=2),
            "car_conv3x3_pad1 layer4_rn (768 -> 256, 8 x 8)  ": conv(8, 768, 256),
            "car_conv3x3_pad1 layer3_rn (768 -> 256, 16 x 16)": conv(16, 768, 256),
            "car_conv3x3_pad1 layer2_rn (512 -> 256, 32 x 32)": conv(32, 512, 256),
            "car_conv3x3_pad1 layer1_rn (256 -> 256, 64 x 64)": conv(64, 256, 256),
            "car_conv3x3_pad1 RCU refinenet4 (256, 8 x 8)    ": conv(8, 256, 256, flags=R, residual=True),
            "car_conv3x3_pad1 RCU refinenet3 (256, 16 x 16)  ": conv(16, 256, 256, flags=R, residual=True),
            "car_conv3x3_pad1 RCU refinenet2 (256, 32 x 32)  ": conv(32, 256, 256, flags=R, residual=True),
            "car_conv3x3_pad1 RCU refinenet1 (256, 64 x 64)  ": conv(64, 256, 256, flags=R, residual=True),
            "car_upsample2x_bilinear 64 x 64 -> 128 x 128    ": up(64),
            "car_linear_x3 out_conv refinenet1 (128 x 128)   ": lin(BV * 16384, 256, 256),
            "car_conv7x7_pad3 256 x 256                      ": lambda: lib.car_conv7x7_pad3(P(img), BV, 256, 256, P(map_w), P(map_b), P(map_y), st),
            "car_normalize_rgb 256 x 256                     ": lambda: lib.car_normalize_rgb(P(rgb), BV, 256, 256, P(norm_y), st),
        }
        for n, ms in alternate(entries, opt.windows, max(opt.entry_reps // (4 if BV > 4 else 1), 2)).items():
            print(f"  {n}: {show(ms)}")

    params = [q.detach().contiguous() for q in enc._decoder_parameters()]
    src = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
    packed = torch.empty(lib.car_decoder_packed_floats(), device=dev)
    ms = alternate({"pack": lambda: lib.car_decoder_pack(src, len(params), ctypes.c_void_p(packed.data_ptr()), st)}, opt.windows, 5)["pack"]
    print(f"\ncar_decoder_pack ({packed.numel() * 4 / 1e6:.0f} MB packed): {show(ms)}")


if __name__ == "__main__":
    main()
