"""Times get_z's transformer stage on its two routes for profiles/encoder_vit.md: the 12 blocks alone and the whole get_z, torch route
against device route (encoder_route; car_vit_blocks), in the same process on the same GPU, in alternation; then the device route's split
per stage entry, car_vit_pack, and car_mha against its own operation count at the split-fp16 roof.  Random weights: the arithmetic does
not depend on the values.

    python tools/encoder_vit_timing.py [--windows 5] [--reps 10] [--shapes 1x2,1x3,8x2]
    python tools/encoder_vit_timing.py --backward [--shapes 1x2,12x2,12x3] [--train-steps 12]
        (for profiles/encoder_vit_backward.md: forward + backward of the stage and of the whole get_z, torch autograd against
        encoder_route = "device_train"; the backward's split per entry; car_vit_pack_train; and the training step of
        experiment_scripts/train_realestate10k.py on synthetic scenes with the encoder, 12 scenes x 192 rays, under both routes)
    rocprofv3 --kernel-trace --stats -d DIR/trace -o vit -- python tools/encoder_vit_timing.py --trace-stage 20
        (a run of its own: only the device route's stage at b = 1, V = 2, N times; tools/summarize_prof.py DIR prints the kernels' table)

A window is `reps` calls between one pair of HIP events (fewer for the large shape), after a warm-up of every shape and route; a figure is
the per-call time of a window, reported as min .. max over the windows (median in brackets).  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from cross_attention_renderer_amd import _lib  # noqa: E402
from cross_attention_renderer_amd.encoder import MultiViewDPTEncoder  # noqa: E402
from cross_attention_renderer_amd.models import CrossAttentionRenderer  # noqa: E402

ROOF_TFLOPS = 2500.0 / 3.0            # three fp16 products per term on the 2500 TFLOP/s f16 matrix pipe (README)


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


def backward_mode(opt, enc, dev):
    """Forward + backward: the stage and get_z on the torch route and on "device_train", the backward entry by entry, the train pack, and the
    training script's step under both routes."""
    import subprocess
    vit, T, dim = enc.pretrained.model, enc.TOKENS_PER_VIEW, 768
    lib, st = _lib.api(), _lib.stream()
    params = enc._vit_parameters()
    for shape in opt.shapes.split(","):
        b, V = (int(v) for v in shape.split("x"))
        S, M, heads = V * T, b * V * T, dim // 64
        reps = max(opt.reps // (5 if b * V > 4 else 1), 2)
        need = lib.car_vit_saved_bytes(b, S, dim, 12) + 4 * lib.car_vit_packed_train_floats(dim, 12) + lib.car_vit_backward_workspace_bytes(b, S, dim)
        free = torch.cuda.mem_get_info()[0]
        print(f"\n== b = {b}, V = {V}: {b} sequence(s) of {S} tokens, {reps} calls per window; the recorded stage holds {need / 1e9:.2f} GB "
              f"(saved {lib.car_vit_saved_bytes(b, S, dim, 12) / 1e9:.2f}), {free / 1e9:.0f} GB free ==")
        if need * 2 > free:
            print("   skipped: memory does not allow it")
            continue
        model = CrossAttentionRenderer(model="midas_vit", n_view=V, encoder=enc).eval().to(dev)
        inp = context(b, V, dev)
        tok0 = torch.randn(b, S, dim, device=dev)
        w = [torch.randn(b * V, T, dim, device=dev) for _ in enc.VIT_TAPS]

        def finish(taps):
            for q in enc.parameters():
                q.grad = None
            sum((t * c).sum() for t, c in zip(taps, w)).backward()

        def stage_torch():
            tok, taps = tok0.clone().requires_grad_(True), []
            for i, blk in enumerate(vit.blocks):
                tok = blk(tok)
                if i in enc.VIT_TAPS:
                    taps.append(tok.reshape(b * V, T, -1))
            finish(taps)

        def stage_device():
            enc.vit_route = "device_train"
            taps = enc._blocks_recorded_on_device(tok0.clone().requires_grad_(True), b * V, T)
            enc.vit_route = "torch"
            finish([taps[i] for i in enc.VIT_TAPS])

        def getz(route):
            def run():
                model.encoder_route = route
                z = model.get_z(inp)
                model.encoder_route = "torch"
                for q in model.parameters():
                    q.grad = None
                sum(t.sum() for t in z).backward()
            return run
        res = alternate({"stage  fwd+bwd torch       ": stage_torch, "stage  fwd+bwd device_train": stage_device}, opt.windows, reps)
        res.update(alternate({"get_z  fwd+bwd torch       ": getz("torch"), "get_z  fwd+bwd device_train": getz("device_train")}, opt.windows, reps))
        for n, ms in res.items():
            print(f"{n}: {show(ms)}")
        for what in ("stage ", "get_z "):
            t, d = statistics.median(res[what + " fwd+bwd torch       "]), statistics.median(res[what + " fwd+bwd device_train"])
            print(f"{what} fwd+bwd device_train / torch = {d / t:.3f}  ({'device route faster' if d < t else 'DEVICE ROUTE SLOWER'})")

        # the backward entry by entry, at this shape (one block's worth; a stage is 12 of each)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        E = lambda *s: torch.randn(*s, device=dev)
        src = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
        packed = torch.empty(lib.car_vit_packed_train_floats(dim, 12), device=dev)
        lib.car_vit_pack_train(src, len(params), dim, 12, P(packed), st)
        off = [lib.car_vit_packed_offset(dim, i) for i in range(13)]
        tr = [lib.car_vit_packed_train_offset(dim, 12, i) for i in range(6)]
        at = lambda i: ctypes.c_void_p(packed.data_ptr() + 4 * off[i])
        att_ = lambda t: ctypes.c_void_p(packed.data_ptr() + 4 * (tr[5] + tr[t]))
        x, g, norm, small, att = E(M, dim), E(M, dim), E(M, dim), E(M, dim), torch.empty(M, dim, device=dev)
        qkv, u, wide, dwide = E(M, 3 * dim), E(M, 4 * dim), torch.empty(M, 4 * dim, device=dev), E(M, 4 * dim)
        stats = torch.empty(lib.car_mha_stats_floats(b, S, heads), device=dev)
        fb, bb, lb = lib.car_mha_workspace_bytes(b, S, heads), lib.car_mha_backward_workspace_bytes(b, S, heads), lib.car_layernorm_backward_workspace_bytes(M, dim)
        fw, bw, lw = torch.empty(fb // 4, device=dev), torch.empty(bb // 4, device=dev), torch.empty(lb // 4, device=dev)
        lib.car_mha_stats(P(qkv), 3 * dim, b, S, heads, P(att), dim, P(stats), P(fw), fb, st)
        go = [lib.car_vit_grad_offset(dim, i) for i in range(13)]
        dp = torch.zeros(go[12], device=dev)
        gp = lambda i: ctypes.c_void_p(dp.data_ptr() + 4 * go[i])
        d3, d4 = 3 * dim, 4 * dim
        entries = {
            "car_layernorm, recomputed (x2)   ": lambda: lib.car_layernorm(P(x), dim, at(6), at(7), dim, 1e-6, P(norm), dim, M, st),
            "copy u + car_gelu, recomputed    ": lambda: (wide.copy_(u), lib.car_gelu(P(wide), d4, M, d4, st)),
            "car_linear_wgrad fc2             ": lambda: lib.car_linear_wgrad(P(g), dim, P(wide), d4, M, dim, d4, 0, gp(10), d4, gp(11), st),
            "car_linear_x3 fc2^T (dX)         ": lambda: lib.car_linear_x3(P(g), dim, att_(3), None, dim, d4, P(dwide), d4, M, 0, st),
            "car_gelu_backward                ": lambda: lib.car_gelu_backward(P(u), d4, P(dwide), d4, M, d4, st),
            "car_linear_wgrad fc1             ": lambda: lib.car_linear_wgrad(P(dwide), d4, P(norm), dim, M, d4, dim, 0, gp(8), dim, gp(9), st),
            "car_linear_x3 fc1^T (dX)         ": lambda: lib.car_linear_x3(P(dwide), d4, att_(2), None, d4, dim, P(small), dim, M, 0, st),
            "car_layernorm_backward (x2)      ": lambda: lib.car_layernorm_backward(P(x), dim, at(6), dim, 1e-6, P(small), dim, P(g), dim, M, 4, gp(6), gp(7), P(lw), lb, st),
            "car_linear_wgrad proj            ": lambda: lib.car_linear_wgrad(P(g), dim, P(att), dim, M, dim, dim, 0, gp(4), dim, gp(5), st),
            "car_linear_x3 proj^T (dX)        ": lambda: lib.car_linear_x3(P(g), dim, att_(1), None, dim, dim, P(small), dim, M, 0, st),
            "car_mha_backward (5 launches)    ": lambda: lib.car_mha_backward(P(qkv), d3, P(stats), P(att), dim, P(small), dim, b, S, heads, P(dwide), d3, P(bw), bb, st),
            "car_linear_wgrad qkv             ": lambda: lib.car_linear_wgrad(P(dwide), d3, P(norm), dim, M, d3, dim, 0, gp(2), dim, gp(3), st),
            "car_linear_x3 qkv^T (dX)         ": lambda: lib.car_linear_x3(P(dwide), d3, att_(0), None, d3, dim, P(small), dim, M, 0, st),
        }
        split = alternate(entries, opt.windows, 10)
        total = 0.0
        for n, ms in split.items():
            med = statistics.median(ms)
            total += med * (2 if "x2" in n else 1)
            print(f"  {n}: {show(ms)}")
        print(f"  one block's backward by its entries: {total:.3f} ms; x 12 = {12 * total:.3f} ms")
        mha = statistics.median(split["car_mha_backward (5 launches)    "])
        macs = 7.0 * b * heads * S * S * 64                                # s and dp in both kernels, dq, dk, dv
        roof_ms = 2.0 * macs / (ROOF_TFLOPS * 1e12) * 1e3
        print(f"  car_mha_backward: {macs / 1e9:.3f} GMAC (7 products: the logits and dp are formed in both kernels), {roof_ms:.4f} ms at the split-fp16 "
              f"roof -> {100 * roof_ms / mha:.2f} % of the roof")
        del packed, x, g, norm, small, att, qkv, u, wide, dwide, bw, model
        torch.cuda.empty_cache()

    src = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
    packed = torch.empty(lib.car_vit_packed_train_floats(dim, 12), device=dev)
    ms = alternate({"pack": lambda: lib.car_vit_pack_train(src, len(params), dim, 12, ctypes.c_void_p(packed.data_ptr()), st)}, opt.windows, 5)["pack"]
    print(f"\ncar_vit_pack_train, 12 blocks ({packed.numel() * 4 / 1e6:.0f} MB packed; once per recorded forward): {show(ms)}")
    del packed
    torch.cuda.empty_cache()

    if opt.train_steps:
        print(f"\n== experiment_scripts/train_realestate10k.py, synthetic scenes with the encoder, 12 scenes x 192 rays, {opt.train_steps} steps per run ==")
        import tempfile
        for rnd in range(2):
            for route in ("torch", "device_train"):
                with tempfile.TemporaryDirectory() as tmp:
                    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py"), "--experiment_name", "t", "--views", "2",
                           "--img_sidelength", "256", "--batch_size", "12", "--query_sparsity", "192", "--with_encoder", "--encoder_route", route,
                           "--max_steps", str(opt.train_steps), "--steps_til_summary", str(10 ** 6), "--logging_root", tmp]
                    out = subprocess.run(cmd, capture_output=True, text=True)
                    line = [l for l in out.stdout.splitlines() if l.startswith("steady state")]
                    print(f"  run {rnd} {route:12s}: {line[0] if line else 'FAILED: ' + out.stderr[-400:]}")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--shapes", type=str, default=None, help="comma-separated b x V (default 1x2,1x3,8x2; with --backward 1x2,12x2,12x3)")
    p.add_argument("--backward", action="store_true", help="time forward + backward (encoder_route = 'device_train' against torch autograd)")
    p.add_argument("--train-steps", type=int, default=12, metavar="N", help="--backward: steps per run of the training script (0: skip it)")
    p.add_argument("--trace-stage", type=int, default=0, metavar="N",
                   help="run only the device route's 12 blocks at b = 1, V = 2, N times after a warm-up, and exit (for a kernel trace)")
    opt = p.parse_args()
    opt.shapes = opt.shapes or ("1x2,12x2,12x3" if opt.backward else "1x2,1x3,8x2")
    if not torch.cuda.is_available():
        raise SystemExit("encoder_vit_timing needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = MultiViewDPTEncoder().eval()
    with torch.no_grad():
        for q in enc.parameters():
            q.add_(0.02 * torch.randn_like(q))
    enc = enc.to(dev)
    vit, T, dim = enc.pretrained.model, enc.TOKENS_PER_VIEW, 768
    lib, st = _lib.api(), _lib.stream()
    print(f"device: {torch.cuda.get_device_name(0)}, {lib.car_device_cu_count()} CUs; windows {opt.windows}, reps {opt.reps}")

    if opt.backward:
        return backward_mode(opt, enc, dev)

    if opt.trace_stage:
        tok0 = torch.randn(1, 2 * T, dim, device=dev)
        with torch.no_grad():
            for _ in range(3 + opt.trace_stage):
                enc._blocks_on_device(tok0.clone(), tok0, 2, T)
        torch.cuda.synchronize()
        print(f"ran the device route's stage {3 + opt.trace_stage} times (3 of them warm-up, the pack in the first)")
        return

    for shape in opt.shapes.split(","):
        b, V = (int(v) for v in shape.split("x"))
        S, reps = V * T, max(opt.reps // (4 if b * V > 4 else 1), 2)
        model = CrossAttentionRenderer(model="midas_vit", n_view=V, encoder=enc).eval().to(dev)
        inp = context(b, V, dev)
        tok0 = torch.randn(b, S, dim, device=dev)
        print(f"\n== b = {b}, V = {V}: {b} sequence(s) of {S} tokens, {reps} calls per window ==")

        def stage_torch():
            tok, taps = tok0, []
            for i, blk in enumerate(vit.blocks):
                tok = blk(tok)
                if i in enc.VIT_TAPS:
                    taps.append(tok.reshape(b * V, T, -1))
            return taps

        def stage_device():
            return enc._blocks_on_device(tok0.clone(), tok0, b * V, T)

        def getz(route):
            def run():
                model.encoder_route = route
                return model.get_z(inp)
            return run
        with torch.no_grad():
            res = alternate({"stage  torch ": stage_torch, "stage  device": stage_device}, opt.windows, reps)
            res.update(alternate({"get_z  torch ": getz("torch"), "get_z  device": getz("device")}, opt.windows, reps))
            model.encoder_route = "torch"
        for n, ms in res.items():
            print(f"{n}: {show(ms)}")
        for what in ("stage ", "get_z "):
            t, d = statistics.median(res[what + " torch "]), statistics.median(res[what + " device"])
            print(f"{what} device / torch = {d / t:.3f}  ({'device route faster' if d < t else 'DEVICE ROUTE SLOWER'})")

        # the device route entry by entry, at this shape (one block's worth; a stage is 12 of each)
        M, heads = b * S, dim // 64
        packed = enc._vit_packed.value
        off = [lib.car_vit_packed_offset(dim, i) for i in range(13)]
        at = lambda i: ctypes.c_void_p(packed.data_ptr() + 4 * off[i])
        norm, att, wide = torch.randn(M, dim, device=dev), torch.randn(M, dim, device=dev), torch.randn(M, 4 * dim, device=dev)
        tok = tok0.reshape(M, dim).clone()
        nbytes = lib.car_mha_workspace_bytes(b, S, heads)
        work = torch.empty(nbytes // 4, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        entries = {
            "car_layernorm (x2)       ": lambda: lib.car_layernorm(P(tok), dim, at(0), at(1), dim, 1e-6, P(norm), dim, M, st),
            "car_linear_x3 qkv        ": lambda: lib.car_linear_x3(P(norm), dim, at(2), at(3), dim, 3 * dim, P(wide), 3 * dim, M, 0, st),
            "car_mha (3 launches)     ": lambda: lib.car_mha(P(wide), 3 * dim, b, S, heads, P(att), dim, P(work), nbytes, st),
            "car_linear_x3 proj, accum": lambda: lib.car_linear_x3(P(att), dim, at(4), at(5), dim, dim, P(tok), dim, M, 4, st),
            "car_linear_x3 fc1        ": lambda: lib.car_linear_x3(P(norm), dim, at(8), at(9), dim, 4 * dim, P(wide), 4 * dim, M, 0, st),
            "car_gelu                 ": lambda: lib.car_gelu(P(wide), 4 * dim, M, 4 * dim, st),
            "car_linear_x3 fc2, accum ": lambda: lib.car_linear_x3(P(wide), 4 * dim, at(10), at(11), 4 * dim, dim, P(tok), dim, M, 4, st),
        }
        split = alternate(entries, opt.windows, 20)
        total = 0.0
        for n, ms in split.items():
            med = statistics.median(ms)
            total += med * (2 if "x2" in n else 1)
            print(f"  {n}: {show(ms)}")
        print(f"  one block by its entries: {total:.3f} ms; x 12 = {12 * total:.3f} ms")
        mha = statistics.median(split["car_mha (3 launches)     "])
        macs = 2.0 * b * heads * S * S * 64                                # q k^T and p v
        roof_ms = 2.0 * macs / (ROOF_TFLOPS * 1e12) * 1e3
        waves = b * heads * ((S + 31) // 32)
        print(f"  car_mha: {macs / 1e9:.3f} GMAC, {roof_ms:.4f} ms at the split-fp16 roof ({ROOF_TFLOPS:.0f} TFLOP/s) -> {100 * roof_ms / mha:.2f} % of the roof; "
              f"{waves} waves of 32 queries on {lib.car_device_cu_count()} CUs")

    # the pack: 144 tensors -> one array
    params = enc._vit_parameters()
    src = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
    packed = torch.empty(lib.car_vit_packed_floats(dim, 12), device=dev)
    ms = alternate({"pack": lambda: lib.car_vit_pack(src, len(params), dim, 12, ctypes.c_void_p(packed.data_ptr()), st)}, opt.windows, 5)["pack"]
    print(f"\ncar_vit_pack, 12 blocks ({packed.numel() * 4 / 1e6:.0f} MB packed): {show(ms)}")


if __name__ == "__main__":
    main()
