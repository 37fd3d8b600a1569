"""Times the fused per-sample kernel (csrc/car_fused.hip) alone on one 8192-ray chunk of the bench frame (256x256x64), through the
product library's entries:
  0 car_fused_samples | 1 car_fused_samples_parts (the launch as the fp32 forward issues it, with the first round's partial sums)
  2 car_fused_samples_f16 (the opt-in fp16 precision, with the partial sums)
Variants 0 and 1 must agree bit for bit on e, logit, pt and g.  CAR_LOOP=n launches per variant (median over all but the first two);
power / occupancy probes: CAR_ZERO=w|l|wl runs over zero weights and / or a zero lattice, CAR_CU_MASK=n on n compute units.
Usage (GPU box): python tools/bench_fused.py [variants...]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from cross_attention_renderer_amd import _lib  # noqa: E402
from cross_attention_renderer_amd.engine import RenderEngine  # noqa: E402

P_ = ctypes.c_void_p
NAMES = {0: "car_fused_samples", 1: "car_fused_samples_parts", 2: "car_fused_samples_f16"}


def _up64(n):
    return (n + 63) & ~63


def main():
    lib = _lib.load()
    f16 = lib.car_fused_samples_f16                     # the engine reaches it through car_render_forward_f16 only: bound here (declared in csrc/car_common.h)
    f16.restype = ctypes.c_int
    f16.argtypes = _lib.SIGNATURES["car_fused_samples_parts"][1]
    lib.car_fused_blob16_floats.restype = ctypes.c_size_t
    dev = torch.device("cuda:0")
    model = bench.build_model(dev)
    eng = model._engine = RenderEngine(model)
    inp, z = bench.make_frame(0.5, dev)
    R = 8192
    uv = inp["query"]["uv"][:, :, 96 * 256: 96 * 256 + R].contiguous()
    chunk = {"context": inp["context"], "query": dict(inp["query"], uv=uv)}
    with torch.no_grad():
        model(chunk, z=z)                              # plan, projected maps, workspace (and the rays of this chunk inside it)
    poses = eng._pose.value
    if poses is None:                                  # cameras on the GPU: the engine made the records with car_pose_setup
        from cross_attention_renderer_amd.poses import pack_poses
        poses = pack_poses({k: {kk: vv.cpu() for kk, vv in v.items()} for k, v in chunk.items()}, bench.H).to(dev)
    torch.cuda.synchronize()
    d = eng._dims(1, R, z)
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()

    def ws_range(name):
        _lib.check(lib.car_workspace_find(ctypes.byref(d), name.encode(), ctypes.byref(off), ctypes.byref(cnt)), name)
        return off.value, cnt.value

    def ws(name):
        return eng._work.data_ptr() + 4 * ws_range(name)[0]
    # the fused layers, packed once more into buffers of our own (the plan's offsets are private)
    keep = []

    def dptr(t):
        t = t.detach().float().reshape(t.shape[0], -1).contiguous() if t.dim() > 1 else t.detach().float().contiguous()
        keep.append(t)
        return t.data_ptr()
    w = _lib.CarWeights()
    sd = dict(model.named_parameters())
    for n in _lib.WEIGHT_FIELDS[0]:
        setattr(w, f"{n.replace('.', '_')}_w", dptr(sd[n + ".weight"]))
        setattr(w, f"{n.replace('.', '_')}_b", dptr(sd[n + ".bias"]))
    blob = torch.empty(lib.car_fused_blob_floats(), device=dev)
    bias = torch.empty(lib.car_fused_bias_floats(), device=dev)
    wpt = torch.empty(576 * 4, device=dev)
    st = P_(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.car_fused_pack(ctypes.byref(w), blob.data_ptr(), bias.data_ptr(), wpt.data_ptr(), st), "car_fused_pack")
    # the fp16 precision's plan (car_plan_f16_build): compact blob | bias table | point table, each rounded up to 64 floats (car_render.hip plan16_layout)
    plan16 = eng._plan16_for(d, dev)
    o_bias16 = _up64(lib.car_fused_blob16_floats())
    o_wpt16 = o_bias16 + _up64(lib.car_fused_bias_floats())
    assert o_wpt16 + _up64(576 * 4) == plan16.numel(), "car_plan_f16_build's layout changed"
    lh, lw, lpad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.car_lattice_shape(ctypes.byref(d), ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(lpad)), "car_lattice_shape")
    gmeta = eng._pair.data_ptr() + 4 * lib.car_gmeta_offset(ctypes.byref(d))
    steps = eng._linspace(0.0, 1.0, bench.P, dev)
    pixel_val = torch.empty(2 * R * bench.P * 2, device=dev)
    S = 2 * R * bench.P
    flop = 2.0 * S * bench.FUSED_MACS
    variants = [int(v) for v in sys.argv[1:]] or sorted(NAMES)
    if os.environ.get("CAR_ZERO"):                       # power probe: the same instruction stream over zeros (weights and / or lattice)
        if "w" in os.environ["CAR_ZERO"]:
            blob.zero_()
            plan16[:o_bias16].zero_()
        if "l" in os.environ["CAR_ZERO"]:
            eng._pair.zero_()
        torch.cuda.synchronize()
    outs = {}
    # power / occupancy probe: CAR_CU_MASK=n runs the launches on a stream restricted to n compute units (every (256 / n)-th one),
    # CAR_R=rays shrinks the launch with it
    Rk = int(os.environ.get("CAR_R", R))
    ext = None
    if os.environ.get("CAR_CU_MASK"):
        ncu = int(os.environ["CAR_CU_MASK"])
        hip = ctypes.CDLL("libamdhip64.so")
        words = (ctypes.c_uint32 * 8)()
        mode = os.environ.get("CAR_CU_MODE", "stride")
        for i in range(ncu):
            c = i * (256 // ncu) if mode == "stride" else i
            words[c // 32] |= 1 << (c % 32)
        hs = ctypes.c_void_p()
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(hs), 8, words)
        assert rc == 0, rc
        ext = torch.cuda.ExternalStream(hs.value)
        st = P_(hs.value)
        flop = flop * Rk / R
        print(f"stream restricted to {ncu} CUs ({mode}), {Rk} rays per launch")
    for v in variants:
        if v not in NAMES:
            raise SystemExit(f"unknown variant {v}: one of {NAMES}")
        p16 = v == 2
        args = (poses.data_ptr(), ws("rays"), steps.data_ptr(), eng._pair.data_ptr(), lh.value, lw.value, lpad.value, gmeta,
                plan16.data_ptr() + 4 * o_wpt16 if p16 else wpt.data_ptr(), plan16.data_ptr() if p16 else blob.data_ptr(),
                plan16.data_ptr() + 4 * o_bias16 if p16 else bias.data_ptr(), 1, 2, Rk, bench.P, bench.H, bench.H, 0,
                ws("e"), ws("g"), ws("logit"), ws("pt"), pixel_val.data_ptr())
        lat = []
        for it in range(int(os.environ.get("CAR_LOOP", 7))):
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ext) if ext is not None else a.record()
            if v == 0:
                rc = lib.car_fused_samples(*args, st)
            elif v == 1:
                rc = lib.car_fused_samples_parts(*args, ws("part"), st)
            else:
                rc = f16(*args, ws("part"), st)
            b_.record(ext) if ext is not None else b_.record()
            assert rc == 0, lib.car_last_error()
            lat.append((a, b_))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b_) for a, b_ in lat[2:])
        if v in (0, 1):                                  # with and without the partial sums: the same outputs, bit for bit
            outs[v] = [eng._work[o_:o_ + n_].clone() for o_, n_ in map(ws_range, ("e", "logit", "pt", "g"))]
            if v == 1 and 0 in outs:
                for n_, x, y in zip(("e", "logit", "pt", "g"), outs[1], outs[0]):
                    print(f"   (1) vs (0) {n_:6s} max |diff| {(x - y).abs().max().item():.3e}  max |ref| {y.abs().max().item():.3e}  equal {torch.equal(x, y)}")
        print(f"{v} {NAMES[v]}: fused kernel median {ms[len(ms) // 2]:.3f} ms  min {ms[0]:.3f} ms  -> {flop / ms[len(ms) // 2] / 1e9:.1f} TFLOP/s "
              "(nominal flops)", flush=True)


if __name__ == "__main__":
    main()
