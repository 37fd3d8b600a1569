"""The stream contract of the C ABI and of the package, held to gated tests (tests/stream_gate.py, which tests/test_stream_gate.py holds to
its word first): "All work is enqueued asynchronously on `stream` ... No call synchronises the device" (include/car_hip.h).

ROWS: one case per entry that no other entry calls and whose launcher enqueues more than one operation, and one single-launch entry of every
other translation unit, each at the smallest shape of its existing "fits its workspace exactly" / parity case.  Behind a gate on a side stream
the row's real inputs replace a decoy, every output and workspace is poisoned and the entry is called; the row asserts that the step was
conclusive (the call returned while the gate was running: it synchronised nothing), that the result is bit-identical to the eager call on the
default stream, and that no guarded margin was written.  A launch, memset or copy the entry issues on another stream fails the row.

A CPU test reads `_lib`'s signature tables and the launchers in csrc/: every entry whose prototype ends in the stream is a row, is called by a
row's entry, or is an exception with its reason; what is left — single launches of units a row reaches — is named as not gated, its stream
argument read from the source.

Then the package under a side stream (PACKS: a spy on every C entry's stream argument, behind a gate), and the three hand-offs between
streams — RenderEngine.prefetch, dataio.TrainLoader, sharding.TileGather — with the gate on the PRODUCER's stream.
profiles/stream_order.md has the gate lengths, the exceptions and what the tests found."""
import ctypes
import functools
import os
import re

import pytest
import torch

import abi_harness as A
import stream_gate as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I32 = torch.float32, torch.float64, torch.int32


def lib():
    return A.lib()


def ok(rc, what=""):
    assert rc == 0, (what, lib().car_last_error())


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------------
def row_add():
    """car_backward.hip's single launch: out = alpha a + beta b, more than one block, odd sizes, padded rows."""
    M, N, LD = 257, 131, 136
    g, b = gen(11), SG.Built()
    a_, b_ = (b.inp(torch.randn(M, LD, generator=g), torch.randn(M, LD, generator=g)) for _ in range(2))
    out = b.out((M, N), ld=LD)
    b.call = lambda st: ok(lib().car_add(out.ptr, LD, A.ptr(a_), LD, 0.75, A.ptr(b_), LD, -1.5, M, N, st), "car_add")
    return b


@functools.lru_cache(maxsize=None)
def _render_setup(repeat_attention):
    """The one-call forward at the smallest sizes tests/test_hip_parity.py renders (two scenes of 16 rays x 8 samples, H = 64): the engine's own
    plan, poses, sample steps and projected pair for two seeds (real and decoy), each in a copy of its own."""
    import cases as C
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    from hip_harness import to_device
    dev = A.dev()
    H, P, R, b = 64, 8, 16, 2
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=P, repeat_attention=repeat_attention, with_encoder=False).eval()
    S.perturb_parameters(m, seed=4)
    m.H = m.W = H
    md = m.to(dev)
    sides = {}
    for side, (seed_s, seed_z, alpha) in {"decoy": (8, 5, 0.6), "real": (7, 2, 0.35)}.items():       # real last: the engine's caches end on it
        inp = to_device(S.stereo_scene(H, b=b, uv=C.select_rays(H, R), seed=seed_s, alpha=alpha), dev, cameras_on_host=True)
        dz = [t.to(dev) for t in S.feature_maps(b, 2, H, seed=seed_z)]
        with torch.no_grad():
            ref = md(inp, z=dz)
        eng = md._engine
        assert eng.last_calls == 1
        d = eng._dims(b, R, dz)
        plan = eng._plan_for(d, dev)
        pair, d_pair = eng._pair_for(plan, dz, dev, 0, b, R)
        uv = inp["query"]["uv"].reshape(b, R, 2).float().contiguous()
        if side == "decoy":
            uv = uv.flip(1).contiguous()                          # the same pixels, every ray another one
        sides[side] = dict(maps=[t.clone() for t in eng._channel_last(dz)], pair=pair.clone(), poses=eng._poses(inp, H, 2, dev).clone(), uv=uv.clone(), ref={k: v.clone() for k, v in ref.items() if torch.is_tensor(v)})
        torch.cuda.synchronize()
    steps = eng._linspace(0.0, 1.0, P, dev).clone()
    gmeta_off = 4 * lib().car_gmeta_offset(ctypes.byref(d_pair))
    return dict(md=md, eng=eng, d=d, d_pair=d_pair, plan=plan, steps=steps, gmeta_off=gmeta_off, sides=sides, shape=(H, P, R, b))


ORDER = ("rgb", "valid_mask", "depth_ray", "at_wt", "at_wt_max", "coords", "pixel_val")


def _render_built(repeat_attention, call_of):
    from cross_attention_renderer_amd import _lib
    s = _render_setup(repeat_attention)
    H, P, R, b = s["shape"]
    real, decoy = s["sides"]["real"], s["sides"]["decoy"]
    B = SG.Built()
    pair, poses, uv = (B.inp(real[k], decoy[k]) for k in ("pair", "poses", "uv"))
    steps = B.idx(s["steps"])                                       # the sample table: never decoyed
    o = {"rgb": B.out((b, 1, R, 3)), "valid_mask": B.out((b, R, 1)), "depth_ray": B.out((b, R, 1)), "at_wt": B.out((2 * b, R, P)),
         "at_wt_max": B.out((2 * b, R, 1), dtype=I32), "coords": B.out((2 * b, R, 9)), "pixel_val": B.out((2 * b, R, P, 2))}
    B.loose = (1,)                                                  # valid_mask: ones wherever a ray is valid, whatever the pair holds
    ci = _lib.CarInputs()
    ci.poses, ci.uv, ci.lattice, ci.steps = poses.data_ptr(), uv.data_ptr(), pair.data_ptr(), steps.data_ptr()
    ci.gmeta = pair.data_ptr() + s["gmeta_off"]
    co = _lib.CarOutputs(*[o[k].view.data_ptr() for k in ORDER])
    need = lib().car_workspace_bytes(ctypes.byref(s["d"]))
    work = B.work(need)
    B.keep += [ci, co, s]
    B.call = call_of(s, ci, co, work, need)
    return B, s


def _row_render_forward(repeat_attention):
    def call_of(s, ci, co, work, need):
        return lambda st: ok(lib().car_render_forward(ctypes.byref(s["d"]), A.ptr(s["plan"]), ctypes.byref(ci), ctypes.byref(co), work.ptr, need, st), "car_render_forward")
    B, s = _render_built(repeat_attention, call_of)
    return B


def row_render_forward():
    return _row_render_forward(True)


def row_render_forward_one_round():
    return _row_render_forward(False)


def row_render_forward_phases():
    """Phase 1 (per sample) and phase 2 (per ray) as two calls on the one stream over the one workspace."""
    def call_of(s, ci, co, work, need):
        def call(st):
            for phase in (1, 2):
                ok(lib().car_render_forward_phase(ctypes.byref(s["d"]), A.ptr(s["plan"]), ctypes.byref(ci), ctypes.byref(co), work.ptr, need, phase, st), f"phase {phase}")
        return call
    B, s = _render_built(True, call_of)
    return B


def row_project_maps():
    """The pyramid of the render rows -> their lattice buffer: the first layer per texel of each level, the merge on the common lattice with
    its maximum (gmeta) — several launches and the memset of the maximum."""
    from cross_attention_renderer_amd.engine import _levels
    s = _render_setup(True)
    real, decoy = s["sides"]["real"], s["sides"]["decoy"]
    B = SG.Built()
    maps = [B.inp(r, d_) for r, d_ in zip(real["maps"], decoy["maps"])]
    n = lib().car_gmaps_floats(ctypes.byref(s["d_pair"]))
    assert n == real["pair"].numel()
    pair = B.out((n,))
    ptrs = _levels(maps)[0]
    B.keep += [ptrs, s]
    B.call = lambda st: ok(lib().car_project_maps(ctypes.byref(s["d_pair"]), A.ptr(s["plan"]), ptrs, pair.ptr, st), "car_project_maps")
    return B


def _weights_as_inputs(B, w, seed):
    """The tensors a struct CarWeights points to become inputs: the decoy is the same layers moved by N(0, 0.05^2)."""
    g = gen(seed)
    for t in w.keep:
        real = t.clone()
        B.inputs.append((t, real, (real.cpu() + 0.05 * torch.randn(real.shape, generator=g)).to(t.device)))


def row_plan_f16_build():
    s = _render_setup(True)
    w = s["eng"]._car_weights(A.dev())                               # a struct of its own: the engine's cached one keeps the real weights
    B = SG.Built()
    _weights_as_inputs(B, w, 21)
    nbytes = lib().car_plan_f16_bytes(ctypes.byref(s["d"]))
    assert nbytes > 0 and nbytes % 4 == 0, lib().car_last_error()
    plan16 = B.out((nbytes // 4,))
    B.keep += [w, s]
    B.call = lambda st: ok(lib().car_plan_f16_build(ctypes.byref(s["d"]), ctypes.byref(w), plan16.ptr, st), "car_plan_f16_build")
    return B


def row_render_forward_f16():
    def call_of(s, ci, co, work, need):
        plan16 = s["eng"]._plan16_for(s["d"], A.dev())
        torch.cuda.synchronize()
        return lambda st: ok(lib().car_render_forward_f16(ctypes.byref(s["d"]), A.ptr(s["plan"]), A.ptr(plan16), ctypes.byref(ci), ctypes.byref(co), work.ptr, need, 3, st),
                             "car_render_forward_f16")
    B, s = _render_built(True, call_of)
    return B


def row_getz():
    """tests/test_decoder_hip.py's small get_z: a 32 x 32 pair, one block per trunk stage, two transformer blocks of the real width."""
    import test_decoder_hip as TD
    c = TD.GETZ
    trunk, toks, vit, dec, map_w, map_b = TD.getz_packs()
    rgb, pose = TD.getz_inputs()
    g = gen(31)
    B = SG.Built()
    R = B.inp(rgb, torch.rand(rgb.shape, generator=g) * 2 - 1)
    Po = B.inp(pose, 0.5 * torch.randn(pose.shape, generator=g))
    BV, H, W, P = c["BV"], c["H"], c["W"], c["gh"] * c["gw"]
    z = [B.out((BV, 16 * P, 256)), B.out((BV, 64 * P, 256)), B.out((BV, H * W, 64))]
    depths, taps = A.ints(c["depths"]), A.ints(c["taps"])
    nbytes = lib().car_getz_workspace_bytes(BV, H, W, c["gh"], c["gw"], c["nviews"], depths, c["vit_depth"])
    assert nbytes > 0, lib().car_last_error()
    work = B.work(nbytes)
    B.keep += [depths, taps]
    B.call = lambda st: ok(lib().car_getz(A.ptr(R), A.ptr(Po), BV, H, W, c["gh"], c["gw"], c["nviews"], depths, A.ptr(trunk), A.ptr(toks), A.ptr(vit), c["vit_depth"],
                                          taps, dec.ptr, A.ptr(map_w), A.ptr(map_b), 0, z[0].ptr, z[1].ptr, z[2].ptr, work.ptr, nbytes, st), "car_getz")
    return B


def row_ssim():
    """Two pairs of 13 x 21 x 3 (more than the 11-wide window by an odd amount on both axes): the two launches over the fp64 scratch."""
    Bn, H, W, C = 2, 13, 21, 3
    g, B = gen(5), SG.Built()
    x, y = (B.inp(torch.rand(Bn, H, W, C, generator=g), torch.rand(Bn, H, W, C, generator=g)) for _ in range(2))
    out = B.out((Bn,), dtype=F64)
    n = lib().car_ssim_scratch_doubles(Bn, H, W, C)
    work = B.work(8 * n)
    B.call = lambda st: ok(lib().car_ssim(A.ptr(x), A.ptr(y), Bn, H, W, C, 2.0, out.ptr, work.ptr, n, st), "car_ssim")
    return B


def row_attention_entropy():
    rows, S = 300, 37
    g, B = gen(6), SG.Built()
    w = B.inp(torch.softmax(torch.randn(rows, S, generator=g), -1), torch.softmax(2 * torch.randn(rows, S, generator=g), -1))
    out = B.out((1,), dtype=F64)
    n = lib().car_attention_entropy_scratch_doubles(rows, S)
    work = B.work(8 * n)
    B.call = lambda st: ok(lib().car_attention_entropy(A.ptr(w), rows, S, 1, out.ptr, work.ptr, n, st), "car_attention_entropy")
    return B


def row_image_grid():
    N, H, W = 15, 13, 15                                             # two rows of tiles, the second ragged; two thirds of the grid are tiles
    g, B = gen(7), SG.Built()
    x = B.inp(torch.randn(N, H, W, 3, generator=g), 2 * torch.randn(N, H, W, 3, generator=g) + 1)
    out = B.out((3, (H + 2) * 2 + 2, (W + 2) * 8 + 2))
    n = lib().car_image_grid_scratch_floats(N, H, W)
    assert n > 0, lib().car_last_error()
    work = B.work(4 * n)
    B.call = lambda st: ok(lib().car_image_grid(A.ptr(x), N, H, W, 1, 0, 0.0, 0.0, out.ptr, work.ptr, n, st), "car_image_grid")
    return B


def row_superpoint_nms():
    """Radius 0 keeps every pixel, so every entry of the output depends on the input; the five launches are issued whatever the radius."""
    import test_matcher_hip as TM
    n, H, W = 2, 8, 8
    B = SG.Built()
    maps = B.inp(TM.images(n, H, W, seed=4) + 0.5, TM.images(n, H, W, seed=9) + 0.5)
    out = B.out((n, H, W))
    nbytes = lib().car_superpoint_nms_workspace_bytes(n, H, W)
    work = B.work(nbytes, zero=True)
    B.call = lambda st: ok(lib().car_superpoint_nms(A.ptr(maps), n, H, W, 0, out.ptr, work.ptr, nbytes, st), "car_superpoint_nms")
    return B


def _pack_row(tensors, seed, scale=0.05):
    """A packer's parameters as inputs (the decoy: the same arrays moved by N(0, scale^2)); -> (Built, their device buffers)."""
    g, B = gen(seed), SG.Built()
    return B, [B.inp(t.float(), t.float() + scale * torch.randn(t.shape, generator=g)) for t in tensors]


def _matcher():
    sys_path_golden()
    import matcher_cases as C
    return C


@functools.lru_cache(maxsize=None)
def _matcher_weights(layers=("self", "cross")):
    from cross_attention_renderer_amd import matching as M
    C = _matcher()
    return M.MatcherWeights(C.superpoint_state(), C.superglue_state(len(layers)), layers)


def row_superpoint_pack():
    w = _matcher_weights()
    B, dev = _pack_row([*w.conv_w, *w.conv_b], 41)
    n = len(w.conv_w)
    out = B.out((lib().car_superpoint_packed_floats(),))
    tw, tb = A.ptrs(dev[:n]), A.ptrs(dev[n:])
    B.keep += [tw, tb]
    B.call = lambda st: ok(lib().car_superpoint_pack(tw, tb, out.ptr, st), "car_superpoint_pack")
    return B


def row_superglue_pack():
    w = _matcher_weights()
    B, dev = _pack_row(list(w.glue), 42)
    layers = len(w.gnn_layers)
    out = B.out((lib().car_superglue_packed_floats(layers),))
    table = A.ptrs(dev)
    B.keep.append(table)
    B.call = lambda st: ok(lib().car_superglue_pack(table, len(dev), layers, out.ptr, st), "car_superglue_pack")
    return B


def row_superpoint_dense():
    """One 16 x 16 image: 2 x 2 cells, both maps of the workspace and the heads' two pieces inside the second."""
    import test_matcher_hip as TM
    n, H, W = 1, 16, 16
    packed = _matcher_weights().packed(A.dev())
    B = SG.Built()
    im = B.inp(TM.images(n, H, W, seed=5), TM.images(n, H, W, seed=6))
    scores, desc = B.out((n, H, W)), B.out((n, H // 8, W // 8, 256))
    nbytes = lib().car_superpoint_workspace_bytes(n, H, W)
    work = B.work(nbytes)
    B.call = lambda st: ok(lib().car_superpoint_dense(A.ptr(im), n, H, W, A.ptr(packed), scores.ptr, desc.ptr, work.ptr, nbytes, st), "car_superpoint_dense")
    return B


def row_superpoint_select():
    """The 16 best of a 24 x 40 map with every pixel above the threshold: every slot of the outputs is filled on both sides."""
    import test_matcher_hip as TM
    n, H, W, maxk = 1, 24, 40, 16
    B = SG.Built()
    kept = B.inp(TM.images(n, H, W, seed=7) + 0.25, TM.images(n, H, W, seed=8) + 0.25)
    kp, sc, cnt = B.out((n, maxk, 2)), B.out((n, maxk)), B.out((n,), dtype=I32)
    nbytes = lib().car_superpoint_select_workspace_bytes(n, H, W)
    work = B.work(nbytes, zero=True)
    B.call = lambda st: ok(lib().car_superpoint_select(A.ptr(kept), n, H, W, ctypes.c_float(0.005), 0, maxk, kp.ptr, sc.ptr, cnt.ptr, work.ptr, nbytes, st),
                           "car_superpoint_select")
    return B


def _glue_inputs(B, N0, N1, H, W, seeds):
    def side(seed):
        g = gen(seed)
        k = [torch.rand(N, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0]) for N in (N0, N1)]
        sc = [torch.rand(N, generator=g) for N in (N0, N1)]
        d = [torch.nn.functional.normalize(torch.randn(N, 256, generator=g), dim=1) for N in (N0, N1)]
        return k + sc + d
    return [B.inp(r, d_) for r, d_ in zip(side(seeds[0]), side(seeds[1]))]


def row_superglue_descriptors():
    """N0 = 3 against N1 = 5 keypoints, two layers (self, cross): tests/test_matcher_hip.py's smallest."""
    (N0, N1), (H, W), layers = (3, 5), (48, 64), ("self", "cross")
    packed = _matcher_weights(layers).packed_glue(A.dev())
    B = SG.Built()
    k0, k1, s0, s1, d0, d1 = _glue_inputs(B, N0, N1, H, W, (13, 14))
    out = B.out((N0 + N1, 256))
    nbytes = lib().car_superglue_workspace_bytes(N0, N1)
    work = B.work(nbytes)
    cross = B.keep_host(A.ints([0, 1]))                              # the `cross` flags: never decoyed
    B.call = lambda st: ok(lib().car_superglue_descriptors(A.ptr(k0), A.ptr(s0), A.ptr(d0), N0, H, W, A.ptr(k1), A.ptr(s1), A.ptr(d1), N1, H, W, A.ptr(packed),
                                                           len(layers), cross, out.ptr, work.ptr, nbytes, st), "car_superglue_descriptors")
    return B


def row_superglue_transport():
    C = _matcher()
    m, n = 3, 5
    g, B = gen(15), SG.Built()
    a, b = (B.inp(torch.randn(k, 256, generator=g) * 0.6, torch.randn(k, 256, generator=g) * 0.6) for k in (m, n))
    Z = B.out((m + 1, n + 1))
    nbytes = lib().car_superglue_transport_workspace_bytes(m, n)
    work = B.work(nbytes)
    B.call = lambda st: ok(lib().car_superglue_transport(A.ptr(a), m, A.ptr(b), n, ctypes.c_float(C.BIN_SCORE), 2, Z.ptr, work.ptr, nbytes, st), "car_superglue_transport")
    return B


def row_superglue_matches():
    C = _matcher()
    m, n = 63, 65
    g, B = gen(16), SG.Built()
    Z = B.inp(torch.randn(m + 1, n + 1, generator=g) - 1.6, torch.randn(m + 1, n + 1, generator=g) - 1.6)
    m0, m1, s0, s1 = B.out((m,), dtype=I32), B.out((n,), dtype=I32), B.out((m,)), B.out((n,))
    nbytes = lib().car_superglue_matches_workspace_bytes(m, n)
    work = B.work(nbytes, zero=True)
    B.call = lambda st: ok(lib().car_superglue_matches(A.ptr(Z), m, n, ctypes.c_float(C.MATCH_THRESHOLD), m0.ptr, m1.ptr, s0.ptr, s1.ptr, work.ptr, nbytes, st),
                           "car_superglue_matches")
    return B


def row_essential_ransac():
    """N = 6 matches, H = 3 hypotheses (tests/test_pose_hip.py's exact-workspace case): solve, score and select over the one workspace."""
    import numpy as np
    import pose_reference as P
    N, H = 6, 3

    def scene(seed):
        k0, k1, _, _, _ = P.scene(N, seed, noise=0.5)
        x0, x1, nt = P.normalise(k0, k1, P.K, P.K, 1.0)
        return torch.from_numpy(np.ascontiguousarray(x0)), torch.from_numpy(np.ascontiguousarray(x1)), nt
    (x0, x1, nt), (y0, y1, _) = scene(40 + N), scene(90 + N)
    B = SG.Built()
    d0, d1 = B.inp(x0, y0), B.inp(x1, y1)
    samples = B.idx(torch.from_numpy(P.sample_table(N, H, seed=N).astype(np.int32)))       # the sample table: never decoyed
    E, best, inl = B.out((9,), dtype=F64), B.out((3,), dtype=I32), B.out_bytes(N)
    nbytes = lib().car_essential_workspace_bytes(N, H)
    work = B.work((nbytes + 3) // 4 * 4, zero=True)
    B.call = lambda st: ok(lib().car_essential_ransac(A.ptr(d0), A.ptr(d1), N, A.ptr(samples), H, ctypes.c_double(nt), E.ptr, best.ptr, inl.ptr, work.ptr, nbytes, st),
                           "car_essential_ransac")
    return B


def row_epipolar_overlay():
    Bn, V, H, W, rays, probe, S = 2, 2, 16, 24, 5, 3, 7
    g, B = gen(17), SG.Built()
    r = lambda *s: torch.rand(*s, generator=g)
    trgt, ctxt = B.inp(r(Bn, H, W, 3), r(Bn, H, W, 3)), B.inp(r(Bn * V, H, W, 3), r(Bn * V, H, W, 3))
    pv = B.inp(r(Bn * V, rays, S, 2) * 2 - 1, r(Bn * V, rays, S, 2) * 2 - 1)
    uv = B.inp(r(Bn, rays, 2) * torch.tensor([W - 1.0, H - 1.0]), r(Bn, rays, 2) * torch.tensor([W - 1.0, H - 1.0]))
    amax = B.idx(torch.randint(0, S, (Bn * V, rays), generator=g))                          # the arg-max indices: never decoyed
    panel = B.out((Bn + Bn * V, H, W, 3))
    B.call = lambda st: ok(lib().car_epipolar_overlay(A.ptr(trgt), A.ptr(ctxt), A.ptr(pv), A.ptr(amax), A.ptr(uv), Bn, V, H, W, rays, probe, S, panel.ptr, st),
                           "car_epipolar_overlay")
    return B


def row_merge_lattice_max():
    """The (4, 8, 16)^2 pyramid of tests/test_encode_hip.py: the memset of the maximum and the merge."""
    import encode_reference as ER
    sizes, n_maps = ER.PYRAMIDS["p3"], 3
    B = SG.Built()
    levels = [B.inp(r, d_) for r, d_ in zip(ER.levels_of(sizes, n_maps, ER.C, 500 + len(sizes)), ER.levels_of(sizes, n_maps, ER.C, 700))]
    lh, lw, _ = ER.lattice_of(sizes)[:3]
    lat, gmax = B.out((n_maps, 2, lh, lw, ER.C)), B.out((1,))
    ptrs, hs, ws = A.ptrs(levels), A.ints([h for h, _ in sizes]), A.ints([w for _, w in sizes])
    B.keep += [ptrs, hs, ws]
    B.call = lambda st: ok(lib().car_merge_lattice_max(ptrs, hs, ws, len(sizes), n_maps, lat.ptr, gmax.ptr, st), "car_merge_lattice_max")
    return B


def _row_linear_wgrad(case):
    """dW += dY^T X, db += column sums (fp32 atomics: two runs differ): onto zeros, held to the float64 reference by the yardstick of
    tests/test_linear_hip.py's own parity test."""
    import linear_reference as LR
    import test_linear_hip as TL
    M, N, K, has_db, relu, flags = LR.WGRAD_SHAPES[case]
    assert has_db
    dY, X, _, _, dW, db, BW, Bb, r32, r16 = TL._wgrad_reference("gauss", case, False)
    ldy, ldx, lddw = A.up4(N) + 4, A.up4(K) + (4 if K % 4 == 0 else 0), K + 5
    g, B = gen(M + N), SG.Built()
    ddY = B.inp(LR.padded(dY, ldy), LR.padded(torch.randn(dY.shape, generator=g), ldy))
    dX = B.inp(LR.padded(X, ldx), LR.padded(torch.randn(X.shape, generator=g), ldx))
    out, dbo = B.out((N, K), ld=lddw, zero=True), B.out((N,), zero=True)
    B.call = lambda st: ok(lib().car_linear_wgrad(A.ptr(ddY), ldy, A.ptr(dX), ldx, M, N, K, (LR.RELU_IN if relu else 0) | flags, out.ptr, lddw, dbo.ptr, st),
                           "car_linear_wgrad")
    kernel = LR.wgrad_dispatch(M, N, K, has_db, flags)
    r, what = (r16, "bf16-emulation") if kernel == "bf16" else (r32, "fp32")

    def bound(got, want):
        for name, run in (("behind the gate", got), ("eager", want)):
            TL._judge("linear_wgrad dW", f"{case} {name}", run[0], dW, BW, r, what)
            TL._judge("linear_wgrad db", f"{case} {name}", run[1], db, Bb, r, what)
    B.bound = bound
    return B


def row_linear_wgrad_fp32():
    return _row_linear_wgrad("tile35-K128-db")


def row_linear_wgrad_bf16():
    return _row_linear_wgrad("bf16-at-dispatch")


def row_scatter_binned():
    """tests/test_gather_hip.py's `wave3` set through the binned scatter: counters and indices in the workspace (poisoned with zeros), every
    texel written once.  Pass 3 adds in the order the records landed: held to the float64 reference by the parity test's own yardstick."""
    import test_gather_hip as TG
    import gather_reference as GR
    key, mode = "wave3", 0
    s = GR.edge_set(key)
    gathers = TG._gathers_of(s, mode)
    named = TG._named_rows(s["n_maps"], s["pts"], s["V"], [p for _, _, p in gathers])
    real = TG._dout(s["dout"], s["ld"], s["col_out"], named).view.clone()
    decoy = TG._dout(torch.randn(s["dout"].shape, generator=gen(23)), s["ld"], s["col_out"], named).view.clone()
    B = SG.Built()
    dout = B.inp(real, decoy)
    grids = [B.idx(g_) for g_, _, _ in gathers]                      # sample positions: never decoyed
    shapes, n_maps = s["shapes"], s["n_maps"]
    dmaps = [B.out((n_maps, H, W, C)) for H, W, C in shapes]
    cs, hs, ws = TG._levels(shapes)
    G = len(gathers)
    nbytes = lib().car_scatter_workspace_bytes(hs, ws, len(shapes), n_maps, s["pts"], G)
    assert nbytes > 0, lib().car_last_error()
    work = B.work((nbytes + 3) // 4 * 4, zero=True)
    tabs = (A.ptrs([d.view for d in dmaps]), A.ptrs(grids), A.ints([m for _, m, _ in gathers]), A.ints([p for _, _, p in gathers]))
    B.keep += [cs, hs, ws, tabs]
    B.call = lambda st: ok(lib().car_gather_bilinear_backward_binned(tabs[0], cs, hs, ws, len(shapes), n_maps, tabs[1], tabs[2], tabs[3], G, s["pts"], s["V"], A.ptr(dout),
                                                                     s["ld"], s["col_out"], work.ptr, nbytes, st), "car_gather_bilinear_backward_binned")

    def bound(got, want):
        ref, bnd, r32 = TG._scatter_reference(key, mode, False)
        for name, run in (("behind the gate", got), ("eager", want)):
            TG._judge("binned", f"{key} {name}", [(d.to(A.dev()), r, b) for d, r, b in zip(run, ref, bnd)], r32)
    B.bound = bound
    return B


# ---- the encoder's packers, its recorded forward and its backward ------------------------------------------------------------------------------------
def row_trunk_pack():
    import trunk_reference as TR
    depths = (1, 1, 1)
    B, dev = _pack_row(TR.seeded_trunk(depths), 51, 0.01)
    d = A.ints(depths)
    out = B.out((lib().car_trunk_packed_floats(d),))
    table = A.ptrs(dev)
    B.keep += [d, table]
    B.call = lambda st: ok(lib().car_trunk_pack(table, len(dev), d, out.ptr, st), "car_trunk_pack")
    return B


def row_vit_tokens_pack():
    import trunk_reference as TR
    grid, gh, gw = 4, 2, 2
    B, tp = _pack_row(TR.seeded_tokens(grid), 52, 0.01)
    out = B.out((lib().car_vit_tokens_packed_floats(gh, gw),))
    B.call = lambda st: ok(lib().car_vit_tokens_pack(A.ptr(tp[0]), A.ptr(tp[1]), A.ptr(tp[2]), A.ptr(tp[3]), grid, A.ptr(tp[4]), A.ptr(tp[5]), gh, gw, out.ptr, st),
                           "car_vit_tokens_pack")
    return B


def row_decoder_pack():
    import decoder_reference as DR
    B, dev = _pack_row(DR.seeded_decoder(), 53, 0.01)
    out = B.out((lib().car_decoder_packed_floats(),))
    table = A.ptrs(dev)
    B.keep.append(table)
    B.call = lambda st: ok(lib().car_decoder_pack(table, len(dev), out.ptr, st), "car_decoder_pack")
    return B


VIT = dict(dim=128, depth=3, taps=(1, 2), b=2, S=10)                  # tests/test_vit_backward_hip.py's first stage case


def row_vit_pack_train():
    import vit_reference as VR
    dim, depth = VIT["dim"], VIT["depth"]
    B, dev = _pack_row(VR.seeded_stage(dim, depth), 54, 0.01)
    out = B.out((lib().car_vit_packed_train_floats(dim, depth),))
    table = A.ptrs(dev)
    B.keep.append(table)
    B.call = lambda st: ok(lib().car_vit_pack_train(table, len(dev), dim, depth, out.ptr, st), "car_vit_pack_train")
    return B


def _vit_train_parts(B):
    """The recorded forward's buffers on `B`: tok (in place), the taps, the saved record, the workspace; -> (call, tok0, the pack)."""
    import test_vit_backward_hip as TV
    import vit_backward_reference as BR
    import vit_reference as VR
    dim, depth, taps, b, S = (VIT[k] for k in ("dim", "depth", "taps", "b", "S"))
    M = b * S
    packed, _ = TV._pack_train(VR.seeded_stage(dim, depth), dim, depth)
    tok0 = BR.autograd_stage(dim, depth, taps, b, S)[0].float()      # the parity test's tokens
    tok = B.inout(tok0, torch.randn(M, dim, generator=gen(dim + S + 1)))
    outs = [B.out((M, dim)) for _ in taps]
    sb, wb = lib().car_vit_saved_bytes(b, S, dim, depth), lib().car_vit_workspace_bytes(b, S, dim)
    saved, work = B.out((sb // 4,)), B.work(wb)
    ti, tp = A.ints(taps), A.ptrs([o.view for o in outs])
    B.keep += [ti, tp, packed]
    call = lambda st: ok(lib().car_vit_blocks_train(A.ptr(tok), b, S, dim, packed.ptr, depth, ti, len(taps), tp, saved.ptr, sb, work.ptr, wb, st), "car_vit_blocks_train")
    return call, tok0, packed, saved, sb, ti


def row_vit_blocks_train():
    B = SG.Built()
    B.call = _vit_train_parts(B)[0]
    return B


def row_vit_blocks_backward():
    """The recorded forward, then the backward over its record, both on the one stream.  dtok is bit-identical by the entry's own word; the
    matrices' and biases' gradients come from car_linear_wgrad (atomics) and are held, like the LayerNorm items, to float64 autograd by the
    yardsticks of tests/test_vit_backward_hip.py's own parity test."""
    import linear_reference as LR
    import parity_rule as PRU
    import test_vit_backward_hip as TV
    import vit_backward_reference as BR
    import vit_reference as VR
    dim, depth, taps, b, S = (VIT[k] for k in ("dim", "depth", "taps", "b", "S"))
    M, flags = b * S, 0
    B = SG.Built()
    forward, tok0, packed, saved, sb, ti = _vit_train_parts(B)
    a_tok0, dtaps, dout, a_tok, a_params = BR.autograd_stage(dim, depth, taps, b, S)
    assert torch.equal(a_tok0.float(), tok0), "the row's tokens are the parity test's"
    g = gen(77)
    dtok = B.inout(dout, torch.randn(M, dim, generator=g))
    dd = [B.inp(d, torch.randn(M, dim, generator=g)) for d in dtaps]
    off = TV._grad_offsets(dim)
    DP = B.out((depth * off[12],), zero=True)                        # "one flat buffer the CALLER ZEROES"
    wb = lib().car_vit_backward_workspace_bytes(b, S, dim)
    work = B.work(wb)
    tdd = A.ptrs(dd)
    B.keep.append(tdd)

    def call(st):
        forward(st)
        ok(lib().car_vit_blocks_backward(A.ptr(dtok), b, S, dim, packed.ptr, depth, ti, len(taps), tdd, saved.ptr, sb, DP.ptr, flags, work.ptr, wb, st),
           "car_vit_blocks_backward")
    B.call = call
    i_dp, i_dtok = len(B.outputs) - 1, len(B.outputs) + 1            # clones: the guarded outputs, then tok and dtok (the in-place ones)

    def bound(got, want):
        for i, (a, w) in enumerate(zip(got, want)):
            if i != i_dp:
                assert SG.same_bits(a, w), f"car_vit_blocks_train + backward: output {i} behind the gate differs from the eager one"
        ((y_tok, _), y_params), ops = TV._stage_yardstick(dim, depth, taps, b, S)
        params = VR.seeded_stage(dim, depth)
        for name, run in (("behind the gate", got), ("eager", want)):
            flat = run[i_dp]
            grads = [flat[(i // 12) * off[12] + off[i % 12]:][:params[i].numel()].reshape(params[i].shape) for i in range(12 * depth)]
            Bt = a_tok.abs().amax(dim=1, keepdim=True)
            entries = {"dtok": ((run[i_dtok], a_tok, Bt), TV._yard(y_tok, a_tok, Bt))}
            for i, (gr, a, (y, _)) in enumerate(zip(grads, a_params, y_params)):
                Bd = torch.full((), float(a.abs().max()), dtype=F64)
                yard = {"fp32": TV._yard(y, a, Bd)}
                item, blk = i % 12, i // 12
                if item in (2, 4, 8, 10) and LR.wgrad_dispatch(M, a.shape[0], a.shape[1], True, flags) == "bf16":
                    dY, X = next((dY, X) for it, dY, X in ops[blk] if it == item)
                    yard = {"bf16": TV._yard(LR.wgrad_bf16(dY, X, False, torch.zeros(a.shape), None)[0], a, Bd)}
                entries[f"b{blk}.{VR.PARAM_ORDER[item]}"] = ((gr, a, Bd), yard)
            PRU.judge("vit_blocks_backward", f"stream order, {name}", entries, finite=True)
    B.bound = bound
    return B


# ---- LPIPS ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lpips_weights():
    import lpips_restatement as LR
    from cross_attention_renderer_amd import harness
    return harness.LpipsWeights(*LR.seeded_weights(0))


def row_lpips_pack():
    w = _lpips_weights()
    B, dev = _pack_row([*w.conv_w, *w.conv_b, *w.lin], 61, 0.01)
    n, m = len(w.conv_w), len(w.conv_b)
    tabs = (A.ptrs(dev[:n]), A.ptrs(dev[n:n + m]), A.ptrs(dev[n + m:]))
    out = B.out((lib().car_lpips_packed_floats(),))
    B.keep.append(tabs)
    B.call = lambda st: ok(lib().car_lpips_pack(*tabs, out.ptr, st), "car_lpips_pack")
    return B


def row_lpips_pack_backward():
    w = _lpips_weights()
    B, dev = _pack_row(list(w.conv_w), 62, 0.01)
    table = A.ptrs(dev)
    out = B.out((lib().car_lpips_backward_packed_floats(),))
    B.keep.append(table)
    B.call = lambda st: ok(lib().car_lpips_pack_backward(table, out.ptr, st), "car_lpips_pack_backward")
    return B


def _lpips_pairs(B, Bn, H, W):
    import test_lpips_backward as TLB
    (x, y), (dx, dy) = TLB._pair_pm1("unrelated", Bn, H, W, 14), TLB._pair_pm1("unrelated", Bn, H, W, 15)
    return B.inp(x, dx), B.inp(y, dy)


def row_lpips():
    """B = 1, 16 x 16: the smallest image (the last tap is one pixel)."""
    Bn, H, W = 1, 16, 16
    packed = _lpips_weights().packed(A.dev())
    B = SG.Built()
    x, y = _lpips_pairs(B, Bn, H, W)
    value, taps = B.out((Bn,), dtype=F64), B.out((Bn, 5), dtype=F64)
    nbytes = lib().car_lpips_workspace_bytes(Bn, H, W)
    work = B.work(nbytes)
    B.call = lambda st: ok(lib().car_lpips(A.ptr(x), A.ptr(y), Bn, H, W, A.ptr(packed), value.ptr, taps.ptr, work.ptr, nbytes, st), "car_lpips")
    return B


def row_lpips_train_chain():
    """car_lpips_forward_train, then car_lpips_backward over the maps it retained, on the one stream and the one workspace."""
    import test_lpips_backward as TLB
    Bn, H, W = 1, 16, 16
    w = _lpips_weights()
    packed, packed_b = w.packed(A.dev()), w.packed_backward(A.dev())
    B = SG.Built()
    x, y = _lpips_pairs(B, Bn, H, W)
    gd = B.inp(TLB._cotangent(Bn, 14), TLB._cotangent(Bn, 15))
    value, gx, gy = B.out((Bn,), dtype=F64), B.out((Bn, H, W, 3)), B.out((Bn, H, W, 3))
    nbytes = lib().car_lpips_train_workspace_bytes(Bn, H, W)
    work = B.work(nbytes)

    def call(st):
        ok(lib().car_lpips_forward_train(A.ptr(x), A.ptr(y), Bn, H, W, A.ptr(packed), value.ptr, None, work.ptr, nbytes, st), "car_lpips_forward_train")
        ok(lib().car_lpips_backward(A.ptr(gd), gx.ptr, gy.ptr, Bn, H, W, A.ptr(packed), A.ptr(packed_b), work.ptr, nbytes, st), "car_lpips_backward")
    B.call = call
    return B


# ---- the training reader's frames ----------------------------------------------------------------------------------------------------------------------
def row_frames_resize():
    """Two raw 360 x 640 frames as the loader lays a batch out: stage A (uint8 resize and crop into the scratch behind the upload), then stage
    B (crop, flip, resize, conversion to float32) reading it; the frame records and the tables are index-like and never decoyed."""
    import numpy as np
    import test_train_frames_hip as TF
    from cross_attention_renderer_amd import dataio
    SIDE = TF.SIDE
    records = [TF._record(True), TF._record(True, True, True, 5, 13)]

    def frames(seed):
        rng = np.random.RandomState(seed)
        return [rng.randint(0, 256, size=(360, 640, 3)).astype(np.uint8) for _ in records]
    real, decoy = frames(5), frames(6)
    offs, at = [], 0
    for f in real:
        offs.append(at)
        at = dataio._align(at + f.nbytes)
    upload, scratch = at, len(records) * SIDE * SIDE * 3
    recs_a, recs_b, idx = dataio.stage_records([f.shape for f in real], records, [None] * len(records), offs, upload)
    assert len(idx) == 0

    def laid_out(fs):
        host = np.zeros(upload, np.uint8)
        for f, o in zip(fs, offs):
            host[o:o + f.nbytes] = f.reshape(-1)
        return torch.from_numpy(host)
    B = SG.Built()
    buf = torch.zeros(upload + scratch + 64, dtype=torch.uint8, device=A.dev())
    B.inputs.append((buf[:upload], laid_out(real).to(A.dev()), laid_out(decoy).to(A.dev())))
    B.extra_poison.append((buf[upload:], 0xAB))
    B.extra_out.append(buf[upload:upload + scratch])
    tables = B.idx(torch.from_numpy(dataio.frame_tables()))
    ra, rb = B.idx(torch.from_numpy(recs_a.view(np.uint8).copy())), B.idx(torch.from_numpy(recs_b.view(np.uint8).copy()))
    n_out = int(recs_b["dst_off"][-1]) + dataio._align(SIDE * SIDE * 3, 4)
    out = B.out((n_out,))
    B.keep += [recs_a, recs_b]

    def call(st):
        ok(lib().car_frames_resize_u8(buf.data_ptr(), upload, recs_a.ctypes.data, A.ptr(ra), len(records), A.ptr(tables), buf.data_ptr() + upload, scratch, st),
           "car_frames_resize_u8")
        ok(lib().car_frames_resize_f32(buf.data_ptr(), upload + scratch, recs_b.ctypes.data, A.ptr(rb), len(records), None, None, 0, A.ptr(tables), out.ptr, n_out, st),
           "car_frames_resize_f32")
    B.call = call
    return B


def row_gather_bilinear():
    """car_gather.hip through its forward entry, tests/test_gather_hip.py's `wave4` set (four levels with a 512-channel one, plain placement:
    every row of the output is written); the sample positions are index-like and never decoyed."""
    import gather_reference as GR
    import test_gather_hip as TG
    s = GR.edge_set("wave4")
    shapes, n_maps, pts, place, V = s["shapes"], s["n_maps"], s["pts"], s["place"], s["V"]
    assert place == GR.PLAIN
    C = sum(c for _, _, c in shapes)
    rows, ld, col_out = GR.n_rows(place, V, n_maps, pts), s["ld"], s["col_out"]
    g, B = gen(71), SG.Built()
    maps = [B.inp(t, torch.randn(t.shape, generator=g)) for t in s["maps"]]
    grid = B.idx(s["grid"])
    out = B.out((rows, ld))                                          # the windows [col_out, col_out + C) are written; the padding stays the guard
    cs, hs, ws = TG._levels(shapes)
    ptrs = A.ptrs(maps)
    B.keep += [cs, hs, ws, ptrs]
    B.call = lambda st: ok(lib().car_gather_bilinear(ptrs, cs, hs, ws, len(shapes), n_maps, A.ptr(grid), pts, s["run"], 0, place, V, out.ptr, ld, col_out, st), "car_gather_bilinear")
    return B


def row_lattice_encode_rows():
    """car_encode.hip's single launch: 148 rows of four taps of a 19 x 19 lattice (tests/test_encode_hip.py); the row table and the positions are
    index-like, the lattice is the input that has a decoy."""
    import encode_reference as ER
    import fused_reference as FR
    rows, pad = 148, 2
    lat, decoy = FR.random_lattice("gauss", 3, 8, 8, pad, seed=17), FR.random_lattice("gauss", 3, 8, 8, pad, seed=18)
    lh, lw = lat.shape[2:4]
    src, grid, pe = ER.edge_rows(3, rows, 50 + rows)
    B = SG.Built()
    dlat = B.inp(lat, decoy)
    dsrc, dgrid, dpe, dwpt = B.idx(src), B.idx(grid), B.idx(pe), B.idx(ER.point_table(ER.C, 530))
    out = B.out((rows, ER.C), ld=ER.C + 8)
    B.call = lambda st: ok(lib().car_lattice_encode_rows(A.ptr(dlat), lh, lw, pad, ER.C, A.ptr(dsrc), A.ptr(dgrid), A.ptr(dpe), A.ptr(dwpt), 3, rows, out.ptr, ER.C + 8, st),
                           "car_lattice_encode_rows")
    return B


def _weights_row(outputs, call_of, seed):
    """A packer of the staged route over the renderer's own layers (struct CarWeights of the render rows' module)."""
    s = _render_setup(True)
    w = s["eng"]._car_weights(A.dev())
    B = SG.Built()
    _weights_as_inputs(B, w, seed)
    outs = [B.out((int(n),)) for n in outputs]
    B.keep += [w, s]
    B.call = call_of(w, outs)
    return B


def row_kq_pack():
    L = lib()
    return _weights_row((L.car_kq_tail_floats(), L.car_kq_bias_floats()), lambda w, o: lambda st: ok(L.car_kq_pack(
        w.key_map_2_w, w.key_map_2_b, w.query_embed_w, w.query_embed_b, w.query_embed_2_w, w.query_embed_2_b, o[0].ptr, o[1].ptr, st), "car_kq_pack"), 81)


def row_round2_pack():
    L = lib()
    return _weights_row((L.car_round2_packed_floats(), L.car_round2_bias_floats()), lambda w, o: lambda st: ok(L.car_round2_pack(
        w.query_repeat_embed_w, w.query_repeat_embed_b, w.query_repeat_embed_2_w, w.query_repeat_embed_2_b, o[0].ptr, o[1].ptr, st), "car_round2_pack"), 82)


def row_fused_pack_rows():
    """Its second output is the fused kernel's bias table, of which this entry fills b2 and three scale slots and ZEROES the rest (400 of the
    688 entries it writes are zeros whatever the layers hold): that output is not held to "the decoy matters"; the tiles and the point table are."""
    L = lib()
    B = _fused_pack_rows_built(L)
    B.loose = (1,)
    return B


def _fused_pack_rows_built(L):
    return _weights_row((L.car_fused_blob_floats(), L.car_fused_bias_floats(), 576 * 4), lambda w, o: lambda st: ok(L.car_fused_pack_rows(
        w.query_encode_latent_w, w.query_encode_latent_b, w.query_encode_latent_2_w, w.query_encode_latent_2_b, o[0].ptr, o[1].ptr, o[2].ptr, st), "car_fused_pack_rows"), 83)


# ---- stage entries that are wrappers around a launcher another row's entry uses too: the wrapper itself hands the stream on ----------------------------
def row_render_forward_row_form():
    """car_render_forward_phase with CAR_PHASE_ROWS_FIRST_ROUND | CAR_PHASE_SPLIT_SECOND_ROUND beside the two phases: the branches the other
    render rows never issue — car_fused_samples, the first round's car_attend over the rows, car_round2_logits_from_g and the second
    car_attend."""
    def call_of(s, ci, co, work, need):
        return lambda st: ok(lib().car_render_forward_phase(ctypes.byref(s["d"]), A.ptr(s["plan"]), ctypes.byref(ci), ctypes.byref(co), work.ptr, need, 1 | 2 | 4 | 8, st),
                             "car_render_forward_phase")
    return _render_built(True, call_of)[0]


def row_merge_lattice():
    import encode_reference as ER
    sizes, n_maps = ER.PYRAMIDS["p3"], 3
    B = SG.Built()
    levels = [B.inp(r, d_) for r, d_ in zip(ER.levels_of(sizes, n_maps, ER.C, 500 + len(sizes)), ER.levels_of(sizes, n_maps, ER.C, 700))]
    lh, lw, _ = ER.lattice_of(sizes)[:3]
    lat = B.out((n_maps, 2, lh, lw, ER.C))
    ptrs, hs, ws = A.ptrs(levels), A.ints([h for h, _ in sizes]), A.ints([w for _, w in sizes])
    B.keep += [ptrs, hs, ws]
    B.call = lambda st: ok(lib().car_merge_lattice(ptrs, hs, ws, len(sizes), n_maps, lat.ptr, None, None, None, st), "car_merge_lattice")
    return B


def row_round2_logits():
    """b = 2, R = 50, P = 5 (tests/test_hip_parity.py's ragged case): the stored-query form of the second round's logits."""
    b, V, R, P = 2, 2, 50, 5
    S = b * V * R * P
    L = lib()

    def side_(seed):
        g = gen(seed)
        rnd = lambda *sh: torch.randn(*sh, generator=g)
        return [rnd(S, 16), rnd(b * R, 128), rnd(S, 128), rnd(128, 144) / 4, rnd(128), rnd(128, 128) / 128 ** 0.5, rnd(128)]
    B = SG.Built()
    gq, uh, qrows, wr1, br1, wr2, br2 = [B.inp(r, d_) for r, d_ in zip(side_(91), side_(92))]
    w0, b0 = torch.empty(L.car_round2_packed_floats(), device=A.dev()), torch.empty(L.car_round2_bias_floats(), device=A.dev())
    logit = B.out((S,))
    B.keep += [w0, b0]

    def call(st):                                                    # the pack belongs to the call: its layers are inputs with a decoy
        ok(L.car_round2_pack(A.ptr(wr1), A.ptr(br1), A.ptr(wr2), A.ptr(br2), A.ptr(w0), A.ptr(b0), st), "car_round2_pack")
        ok(L.car_round2_logits(A.ptr(gq), A.ptr(uh), A.ptr(qrows), A.ptr(w0), A.ptr(b0), b, V, R, P, logit.ptr, st), "car_round2_logits")
    B.call = call
    return B


LPIPS_TAPS = (64, 128, 256, 512, 512)


def _lpips_maps(B, Bn, H, W, seeds):
    """The five tap maps [2 Bn, H >> k, W >> k, C_k] of the head (images 0 .. Bn - 1 against Bn .. 2 Bn - 1) as inputs."""
    def side_(seed):
        g = gen(seed)
        return [torch.relu(torch.randn(2 * Bn, H >> k, W >> k, c, generator=g)) + 0.05 for k, c in enumerate(LPIPS_TAPS)]
    return [B.inp(r, d_) for r, d_ in zip(side_(seeds[0]), side_(seeds[1]))]


def row_lpips_head():
    Bn, H, W = 1, 16, 16
    L, B = lib(), SG.Built()
    maps = _lpips_maps(B, Bn, H, W, (93, 94))
    lin = B.idx(torch.cat([w.float().reshape(-1) for w in _lpips_weights().lin]))
    value, taps = B.out((Bn,), dtype=F64), B.out((Bn, 5), dtype=F64)
    n = L.car_lpips_head_scratch_doubles(Bn, H, W)
    work = B.work(8 * n)
    table = A.ptrs(maps)
    B.keep.append(table)
    B.call = lambda st: ok(L.car_lpips_head(table, Bn, H, W, A.ptr(lin), value.ptr, taps.ptr, work.ptr, n, st), "car_lpips_head")
    return B


def row_lpips_head_backward():
    Bn, H, W = 1, 16, 16
    L, B = lib(), SG.Built()
    maps = _lpips_maps(B, Bn, H, W, (95, 96))
    lin = B.idx(torch.cat([w.float().reshape(-1) for w in _lpips_weights().lin]))
    g = B.inp(torch.tensor([0.75], dtype=F64), torch.tensor([1.5], dtype=F64))
    gx = [B.out((Bn, H >> k, W >> k, c)) for k, c in enumerate(LPIPS_TAPS)]
    gy = [B.out((Bn, H >> k, W >> k, c)) for k, c in enumerate(LPIPS_TAPS)]
    table, tx, ty = A.ptrs(maps), A.ptrs([o.view for o in gx]), A.ptrs([o.view for o in gy])
    B.keep += [table, tx, ty]
    B.call = lambda st: ok(L.car_lpips_head_backward(table, Bn, H, W, A.ptr(lin), A.ptr(g), tx, ty, st), "car_lpips_head_backward")
    return B


def row_conv3x3_backward():
    """The data gradient of a 64 -> 64 layer at 8 x 8, two images, no epilogue: the transposed weights packed beforehand."""
    n, side_, K, N = 2, 8, 64, 64
    L, g, B = lib(), gen(97), SG.Built()
    w = (torch.randn(N, K, 3, 3, generator=g) / (9 * N) ** 0.5).to(A.dev()).contiguous()
    packed = torch.empty(L.car_conv3x3_backward_packed_floats(K, N), device=A.dev())
    ok(L.car_conv3x3_backward_pack(A.ptr(w), K, N, A.ptr(packed), A.stream()), "car_conv3x3_backward_pack")
    torch.cuda.synchronize()
    D = B.inp(torch.randn(n, side_, side_, N, generator=g), torch.randn(n, side_, side_, N, generator=g))
    out = B.out((n, side_, side_, K))
    B.keep += [w, packed]
    B.call = lambda st: ok(L.car_conv3x3_backward(A.ptr(D), n, side_, side_, K, N, A.ptr(packed), None, None, out.ptr, st), "car_conv3x3_backward")
    return B


def row_maxpool2x2_backward():
    """out = (the gradient routed to each window's maximum + add) where act > 0; act is positive throughout here, so every entry of the output
    depends on the inputs that have a decoy."""
    n, H, W, C = 3, 6, 10, 64
    L, g, B = lib(), gen(98), SG.Built()
    act = B.idx(torch.randn(n, H, W, C, generator=g).abs() + 0.1)   # decides the routing: index-like, never decoyed
    T = B.inp(torch.randn(n, H // 2, W // 2, C, generator=g), torch.randn(n, H // 2, W // 2, C, generator=g))
    add = B.inp(torch.randn(n, H, W, C, generator=g), torch.randn(n, H, W, C, generator=g))
    out = B.out((n, H, W, C))
    B.call = lambda st: ok(L.car_maxpool2x2_backward(A.ptr(T), A.ptr(act), A.ptr(add), n, H, W, C, out.ptr, st), "car_maxpool2x2_backward")
    return B


def row_superpoint_conv1a():
    import test_matcher_hip as TM
    n, H, W = 3, 17, 33                                              # odd sizes, more than one workgroup
    packed = _matcher_weights().packed(A.dev())
    B = SG.Built()
    im = B.inp(TM.images(n, H, W, seed=2) - 0.25, TM.images(n, H, W, seed=3) - 0.25)
    out = B.out((n, H, W, 64))
    B.call = lambda st: ok(lib().car_superpoint_conv1a(A.ptr(im), n, H, W, A.ptr(packed), out.ptr, st), "car_superpoint_conv1a")
    return B


def row_lattice_encode_linear():
    """193 rows of the 19 x 19 lattice through the gather-fed second layer (N = 128): tests/test_encode_hip.py's middle case."""
    import encode_reference as ER
    import fused_reference as FR
    import test_encode_hip as TEH
    rows, N, pad = 193, 128, 2
    L = lib()
    lat, decoy = FR.random_lattice("gauss", 3, 8, 8, pad, seed=17), FR.random_lattice("gauss", 3, 8, 8, pad, seed=18)
    lh, lw = lat.shape[2:4]
    src, grid, pe = ER.edge_rows(3, rows, 60 + N)
    W2, b2 = ER.second_layer(N)
    tiles = TEH._packed_layer(L, W2, N)
    B = SG.Built()
    dlat = B.inp(lat, decoy)
    dsrc, dgrid, dpe, dwpt, db2 = B.idx(src), B.idx(grid), B.idx(pe), B.idx(ER.point_table(ER.C, 531)), B.idx(b2)
    out = B.out((rows, N), ld=N + 8)
    B.keep.append(tiles)
    B.call = lambda st: ok(L.car_lattice_encode_linear(A.ptr(dlat), lh, lw, pad, A.ptr(dsrc), A.ptr(dgrid), A.ptr(dpe), A.ptr(dwpt), 3, rows, A.ptr(tiles), A.ptr(db2),
                                                       ER.C, N, out.ptr, N + 8, 0, st), "car_lattice_encode_linear")
    return B


def row_key_query_logits():
    """M = 193 rows of e at Ce = 288 with lde four floats wider (tests/test_linear_hip.py's KQ_SHAPES): the key and query chains and the first
    round's logits in one launch, over layers packed beforehand."""
    import linear_reference as LR
    import test_linear_hip as TL
    M, Ce, extra = 193, 288, 4
    L = lib()
    P = LR.kq_params(Ce, 20 + Ce)
    d = {k: v.to(A.dev()).contiguous() for k, v in P.items()}
    tiles = TL._pack_x3(L, P["Wk1"], Ce, 128)
    tail, tb = torch.empty(L.car_kq_tail_floats(), device=A.dev()), torch.empty(L.car_kq_bias_floats(), device=A.dev())
    ok(L.car_kq_pack(A.ptr(d["Wk2"]), A.ptr(d["bk2"]), A.ptr(d["Wq1"]), A.ptr(d["bq1"]), A.ptr(d["Wq2"]), A.ptr(d["bq2"]), A.ptr(tail), A.ptr(tb), A.stream()), "car_kq_pack")
    torch.cuda.synchronize()
    lde = A.up4(Ce) + extra
    (e, g_), (e2, g2) = LR.kq_rows(M, Ce, 30 + M), LR.kq_rows(M, Ce, 31 + M)
    B = SG.Built()
    de, dg = B.inp(LR.padded(e, lde), LR.padded(e2, lde)), B.inp(g_, g2)
    qry, logit = B.out((M, 128)), B.out((M,))
    B.keep += [d, tiles, tail, tb]
    B.call = lambda st: ok(L.car_key_query_logits(A.ptr(de), lde, A.ptr(tiles), A.ptr(d["bk1"]), Ce, A.ptr(dg), A.ptr(tail), A.ptr(tb), M, qry.ptr, logit.ptr, st),
                           "car_key_query_logits")
    return B


def row_linear_x3_masked():
    """193 x 100 -> 128 with RELU_OUT under a mask: the activations that decide the mask are index-like (never decoyed) and positive but for
    one column in sixteen, so that the masked zeros stay a small part of the output."""
    import linear_reference as LR
    import test_linear_hip as TL
    M, K, N = 193, 100, 128
    L = lib()
    X, W, b, _ = LR.linear_set("gauss", M, K, N, 1)
    X2 = LR.linear_set("gauss", M, K, N, 2)[0]
    tiles = TL._pack_x3(L, W, K, N)
    ldx, ldy, lda = A.up4(K), N + 8, N + 4
    act = torch.randn(M, N, generator=gen(99)).abs() + 0.1
    act[:, ::16] = -1.0
    B = SG.Built()
    dX = B.inp(LR.padded(X, ldx), LR.padded(X2, ldx))
    db, dact = B.idx(b), B.idx(LR.padded(act, lda))
    out = B.out((M, N), ld=ldy)
    B.keep.append(tiles)
    B.call = lambda st: ok(L.car_linear_x3_masked(A.ptr(dX), ldx, A.ptr(tiles), A.ptr(db), K, N, out.ptr, ldy, M, LR.RELU_OUT, A.ptr(dact), lda, st), "car_linear_x3_masked")
    return B


# name -> (builder, the entries the row calls); what THOSE call is read from the sources (stream_gate.entry_calls)
ROWS = {
    "car_add": (row_add, ("car_add",)),
    "car_plan_f16_build": (row_plan_f16_build, ("car_plan_f16_build",)),
    "car_project_maps": (row_project_maps, ("car_project_maps",)),
    "car_render_forward": (row_render_forward, ("car_render_forward",)),
    "car_render_forward, one round": (row_render_forward_one_round, ("car_render_forward",)),
    "car_render_forward_phase 1 + 2": (row_render_forward_phases, ("car_render_forward_phase",)),
    "car_render_forward_phase, rows first round + split second round": (row_render_forward_row_form, ("car_render_forward_phase",)),
    "car_render_forward_f16": (row_render_forward_f16, ("car_render_forward_f16",)),
    "car_merge_lattice_max": (row_merge_lattice_max, ("car_merge_lattice_max",)),
    "car_merge_lattice": (row_merge_lattice, ("car_merge_lattice",)),
    "car_round2_logits": (row_round2_logits, ("car_round2_pack", "car_round2_logits")),
    "car_lattice_encode_linear": (row_lattice_encode_linear, ("car_lattice_encode_linear",)),
    "car_key_query_logits": (row_key_query_logits, ("car_key_query_logits",)),
    "car_linear_x3_masked": (row_linear_x3_masked, ("car_linear_x3_masked",)),
    "car_lpips_head": (row_lpips_head, ("car_lpips_head",)),
    "car_lpips_head_backward": (row_lpips_head_backward, ("car_lpips_head_backward",)),
    "car_conv3x3_backward": (row_conv3x3_backward, ("car_conv3x3_backward",)),
    "car_maxpool2x2_backward": (row_maxpool2x2_backward, ("car_maxpool2x2_backward",)),
    "car_superpoint_conv1a": (row_superpoint_conv1a, ("car_superpoint_conv1a",)),
    "car_gather_bilinear_backward_binned": (row_scatter_binned, ("car_gather_bilinear_backward_binned",)),
    "car_linear_wgrad, fp32 pipe": (row_linear_wgrad_fp32, ("car_linear_wgrad",)),
    "car_linear_wgrad, bf16 pipe": (row_linear_wgrad_bf16, ("car_linear_wgrad",)),
    "car_gather_bilinear": (row_gather_bilinear, ("car_gather_bilinear",)),
    "car_lattice_encode_rows": (row_lattice_encode_rows, ("car_lattice_encode_rows",)),
    "car_kq_pack": (row_kq_pack, ("car_kq_pack",)),
    "car_round2_pack": (row_round2_pack, ("car_round2_pack",)),
    "car_fused_pack_rows": (row_fused_pack_rows, ("car_fused_pack_rows",)),
    "car_getz": (row_getz, ("car_getz",)),
    "car_trunk_pack": (row_trunk_pack, ("car_trunk_pack",)),
    "car_vit_tokens_pack": (row_vit_tokens_pack, ("car_vit_tokens_pack",)),
    "car_decoder_pack": (row_decoder_pack, ("car_decoder_pack",)),
    "car_vit_pack_train": (row_vit_pack_train, ("car_vit_pack_train",)),
    "car_vit_blocks_train": (row_vit_blocks_train, ("car_vit_blocks_train",)),
    "car_vit_blocks_train + car_vit_blocks_backward": (row_vit_blocks_backward, ("car_vit_blocks_train", "car_vit_blocks_backward",)),
    "car_lpips_pack": (row_lpips_pack, ("car_lpips_pack",)),
    "car_lpips_pack_backward": (row_lpips_pack_backward, ("car_lpips_pack_backward",)),
    "car_lpips": (row_lpips, ("car_lpips",)),
    "car_lpips_forward_train + car_lpips_backward": (row_lpips_train_chain, ("car_lpips_forward_train", "car_lpips_backward",)),
    "car_ssim": (row_ssim, ("car_ssim",)),
    "car_attention_entropy": (row_attention_entropy, ("car_attention_entropy",)),
    "car_image_grid": (row_image_grid, ("car_image_grid",)),
    "car_epipolar_overlay": (row_epipolar_overlay, ("car_epipolar_overlay",)),
    "car_superpoint_pack": (row_superpoint_pack, ("car_superpoint_pack",)),
    "car_superpoint_dense": (row_superpoint_dense, ("car_superpoint_dense",)),
    "car_superpoint_nms": (row_superpoint_nms, ("car_superpoint_nms",)),
    "car_superpoint_select": (row_superpoint_select, ("car_superpoint_select",)),
    "car_superglue_pack": (row_superglue_pack, ("car_superglue_pack",)),
    "car_superglue_descriptors": (row_superglue_descriptors, ("car_superglue_descriptors",)),
    "car_superglue_transport": (row_superglue_transport, ("car_superglue_transport",)),
    "car_superglue_matches": (row_superglue_matches, ("car_superglue_matches",)),
    "car_essential_ransac": (row_essential_ransac, ("car_essential_ransac",)),
    "car_frames_resize_u8 + car_frames_resize_f32": (row_frames_resize, ("car_frames_resize_u8", "car_frames_resize_f32",)),
}

# entries that synchronise by contract: tested for value on a side stream with the inputs ready (test_exceptions_on_a_side_stream)
EXCEPTIONS = {
    "car_plan_build": 'include/car_hip.h:375 "car_plan_build synchronises the stream once (it uploads a small host table)"; '
                      "csrc/car_render.hip: the hipStreamSynchronize behind the chain table's upload",
}

@pytest.fixture(scope="module")
def side():
    """The side stream of the gated tests — after stream_gate.instrument() has chosen the gate that sees a stray launch on this runtime (it
    raises where none does), so that this module means the same run alone as run behind tests/test_stream_gate.py."""
    SG.instrument()
    return torch.cuda.Stream()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROWS))
def test_entry_keeps_to_its_stream(name, side):
    """Conclusive (so the call returned while the gate was running: it synchronised nothing), the result of the eager call, no margin written."""
    rec = SG.check_case(ROWS[name][0](), side, name)
    assert rec["conclusive"]


@pytest.mark.gpu
def test_exceptions_on_a_side_stream(side):
    """car_plan_build synchronises, so no gate can stay closed across it: called on a side stream with its inputs ready, its plan renders —
    car_render_forward on the same stream — the bytes the engine rendered with the plan it built on the default stream."""
    s = _render_setup(True)
    d = s["d"]
    w = s["eng"]._car_weights(A.dev())
    nbytes = lib().car_plan_bytes(ctypes.byref(d))
    assert nbytes == s["plan"].numel() * 4
    plan = A.Guarded((nbytes // 4,))

    def call_of(s_, ci, co, work, need):
        return lambda st: ok(lib().car_render_forward(ctypes.byref(d), plan.ptr, ctypes.byref(ci), ctypes.byref(co), work.ptr, need, st), "car_render_forward")
    B, _ = _render_built(True, call_of)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ok(lib().car_plan_build(ctypes.byref(d), ctypes.byref(w), plan.ptr, SG.stream_ptr(side)), "car_plan_build")
        B.load("real")
        B.poison()
        B.call(SG.stream_ptr(side))
        got = dict(zip(ORDER, B.clones()))
    side.synchronize()
    assert plan.margins_untouched() and B.margins_untouched()
    ref = s["sides"]["real"]["ref"]
    for k in ("rgb", "depth_ray", "at_wt", "valid_mask"):
        assert SG.same_bits(got[k].cpu(), ref[k].cpu().reshape(got[k].shape)), f"{k}: the plan built on the side stream renders other bytes than the engine's"


# ---- CPU: the table accounts for every entry --------------------------------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "cross_attention_renderer_amd", "csrc")


def _accounted():
    """How every stream entry is accounted for, in this order:
    rows       a row of the table calls it
    under      a row's entry, or an exception, calls it (read from the sources): {entry: the caller}
    single     NOT run behind a gate.  The table's rule takes one single-launch entry from every translation unit no row otherwise reaches,
               not each of them; these are the others: no other entry calls them, their body has exactly one enqueue site and no helper that
               enqueues, a row reaches their unit, and the stream written at that site is the entry's own `stream` parameter
               (stream_gate.site_streams reads it).  That last check is of the source text, not of the running library."""
    calls, sites, handed = SG.entry_calls(CSRC), SG.launch_sites(CSRC), SG.site_streams(CSRC)
    rows = {e for _, entries in ROWS.values() for e in entries}
    under = {}
    for r in sorted(rows | set(EXCEPTIONS)):
        for e in calls[r]:
            under.setdefault(e, r)
    gated = rows | {e for e, r in under.items() if r in rows}
    units = {e: f for f in sorted(os.listdir(CSRC)) if f.endswith(".hip") for e in re.findall(r'extern "C" int (car_\w+)\(', open(os.path.join(CSRC, f)).read())}
    reached = {units[e] for e in gated}
    single = {e for e, s_ in sites.items() if e not in gated and s_ == {e: 1} and units[e] in reached and handed.get(e) == ["stream"]}
    return dict(calls=calls, sites=sites, handed=handed, rows=rows, under=under, single=single, units=units, reached=reached)


def test_every_stream_entry_is_accounted_for():
    """Every entry whose prototype ends in the stream is a row of the table, is called by a row's entry or by an exception, or is an exception
    with its reason; what is left are single launches of units a row reaches, each handed the entry's own stream in the source — named in
    profiles/stream_order.md as not run behind a gate.  An entry added later without one of these fails here; and every translation unit
    that exports a stream entry is reached by a row."""
    import __graft_entry__ as ge
    ge.build()
    entries = set(SG.stream_entries())
    a = _accounted()
    assert a["rows"] <= entries and set(EXCEPTIONS) <= entries and entries <= set(a["units"])
    assert all(EXCEPTIONS.values())
    nowhere = sorted(entries - a["rows"] - set(a["under"]) - a["single"] - set(EXCEPTIONS))
    assert nowhere == [], f"no row, no caller among the rows, no exception, and not a single launch handed the entry's own stream: {nowhere}"
    stream_units = {a["units"][e] for e in entries}
    unreached = sorted(stream_units - a["reached"])
    assert not unreached, f"no row reaches {unreached}"
    print("single launches, not gated:", sorted(a["single"] - a["rows"] - set(a["under"])))


def test_the_stream_at_a_launch_site_is_read_from_the_source():
    src = ('extern "C" int car_a(float* x, void* stream) { hipLaunchKernelGGL(k, dim3(g(1, 2)), dim3(256), 0, (hipStream_t)stream, x); return 0; }\n'
           'extern "C" int car_b(float* x, void* stream) { hipStream_t st = (hipStream_t)stream; CAR_LAUNCH_LDS("b", k, grid, block, lds, st, x); return 0; }\n'
           'extern "C" int car_c(float* x, void* stream) { hipLaunchKernelGGL(k, grid, block, 0, 0, x); return 0; }\n'
           'extern "C" int car_d(float* x, void* stream) { hipMemsetAsync(x, 0, f(3, 4), (hipStream_t)0); k<<<grid, block, 0, static_cast<hipStream_t>(stream)>>>(x); return 0; }\n')
    bodies = SG.function_bodies(src)
    assert [SG.streams_in(bodies[n]) for n in ("car_a", "car_b", "car_c", "car_d")] == [["stream"], ["stream"], ["0"], ["0", "stream"]]
    handed = _accounted()["handed"]
    assert handed["car_add"] == ["stream"] and handed["car_relu_mask"] == ["stream"] and handed["car_fused_rows"] == ["stream"]


def test_the_call_graph_is_read_from_the_sources():
    """stream_gate.entry_calls on the launchers themselves: through static helpers (car_render_forward's phases), across units (car_getz) and
    not at all (car_lpips drives its kernels itself)."""
    acc = _accounted()
    calls, under = acc["calls"], acc["under"]
    assert {"car_attend", "car_ray_tail", "car_fused_samples"} <= calls["car_render_forward"] == calls["car_render_forward_phase"]
    assert {"car_trunk_forward", "car_vit_blocks", "car_decoder_forward", "car_stem7x7", "car_mha"} <= calls["car_getz"]
    assert calls["car_vit_blocks_backward"] >= {"car_linear_wgrad", "car_mha_backward", "car_add"}
    assert calls["car_lpips"] == set() and calls["car_add"] == set()
    assert calls["car_plan_build"] == {"car_chain_pack", "car_fused_pack", "car_linear_pack", "car_linear_x3_pack", "car_round2q_pack"}
    assert under["car_fused_pack"] == "car_plan_build"
    sites = acc["sites"]
    assert sites["car_add"] == {"car_add": 1} and sites["car_lpips"] == {"pool": 1, "head": 2, "conv": 1} and sites["car_lpips_head"] == {"head": 2}
    assert {"car_relu_mask", "car_colormap", "car_finalize"} <= acc["single"]
    src = 'namespace { static int helper(int a) { return car_x(a); } }\nextern "C" int car_y(void* s) { /* car_z( */ return helper(1) + f("car_w("); }\n'
    bodies = SG.function_bodies(src)
    assert set(bodies) == {"helper", "car_y"} and "car_x" in bodies["helper"] and "car_z" not in bodies["car_y"] and "car_w" not in bodies["car_y"]


# ==== the package under a side stream =====================================================================================================================
# One warm call on the default stream; then the same call under `with torch.cuda.stream(s)` behind a gate on s, the real inputs copied over a
# decoy behind the gate, with a spy on the checked handle: EVERY C entry called in the section received s as its stream (a handle or a stream
# kept from an earlier call would show), the step is conclusive, and the result is bit-identical to the default-stream call — or inside the
# run-to-run bound the package's own tests hold two calls to, where two calls differ.
class Pack:
    """call() -> the list of device tensors the case compares (host code that only enqueues); inputs: (buffer, real, decoy) triples."""

    def __init__(self, call, inputs, bound=None, host_reads=None, loose=(), expect=()):
        self.call, self.inputs, self.bound, self.host_reads, self.loose, self.expect = call, inputs, bound, host_reads, loose, tuple(expect)


def _pair_of(real, decoy):
    real, decoy = real.to(A.dev()).contiguous(), decoy.to(A.dev()).contiguous()
    return decoy.clone(), real, decoy


def run_package(p: Pack, side, what):
    try:
        return _run_package(p, side, what)
    finally:                                                          # the buffers may be somebody's tensors: they hold the real inputs again
        with torch.no_grad():
            for buf, real, _ in p.inputs:
                buf.copy_(real)
        torch.cuda.synchronize()


def _run_package(p: Pack, side, what):
    import time

    def load(which):
        with torch.no_grad():
            for buf, real, decoy in p.inputs:
                buf.copy_(real if which == "real" else decoy)

    host = lambda ts: [t.detach().cpu() for t in ts]
    load("real")
    p.call()                                                          # warm: caches, packed weights, workspaces, on the default stream
    torch.cuda.synchronize()
    load("real")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = p.call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    want = host(outs)
    if p.inputs:
        load("decoy")
        decoy = host(p.call())
        torch.cuda.synchronize()
        SG.decoy_matters(want, decoy, p.loose)
    seen = {}

    def reset():
        load("decoy")
        torch.cuda.synchronize()

    def step():
        with torch.cuda.stream(side), SG.spied() as spy:
            seen["spy"] = spy
            load("real")
            return [t.detach().clone() for t in p.call()]

    reset()
    if p.host_reads:                                                  # a documented host read: no gate can stay closed across it
        got = step()
        side.synchronize()
    else:
        got, rec = SG.gated(side, ms, step, what, reset)
        assert rec["conclusive"]
    spy = seen["spy"]
    assert spy.calls, f"{what}: no C entry was called"
    assert spy.strays(side) == [], f"{what}: entries handed another stream than the current one: {spy.strays(side)}"
    missing = [e for e in p.expect if e not in spy.entries()]
    assert not missing, f"{what}: the case was meant to reach {missing}; it called {spy.entries()}"
    got = host(got)
    if p.bound is None:
        for i, (g, w) in enumerate(zip(got, want)):
            assert SG.same_bits(g, w), f"{what}: output {i} under the side stream differs from the default-stream call in {SG.differing_fraction(g, w):.1%} of its entries"
    else:
        p.bound(got, want)
    return spy


RENDER_KEYS = ("rgb", "depth_ray", "at_wt")            # what depends on the pyramid (pixel_val and coords are geometry alone)


def _render_pack(name, setup=None, expect=()):
    from golden_util import load_case
    from hip_harness import build_module, to_device
    c, inp, z, sd, _ = load_case(name)
    m = build_module(c, sd, A.dev())
    if setup is not None:
        setup(m)
    dinp = to_device(inp, A.dev(), cameras_on_host=True)
    g = gen(101)
    triples = [_pair_of(t, torch.randn(t.shape, generator=g)) for t in z]
    bufs = [t[0] for t in triples]

    def call():
        with torch.no_grad():
            out = m(dinp, z=bufs)
        return [out[k] for k in RENDER_KEYS]
    return Pack(call, triples, expect=expect), m


def pack_one_call():
    p, m = _render_pack("t1_c1", expect=("car_project_maps",))
    return p


def pack_staged():
    def setup(m):
        from cross_attention_renderer_amd.engine import RenderEngine
        m._engine = RenderEngine(m)
        m._engine.fuse_samples = False                               # "the engine's fuse_samples / project_maps switches select the stage route"
    return _render_pack("t1_c1", setup, expect=("car_ray_setup", "car_attend"))[0]


def pack_three_views():
    return _render_pack("t1_nview3", expect=("car_exchange_rows",))[0]


def pack_fp16():
    return _render_pack("t1_c1", lambda m: setattr(m, "render_precision", "fp16"), expect=("car_render_forward_f16",))[0]


def pack_render_train():
    """render_train's forward, its backward and one optimizer step (t0_default).  The forward is bit-identical; the gradients are sums of fp32
    atomics (car_linear_wgrad, the scatter) and are held to tests/test_grad_hip.py's run-to-run bound: 2e-6 of a tensor's largest entry per
    run, two runs compared; the stepped parameters to the same bound times the learning rate."""
    from golden_util import load_case
    from hip_harness import build_module, to_device
    from cross_attention_renderer_amd.training import render_train
    sys_path_golden()
    import grad_cases as G
    c, inp, z, sd, _ = load_case("t0_default")
    m = build_module(c, sd, A.dev()).train()
    dinp = to_device(inp, A.dev(), cameras_on_host=True)
    g = gen(102)
    triples = [_pair_of(t, torch.randn(t.shape, generator=g)) for t in z]
    bufs = [t[0] for t in triples]
    named = dict(m.named_parameters())
    p0 = {k: v.detach().clone() for k, v in named.items()}
    lr = 0.125
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    cots, loose = {}, [1]

    def call():
        with torch.no_grad():
            for k, v in named.items():
                v.copy_(p0[k])                                        # every run starts from the same parameters
        m.zero_grad(set_to_none=True)
        zr = [t.clone().requires_grad_(True) for t in bufs]
        out = render_train(m, dinp, z=zr)
        if not cots:
            c_rgb, c_depth = G.cotangents(out["rgb"].shape, out["depth_ray"].shape)
            cots["rgb"], cots["depth"] = c_rgb.to(A.dev()), c_depth.to(A.dev())
        ((out["rgb"] * cots["rgb"]).sum() + (out["depth_ray"] * cots["depth"]).sum()).backward()
        with_grad = [k for k in sorted(named) if named[k].grad is not None]
        grads = [named[k].grad.clone() for k in with_grad] + [t.grad for t in zr]
        opt.step()
        stepped = [named[k].detach().clone() for k in with_grad]
        if len(loose) == 1:
            # not held to "the decoy matters": depth_ray (read off the arg-max sample: on this 16 x 16 case another pyramid moves it on one ray
            # in seven); the last layer's bias gradient (the sum of the cotangent, whatever the pyramid holds); and the stepped parameters,
            # p0 - lr g, which follow the gradients that ARE held to it
            loose.extend([2 + with_grad.index("phi.lin_out.bias"), *range(2 + len(grads), 2 + len(grads) + len(stepped))])
        return [out["rgb"].detach(), out["depth_ray"].detach(), *grads, *stepped]

    def bound(got, want):
        n = sum(1 for k in named if named[k].grad is not None)       # got = rgb, depth_ray | n parameter gradients | the pyramid's | n stepped parameters
        assert len(got) == len(want) == 2 + n + len(bufs) + n
        for i in (0, 1):
            assert SG.same_bits(got[i], want[i]), f"render_train: forward output {i} differs under the side stream"
        for i in range(2, 2 + n + len(bufs)):
            a, w = got[i].double(), want[i].double()
            assert bool(torch.isfinite(a).all()) and float((a - w).abs().max()) <= 4e-6 * float(w.abs().max()), ("render_train gradient", i)
        for j in range(n):                                           # p0 - lr g: the gradient's bound times lr, and one rounding of the parameter
            a, w, gscale = got[2 + n + len(bufs) + j].double(), want[2 + n + len(bufs) + j].double(), float(want[2 + j].abs().max())
            assert float((a - w).abs().max()) <= lr * 4e-6 * gscale + 2.0 ** -23 * float(w.abs().max()), ("render_train stepped parameter", j)
    return Pack(call, triples, bound=bound, loose=loose, expect=("car_linear_wgrad", "car_attend_backward"))


def sys_path_golden():
    import sys
    p = os.path.join(ROOT, "tests", "golden")
    if p not in sys.path:
        sys.path.insert(0, p)


TORCH_LINES = ("models.py get_z: the relative pose is torch's own torch.inverse, which reads the factorisation's status on the host, and the "
               "normalisation's mean and std are new_tensor uploads from the host, which torch waits for")


def _getz_pack(route):
    """get_z at the small image of the existing route tests (tests/test_encoder_train_route.py).

    device_full is all C but for the relative pose's 4x4 algebra, torch's own lines.  torch.inverse reads its status on the host, so no gate
    can stay closed across it: its result for these cameras (which have no decoy) is computed before the gate closes and handed to get_z in
    its place, and everything else of the call is behind the gate, conclusive and bit-identical.
    On the other routes get_z also normalises the images in torch — two new_tensor uploads that torch waits for, which ARE the normalisation,
    between the inverse and the encoder — and torch stages surround the kernels.  Those three cases are VALUE ONLY: they run under the side
    stream with no gate at all, so they show the stream every entry was handed (the spy) and that two calls agree to twice the fixture bound
    of each other, as that file holds them — nothing about the order of the launches inside."""
    import test_encoder_train_route as TE
    m, inp = TE._renderer()
    rgb = inp["context"]["rgb"]
    g = gen(103)
    triple = _pair_of(rgb, (torch.rand(rgb.shape, generator=g) * 2 - 1).to(rgb.dtype))
    inp = {k: dict(v) for k, v in inp.items()}
    inp["context"]["rgb"] = triple[0]
    train, full = route == "device_train", route == "device_full"
    cams = inp["context"]["cam2world"]
    inverse, real_inverse = torch.inverse(cams[:, :1]), torch.inverse
    torch.cuda.synchronize()

    def known_inverse(a):
        assert a.shape == inverse.shape and a.data_ptr() == cams[:, :1].data_ptr(), "get_z inverts the first context camera"
        return inverse

    def call():
        m.encoder_route = route
        if full:
            torch.inverse = known_inverse
        try:
            if not train:
                with torch.no_grad():
                    return [t.float() for t in m.get_z(inp)]
            m.zero_grad(set_to_none=True)                             # the recorded forward and its backward: both must follow the current stream
            z = m.get_z(inp)
            sum(t.sum() for t in z).backward()
            return [t.detach().float() for t in z]
        finally:
            torch.inverse = real_inverse
            m.encoder_route = "torch"

    def bound(got, want):
        for x, y in zip(got, want):
            rms = float(y.double().pow(2).mean().sqrt())
            assert float((x - y).abs().max()) <= 2 * (1e-3 * rms + 1e-6), (route, float((x - y).abs().max()), rms)
    expect = {"device": ("car_vit_blocks",), "device_trunk": ("car_trunk_forward", "car_vit_tokens", "car_vit_blocks"), "device_full": ("car_normalize_rgb", "car_trunk_forward", "car_vit_tokens", "car_vit_blocks", "car_decoder_forward", "car_conv7x7_pad3"),
              "device_train": ("car_vit_blocks_train", "car_vit_blocks_backward")}[route]
    return Pack(call, [triple], bound=None if full else bound, host_reads=None if full else TORCH_LINES, expect=expect)


def _images(seed, B=2, H=32, W=48):
    g = gen(seed)
    return torch.rand(B, H, W, 3, generator=g)


def pack_ssim():
    from cross_attention_renderer_amd import harness
    x, y = _pair_of(_images(1), _images(2)), _pair_of(_images(3), _images(4))
    return Pack(lambda: [harness.ssim(x[0], y[0])], [x, y], expect=("car_ssim",))


def pack_lpips():
    from cross_attention_renderer_amd import harness
    w = _lpips_weights()
    x, y = _pair_of(_images(5), _images(6)), _pair_of(_images(7), _images(8))
    return Pack(lambda: list(harness.lpips(x[0], y[0], w, return_taps=True)), [x, y], expect=("car_lpips",))


def pack_lpips_loss():
    from cross_attention_renderer_amd import harness
    w = _lpips_weights()
    x, y = _pair_of(_images(9) * 2 - 1, _images(10) * 2 - 1), _pair_of(_images(11) * 2 - 1, _images(12) * 2 - 1)

    def call():
        a = x[0].clone().requires_grad_(True)
        loss = harness.lpips_loss(a, y[0], w)
        loss.sum().backward()
        return [loss.detach(), a.grad]
    return Pack(call, [x, y], expect=("car_lpips_forward_train", "car_lpips_backward"))


def pack_attention_entropy():
    from cross_attention_renderer_amd import summaries
    g = gen(104)
    w = _pair_of(torch.softmax(torch.randn(4, 96, 24, generator=g), -1), torch.softmax(2 * torch.randn(4, 96, 24, generator=g), -1))
    return Pack(lambda: [summaries.attention_entropy(w[0]), summaries.attention_entropy(w[0], nan_rows_zero=False)], [w], expect=("car_attention_entropy",))


def pack_img_summaries():
    """summaries.img_summaries on a fixture's batch: its grids, its panel and its scalars, all device tensors ("nothing here waits")."""
    import test_summaries_hip as TS
    import summary_cases
    from cross_attention_renderer_amd import summaries
    name = sorted(summary_cases.CASES)[0]
    B, V, H, W = summary_cases.CASES[name]
    inp, out, _ = summary_cases.load(name)
    to = lambda d: {k: (v.to(A.dev()) if torch.is_tensor(v) else v) for k, v in d.items()}
    inp_d, out_d = {k: to(v) for k, v in inp.items()}, to(out)
    g = gen(105)
    triples = []
    for d, k, make in ((out_d, "rgb", lambda t: torch.rand(t.shape, generator=g) * 2 - 1), (out_d, "depth_ray", lambda t: torch.rand(t.shape, generator=g) + 0.5),
                       (out_d, "at_wt", lambda t: torch.softmax(torch.randn(t.shape, generator=g), -1)),
                       (inp_d["context"], "rgb", lambda t: torch.rand(t.shape, generator=g) * 2 - 1), (inp_d["query"], "rgb", lambda t: torch.rand(t.shape, generator=g) * 2 - 1)):
        if k in d and torch.is_tensor(d[k]) and d[k].is_floating_point():
            t = _pair_of(d[k], make(d[k]).to(d[k].dtype))
            d[k] = t[0]
            triples.append(t)

    def call():
        rec = TS.Recorder()
        summaries.img_summaries(None, inp_d, None, {}, out_d, rec, 40, prefix="val_", img_shape=(H, W), n_view=V)
        return [v.float() if v.dtype != F64 else v for _, v, _ in rec.calls if torch.is_tensor(v)]
    return Pack(call, triples, expect=("car_image_grid", "car_epipolar_overlay", "car_attention_entropy"))


def pack_estimate_pose():
    """harness.estimate_pose downloads E, the winner and the inlier mask (its recoverPose is the host's): only the spy and the value apply."""
    import numpy as np
    import pose_reference as P
    from cross_attention_renderer_amd import harness
    k0, k1, _, _, _ = P.scene(64, 104, noise=0.5, outliers=0.4)

    def call():
        got = harness.estimate_pose(k0, k1, P.K, P.K, 1.0, hypotheses=64, seed=3)
        assert got is not None
        R_, t_, inl = got[:3]
        return [torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(A.dev()) for x in (R_, t_, inl)]
    return Pack(call, [], host_reads="harness.py: E, best and the inlier mask are read on the host for recoverPose", expect=("car_essential_ransac",))


def pack_match_pair():
    """matching.match_pair reads the keypoint counts on the host between its stages: only the spy and the value apply."""
    from cross_attention_renderer_amd import matching as M
    C = _matcher()
    w = M.MatcherWeights(C.superpoint_state(), C.superglue_state(), C.GNN_LAYERS)
    name = sorted(C.PAIRS)[0]
    _, _, _, radius, thr, maxk, border = C.PAIRS[name]
    im = C.pair_images(name)
    im = (im if torch.is_tensor(im) else torch.from_numpy(im)).float()
    a, b = _pair_of(im[0], im[0].flip(0)), _pair_of(im[1], im[1].flip(0))

    def call():
        got = M.match_pair(a[0], b[0], w, radius, thr, maxk, border, C.SINKHORN_ITERATIONS, C.MATCH_THRESHOLD)
        return [got[k].float() for k in ("keypoints0", "keypoints1", "matching_scores0", "matching_scores1")]
    return Pack(call, [a, b], host_reads="matching.py: the keypoint counts are read on the host between SuperPoint and SuperGlue", loose=(0, 1, 2, 3),
                expect=("car_superpoint_dense", "car_superglue_descriptors", "car_superglue_matches"))


PACKS = {
    "model(inp, z=z), one call": pack_one_call,
    "model(inp, z=z), staged": pack_staged,
    "model(inp, z=z), three views": pack_three_views,
    "model(inp, z=z), render_precision fp16": pack_fp16,
    "render_train: forward, backward, optimizer step": pack_render_train,
    "get_z, device (value only, not gated: host reads)": lambda: _getz_pack("device"),
    "get_z, device_trunk (value only, not gated: host reads)": lambda: _getz_pack("device_trunk"),
    "get_z, device_full": lambda: _getz_pack("device_full"),
    "get_z, device_train, with its backward (value only, not gated: host reads)": lambda: _getz_pack("device_train"),
    "harness.ssim": pack_ssim,
    "harness.lpips": pack_lpips,
    "harness.lpips_loss and its backward": pack_lpips_loss,
    "summaries.attention_entropy": pack_attention_entropy,
    "summaries.img_summaries": pack_img_summaries,
    "harness.estimate_pose (value only, not gated: host reads)": pack_estimate_pose,
    "matching.match_pair (value only, not gated: host reads)": pack_match_pair,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PACKS))
def test_package_follows_the_current_stream(name, side):
    run_package(PACKS[name](), side, name)


# ==== the three hand-offs between streams =================================================================================================================
# Here the gate goes on the PRODUCER's stream: the consumer is enqueued while the producer has not run yet, so a missing wait reads memory the
# producer has not written — deterministically, not only when the producer happens to be slow.
HANDOFF_KEYS = ("rgb", "depth_ray", "at_wt", "valid_mask", "pixel_val")


def _handoff_module(seed=3):
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=16, with_encoder=False).eval()
    S.perturb_parameters(m, seed=seed)
    m.H = m.W = 64
    return m


def _render(m, inp, z):
    with torch.no_grad():
        return [m(inp, z=z)[k].clone() for k in HANDOFF_KEYS]


def _timed(fn):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


@pytest.mark.gpu
def test_prefetch_hands_the_pair_over_behind_its_event():
    """RenderEngine.prefetch projects the next pair on its side stream; the forward that receives those tensors waits for the side stream's
    event.  With the side stream gated: announce pair 1 and render it at once — the step is conclusive and the result is a fresh module's inline
    forward of pair 1.  Then the reverse hazard (tests/test_engine_cache.py's weight change): with the side stream gated, announce a pair,
    replace the weights and render — the side stream still reads the old plan and still writes the announced buffers behind the gate, and the
    forward, which re-projects with the new plan, gives a fresh module's result."""
    SG.instrument()
    import cases as C
    from cross_attention_renderer_amd import synthetic as S
    from hip_harness import to_device
    dev = A.dev()
    H, R, b = 64, 120, 2
    torch.manual_seed(0)
    m = _handoff_module().to(dev)
    inp = to_device(S.stereo_scene(H, b=b, uv=C.select_rays(H, R), seed=4, alpha=0.4), dev, cameras_on_host=True)
    zs = {sd: [t.to(dev) for t in S.feature_maps(b, 2, H, seed=sd)] for sd in (1, 2, 3, 4)}
    fresh = _handoff_module()
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev)
    want = {sd: [t.cpu() for t in _render(fresh, inp, zs[sd])] for sd in (2, 4)}
    _render(m, inp, zs[1])                                            # warm forward on pair 0: the plan exists
    eng = m._engine
    if eng._pf_stream is None:
        eng._pf_stream = torch.cuda.Stream(device=dev)               # prefetch only makes one when it is None
    side = eng._pf_stream

    def announce_and_render(z):
        assert m.prefetch_pair(z), "the pair was not announced"
        return _render(m, inp, z)
    _, ms = _timed(lambda: announce_and_render(zs[3]))                # the same warm step, ungated, on a pair of its own
    assert not eng._pf, "the forward did not take the announced pair over"
    tries = iter([zs[2], [t.clone() for t in zs[2]]])                # a retry announces tensors of its own: the first ones are already in place
    got, rec = SG.gated(side, ms, lambda: announce_and_render(next(tries)), "RenderEngine.prefetch -> forward", eng.drop_prefetched)
    assert rec["conclusive"] and not eng._pf
    for k, g, w in zip(HANDOFF_KEYS, got, want[2]):
        assert SG.same_bits(g.cpu(), w), f"{k}: the forward read the announced pair before the side stream had made it"

    # the reverse hazard
    def change_and_render(z):
        with torch.no_grad():
            assert m.prefetch_pair(z)
            m.phi.lin_out.weight.mul_(1.5)
            return _render(m, inp, z)
    with torch.no_grad():
        fresh.phi.lin_out.weight.mul_(1.5)
    want4 = [t.cpu() for t in _render(fresh, inp, zs[4])]
    got, rec = SG.gated(side, ms, lambda: change_and_render(zs[4]), "RenderEngine.prefetch across a weight change")
    assert rec["attempt"] == 0, "the weights were changed once: a retry would change them again"
    for k, g, w in zip(HANDOFF_KEYS, got, want4):
        assert SG.same_bits(g.cpu(), w), f"{k}: differs from a fresh module's forward with the new weights"
    eng.drop_prefetched()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_train_loader_hands_its_batches_over_behind_their_events():
    """dataio.TrainLoader's device path stages, uploads and runs car_frames_resize_u8 / _f32 on a stream of its own, from a second host
    thread, and hands each batch over with an event and record_stream.  With the loader's stream gated before the epoch starts, every tensor of
    every yielded batch is cloned on the current stream at once: the first batch arrives while the gate is still closed (conclusive), and all
    of them equal the host-collated batches bit for bit.  Three batches over prefetch = 2, two epochs: the staging slots are reused."""
    SG.instrument()
    sys_path_golden()
    import train_scene
    from cross_attention_renderer_amd import dataio
    ds = dataio.RealEstate10k(train_scene.img_root(), train_scene.pose_root(), num_ctxt_views=2, num_query_views=1, query_sparsity=192, augment=True)
    dev = A.dev()
    host = dataio.TrainLoader(ds, batch_size=1, seed=21, num_workers=8, prefetch=2)
    device = dataio.TrainLoader(ds, batch_size=1, seed=21, num_workers=8, device=dev, prefetch=2)
    want = [list(host) for _ in range(5)]                             # epoch 0 warms; two gated rounds, each with one retry at the most
    assert len(want[0]) == 3, "the committed scenes give three batches of one"
    spy = SG.Spy(device._device_state()["lib"], SG.all_signatures()).install()
    try:
        _, ms = _timed(lambda: [1 for _ in device])                  # epoch 0, ungated: warm (the tables, the slots) and the gate's measure
        side = device._device_state()["stream"]
        epoch = 1
        for _ in range(2):
            for attempt in (0, 1):
                torch.cuda.synchronize()
                ev, pending, got = SG.gate(side, SG.gate_ms_for(ms) * SG.RETRY ** attempt), None, []
                for inp_d, _ in device:
                    got.append({part: {k: (t.clone() if torch.is_tensor(t) and t.is_cuda else t) for k, t in d.items()} for part, d in inp_d.items()})
                    pending = (not ev.query()) if pending is None else pending       # decided when the FIRST batch has been handed over and cloned
                torch.cuda.synchronize()
                assert len(got) == 3
                for (h_inp, _), d_inp in zip(want[epoch], got):
                    for part in ("query", "context"):
                        assert list(h_inp[part]) == list(d_inp[part])
                        for k, w in h_inp[part].items():
                            assert torch.equal(d_inp[part][k].cpu(), w), (epoch, part, k, "read before the loader's stream had written it")
                epoch += 1
                SG.log(dict(what="TrainLoader, first batch of an epoch", kind=SG.kind(), ungated_ms=round(ms, 3), gate_ms=round(min(SG.gate_ms_for(ms) * SG.RETRY ** attempt, SG.CAP_MS), 3),
                            attempt=attempt, conclusive=bool(pending)))
                if pending:
                    break
            else:
                raise SG.Inconclusive("the loader's gate had ended before the first batch was handed over, twice")
    finally:
        spy.remove()
    assert {"car_frames_resize_f32"} <= set(spy.entries()) and spy.strays(device._device_state()["stream"]) == []


@pytest.fixture()
def one_rank_nccl():
    import socket
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    before = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        dist.init_process_group("nccl", rank=0, world_size=1)
        try:
            yield dist
        finally:
            dist.destroy_process_group()
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_tile_gather_joins_its_side_stream_both_ways(one_rank_nccl):
    """sharding.TileGather snapshots and all-gathers on a side stream (a one-rank "nccl" group).  (a) the caller's stream gated, the tile
    produced behind the gate: out[0] is the tile — the side stream waited for the caller's.  (b) the gather's stream gated: wait(), then a read
    of `out` on the caller's stream at once, is complete — the caller's stream waited for the gather's.  (c) the tile overwritten right after
    __call__: the snapshot does not see the overwrite."""
    SG.instrument()
    from cross_attention_renderer_amd import sharding as Sh
    rows, ch = 512, 5
    g = gen(31)
    tiles = [torch.randn(rows, ch, generator=g).to(A.dev()) for _ in range(4)]
    caller = torch.cuda.Stream()
    tg = Sh.TileGather(1, rows, ch, A.dev())
    with torch.cuda.stream(caller):
        tg(tiles[3])                                                   # warm: the first collective makes the communicator (seconds)
        tg.wait()
        _, ms = _timed(lambda: (tg(tiles[0]), tg.wait().clone()))
    tile = torch.zeros(rows, ch, device=A.dev())

    def produced_behind_the_gate():                                    # (a) and (c)
        with torch.cuda.stream(caller):
            tile.copy_(tiles[1])
            tg(tile)
            tile.fill_(-7.0)                                           # "the caller may overwrite `tile` as soon as the snapshot is taken"
            return tg.wait().clone()
    tile.zero_()
    got, rec = SG.gated(caller, ms, produced_behind_the_gate, "TileGather, the caller's stream gated", tile.zero_)
    assert rec["conclusive"] and torch.equal(got[0], tiles[1]), "the gather read the tile before the caller's stream had produced it, or after it was overwritten"

    def gathered_behind_the_gate():                                    # (b): the gate sits on tg.stream, in front of the snapshot and the collective
        with torch.cuda.stream(caller):
            tg(tiles[2])
            return tg.wait().clone()
    tg.out.fill_(float("nan"))
    got, rec = SG.gated(tg.stream, ms, gathered_behind_the_gate, "TileGather, the gather's stream gated", lambda: tg.out.fill_(float("nan")))
    assert rec["conclusive"] and torch.equal(got[0], tiles[2]), "`out` was read on the caller's stream before the gather had written it"
    torch.cuda.synchronize()
