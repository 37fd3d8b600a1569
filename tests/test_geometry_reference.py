"""CPU checks of tests/geometry_reference.py, the checker test_geometry_hip.py holds the geometry kernels to.

  * its float32 mode equals the host shim (tests/host/car_geom_host.cpp: the header's own inline functions, compiled by g++ with
    -ffp-contract=off) BIT FOR BIT on every input set and every field; the tanhf outputs (g[9..12], xenc) to 1e-6 as test_geom_host.py
    holds them (libm against SLEEF);
  * its float64 mode agrees with oracle/car_oracle.py's stage functions on the fixtures' cameras at the rule of the GPU suite;
  * the input sets hold the edges they were built for;
  * the float32 mode alone stays inside the cap: at most 2 % of a set's rays or samples outside a decided mask; no sample is left out of
    the pt comparison as parallel (M_pt carries 1 / sin^2), which the ceilings on r32 — also on the near-parallel samples alone — hold
    it to; outside the masks everything is still finite and `overlaps` 0 or 1."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import geometry_reference as GR
from geometry_reference import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "car_geom_host.cpp")
INC = os.path.join(ROOT, "cross_attention_renderer_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "host", "_build", "libcar_geom_host.so")
SAMPLE_FLOATS = 36                                         # CarSample: grid 2, pt 3, g 16, pt_in 9, grid_in 6
NAMES = tuple(GR.SETS)


@functools.lru_cache(maxsize=None)
def shim():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(INC, "car_geom.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-I", INC, SRC, "-o", OUT])
    lib = ctypes.CDLL(OUT)
    assert lib.host_sizeof_pose() == 96 * 4 and lib.host_sizeof_ray() == 12 * 4 and lib.host_sizeof_sample() == SAMPLE_FLOATS * 4
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _np(t, dtype=np.float32):
    return np.ascontiguousarray(t.numpy(), dtype=dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, what):
    got = torch.as_tensor(got)
    d = _bits(got) != _bits(want.reshape(got.shape))
    assert not bool(d.any()), f"{what}: {int(d.sum())} of {d.numel()} floats differ from the host shim, first at {d.nonzero()[0].tolist()}"


# ---- the shim's side ---------------------------------------------------------------------------------------------------------------------
def shim_poses(c):
    out = np.zeros((c["b"] * c["V"], 96), np.float32)
    shim().host_pose_setup(_ptr(_np(c["c2w_ctx"])), _ptr(_np(c["c2w_q"])), _ptr(_np(c["K_ctx"])), _ptr(_np(c["K_q"])), c["b"], c["V"], c["H"], _ptr(out))
    return torch.from_numpy(out)


def shim_rays(c, P32):
    out = np.zeros((c["b"] * c["V"], c["R"], 12), np.float32)
    if c["no_sample"]:
        shim().host_ray_setup_depth(_ptr(_np(P32)), _ptr(_np(c["uv"])), _ptr(_np(c["steps"])), c["b"], c["V"], c["R"], c["H"], c["W"], c["P"], _ptr(out))
    else:
        shim().host_ray_setup(_ptr(_np(P32)), _ptr(_np(c["uv"])), c["b"], c["V"], c["R"], _ptr(out))
    return torch.from_numpy(out)


def shim_samples(c, P32, R32):
    S = c["b"] * c["V"] * c["R"] * c["P"]
    out = np.zeros((S, SAMPLE_FLOATS), np.float32)
    fn = shim().host_sample_setup_depth if c["no_sample"] else shim().host_sample_setup
    fn(_ptr(_np(P32)), _ptr(_np(R32)), _ptr(_np(c["steps"])), c["b"], c["V"], c["R"], c["P"], c["H"], c["W"], _ptr(out))
    xe = np.zeros((S, 6) if c["V"] == 1 else (S, c["V"], 3), np.float32)
    shim().host_xenc(_ptr(out), ctypes.c_long(S), c["V"], _ptr(xe))
    t = torch.from_numpy(out)
    return {"grid": t[:, 0:2], "pt": t[:, 2:5], "g": t[:, 5:21], "pt_in": t[:, 21:30].reshape(S, 3, 3)[:, :c["V"]],
            "grid_in": t[:, 30:36].reshape(S, 3, 2)[:, :c["V"]], "xenc": torch.from_numpy(xe)}


stage = GR.stage


# ---- 1. float32 == the host shim, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + ("pose-65",))
def test_float32_poses_equal_the_shim(name):
    c = GR.pose_set() if name == "pose-65" else GR.cameras(name)
    got = GR.poses(c["c2w_ctx"], c["c2w_q"], c["K_ctx"], c["K_q"], c["H"], dtype=F32)["rec"]
    _same(got, shim_poses(c), "CarPose")


@pytest.mark.parametrize("name", NAMES)
def test_float32_rays_equal_the_shim(name):
    st = stage(name)
    want = shim_rays(st["c"], st["P32"])
    for f, (a, b) in {"d": (0, 3), "m": (3, 6), "start": (6, 8), "end": (8, 10), "overlaps": (10, 11), "pad": (11, 12)}.items():
        _same(st["r32"]["rec"][..., a:b], want[..., a:b], f"{name} CarRay.{f}")


@pytest.mark.parametrize("name", NAMES)
def test_float32_samples_equal_the_shim(name):
    st = stage(name)
    want = shim_samples(st["c"], st["P32"], st["R32"])
    got = st["s32"]
    for f in ("grid", "pt", "pt_in", "grid_in"):
        _same(got[f], want[f], f"{name} {f}")
    tanh = torch.zeros(16, dtype=torch.bool)
    tanh[9:13] = True
    _same(got["g"][:, ~tanh], want["g"][:, ~tanh], f"{name} g")
    assert float((got["g"][:, tanh] - want["g"][:, tanh]).abs().max()) < 1e-6
    assert float((got["xenc"] - want["xenc"]).abs().max()) < 1e-6


@pytest.mark.parametrize("V", (2, 3))
def test_float32_exchange_rows_equal_the_shim(V):
    c = GR.cameras("v3" if V == 3 else "wide")
    P32 = GR.poses(c["c2w_ctx"], c["c2w_q"], c["K_ctx"], c["K_q"], c["H"], dtype=F32)["rec"]
    pv, pin, pe = GR.exchange_inputs(V)
    pts = pv.shape[0] // (2 * V)
    got = GR.exchange_rows(P32, pv, pin, pe, 2, V, pts, c["H"], c["W"], dtype=F32)
    rows = 2 * V * pts * V
    src, grid, rpe = np.zeros(rows, np.int32), np.zeros((rows, 2), np.float32), np.full((rows, 4), np.nan, np.float32)
    shim().host_exchange_rows(_ptr(_np(P32)), _ptr(_np(pv)), _ptr(_np(pin)), _ptr(_np(pe)), 2, V, ctypes.c_long(pts), c["H"], c["W"], _ptr(src),
                              _ptr(grid), _ptr(rpe))
    assert np.array_equal(src, got["row_src"].numpy())
    _same(got["row_grid"], torch.from_numpy(grid), "row_grid")
    _same(got["row_pe"], torch.from_numpy(rpe), "row_pe")
    assert bool((got["row_pe"][:, 3] == 0).all())
    # the definition, spelled out once more: component k of context c reads view o = the k-th of (c, then the others ascending)
    for c_, want_o in ((0, [0, 1, 2][:V]), (1, [1, 0, 2][:V]), (2, [2, 0, 1])):
        if c_ < V:
            first = got["row_src"].reshape(2, V, pts, V)[1, c_, 0]
            assert [int(x) & 0x3fffffff for x in first] == [V + o for o in want_o] and [int(x) >> 30 for x in first] == [0] + [1] * (V - 1)
    d = got["D_row_grid"]
    assert bool((got["row_grid"][~d.any(dim=-1)] if (~d).any() else torch.zeros(1)).isfinite().all())
    assert bool((got["row_grid"].abs() > 1e8).any()), "no 1e10 landing point"


@pytest.mark.parametrize("view", (0, 1))
def test_float32_project_points_equal_the_shim(view):
    c = GR.cameras("wide")
    P32 = GR.poses(c["c2w_ctx"], c["c2w_q"], c["K_ctx"], c["K_q"], c["H"], dtype=F32)["rec"]
    pts = GR.project_inputs()
    got = GR.project_points(P32, pts, 2, c["V"], view, c["H"], c["W"], dtype=F32)
    out = np.zeros((2, pts.shape[1], 2), np.float32)
    shim().host_project_points(_ptr(_np(P32)), _ptr(_np(pts)), 2, ctypes.c_long(pts.shape[1]), c["V"], view, c["H"], c["W"], _ptr(out))
    _same(got["grid"], torch.from_numpy(out), "grid")
    g = got["grid"]
    x1e10 = torch.tensor(1e10, dtype=F32) / float(c["W"] - 1) * 2.0 - 1.0
    assert g[0, 3, 0] == x1e10 or abs(float(g[0, 3, 0])) > 1e10          # z = -1e-12f: zz exactly 0: inf (or 0 / 0) scrubbed
    assert g[0, 5, 0] == x1e10 and g[1, 7, 1] == torch.tensor(1e10, dtype=F32) / float(c["H"] - 1) * 2.0 - 1.0


# ---- 2. float64 against the oracle's stage functions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("t0_default", "t0_no_sample", "t0_nview3", "t0_nview1"))
def test_float64_agrees_with_the_oracle(name):
    """oracle/car_oracle.py's fp32 stage functions on a fixture's cameras, fed the same fp32 pose records, within 8 x max(r32, 2^-22) of the
    summed magnitudes on the decided elements — r32 the float32 mode's own ratio there."""
    import cases as C
    from cross_attention_renderer_amd.poses import pack_poses
    from oracle import car_oracle as O
    c = C.case_config(name)
    inp, _ = C.build_inputs(c)
    b, V, P, H = c["b"], c["n_view"], c["P"], c["H"]
    no_sample = int(bool(c.get("no_sample", False)))
    uv = inp["query"]["uv"][:, 0].float().contiguous()
    R = uv.shape[1]
    P32 = pack_poses(inp, H)
    pz = P32.reshape(b, V, 96)
    q_rel, c_rel = O._rows_to_4x4(pz[..., 0:12]), O._rows_to_4x4(pz[..., 12:24])
    K_ctx, K_q = inp["context"]["intrinsics"].float(), inp["query"]["intrinsics"].float()
    lf = O.pluecker_rays(q_rel.flatten(0, 1), uv[:, None].expand(-1, V, -1, -1).flatten(0, 1), K_q.expand(-1, V, -1, -1).flatten(0, 1))
    steps = torch.linspace(0.1, 10.0, P) if no_sample else torch.linspace(0, 1, P)
    r32 = GR.rays(P32, uv, b, V, R, H, H, no_sample, steps, dtype=F32)
    r64 = GR.rays(P32, uv, b, V, R, H, H, no_sample, steps, dtype=F64, d32=lf[..., 0:3])
    o_q = q_rel[..., :3, 3].flatten(0, 1)
    if no_sample:
        pv, valid = O.volumetric_samples(lf.reshape(b, V, R, 6), q_rel, K_ctx, H, H, P)
        pixel_val, ov = pv.flatten(0, 1), valid.flatten(0, 1)
        start, end = pixel_val[:, :, 0], pixel_val[:, :, -1]
    else:
        K01 = K_ctx.clone()
        K01[:, :, :2, :] = K01[:, :, :2, :] / H
        seg = O.project_rays(o_q[:, None, :].expand(-1, R, -1), lf[..., :3], K01.flatten(0, 1)[:, :3, :3])
        start, end, ov = O._scrub((seg["xy_min"] - 0.5) * 2, 0.0), O._scrub((seg["xy_max"] - 0.5) * 2, 0.0), seg["overlaps_image"]
        pixel_val = start[:, :, None, :] + (end - start)[:, :, None, :] * steps[None, None, :, None]
    ora_ray = torch.cat([lf, start, end, ov.float()[..., None], torch.zeros_like(ov.float()[..., None])], dim=-1)
    D = r64["D"][..., None]
    assert float(D.double().mean()) > 1 - GR.CAP_UNDECIDED
    for f, (a, z) in {"d": (0, 3), "m": (3, 6), "start": (6, 8), "end": (8, 10)}.items():
        yard = GR.ratio(r32["rec"][..., a:z], r64["rec"][..., a:z], r64["M_rec"][..., a:z], D)
        got = GR.ratio(ora_ray[..., a:z], r64["rec"][..., a:z], r64["M_rec"][..., a:z], D)
        assert got <= GR.tolerance(yard), (name, f, got, yard)
    assert torch.equal(ora_ray[..., 10][r64["D"]].double(), r64["rec"][..., 10][r64["D"]])
    # the sample stage, fed the oracle's own ray records
    R32 = ora_ray.contiguous()
    pt = O.epipolar_points(lf, pixel_val, c_rel.flatten(0, 1), K_ctx.flatten(0, 1), H, H)
    sd = (b, V, R, P, H, H, no_sample)
    s32 = GR.samples(P32, R32, steps, *sd, dtype=F32)
    s64o = GR.samples(P32, R32, steps, *sd, dtype=F64, grid32=pixel_val.reshape(-1, 2), pt32=pt.reshape(-1, 3))
    s64 = GR.samples(P32, R32, steps, *sd, dtype=F64, grid32=s32["grid"], pt32=s32["pt"])
    ptv = pt.reshape(b, V, R, P, 3)
    T = [O._rows_to_4x4(pz[..., 24 + 12 * s:36 + 12 * s]) for s in range(V)]
    pts_in = torch.stack([O._apply_4x4(T[s][:, :, None, None], ptv) for s in range(V)], dim=-2)             # (b, V, R, P, s, 3)
    grid_in = torch.stack([O._norm_for_grid(O._project_pixels(pts_in[..., s, :], K_ctx[:, s, None, None, None]), H, H) for s in range(V)], dim=-2)
    cam = O.camera_ray_dirs(pixel_val, K_ctx.flatten(0, 1), H, H)
    ora = {"grid": pixel_val.reshape(-1, 2), "pt": pt.reshape(-1, 3), "pt_in": torch.nan_to_num(pts_in, 0.0).reshape(-1, V, 3),
           "grid_in": grid_in.reshape(-1, V, 2)}
    for f in ("grid", "pt", "pt_in", "grid_in"):
        yard = GR.ratio(s32[f], s64[f], s64["M_" + f], s64["D_" + f])
        got = GR.ratio(ora[f], s64o[f], s64o["M_" + f], s64o["D_" + f])
        assert got <= GR.tolerance(yard), (name, f, got, yard)
    yard = GR.ratio(s32["g"][:, 0:3], s64["g"][:, 0:3], s64["M_g"][:, 0:3])
    got = GR.ratio(cam.reshape(-1, 3), s64o["g"][:, 0:3], s64o["M_g"][:, 0:3])
    assert got <= GR.tolerance(yard), (name, "g[0:3]", got, yard)
    # g[6..15] and xenc: the documented formulas (models.py:494-528, 482-483, 335-342; oracle/car_oracle.py:404, 433, 475-477) written out in
    # plain torch from the oracle's own pt and T pt — the divisors 1 / 10 / 100 / 1000 of the depth, 5 and 100 of the point, the 6-wide
    # window of V = 1 (t0_nview1) and the 3 per view otherwise
    o64 = o_q.double()[:, None, None, :].expand(b * V, R, P, 3).reshape(-1, 3)
    ptd = pt.reshape(-1, 3).double()
    depth = O._scrub((ptd - o64).norm(p=2, dim=-1, keepdim=True), 1e6)
    want_g = torch.cat([lf[:, :, None, 0:3].double().expand(-1, -1, P, -1).reshape(-1, 3), torch.tanh(depth), torch.tanh(depth / 10.0),
                        torch.tanh(depth / 100.0), torch.tanh(depth / 1000.0), o64], dim=-1)
    yard = GR.ratio(s32["g"][:, 6:16], s64["g"][:, 6:16], s64["M_g"][:, 6:16], s64["D_g"][:, 6:16])
    got = GR.ratio(want_g, s64o["g"][:, 6:16], s64o["M_g"][:, 6:16], s64o["D_g"][:, 6:16])
    assert got <= GR.tolerance(yard), (name, "g[6:16]", got, yard)
    assert bool((s64o["g"][:, 3:6] == 0).all())
    if V == 1:
        ptn = torch.where(torch.isnan(ptd), torch.zeros_like(ptd), ptd)
        want_x = torch.cat([torch.tanh(ptn / 5.0), torch.tanh(ptn / 100.0)], dim=-1)
    else:
        want_x = torch.tanh(torch.nan_to_num(pts_in, 0.0).double() / 5.0).reshape(-1, V, 3)
    assert want_x.shape == s64o["xenc"].shape
    yard = GR.ratio(s32["xenc"], s64["xenc"], s64["M_xenc"], s64["D_xenc"])
    got = GR.ratio(want_x, s64o["xenc"], s64o["M_xenc"], s64o["D_xenc"])
    assert got <= GR.tolerance(yard), (name, "xenc", got, yard)


# ---- 3. the sets hold their edges ------------------------------------------------------------------------------------------------------------
def test_the_sets_hold_their_edges():
    """Over the default-mode sets (decided rays only): both overlaps values; each of the four hits chosen as the minimum and as the
    maximum while it matters (ok0 / oki false); ok0 and oki both ways; depth_zero without at_camera; at_camera; a scrubbed start / end.
    Over the sample stages: a non-finite T pt of each nan_to_num kind, a 1e10 grid coordinate, a sample whose own pixel ray is within
    sin^2 < 1e-6 of the query ray.  Per set what it was built for."""
    seen_min, seen_max, flags = set(), set(), {}
    for name in NAMES:
        st = stage(name)
        c, rec, D = st["c"], st["r32"]["rec"], st["r64"]["D"]
        ov = rec[..., 10][D]
        assert set(ov.tolist()) == {0.0, 1.0}, (name, "overlaps")
        assert name != "backward" or float((rec[..., 2] <= 0).double().mean()) > 0.2, (name, "d_z <= 0")
        if c["no_sample"]:
            continue
        i = st["r32"]["info64"]
        seen_min |= set(i["imin"][D & ~i["ok0"] & i["vmin"]].tolist())
        seen_max |= set(i["imax"][D & ~i["oki"] & i["vmax"]].tolist())
        for k, v in (("ok0", i["ok0"]), ("!ok0", ~i["ok0"]), ("oki", i["oki"]), ("!oki", ~i["oki"]), ("depth_zero", i["depth_zero"] & ~i["at_camera"]),
                     ("at_camera", i["at_camera"]), ("scrubbed", i["scrubbed"])):
            flags.setdefault(k, set())
            if bool((v & D).any()):
                flags[k].add(name)
    assert seen_min == {0, 1, 2, 3} and seen_max == {0, 1, 2, 3}, (seen_min, seen_max)
    assert all(flags[k] for k in flags), flags
    assert {"on-ctx0", "on-ctx1"} <= flags["at_camera"] and "behind" in flags["depth_zero"] and {"on-ctx0", "on-ctx1"} <= flags["scrubbed"]
    o = stage("on-ctx0")["P32"][:, [3, 7, 11]]
    assert bool((o[0::2] == 0).all()), "on-ctx0: the query is not exactly on context 0"
    assert bool((stage("behind")["P32"][:, 11] < 0).all())
    near = stage("near")
    o = near["P32"][0::2][:, [3, 7, 11]].double()
    assert bool((o.norm(dim=-1) > 1.01e-6).all()) and bool((o[:, 2].abs() < 0.995e-6).all()), "near: not depth_zero without at_camera"
    i = near["r32"]["info64"]
    assert bool((i["depth_zero"] & ~i["at_camera"] & ~i["ok0"])[0::2].all()) and bool(near["r64"]["D"][0::2].double().mean() > 0.98)
    for name in NAMES:
        st = stage(name)
        c, s = st["c"], st["s32"]
        assert bool((s["pt_in"] == GR.FMAX).any()) and bool((s["pt_in"] == -GR.FMAX).any()), (name, "+-inf in T pt")
        assert bool(torch.isinf(s["pt"]).any()) and bool((s["pt"][c["P"] * 9:c["P"] * 10] == 0).all()), (name, "pt: overflow and the NaN scrub")
        x1e10 = torch.tensor(1e10, dtype=F32) / float(c["W"] - 1) * 2.0 - 1.0
        assert bool((s["grid_in"][..., 0] == x1e10).any()), (name, "1e10 landing point")
        assert bool(torch.isfinite(s["pt_in"]).all()) and bool(torch.isfinite(st["s64"]["pt_in"]).all())
    for name in NAMES:                                                         # the three kinds, on T pt itself before nan_to_num
        q, t = stage(name)["s32"]["q"], stage(name)["s32"]["pt_in"]
        if name != "backward":                                                 # there no row of T meets +inf and -inf with one sign
            assert bool(torch.isnan(q).any()) and bool((t[torch.isnan(q)] == 0).all()), (name, "NaN in T pt")
        assert bool((q == GR.INF).any()) and bool((t[q == GR.INF] == GR.FMAX).all()), (name, "+inf in T pt")
        assert bool((q == -GR.INF).any()) and bool((t[q == -GR.INF] == -GR.FMAX).all()), (name, "-inf in T pt")
    assert bool((stage("depths")["s32"]["grid"].abs() > 1e8).any()), "depths: no 1e10 in pixel_val"
    assert bool((stage("depths")["r32"]["rec"][..., 6:10].abs() > 3.0).any()), "depths: no start / end far outside"
    rim = stage("rim")["r32"]["rec"]
    assert rim[0, 8, 0:3].tolist() == [0.0, 0.0, 1.0] and rim[0, 8, 6:10].tolist() == [1.0, 0.0, 1.0, 0.0] and float(rim[0, 8, 10]) == 0.0, "rim: grid x is not exactly 1"
    for name in ("on-ctx0", "on-ctx1"):
        assert bool((stage(name)["s64"]["sin2"] < 1e-6).any()), (name, "no parallel sample")
    for name in NAMES:
        uv, c = stage(name)["c"]["uv"], stage(name)["c"]
        assert bool((uv[:, :4] == torch.tensor([[0.0, 0.0], [c["W"] - 1.0, 0.0], [0.0, c["H"] - 1.0], [c["W"] - 1.0, c["H"] - 1.0]])).all())
        assert bool(((uv < 0) | (uv > torch.tensor([c["W"] - 1.0, c["H"] - 1.0]))).any())


# ---- 4. the caps -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_float32_stays_inside_the_caps(name):
    st = stage(name)
    D = st["r64"]["D"]
    und = {"rays": 1.0 - float(D.double().mean())}
    for f in GR.FIELDS:
        und[f] = 1.0 - float(st["s64"]["D_" + f].reshape(D.numel() * st["c"]["P"], -1).all(dim=-1).double().mean())
    print(f"[caps] {name}: undecided " + " ".join(f"{k}={v:.4f}" for k, v in und.items()))
    assert max(und.values()) <= GR.CAP_UNDECIDED, (name, und)
    assert bool(torch.isfinite(st["r32"]["rec"]).all()) and set(st["r32"]["rec"][..., 10].unique().tolist()) <= {0.0, 1.0}
    for f in ("grid", "g", "pt_in", "grid_in", "xenc"):
        assert bool(torch.isfinite(st["s32"][f]).all()), (name, f)
    assert not bool(torch.isnan(st["s32"]["pt"]).any())


@pytest.mark.parametrize("name", NAMES)
def test_float32_ratios_are_what_the_gpu_suite_expects(name):
    """r32 of every output and set, printed (profiles/geometry_parity.md) and held below a ceiling: 1e-6 (four fp32 roundings of the
    summed magnitudes) for every output but pt, 2e-5 for pt, whose bound ignores the second-order terms of its three nested cross
    products.  The GPU tolerance is 8 x max(r32, 2^-22): a summed-magnitude term that is too small would show here as a larger r32.  pt
    also on the samples below sin^2 = 1e-6 alone: nothing is left out of its comparison as parallel."""
    st = stage(name)
    r = {f: GR.ratio(st["r32"]["rec"][..., a:z], st["r64"]["rec"][..., a:z], st["r64"]["M_rec"][..., a:z], st["r64"]["D"][..., None])
         for f, (a, z) in {"d": (0, 3), "m": (3, 6), "start": (6, 8), "end": (8, 10)}.items()}
    for f in GR.FIELDS:
        r[f] = GR.ratio(st["s32"][f], st["s64"][f], st["s64"]["M_" + f], st["s64"]["D_" + f])
    par = st["s64"]["sin2"] < 1e-6
    r["pt_parallel"] = GR.ratio(st["s32"]["pt"], st["s64"]["pt"], st["s64"]["M_pt"], st["s64"]["D_pt"] & par[:, None])
    print(f"[r32] {name}: " + " ".join(f"{k}={v:.2e}" for k, v in r.items()) + f" (sin^2 < 1e-6: {float(par.double().mean()):.4f} of the samples)")
    for k, v in r.items():
        assert v <= GR.R32_CEILING.get(k.split("_parallel")[0], GR.R32_CEILING_OTHER), (name, k, v)
    assert torch.equal(st["r32"]["rec"][..., 10][st["r64"]["D"]].double(), st["r64"]["rec"][..., 10][st["r64"]["D"]])
