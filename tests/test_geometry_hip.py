"""The geometry kernels (csrc/car_geometry.hip over csrc/car_geom.h) through the C ABI against tests/geometry_reference.py: car_pose_setup,
car_ray_setup (both modes), car_sample_setup (both modes), car_project_points, car_exchange_rows and their refusals.

Stage by stage: every entry is fed the fp32 records of the stage before it — the float32 restatement's pose records, its ray records
(geometry_reference.edit_rays applied for the sample stage) — and is judged three ways.

  * bit for bit against the float32 restatement, on EVERY element of every set: every field but the tanhf outputs (g[9..12], xenc).
    test_geometry_reference.py (CPU) holds that restatement bit for bit to the host build of the same header.
  * against float64: ratio = max over the decided elements of |got - fp64| / (summed magnitudes), the float64 run fed the kernel's own
    records of the stage before; the kernel must satisfy ratio <= 8 x max(r32, 2^-22), r32 the float32 restatement's own ratio on that
    output and set — measured against the float64 mode, never against the kernel.  The tanhf outputs are judged this way only.
  * flags and integers exactly on the decided mask: overlaps, pad, row_src and its 1 << 30 bit, g[3..5] == 0, row_pe[3] == 0.

Every output lies inside a larger NaN-filled buffer whose margins must come back untouched.  Every test prints ratio / tolerance as a
``[parity]`` line (profiles/geometry_parity.md)."""
import functools

import pytest
import torch

import abi_harness as abi
import geometry_reference as GR
from abi_harness import CAR_E_ARG, Guarded
from geometry_reference import F32, F64
from parity_rule import judge

pytestmark = pytest.mark.gpu

NAMES = tuple(GR.SETS)


def _d(t):
    return t.contiguous().to(abi.dev())


def _same(got, want, what):
    d = abi.bits(got) != abi.bits(want.reshape(got.shape).to(got.dtype))
    assert not bool(d.any()), f"{what}: {int(d.sum())} of {d.numel()} floats differ from the float32 restatement, first at {d.nonzero()[0].tolist()}"


def _judge(test, name, got, yard):
    """got, yard: {field: ratio}, taken with geometry_reference.ratio on the decided elements."""
    judge(test, name, {k: (rk, yard[k]) for k, rk in got.items()}, what="r32")


# ---- launches ------------------------------------------------------------------------------------------------------------------------------
def run_poses(c):
    lib = abi.lib()
    out = Guarded((c["b"] * c["V"], GR.POSE_FLOATS))
    keep = [_d(c[k]) for k in ("c2w_ctx", "c2w_q", "K_ctx", "K_q")]
    rc = lib.car_pose_setup(*[abi.ptr(t) for t in keep], c["b"], c["V"], c["H"], out.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return out.get("poses")


def run_rays(c, P32, pad_phi=5, coords=True, phi=True):
    lib = abi.lib()
    n, R, V = c["b"] * c["V"], c["R"], c["V"]
    ld = 9 * V + pad_phi
    out = {"rays": Guarded((n, R, 12)), "coords9": Guarded((n, R, 9)), "phi_x": Guarded((c["b"], R, ld))}
    keep = [_d(P32), _d(c["uv"]), _d(c["steps"])]
    rc = lib.car_ray_setup(abi.ptr(keep[0]), abi.ptr(keep[1]), c["b"], V, R, c["H"], c["W"], c["P"], c["no_sample"], abi.ptr(keep[2]), out["rays"].ptr,
                           out["coords9"].ptr if coords else None, out["phi_x"].ptr if phi else None, ld, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return {k: v.get(k) for k, v in out.items()}


OPTIONAL = ("pixel_val", "pt", "g", "grid_in", "xenc", "pt_in")


def run_samples(c, P32, R32, col=2, tail=3, skip=()):
    """One launch of car_sample_setup; xenc's window starts at column `col` of rows `col + width + tail` wide.  `skip`: outputs given as NULL."""
    lib = abi.lib()
    b, V, R, P = c["b"], c["V"], c["R"], c["P"]
    S = b * V * R * P
    width = 6 if V == 1 else 3
    ld = col + width + tail
    out = {"pixel_val": Guarded((S, 2)), "pt": Guarded((S, 3)), "g": Guarded((S, 16)), "grid_in": Guarded((S, V, 2)),
           "xenc": Guarded((S if V == 1 else S * V, ld)), "pt_in": Guarded((S, V, 3))}
    p = {k: (None if k in skip else v.ptr) for k, v in out.items()}
    keep = [_d(P32), _d(R32), _d(c["steps"])]
    rc = lib.car_sample_setup(abi.ptr(keep[0]), abi.ptr(keep[1]), abi.ptr(keep[2]), b, V, R, P, c["H"], c["W"], c["no_sample"], p["pixel_val"], p["pt"], p["g"],
                              p["grid_in"], p["xenc"], ld, col, p["pt_in"], abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    got = {k: v.get(k) for k, v in out.items()}
    got["grid"] = got["pixel_val"]
    return got, (col, width, ld)


def _xenc_window(got, V, col, width):
    x = got["xenc"][:, col:col + width]
    return x if V == 1 else x.reshape(-1, V, 3)


# ---- 1. poses ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + ("pose-65",))
def test_pose_kernel(name):
    """All 96 floats of every record: bit for bit the float32 restatement (car_inverse4's Gauss-Jordan in double, the FMA-chain products,
    k01 = K / H on both rows, T[s] zero for s >= V, the pad zero); the 89 used floats against torch.linalg.inv and fp64 products, relative
    to |inv| |c2w| summed.  pose-65: b = 65 (the launch with 64-thread blocks: a second block with one live thread), V = 3, translations
    of 1e3, one mildly non-orthonormal scene."""
    c = GR.pose_set() if name == "pose-65" else GR.cameras(name)
    got = run_poses(c)
    args = (c["c2w_ctx"], c["c2w_q"], c["K_ctx"], c["K_q"], c["H"])
    f32, f64 = GR.poses(*args, dtype=F32), GR.poses(*args, dtype=F64)
    _same(got, f32["rec"], f"{name} CarPose")
    V = c["V"]
    assert bool((got[:, GR.PAD:] == 0).all()) and bool((got[:, GR.T0 + 12 * V:GR.KC] == 0).all())
    fields = {"q_rel": (0, 12), "c_rel": (12, 24), "T": (24, 24 + 12 * V), "kc": (60, 64), "k01": (64, 73), "kq": (73, 77), "inv_q": (77, 89)}
    _judge("poses", name, {k: GR.ratio(got[:, a:z], f64["rec"][:, a:z], f64["M_rec"][:, a:z]) for k, (a, z) in fields.items()},
           {k: GR.ratio(f32["rec"][:, a:z], f64["rec"][:, a:z], f64["M_rec"][:, a:z]) for k, (a, z) in fields.items()})


# ---- 2. rays -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rays_of(name):
    st = GR.stage(name)
    return run_rays(st["c"], st["P32"])


@pytest.mark.parametrize("name", NAMES)
def test_ray_kernel(name):
    """car_ray_setup, the default mode and (set `depths`) no_sample = 1 with depths at, behind and infinitely far from the camera plane:
    all twelve floats of every record bit for bit; d, m, start, end against float64 on the decided rays, overlaps and pad exactly."""
    st = GR.stage(name)
    c = st["c"]
    got = _rays_of(name)["rays"]
    for f, (a, z) in dict(GR.RAY_FIELDS, overlaps=(10, 11), pad=(11, 12)).items():
        _same(got[..., a:z], st["r32"]["rec"][..., a:z], f"{name} CarRay.{f}")
    r64 = GR.rays(st["P32"], c["uv"], c["b"], c["V"], c["R"], c["H"], c["W"], c["no_sample"], c["steps"], dtype=F64, d32=got[..., 0:3])
    D = r64["D"]
    assert 1.0 - float(D.double().mean()) <= GR.CAP_UNDECIDED
    assert bool(torch.isfinite(got).all()) and set(got[..., 10].unique().tolist()) <= {0.0, 1.0} and bool((got[..., 11] == 0).all())
    assert torch.equal(got[..., 10][D].double(), r64["rec"][..., 10][D]), "overlaps"
    _judge("rays", name, GR.ray_ratios(got, r64), GR.ray_ratios(st["r32"]["rec"], st["r64"]))


@pytest.mark.parametrize("name", ("wide", "v1", "v3", "depths"))
def test_ray_kernel_layout(name):
    """coords9 [n, R, 9] and phi_x [b, R, ld_phi] (ld_phi = 9 V + 5: view v's nine floats at column 9 v) carry [d, m, o] with the ray
    record's own bits, the padding columns untouched; with either or both given as NULL the records are the same bit for bit."""
    st = GR.stage(name)
    c, V = st["c"], st["c"]["V"]
    out = _rays_of(name)
    want = GR.coords9(out["rays"], st["P32"], V)
    _same(out["coords9"], want, "coords9")
    phi = out["phi_x"]
    _same(phi[..., :9 * V], want.reshape(c["b"], V, c["R"], 9).permute(0, 2, 1, 3).reshape(c["b"], c["R"], 9 * V), "phi_x")
    assert bool(torch.isnan(phi[..., 9 * V:]).all()), "phi_x: padding written"
    for coords, ph in ((False, True), (True, False), (False, False)):
        o2 = run_rays(c, st["P32"], coords=coords, phi=ph)
        assert torch.equal(abi.bits(o2["rays"]), abi.bits(out["rays"]))
        assert torch.equal(abi.bits(o2["coords9"]), abi.bits(out["coords9"])) if coords else bool(torch.isnan(o2["coords9"]).all())
        assert torch.equal(abi.bits(o2["phi_x"]), abi.bits(out["phi_x"])) if ph else bool(torch.isnan(o2["phi_x"]).all())
    tight = run_rays(c, st["P32"], pad_phi=0)
    assert torch.equal(abi.bits(tight["phi_x"]), abi.bits(phi[..., :9 * V]))


# ---- 3. samples ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _samples_of(name):
    st = GR.stage(name)
    return run_samples(st["c"], st["P32"], st["R32"])


@pytest.mark.parametrize("name", NAMES)
def test_sample_kernel(name):
    """car_sample_setup (no_sample = 1 for `depths`) on ray records that hold a NaN moment and moments of +-3e38: pixel_val, pt, g (but
    g[9..12]), pt_in and grid_in bit for bit; every output against float64 on its decided elements, pt from the kernel's own pixel_val,
    pt_in / grid_in / g / xenc from the kernel's own pt; g[3..5] == 0; xenc's window (6 wide for V = 1, 3 per view otherwise) at column 2
    of wider rows, the other columns untouched."""
    st = GR.stage(name)
    c, f32 = st["c"], st["s32"]
    got, (col, width, ld) = _samples_of(name)
    for f in ("grid", "pt", "pt_in", "grid_in"):
        _same(got[f], f32[f], f"{name} {f}")
    tanh = torch.zeros(16, dtype=torch.bool)
    tanh[9:13] = True
    _same(got["g"][:, ~tanh], f32["g"][:, ~tanh], f"{name} g")
    assert bool((got["g"][:, 3:6] == 0).all())
    keep = torch.ones(ld, dtype=torch.bool)
    keep[col:col + width] = False
    assert bool(torch.isnan(got["xenc"][:, keep]).all()), "xenc: wrote outside its window"
    got = dict(got, xenc=_xenc_window(got, c["V"], col, width))
    for f in ("grid", "g", "pt_in", "grid_in", "xenc"):
        assert bool(torch.isfinite(got[f]).all()), (name, f)
    s64 = GR.samples(st["P32"], st["R32"], c["steps"], c["b"], c["V"], c["R"], c["P"], c["H"], c["W"], c["no_sample"], dtype=F64, grid32=got["grid"],
                     pt32=got["pt"])
    for f in GR.FIELDS:
        assert 1.0 - float(s64["D_" + f].reshape(got["grid"].shape[0], -1).all(dim=-1).double().mean()) <= GR.CAP_UNDECIDED, (name, f)
    _judge("samples", name, GR.sample_ratios(got, s64), GR.sample_ratios(f32, st["s64"]))


@pytest.mark.parametrize("name", ("wide", "v1", "v3", "depths"))
def test_sample_kernel_null_outputs(name):
    """Every optional output given as NULL in turn: it stays untouched, the others are the same bit for bit.  xenc at column 0 of rows
    exactly as wide as the window is the same window."""
    st = GR.stage(name)
    c = st["c"]
    full, (col, width, ld) = _samples_of(name)
    for skip in OPTIONAL:
        got, _ = run_samples(c, st["P32"], st["R32"], skip=(skip,))
        for k in OPTIONAL:
            if k == skip:
                assert bool(torch.isnan(got[k]).all()), f"{k} written though NULL"
            else:
                assert torch.equal(abi.bits(got[k]), abi.bits(full[k])), f"{k} changed when {skip} is NULL"
    tight, _ = run_samples(c, st["P32"], st["R32"], col=0, tail=0)
    assert torch.equal(abi.bits(tight["xenc"]), abi.bits(full["xenc"][:, col:col + width]))


# ---- 4. car_project_points, car_exchange_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", (0, 1))
def test_project_points_kernel(view):
    """Two scenes whose two views have different intrinsics (fx != fy, the principal point off centre, H != W): points in front of, on
    (z = -1e-12f: zz exactly 0), and behind the camera plane, +-inf and NaN coordinates."""
    lib = abi.lib()
    st = GR.stage("wide")
    c, pts = st["c"], GR.project_inputs()
    npts = pts.shape[1]
    out = Guarded((2, npts, 2))
    keep = [_d(st["P32"]), _d(pts)]
    rc = lib.car_project_points(abi.ptr(keep[0]), abi.ptr(keep[1]), 2, npts, c["V"], view, c["H"], c["W"], out.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    got = out.get("grid")
    f32 = GR.project_points(st["P32"], pts, 2, c["V"], view, c["H"], c["W"], dtype=F32)
    f64 = GR.project_points(st["P32"], pts, 2, c["V"], view, c["H"], c["W"], dtype=F64)
    _same(got, f32["grid"], "grid")
    assert bool(torch.isfinite(got).all()) and bool((got.abs() > 1e8).any())
    _judge("project_points", f"view{view}", {"grid": GR.ratio(got, f64["grid"], f64["M_grid"], f64["D_grid"])},
           {"grid": GR.ratio(f32["grid"], f64["grid"], f64["M_grid"], f64["D_grid"])})


@pytest.mark.parametrize("V", (2, 3))
def test_exchange_rows_kernel(V):
    """row_src (the view and its 1 << 30 flag) exactly; row_grid bit for bit and against float64 (component 0: the sample's own pixel_val
    bits); row_pe the point encoding's bits with the fourth float 0 whatever ptenc holds there (NaN here)."""
    lib = abi.lib()
    st = GR.stage("v3" if V == 3 else "wide")
    c = st["c"]
    pv, pin, pe = GR.exchange_inputs(V)
    pts = pv.shape[0] // (2 * V)
    rows = 2 * V * pts * V
    src, grid, rpe = Guarded((rows,), dtype=torch.int32), Guarded((rows, 2)), Guarded((rows, 4))
    keep = [_d(st["P32"]), _d(pv), _d(pin), _d(pe)]
    rc = lib.car_exchange_rows(*[abi.ptr(t) for t in keep], 2, V, pts, c["H"], c["W"], src.ptr, grid.ptr, rpe.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    f32 = GR.exchange_rows(st["P32"], pv, pin, pe, 2, V, pts, c["H"], c["W"], dtype=F32)
    f64 = GR.exchange_rows(st["P32"], pv, pin, pe, 2, V, pts, c["H"], c["W"], dtype=F64)
    got_src, got_grid, got_pe = src.get("row_src"), grid.get("row_grid"), rpe.get("row_pe")
    assert torch.equal(got_src, f32["row_src"]), "row_src"
    assert torch.equal(got_src >> 30, (torch.arange(rows) % V != 0).int())
    _same(got_grid, f32["row_grid"], "row_grid")
    _same(got_pe, f32["row_pe"], "row_pe")
    assert bool((got_pe[:, 3] == 0).all())
    _judge("exchange_rows", f"V{V}", {"row_grid": GR.ratio(got_grid, f64["row_grid"], f64["M_row_grid"], f64["D_row_grid"])},
           {"row_grid": GR.ratio(f32["row_grid"], f64["row_grid"], f64["M_row_grid"], f64["D_row_grid"])})


# ---- 5. the two pose routes against a float64 chain: a measurement, not an assertion -----------------------------------------------------------
@pytest.mark.parametrize("name", ("t1_c1_diverging", "t2_c2"))
def test_pose_routes_against_the_float64_chain(name):
    """cameras -> poses -> rays -> pixel_val -> pt once in float64 throughout (nothing rounded to fp32 on the way), and the same chain
    through the kernels from car_pose_setup's records and from poses.pack_poses' records (fp32 LAPACK inverse and matmul).  Printed for
    profiles/geometry_parity.md: how far each route's pose records (in units of 2^-24 x |inv| |c2w|) and closest points land from it."""
    import cases as C
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.poses import pack_poses
    k = C.case_config(name)
    uv = C.select_rays(k["H"], k["rays"])
    inp = S.stereo_scene(k["H"], b=k["b"], alpha=k["alpha"], baseline=k["baseline"], yaw_deg=k["yaw_deg"], uv=uv, seed=k["scene_seed"], n_view=k["n_view"])
    c = dict(b=k["b"], V=k["n_view"], R=uv.shape[0], P=k["P"], H=k["H"], W=k["H"], no_sample=0, c2w_ctx=inp["context"]["cam2world"],
             c2w_q=inp["query"]["cam2world"], K_ctx=inp["context"]["intrinsics"], K_q=inp["query"]["intrinsics"],
             uv=inp["query"]["uv"][:, 0].contiguous(), steps=torch.linspace(0, 1, k["P"]))
    p64 = GR.poses(c["c2w_ctx"], c["c2w_q"], c["K_ctx"], c["K_q"], c["H"], dtype=F64)
    r64 = GR.rays(p64["rec"], c["uv"], c["b"], c["V"], c["R"], c["H"], c["W"], dtype=F64)
    s64 = GR.samples(p64["rec"], r64["rec"], c["steps"], c["b"], c["V"], c["R"], c["P"], c["H"], c["W"], dtype=F64)
    for route, P32 in (("car_pose_setup", run_poses(c)), ("pack_poses", pack_poses(inp, c["H"]))):
        rays = run_rays(c, P32)["rays"]
        pt = run_samples(c, P32, rays)[0]["pt"]
        rec = GR.ratio(P32[:, :89], p64["rec"][:, :89], p64["M_rec"][:, :89]) * 2.0 ** 24
        err = ((pt.double() - s64["pt"]).abs() / s64["pt"].abs().clamp_min(1.0)).amax(dim=-1)
        print(f"[parity] pose_routes {name} {route}: records {rec:.2f} x 2^-24; pt beyond 1e-4: {float((err > 1e-4).double().mean()):.4f}, "
              f"median {float(err.median()):.2e}, worst {float(err.max()):.2e}")
        assert bool(torch.isfinite(pt).all())


# ---- 6. refusals: all return before any launch ---------------------------------------------------------------------------------------------------
def _refused(fn, args, outs):
    assert fn(*args, abi.stream()) == CAR_E_ARG, (fn.__name__, args)
    assert abi.lib().car_last_error()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)


def _edit(args, field, value):
    args = dict(args)
    args[field] = value
    return list(args.values())


@pytest.mark.parametrize("field,value", [(k, None) for k in ("c2w_ctx", "c2w_q", "K_ctx", "K_q", "poses")] + [("b", 0), ("b", -1), ("V", 0), ("V", 4), ("H", 0)],
                         ids=str)
def test_pose_setup_refusals(field, value):
    c = GR.cameras("square")
    out = Guarded((4, 96))
    keep = {k: _d(c[k]) for k in ("c2w_ctx", "c2w_q", "K_ctx", "K_q")}
    args = dict({k: abi.ptr(t) for k, t in keep.items()}, b=2, V=2, H=16, poses=out.ptr)
    _refused(abi.lib().car_pose_setup, _edit(args, field, value), [out])


@pytest.mark.parametrize("field,value", [(k, None) for k in ("poses", "uv", "rays")] +
                         [("b", 0), ("V", 0), ("V", 4), ("R", 0), ("H", 1), ("W", 1), ("P", 0), ("no_sample+steps", None), ("ld_phi", 17), ("ld_phi", 0)], ids=str)
def test_ray_setup_refusals(field, value):
    """Null inputs and records; non-positive sizes, V above 3, H or W of 1; no_sample without depth_steps; phi_x with ld_phi below 9 V."""
    st = GR.stage("square")
    c = st["c"]
    outs = {"rays": Guarded((4, c["R"], 12)), "coords9": Guarded((4, c["R"], 9)), "phi_x": Guarded((2, c["R"], 18))}
    keep = [_d(st["P32"]), _d(c["uv"]), _d(c["steps"])]
    args = dict(poses=abi.ptr(keep[0]), uv=abi.ptr(keep[1]), b=2, V=2, R=c["R"], H=16, W=16, P=c["P"], no_sample=0, steps=abi.ptr(keep[2]), rays=outs["rays"].ptr,
                coords9=outs["coords9"].ptr, phi_x=outs["phi_x"].ptr, ld_phi=18)
    if field == "no_sample+steps":
        args["no_sample"], field = 1, "steps"
    _refused(abi.lib().car_ray_setup, _edit(args, field, value), outs.values())


@pytest.mark.parametrize("V,field,value", [(2, k, None) for k in ("poses", "rays", "steps")] +
                         [(2, "b", 0), (2, "V", 0), (2, "V", 4), (2, "R", 0), (2, "P", 0), (2, "H", 1), (2, "W", 1), (2, "ld_xenc", 4), (2, "col_xenc", -1),
                          (1, "ld_xenc", 7)], ids=str)
def test_sample_setup_refusals(V, field, value):
    """Null inputs; non-positive sizes, V above 3, H or W of 1; an xenc window that does not fit its row (3 wide at column 2 of 4; 6 wide
    for V = 1 at column 2 of 7) or starts before it."""
    st = GR.stage("square" if V == 2 else "v1")
    c = st["c"]
    S = c["b"] * V * c["R"] * c["P"]
    outs = {"pixel_val": Guarded((S, 2)), "pt": Guarded((S, 3)), "g": Guarded((S, 16)), "grid_in": Guarded((S, V, 2)), "xenc": Guarded((S * V, 8)), "pt_in": Guarded((S, V, 3))}
    keep = [_d(st["P32"]), _d(st["R32"]), _d(c["steps"])]
    args = dict(poses=abi.ptr(keep[0]), rays=abi.ptr(keep[1]), steps=abi.ptr(keep[2]), b=c["b"], V=V, R=c["R"], P=c["P"], H=16, W=16, no_sample=0,
                pixel_val=outs["pixel_val"].ptr, pt=outs["pt"].ptr, g=outs["g"].ptr, grid_in=outs["grid_in"].ptr, xenc=outs["xenc"].ptr, ld_xenc=8, col_xenc=2,
                pt_in=outs["pt_in"].ptr)
    _refused(abi.lib().car_sample_setup, _edit(args, field, value), outs.values())


@pytest.mark.parametrize("field,value", [(k, None) for k in ("poses", "pts", "grid")] +
                         [("n_scenes", 0), ("npts", 0), ("V", 0), ("view", -1), ("view", 2), ("H", 1), ("W", 1)], ids=str)
def test_project_points_refusals(field, value):
    st = GR.stage("wide")
    pts = GR.project_inputs()
    out = Guarded((2, pts.shape[1], 2))
    keep = [_d(st["P32"]), _d(pts)]
    args = dict(poses=abi.ptr(keep[0]), pts=abi.ptr(keep[1]), n_scenes=2, npts=pts.shape[1], V=2, view=0, H=12, W=20, grid=out.ptr)
    _refused(abi.lib().car_project_points, _edit(args, field, value), [out])


@pytest.mark.parametrize("field,value", [(k, None) for k in ("poses", "pixel_val", "pt_in", "ptenc", "row_src", "row_grid", "row_pe")] +
                         [("n_scenes", 0), ("V", 1), ("V", 4), ("pts", 0), ("H", 1), ("W", 1)], ids=str)
def test_exchange_rows_refusals(field, value):
    st = GR.stage("wide")
    pv, pin, pe = GR.exchange_inputs(2)
    pts = pv.shape[0] // 4
    rows = 2 * 2 * pts * 2
    outs = [Guarded((rows,), dtype=torch.int32), Guarded((rows, 2)), Guarded((rows, 4))]
    keep = [_d(st["P32"]), _d(pv), _d(pin), _d(pe)]
    args = dict(poses=abi.ptr(keep[0]), pixel_val=abi.ptr(keep[1]), pt_in=abi.ptr(keep[2]), ptenc=abi.ptr(keep[3]), n_scenes=2, V=2, pts=pts, H=12, W=20,
                row_src=outs[0].ptr, row_grid=outs[1].ptr, row_pe=outs[2].ptr)
    _refused(abi.lib().car_exchange_rows, _edit(args, field, value), outs)
