"""The fused per-sample kernel (csrc/car_fused.hip) through the C ABI against tests/fused_reference.py: car_fused_samples,
car_fused_samples_parts, car_fused_samples_f16, car_fused_rows and their refusals.

Per case: car_pose_setup / pack_poses -> car_ray_setup -> (edits of a few ray records: fused_reference.patch_rays) -> car_sample_setup
for the records the restatement needs; car_fused_pack for blob / bias / wpt; a seeded lattice whose four (view, mode) maps of a pair all
differ, its zeros-mode ring zero, gmeta its true maximum.  test_fused_reference.py (CPU) asserts that these input sets hold the edges.

Tolerance, measured against the reference and never against the kernel: ratio = max |got - fp64| / (sum of magnitudes, float64); the
same ratio is computed for the restatement run in float32 on the CPU on the same inputs (for the fp16 instance: for the CPU emulation of
one-product fp16 arithmetic), and the kernel must satisfy  ratio_kernel <= 8 x max(ratio_yardstick, 2^-22).  `part` is compared with the
restatement fed the kernel's OWN e and logit, relative to sum_j exp(.) |e_j|.  Every test prints ratio_kernel / tolerance as a
``[parity]`` line (profiles/fused_parity.md).  Every output lies inside a larger NaN-filled buffer whose margins must come back
untouched; pixel_val, pt and g must equal car_sample_setup's bit for bit."""
import ctypes
import functools

import pytest
import torch

import abi_harness as abi
import fused_reference as FR
from abi_harness import CAR_E_ARG, NAN, Guarded
from parity_rule import judge

pytestmark = pytest.mark.gpu


def _L():
    from cross_attention_renderer_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _fused_lib():
    L, lib = _L(), abi.lib()
    f16 = lib.car_fused_samples_f16                       # declared in csrc/car_common.h, reached by the engine through car_render_forward_f16 only
    f16.restype = ctypes.c_int
    f16.argtypes = L.SIGNATURES["car_fused_samples_parts"][1]
    lib.car_fused_blob16_floats.restype = ctypes.c_size_t
    return lib


# ---- setup ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed(kind):
    """(params, blob, bias, wpt, CarWeights, the tensors it points into) of a weight set, packed once by car_fused_pack."""
    L, lib = _L(), _fused_lib()
    params = FR.weights(kind)
    w, keep = L.CarWeights(), []
    for n in FR.SHAPES:
        for k, suffix in (("weight", "w"), ("bias", "b")):
            t = params[f"{n}.{k}"].float().contiguous().to(abi.dev())
            keep.append(t)
            setattr(w, f"{n}_{suffix}", t.data_ptr())
    blob = torch.full((lib.car_fused_blob_floats(),), NAN, device=abi.dev())
    bias = torch.full((lib.car_fused_bias_floats(),), NAN, device=abi.dev())
    wpt = torch.full((FR.C * 4,), NAN, device=abi.dev())
    rc = lib.car_fused_pack(ctypes.byref(w), abi.ptr(blob), abi.ptr(bias), abi.ptr(wpt), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return params, blob, bias, wpt, w, keep


@functools.lru_cache(maxsize=None)
def _plan16(kind):
    """blob16 | bias | wpt of the fp16 instance: car_plan_f16_build's plan (compact blob, bias table, point table, each rounded up to 64
    floats: csrc/car_render.hip plan16_layout, as tests/test_fused_pack.py restates it)."""
    L, lib = _L(), _fused_lib()
    w = _packed(kind)[4]
    up64 = lambda n: (n + 63) & ~63
    dims = L.CarDims()
    dims.b, dims.V, dims.R, dims.P, dims.H, dims.W, dims.n_levels, dims.repeat_attention = 1, 2, 64, 8, 64, 64, 3, 1
    for l, (c, h) in enumerate(((256, 16), (256, 32), (64, 64))):
        dims.level_c[l], dims.level_h[l], dims.level_w[l] = c, h, h
    n16 = lib.car_plan_f16_bytes(ctypes.byref(dims)) // 4
    o_bias = up64(lib.car_fused_blob16_floats())
    o_wpt = o_bias + up64(lib.car_fused_bias_floats())
    assert n16 == o_wpt + up64(FR.C * 4), "car_plan_f16_build's layout changed"
    p16 = torch.zeros(n16, device=abi.dev())
    rc = lib.car_plan_f16_build(ctypes.byref(dims), ctypes.byref(w), abi.ptr(p16), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return p16, p16[:o_bias], p16[o_bias:o_wpt], p16[o_wpt:]


class Setup:
    """Poses, rays, steps and the sample records of a case on the device; the records also on the host."""

    def __init__(self, c, rays_edit=FR.patch_rays, device_poses=False):
        from cross_attention_renderer_amd.poses import pack_poses
        lib, dev, st = _fused_lib(), abi.dev(), abi.stream()
        self.c = c
        b, R, P, H, W = c["b"], c["R"], c["P"], c["H"], c["W"]
        self.n_sets, self.S = 2 * b, 2 * b * R * P
        inp, uv, steps = FR.scene(c)
        if device_poses:
            f = lambda t: t.float().contiguous().to(dev)
            cc, cq, kc, kq = f(inp["context"]["cam2world"]), f(inp["query"]["cam2world"]), f(inp["context"]["intrinsics"]), f(inp["query"]["intrinsics"])
            self.poses = torch.empty(2 * b, 96, device=dev)
            assert lib.car_pose_setup(abi.ptr(cc), abi.ptr(cq), abi.ptr(kc), abi.ptr(kq), b, 2, H, abi.ptr(self.poses), st) == 0, lib.car_last_error()
        else:
            self.poses = pack_poses(inp, H).contiguous().to(dev)
        self.steps = steps.to(dev)
        uvd = inp["query"]["uv"].float().contiguous().to(dev)
        self.rays = torch.empty(2 * b, R, 12, device=dev)
        rc = lib.car_ray_setup(abi.ptr(self.poses), abi.ptr(uvd), b, 2, R, H, W, P, c["no_sample"], abi.ptr(self.steps), abi.ptr(self.rays), None, None, 0, st)
        assert rc == 0, lib.car_last_error()
        rays_edit(self.rays)
        S = self.S
        pv, pt, g = torch.empty(S, 2, device=dev), torch.empty(S, 3, device=dev), torch.empty(S, 16, device=dev)
        gi, pi = torch.empty(S, 2, 2, device=dev), torch.empty(S, 2, 3, device=dev)
        rc = lib.car_sample_setup(abi.ptr(self.poses), abi.ptr(self.rays), abi.ptr(self.steps), b, 2, R, P, H, W, c["no_sample"], abi.ptr(pv), abi.ptr(pt), abi.ptr(g),
                                  abi.ptr(gi), None, 0, 0, abi.ptr(pi), st)
        assert rc == 0, lib.car_last_error()
        torch.cuda.synchronize()
        self.rec = {"grid": pv.cpu(), "pt": pt.cpu(), "g": g.cpu(), "grid_in": gi.cpu(), "pt_in": pi.cpu()}


def _lattice_dev(lat):
    d = lat.contiguous().to(abi.dev())
    return d, lat.abs().max().reshape(1).float().to(abi.dev())


def run_samples(su, lat, gmeta, wpt, blob, bias, entry="parts", dims=None):
    """One launch of car_fused_samples / _parts / _f16 into guarded buffers: dict of host tensors."""
    lib, c = _fused_lib(), su.c
    S, R, P = su.S, c["R"], c["P"]
    pgs = -(-P // lib.car_fused_tile_steps())
    out = {"e": Guarded((S, FR.C)), "g": Guarded((S, 16)), "logit": Guarded((S,)), "pt": Guarded((S, 3)), "pixel_val": Guarded((S, 2))}
    lh, lw = lat.shape[2:4]
    args = [abi.ptr(su.poses), abi.ptr(su.rays), abi.ptr(su.steps), abi.ptr(lat), lh, lw, c["pad"], abi.ptr(gmeta), abi.ptr(wpt), abi.ptr(blob), abi.ptr(bias), c["b"], 2, R, P,
            c["H"], c["W"], c["no_sample"], out["e"].ptr, out["g"].ptr, out["logit"].ptr, out["pt"].ptr, out["pixel_val"].ptr]
    if entry == "plain":
        rc = lib.car_fused_samples(*args, abi.stream())
    else:
        out["part"] = Guarded((su.n_sets, R, pgs, FR.C))
        rc = (lib.car_fused_samples_parts if entry == "parts" else lib.car_fused_samples_f16)(*args, out["part"].ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return {k: v.get(k) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _case(tag):
    """Setup, lattice (host, device, gmeta), float64 and float32 restatement of a case of fused_reference.CASES: made once, shared."""
    c = FR.CASES[tag]
    su = Setup(c, device_poses=tag == "edge-24-8-3")
    lat = FR.case_lattice(c)
    params = _packed(c["wts"])[0]
    ref = FR.samples(params, lat, c["pad"], su.rec, su.n_sets)
    f32 = FR.samples(params, lat, c["pad"], su.rec, su.n_sets, dtype=torch.float32)
    return su, lat, _lattice_dev(lat), ref, f32


def _judge(test, case, got, ref, yard, keys=("e", "logit"), what="fp32"):
    """Every output finite and held to the yardstick run's own ratio against the same float64 run and bound."""
    judge(test, case, {k: ((got[k], ref[k], ref["B_" + k]), FR.ratio(yard[k], ref[k], ref["B_" + k])) for k in keys}, what=what, finite=True)


def _judge_part(test, case, got, su):
    c = su.c
    want, mag = FR.part(got["e"], got["logit"], su.n_sets, c["R"], c["P"], _fused_lib().car_fused_tile_steps())
    y32, _ = FR.part(got["e"], got["logit"], su.n_sets, c["R"], c["P"], _fused_lib().car_fused_tile_steps(), dtype=torch.float32)
    _judge(test, case, {"part": got["part"]}, {"part": want, "B_part": mag}, {"part": y32}, keys=("part",))


def _geometry_equals_sample_setup(got, su):
    for k, r in (("pixel_val", "grid"), ("pt", "pt"), ("g", "g")):
        assert torch.equal(abi.bits(got[k]), abi.bits(su.rec[r].reshape(got[k].shape))), f"{k} differs from car_sample_setup's"


def _check(test, tag):
    su, lat, (dlat, gmeta), ref, f32 = _case(tag)
    _, blob, bias, wpt, _, _ = _packed(su.c["wts"])
    got = run_samples(su, dlat, gmeta, wpt, blob, bias, "parts")
    _geometry_equals_sample_setup(got, su)
    _judge(test, tag, got, ref, f32)
    _judge_part(test, tag, got, su)
    return su, ref, got, (dlat, gmeta, wpt, blob, bias)


# ---- 1. tile edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FR.TILE_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_fused_samples_match_fp64_at_the_tile_edges(shape):
    """(R, P, b): 2, 2, 2, 8, 16, 18 and 6 workgroups — the XCD band permutation with fewer than 8 groups, a multiple of 8 and a
    remainder; one-live-row tiles and clamped duplicates in both directions; (24, 8, 3) with the library's own pose records.  The
    launch without `part` gives the same e, g, logit, pt and pixel_val bit for bit."""
    tag = "edge-" + "-".join(map(str, shape))
    su, ref, got, (dlat, gmeta, wpt, blob, bias) = _check("tile_edges", tag)
    plain = run_samples(su, dlat, gmeta, wpt, blob, bias, "plain")
    for k in ("e", "g", "logit", "pt", "pixel_val"):
        assert torch.equal(abi.bits(plain[k]), abi.bits(got[k])), f"{k}: car_fused_samples differs from car_fused_samples_parts"


# ---- 2. geometry variants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("ctx0", "depths", "wide"))
def test_fused_samples_match_fp64_on_other_geometries(tag):
    """The query camera on context camera 0; no_sample = 1 with `steps` holding depths; H != W with a 6 x 10 finest level at pad 5
    (21 x 29 nodes)."""
    _check("geometry", tag)


# ---- 3. magnitudes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [t for t in FR.CASES if t.startswith("mag-")])
def test_fused_samples_match_fp64_across_magnitudes(tag):
    """Lattice x 1e-4 / x 1e4 (nothing compensated: the metric is relative); a dozen 1e5 outliers; all-zero lattice, point weights and
    bias (hp from the 1e-30 clamp); the ReLU-fed layers x 1e-4 / x 1e4 with their consumers the inverse; all-zero W2; key_map.bias = -1e3
    (logit = u^T x + c from the fold alone); query_embed.bias = -1e3 (logit = r^T v + c)."""
    su, ref, got, _ = _check("magnitudes", tag)
    if tag == "mag-allzero":
        assert torch.equal(got["e"], _packed("nopoint")[0]["query_encode_latent_2.bias"].repeat(2).expand(su.S, -1))
    if tag == "mag-w2zero":
        assert torch.equal(got["e"], _packed("w2zero")[0]["query_encode_latent_2.bias"].repeat(2).expand(su.S, -1))


# ---- 4. exact integers ---------------------------------------------------------------------------------------------------------------------
def test_fused_samples_integer_case_is_bit_exact_in_e():
    """Tap weights of exactly 1/4, lattice values multiples of 4, integer biases, W2 of two +-1 per row: e must equal the float64 result
    bit for bit (h and e only: test_fused_reference.py says why the closing layers cannot be joined)."""
    c = FR.INT_CASE
    su = Setup(c, rays_edit=lambda r: FR.integer_rays(r, c))
    lat = FR.integer_lattice(c)
    params, blob, bias, wpt, _, _ = _packed("int")
    ref = FR.samples(params, lat, c["pad"], su.rec, su.n_sets)
    dlat, gmeta = _lattice_dev(lat)
    got = run_samples(su, dlat, gmeta, wpt, blob, bias, "parts")
    _geometry_equals_sample_setup(got, su)
    assert bool((ref["e"] == ref["e"].round()).all())
    bad = (got["e"].double() != ref["e"]).sum().item()
    print(f"[parity] integers: {bad} of {ref['e'].numel()} entries of e differ")
    assert bad == 0
    assert bool(torch.isfinite(got["logit"]).all())


# ---- 5. the rows instance ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed_rows():
    lib = _fused_lib()
    params, _, _, _, w, _ = _packed("gauss")
    blob = torch.zeros(lib.car_fused_blob_floats(), device=abi.dev())
    bias = torch.zeros(lib.car_fused_bias_floats(), device=abi.dev())
    wpt = torch.zeros(FR.C * 4, device=abi.dev())
    rc = lib.car_fused_pack_rows(w.query_encode_latent_w, w.query_encode_latent_b, w.query_encode_latent_2_w, w.query_encode_latent_2_b, abi.ptr(blob),
                                 abi.ptr(bias), abi.ptr(wpt), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return params, blob, bias, wpt


@pytest.mark.parametrize("tag", list(FR.ROWS_CASES))
def test_fused_rows_match_fp64(tag):
    """car_fused_rows over explicit rows, ncomp 1 and 3, ragged and whole tiles; every (set, component) its own (map, mode); mode-1 rows on
    and beyond the ring; e [rows][288] NaN-guarded."""
    lib, c = _fused_lib(), FR.ROWS_CASES[tag]
    su = Setup(c)
    src, grid, pe = FR.rows_lists(c, su.rec)
    lat = FR.case_lattice(c)
    params, blob, bias, wpt = _packed_rows()
    ref = FR.rows(params, lat, c["pad"], src, grid, pe)
    f32 = FR.rows(params, lat, c["pad"], src, grid, pe, dtype=torch.float32)
    dlat, gmeta = _lattice_dev(lat)
    nc = c["rows_comp"]
    e = Guarded((su.S * nc, FR.E))
    dsrc, dgrid, dpe = src.to(abi.dev()), grid.to(abi.dev()), pe.to(abi.dev())
    lh, lw = lat.shape[2:4]
    rc = lib.car_fused_rows(abi.ptr(dlat), lh, lw, c["pad"], abi.ptr(gmeta), abi.ptr(wpt), abi.ptr(blob), abi.ptr(bias), abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), su.n_sets,
                            c["R"], c["P"], nc, e.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("rows", tag, {"e": e.get("e")}, ref, f32, keys=("e",))


# ---- 6. the fp16 instance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("edge-37-13-2", "edge-24-8-1"))
def test_fused_samples_f16_is_held_to_the_fp16_emulation(tag):
    """car_fused_samples_f16 on car_plan_f16_build's plan: geometry outputs bit-identical to the fp32 instance, e and logit within 8 x the
    ratio of the CPU emulation of one-product fp16 arithmetic (tests/test_render_fp16_cpu.py), part as everywhere."""
    su, lat, (dlat, gmeta), ref, _ = _case(tag)
    params, blob, bias, wpt, _, _ = _packed("gauss")
    _, blob16, bias16, wpt16 = _plan16("gauss")
    emu = FR.samples(params, lat, su.c["pad"], su.rec, su.n_sets, dtype=torch.float32, linear=FR.fp16_linear)
    got = run_samples(su, dlat, gmeta, wpt16, blob16, bias16, "f16")
    fp32 = run_samples(su, dlat, gmeta, wpt, blob, bias, "parts")
    for k in ("g", "pt", "pixel_val"):
        assert torch.equal(abi.bits(got[k]), abi.bits(fp32[k])), k
    _judge("f16", tag, got, ref, emu, what="fp16-emulation")
    _judge_part("f16", tag, got, su)
    assert not torch.equal(got["e"], fp32["e"]), "the fp16 instance did not run"


# ---- 7. refusals: all return before any launch -----------------------------------------------------------------------------------------------
def _refusal_args():
    su, lat, (dlat, gmeta), _, _ = _case("edge-24-8-1")
    _, blob, bias, wpt, _, _ = _packed("gauss")
    c = su.c
    lh, lw = lat.shape[2:4]
    out = {k: Guarded(s) for k, s in (("e", (su.S, FR.C)), ("g", (su.S, 16)), ("logit", (su.S,)), ("pt", (su.S, 3)), ("pixel_val", (su.S, 2)),
                                       ("part", (su.n_sets, c["R"], 1, FR.C)))}
    names = ["poses", "rays", "steps", "lattice", "lat_h", "lat_w", "lat_pad", "gmeta", "wpt", "blob", "bias", "b", "V", "R", "P", "H", "W", "no_sample",
             "e", "g", "logit", "pt", "pixel_val", "part"]
    vals = [abi.ptr(su.poses), abi.ptr(su.rays), abi.ptr(su.steps), abi.ptr(dlat), lh, lw, c["pad"], abi.ptr(gmeta), abi.ptr(wpt), abi.ptr(blob), abi.ptr(bias), c["b"], 2, c["R"],
            c["P"], c["H"], c["W"], 0, out["e"].ptr, out["g"].ptr, out["logit"].ptr, out["pt"].ptr, out["pixel_val"].ptr, out["part"].ptr]
    return dict(zip(names, vals)), out


SAMPLE_REFUSALS = [(k, None) for k in ("poses", "rays", "steps", "lattice", "gmeta", "wpt", "blob", "bias", "e", "g", "logit", "pt", "pixel_val")] + \
    [("V", 1), ("V", 3), ("b", 0), ("b", -1), ("R", 0), ("R", -5), ("P", 0), ("P", -1), ("H", 1), ("W", 1), ("lat_pad", 1), ("lat_pad", 0),
     ("lat_h", 20), ("lat_w", 18), ("lat_h", 5), ("lat_w", 5), ("lat_h+w", 967)]


@pytest.mark.parametrize("field,value", SAMPLE_REFUSALS, ids=lambda v: str(v))
def test_fused_samples_refusals(field, value):
    """Null inputs and outputs; V of 1 and 3; non-positive b / R / P; H or W of 1; pad below 2; even lat - 2 pad; a lattice too small for
    its pad; 967 x 967 nodes (2 GiB per map, no such allocation: refused from lat_h, lat_w alone); null `part` for _parts.  Nothing is written."""
    lib = _fused_lib()
    args, out = _refusal_args()
    if field == "lat_h+w":
        args["lat_h"] = args["lat_w"] = value
    else:
        args[field] = value
    a = list(args.values())
    for fn, n in ((lib.car_fused_samples, 23), (lib.car_fused_samples_parts, 24), (lib.car_fused_samples_f16, 24)):
        assert fn(*a[:n], abi.stream()) == CAR_E_ARG, (fn.__name__, field, value)
        assert lib.car_last_error()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values())


def test_fused_samples_parts_refuses_a_null_part():
    lib = _fused_lib()
    args, out = _refusal_args()
    args["part"] = None
    assert lib.car_fused_samples_parts(*args.values(), abi.stream()) == CAR_E_ARG
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values())


ROWS_REFUSALS = [(k, None) for k in ("lattice", "gmeta", "wpt", "blob", "bias", "row_src", "row_grid", "row_pe", "e")] + \
    [("n_sets", 0), ("R", 0), ("P", -1), ("ncomp", 0), ("lat_pad", 1), ("lat_h", 20), ("lat_w", 18), ("lat_h", 5), ("lat_h+w", 967)]


@pytest.mark.parametrize("field,value", ROWS_REFUSALS, ids=lambda v: str(v))
def test_fused_rows_refusals(field, value):
    lib = _fused_lib()
    su, lat, (dlat, gmeta), _, _ = _case("edge-24-8-1")
    _, blob, bias, wpt = _packed_rows()
    c = su.c
    rows = su.S
    src, grid, pe = torch.zeros(rows, dtype=torch.int32, device=abi.dev()), torch.zeros(rows, 2, device=abi.dev()), torch.zeros(rows, 4, device=abi.dev())
    e = Guarded((rows, FR.E))
    lh, lw = lat.shape[2:4]
    args = dict(lattice=abi.ptr(dlat), lat_h=lh, lat_w=lw, lat_pad=c["pad"], gmeta=abi.ptr(gmeta), wpt=abi.ptr(wpt), blob=abi.ptr(blob), bias=abi.ptr(bias),
                row_src=abi.ptr(src), row_grid=abi.ptr(grid), row_pe=abi.ptr(pe), n_sets=su.n_sets, R=c["R"], P=c["P"], ncomp=1, e=e.ptr)
    if field == "lat_h+w":
        args["lat_h"] = args["lat_w"] = value
    else:
        args[field] = value
    assert lib.car_fused_rows(*args.values(), abi.stream()) == CAR_E_ARG, (field, value)
    assert lib.car_last_error()
    torch.cuda.synchronize()
    assert e.untouched()
