"""The per-texel-projected first layer in its five forms through the C ABI against tests/encode_reference.py: car_gather_encode,
car_gather_encode_rows, car_lattice_encode_rows (csrc/car_encode.hip), car_merge_lattice, car_merge_lattice_max (csrc/car_lattice.hip),
car_lattice_encode_linear (csrc/car_linear16.hip), car_fused_rows (csrc/car_fused.hip) on a merged lattice, and the six entries' refusals.

Tolerance, measured against the reference and never against a kernel: every element must satisfy |got - ref64| <= tol x bound, the bound
the float64 sum of magnitudes that goes with the value (encode_reference.py); where the bound is 0 the value must be exactly 0; a
non-finite result fails.  tol = 8 x max(r32, 2^-22), r32 the worst ratio of the reference run in float32, in the kernel's order, on the
same inputs; for the entries that end in the split-fp16 second layer the yardstick is the CPU emulation of one-product fp16 arithmetic
(fused_reference.fp16_linear, parity_rule.tolerance) and the float32 run's ratio is printed beside it.  Every test prints
ratio_kernel / tolerance as a ``[parity]`` line (profiles/encode_parity.md).

Every output lies inside a larger NaN-filled buffer and starts as NaN itself; row padding and a guard row behind the last row must come
back NaN.  test_encode_reference.py (CPU) asserts that the input sets hold the edges they exist for."""
import ctypes
import functools

import pytest
import torch

import abi_harness as abi
import encode_reference as ER
import fused_reference as FR
from abi_harness import CAR_E_ARG, F32, F64, P_, Guarded, rows_out, take_rows
from parity_rule import judge

pytestmark = pytest.mark.gpu


def _judge(test, case, got, ref, bound, r32):
    """One result, wherever the reference lives, held to the float32 run's ratio."""
    judge(test, case, {"": ((got.to(ref.device), ref, bound), r32)})


def _level_args(levels, sizes):
    dl = [t.to(abi.dev()) for t in levels]
    return dl, abi.ptrs(dl), abi.ints([h for h, _ in sizes]), abi.ints([w for _, w in sizes])


# ---- the per-level forms -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _level_reference(name, form):
    """(src, grid, ref64, bound, r32) of a level set in its implicit or explicit form, computed once."""
    s = ER.level_set(name)
    src, grid = ER.implicit_rows(2, s["n_maps"], s["pts"], s["pixel_val"], s["grid_in"]) if form == "implicit" else (s["src"], s["grid"])
    ref, bound = ER.encode_levels(s["levels"], src, grid, s["pe"], s["wpt"], F64)
    f32, _ = ER.encode_levels(s["levels"], src, grid, s["pe"], s["wpt"], F32)
    return src, grid, ref, bound, ER.ratio(f32, ref, bound)


@pytest.mark.parametrize("name", list(ER.LEVEL_SETS))
def test_gather_encode_matches_fp64(name):
    """car_gather_encode, the implicit two-view row form, against encode_levels on implicit_rows: 1 to 4 levels of 16 x 16, 5 x 3, 1 x 7 and
    1 x 1; Cg 4, 12, 64, 576; one and two scenes; 148 / 296 rows (ragged last block of 16); edge_grid in pixel_val and in grid_in."""
    lib, s = abi.lib(), ER.level_set(name)
    _, _, ref, bound, r32 = _level_reference(name, "implicit")
    dl, ptrs, hs, ws = _level_args(s["levels"], s["sizes"])
    pv, gi, pe, wpt = (s[k].to(abi.dev()) for k in ("pixel_val", "grid_in", "pe", "wpt"))
    rows, Cg = s["rows"], s["Cg"]
    out = rows_out(rows, Cg + 8)
    rc = lib.car_gather_encode(ptrs, hs, ws, len(dl), Cg, abi.ptr(pv), abi.ptr(gi), abi.ptr(pe), abi.ptr(wpt), s["n_maps"], 2, s["pts"], abi.ptr(out.view), Cg + 8, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("gather_encode", name, take_rows(out, rows, Cg, name), ref, bound, r32)


@pytest.mark.parametrize("name", list(ER.LEVEL_SETS))
def test_gather_encode_rows_matches_fp64(name):
    """car_gather_encode_rows on the same levels with an explicit list whose maps and padding modes change within every 16-row block."""
    lib, s = abi.lib(), ER.level_set(name)
    src, grid, ref, bound, r32 = _level_reference(name, "explicit")
    dl, ptrs, hs, ws = _level_args(s["levels"], s["sizes"])
    dsrc, dgrid, pe, wpt = src.to(abi.dev()), grid.to(abi.dev()), s["pe"].to(abi.dev()), s["wpt"].to(abi.dev())
    rows, Cg = s["rows"], s["Cg"]
    out = rows_out(rows, Cg + 8)
    rc = lib.car_gather_encode_rows(ptrs, hs, ws, len(dl), Cg, abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(pe), abi.ptr(wpt), s["n_maps"], rows, abi.ptr(out.view), Cg + 8, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("gather_encode_rows", name, take_rows(out, rows, Cg, name), ref, bound, r32)


# ---- the merge -------------------------------------------------------------------------------------------------------------------------------------
MERGE_PYRAMIDS = dict(ER.PYRAMIDS, table_free=ER.TABLE_FREE)


def _merge_maps(name):
    return 2 if name == "table_free" else 3


@functools.lru_cache(maxsize=2)
def _merge_reference(name):
    """(levels on the device, ref64, B_lat, r32, dims) of a pyramid, 576 wide: the reference runs on the device in float64 torch (the
    33 x 433 lattice in seconds); the float32 run beside it."""
    sizes = MERGE_PYRAMIDS[name]
    levels = [t.to(abi.dev()) for t in ER.levels_of(sizes, _merge_maps(name), ER.C, 500 + len(sizes))]
    ref, B, dims = ER.merge(levels, F64)
    f32, _, _ = ER.merge(levels, F32)
    return levels, ref, B, ER.ratio(f32, ref, B), dims


def _run_merge(lib, levels, sizes, n_maps, with_max=None):
    """car_merge_lattice (or car_merge_lattice_max with gmax = with_max) into a NaN-filled lattice."""
    ptrs, hs, ws = abi.ptrs(levels), abi.ints([h for h, _ in sizes]), abi.ints([w for _, w in sizes])
    lh, lw, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.car_merge_lattice(ptrs, hs, ws, len(sizes), n_maps, None, ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(pad), abi.stream())
    assert rc == 0, lib.car_last_error()
    assert (lh.value, lw.value, pad.value) == ER.lattice_of(sizes)[:3]
    lat = Guarded((n_maps, 2, lh.value, lw.value, ER.C))
    if with_max is None:
        rc = lib.car_merge_lattice(ptrs, hs, ws, len(sizes), n_maps, abi.ptr(lat.view), None, None, None, abi.stream())
    else:
        rc = lib.car_merge_lattice_max(ptrs, hs, ws, len(sizes), n_maps, abi.ptr(lat.view), abi.ptr(with_max), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert lat.margins_untouched(), "wrote outside the lattice"
    return lat.view, pad.value


@pytest.mark.parametrize("name", list(MERGE_PYRAMIDS))
def test_merge_lattice_matches_fp64(name):
    """car_merge_lattice against merge: every node of both modes of three maps held to B_lat (an unwritten node stays NaN and fails):
    (4, 8, 16)^2; factor 3 on 2 x 3 / 6 x 9; one level; four non-square levels; and (1, 26) .. (8, 208), two maps: its axis tables
    (4 levels x 2 modes x (433 + ny >= 2) entries x 16 bytes = 55 680 bytes at least) exceed the 52 KB car_launch_merge keeps in LDS, so
    it takes the table-free kernel (encode_reference.takes_table_free_kernel restates the rule)."""
    sizes = MERGE_PYRAMIDS[name]
    assert ER.takes_table_free_kernel(sizes) == (name == "table_free")
    levels, ref, B, r32, _ = _merge_reference(name)
    lat, _ = _run_merge(abi.lib(), levels, sizes, _merge_maps(name))
    _judge("merge_lattice", name, lat, ref, B, r32)


@pytest.mark.parametrize("name", ["p3", "f3", "table_free"])
def test_merge_lattice_max_matches_fp64_and_its_own_lattice(name):
    """car_merge_lattice_max: its lattice against merge and bit-identical to car_merge_lattice's; gmax = the largest magnitude of the
    lattice it wrote, bit for bit, although it held 1e30 before the call (the entry zeroes it)."""
    sizes = MERGE_PYRAMIDS[name]
    levels, ref, B, r32, _ = _merge_reference(name)
    gmax = torch.full((1,), 1e30, device=abi.dev())
    lat, _ = _run_merge(abi.lib(), levels, sizes, _merge_maps(name), with_max=gmax)
    _judge("merge_lattice_max", name, lat, ref, B, r32)
    plain, _ = _run_merge(abi.lib(), levels, sizes, _merge_maps(name))
    assert torch.equal(abi.bits(lat), abi.bits(plain)), "the two entries' lattices differ"
    assert torch.equal(abi.bits(gmax), abi.bits(ER.lattice_max(lat).reshape(1))), (float(gmax), float(ER.lattice_max(lat)))
    # and against the reference: the largest magnitude moves by no more than the largest node error
    tol = ER.tolerance(r32)
    assert abs(float(gmax) - float(ER.lattice_max(ref))) <= tol * float(B.max())


# ---- the lattice rows ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _test_lattice(kind):
    """(lattice [3][2][lh][lw][576] float32 on the host, pad) the test makes itself, so that the merge kernel is not in the loop: seeded
    values on 19 x 19 nodes at pad 2, or the float64 merge of the (4, 8, 16)^2 pyramid rounded to float32 (41 x 41 nodes, pad 5)."""
    if kind == "random":
        return FR.random_lattice("gauss", 3, 8, 8, 2, seed=17), 2
    lat, _, (_, _, pad) = ER.merge(ER.levels_of(ER.PYRAMIDS["p3"], 3, ER.C, 520), F64)
    return lat.float().contiguous(), pad


@functools.lru_cache(maxsize=None)
def _lattice_dev(kind):
    return _test_lattice(kind)[0].to(abi.dev())


@pytest.mark.parametrize("rows", ER.LATTICE_ROWS)
@pytest.mark.parametrize("kind", ["random", "merged"])
def test_lattice_encode_rows_matches_fp64(kind, rows):
    """car_lattice_encode_rows against encode_lattice: three maps, both modes, edge_grid's points, 1, 15, 17 and 148 rows; a dead row
    (zeros mode, on or beyond the outer ring) is exactly relu(point term)."""
    lib = abi.lib()
    lat, pad = _test_lattice(kind)
    lh, lw = lat.shape[2:4]
    src, grid, pe = ER.edge_rows(3, rows, 50 + rows)
    wpt = ER.point_table(ER.C, 530)
    ref, bound = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F64)
    f32, _ = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F32)
    out = rows_out(rows, ER.C + 8)
    dsrc, dgrid, dpe, dwpt = src.to(abi.dev()), grid.to(abi.dev()), pe.to(abi.dev()), wpt.to(abi.dev())
    rc = lib.car_lattice_encode_rows(abi.ptr(_lattice_dev(kind)), lh, lw, pad, ER.C, abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), abi.ptr(dwpt), 3, rows, abi.ptr(out.view),
                                     ER.C + 8, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    got = take_rows(out, rows, ER.C, f"{kind}-{rows}")
    _judge("lattice_encode_rows", f"{kind} rows={rows}", got, ref, bound, ER.ratio(f32, ref, bound))
    _, ring, _ = FR.lattice_taps(grid, lw, lh, pad, F32)
    dead = ring & (ER.split_src(src)[1] == 1)
    assert bool(dead.any())
    point = torch.relu(ER._point_term(pe, wpt, F32)[0])
    assert torch.equal(abi.bits(got[dead]), abi.bits(point[dead])), "a dead row is not relu(point term)"


def _packed_layer(lib, W, N):
    tiles = torch.empty(lib.car_linear_x3_packed_floats(ER.C, N), device=abi.dev())
    dW = W.to(abi.dev())
    rc = lib.car_linear_x3_pack(abi.ptr(dW), ER.C, ER.C, N, abi.ptr(tiles), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return tiles


def _judge_linear(test, case, got, h32, ref, bound, W2, b2, flags=0, Y0=None):
    """The entries that end in the split-fp16 second layer.  Two yardsticks on the float32 rows: the one-product fp16 emulation of the
    layer (parity_rule.tolerance's rule for this arithmetic) and the float32 layer.  The kernels form three products per term and keep
    22 bits of each operand (csrc/car_split.h; the 4 in parity_rule.FACTOR), so they are held to the float32 yardstick as well, as
    tests/test_fused_hip.py holds car_fused_rows: the tighter of the two decides."""
    nobound = torch.zeros(h32.shape, dtype=F64)                          # the yardsticks' own bounds are not used: they are judged on the reference's
    yard, _ = ER.encode_linear(h32, nobound, W2, b2, flags, F32, linear=ER.fp16_linear, Y0=Y0)
    y32, _ = ER.encode_linear(h32, nobound, W2, b2, flags, F32, Y0=Y0)
    judge(test, case, {"": ((got, ref, bound), {"fp32": ER.ratio(y32, ref, bound), "fp16-emulation": ER.ratio(yard, ref, bound)})})


@pytest.mark.parametrize("flags", [0, ER.RELU_OUT, ER.ACCUM], ids=["plain", "relu_out", "accum"])
@pytest.mark.parametrize("rows,N", ER.LINEAR_CASES)
def test_lattice_encode_linear_matches_fp64(rows, N, flags):
    """car_lattice_encode_linear against encode_linear(encode_lattice): N 32, 128, 288 on 64, 193 and 4097 rows; no flag, RELU_OUT, and
    ACCUM onto a random Y0 whose magnitude joins the bound."""
    lib = abi.lib()
    lat, pad = _test_lattice("random")
    lh, lw = lat.shape[2:4]
    src, grid, pe = ER.edge_rows(3, rows, 60 + N)
    wpt = ER.point_table(ER.C, 531)
    W2, b2 = ER.second_layer(N)
    Y0 = torch.randn(rows, N, generator=ER.gen(70 + N)) if flags & ER.ACCUM else None
    h64, Bh = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F64)
    h32, _ = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F32)
    ref, bound = ER.encode_linear(h64, Bh, W2, b2, flags, F64, Y0=Y0)
    out = rows_out(rows, N + 8)
    if Y0 is not None:
        out.view[:rows, :N] = Y0.to(abi.dev())
    tiles = _packed_layer(lib, W2, N)
    dsrc, dgrid, dpe, dwpt, db2 = src.to(abi.dev()), grid.to(abi.dev()), pe.to(abi.dev()), wpt.to(abi.dev()), b2.to(abi.dev())
    rc = lib.car_lattice_encode_linear(abi.ptr(_lattice_dev("random")), lh, lw, pad, abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), abi.ptr(dwpt), 3, rows, abi.ptr(tiles), abi.ptr(db2),
                                       ER.C, N, abi.ptr(out.view), N + 8, flags, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge_linear("lattice_encode_linear", f"rows={rows} N={N} flags={flags}", take_rows(out, rows, N, "Y"), h32, ref, bound, W2, b2, flags, Y0)


# ---- one function, five forms -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forms_reference(name):
    """Everything the five forms are held to, from the LEVELS alone: h64 / B_h, y64, the lattice forms' bounds (B_lat carried through the
    four taps: the merge's rounding is theirs) and the float32 runs."""
    s = ER.forms_set(name)
    a = (s["src"], s["grid"], s["pe"], s["wpt"])
    h64, Bh = ER.encode_levels(s["levels"], *a, F64)
    h32, _ = ER.encode_levels(s["levels"], *a, F32)
    lat64, B_lat, (lh, lw, pad) = ER.merge(s["levels"], F64)
    lat32, _, _ = ER.merge(s["levels"], F32)
    _, Bh_lat = ER.encode_lattice(lat64, pad, *a, F64, mag=B_lat)
    h32_lat, _ = ER.encode_lattice(lat32, pad, *a, F32)
    y64, By_lat = ER.encode_linear(h64, Bh_lat, s["W2"], s["b2"])
    return {"h64": h64, "Bh": Bh, "r32_levels": ER.ratio(h32, h64, Bh), "Bh_lat": Bh_lat, "h32_lat": h32_lat,
            "r32_lat": ER.ratio(h32_lat, h64, Bh_lat), "y64": y64, "By_lat": By_lat, "dims": (lh, lw, pad)}


@pytest.mark.parametrize("name", list(ER.FORMS))
def test_one_function_five_forms(name):
    """Dyadic rows (nodes, ring, +-1, points beyond the ring; float32 taps = float64 taps) over (4, 8, 16)^2 and over 2 x 3 / 6 x 9
    (factor 3), two maps: car_gather_encode_rows on the levels, car_lattice_encode_rows on car_merge_lattice's output,
    car_lattice_encode_linear and car_fused_rows (gmeta from car_merge_lattice_max), each held to the single float64 encode_levels /
    encode_linear reference computed from the levels.  No form is compared with another."""
    lib, s, r = abi.lib(), ER.forms_set(name), _forms_reference(name)
    rows, Cc, N = s["rows"], ER.C, FR.E
    sizes = s["sizes"]
    dl, ptrs, hs, ws = _level_args(s["levels"], sizes)
    dsrc, dgrid, dpe, dwpt = (s[k].to(abi.dev()) for k in ("src", "grid", "pe", "wpt"))
    # 1. the per-level rows
    out = rows_out(rows, Cc + 8)
    rc = lib.car_gather_encode_rows(ptrs, hs, ws, len(dl), Cc, abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), abi.ptr(dwpt), 2, rows, abi.ptr(out.view), Cc + 8, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("five_forms", f"{name} gather_encode_rows", take_rows(out, rows, Cc, "levels"), r["h64"], r["Bh"], r["r32_levels"])
    # 2. the lattice rows on the library's own merge
    gmax = torch.full((1,), 1e30, device=abi.dev())
    lat, pad = _run_merge(lib, dl, sizes, 2, with_max=gmax)
    lh, lw = lat.shape[2:4]
    assert (lh, lw, pad) == r["dims"]
    out = rows_out(rows, Cc + 8)
    rc = lib.car_lattice_encode_rows(abi.ptr(lat), lh, lw, pad, Cc, abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), abi.ptr(dwpt), 2, rows, abi.ptr(out.view), Cc + 8, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("five_forms", f"{name} lattice_encode_rows", take_rows(out, rows, Cc, "lattice"), r["h64"], r["Bh_lat"], r["r32_lat"])
    # 3. the gather-fed second layer
    tiles, db2 = _packed_layer(lib, s["W2"], N), s["b2"].to(abi.dev())
    out = rows_out(rows, N + 8)
    rc = lib.car_lattice_encode_linear(abi.ptr(lat), lh, lw, pad, abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), abi.ptr(dwpt), 2, rows, abi.ptr(tiles), abi.ptr(db2), Cc, N,
                                       abi.ptr(out.view), N + 8, 0, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge_linear("five_forms", f"{name} lattice_encode_linear", take_rows(out, rows, N, "Y"), r["h32_lat"], r["y64"], r["By_lat"], s["W2"], s["b2"])
    # 4. the fused kernel's source pass: W1's 576 feature columns are inside the lattice, only its point columns and b1 enter
    W1 = torch.cat([torch.randn(Cc, Cc, generator=ER.gen(7)), s["W1pt"]], dim=1).contiguous().to(abi.dev())
    db1, dW2 = s["b1"].to(abi.dev()), s["W2"].to(abi.dev())
    blob = torch.zeros(lib.car_fused_blob_floats(), device=abi.dev())
    bias = torch.zeros(lib.car_fused_bias_floats(), device=abi.dev())
    fwpt = torch.zeros(Cc * 4, device=abi.dev())
    rc = lib.car_fused_pack_rows(abi.ptr(W1), abi.ptr(db1), abi.ptr(dW2), abi.ptr(db2), abi.ptr(blob), abi.ptr(bias), abi.ptr(fwpt), abi.stream())
    assert rc == 0, lib.car_last_error()
    e = Guarded((rows, N))
    rc = lib.car_fused_rows(abi.ptr(lat), lh, lw, pad, abi.ptr(gmax), abi.ptr(fwpt), abi.ptr(blob), abi.ptr(bias), abi.ptr(dsrc), abi.ptr(dgrid), abi.ptr(dpe), ER.FORMS_SETS, s["R"],
                            s["P"], ER.FORMS_COMP, abi.ptr(e.view), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert e.margins_untouched()
    _judge_linear("five_forms", f"{name} fused_rows", e.view.cpu(), r["h32_lat"], r["y64"], r["By_lat"], s["W2"], s["b2"])


# ---- refusals: all return CAR_E_ARG before any launch, leave the fired check's message and write nothing ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _refusal_inputs():
    """Small valid arguments of every entry: two 576-wide levels of 2 x 2 and 4 x 4 (lattice 13 x 13, pad 3), two maps, 16 rows, N = 32."""
    lib = abi.lib()
    sizes, n_maps, rows, N = ((2, 2), (4, 4)), 2, 16, 32
    levels = [t.to(abi.dev()) for t in ER.levels_of(sizes, n_maps, ER.C, 600)]
    lh, lw, pad, _ = ER.lattice_of(sizes)
    z = lambda *shape: torch.zeros(*shape, device=abi.dev())
    W2, b2 = ER.second_layer(N)
    t = {"levels": levels, "lattice": z(n_maps, 2, lh, lw, ER.C), "src": torch.zeros(rows, dtype=torch.int32, device=abi.dev()), "grid": z(rows, 2), "pe": z(rows, 4),
         "wpt": z(ER.C, 4), "pixel_val": z(rows // 2, 2), "grid_in": z(rows // 2, 2, 2), "tiles": _packed_layer(lib, W2, N), "bias": b2.to(abi.dev())}
    return sizes, n_maps, rows, N, (lh, lw, pad), t


def _entry(name):
    """(function, ordered argument dict, outputs) of an entry, valid as it stands; the stream is appended by the caller."""
    lib = abi.lib()
    sizes, n_maps, rows, N, (lh, lw, pad), t = _refusal_inputs()
    hs, ws = [h for h, _ in sizes], [w for _, w in sizes]
    lv = dict(gmaps=t["levels"], level_h=hs, level_w=ws, n_levels=len(sizes))
    out = {"out": Guarded((rows, ER.C))}
    if name == "car_gather_encode":
        a = dict(lv, Cg=ER.C, pixel_val=t["pixel_val"], grid_in=t["grid_in"], ptenc=t["pe"], wpt=t["wpt"], n_maps=n_maps, V=2, pts=rows // 4, out=out["out"], ld_out=ER.C)
    elif name == "car_gather_encode_rows":
        a = dict(lv, Cg=ER.C, row_src=t["src"], row_grid=t["grid"], row_pe=t["pe"], wpt=t["wpt"], n_maps=n_maps, rows=rows, out=out["out"], ld_out=ER.C)
    elif name == "car_lattice_encode_rows":
        a = dict(lattice=t["lattice"], lat_h=lh, lat_w=lw, lat_pad=pad, Cg=ER.C, row_src=t["src"], row_grid=t["grid"], row_pe=t["pe"], wpt=t["wpt"], n_maps=n_maps,
                 rows=rows, out=out["out"], ld_out=ER.C)
    elif name == "car_lattice_encode_linear":
        out = {"Y": Guarded((rows, N))}
        a = dict(lattice=t["lattice"], lat_h=lh, lat_w=lw, lat_pad=pad, row_src=t["src"], row_grid=t["grid"], row_pe=t["pe"], wpt=t["wpt"], n_maps=n_maps, rows=rows,
                 packed=t["tiles"], bias=t["bias"], K=ER.C, N=N, Y=out["Y"], ldy=N, flags=0)
    elif name == "car_merge_lattice":
        out = {"lattice": Guarded((n_maps, 2, lh, lw, ER.C))}
        a = dict(lv, n_maps=n_maps, lattice=out["lattice"], lat_h=None, lat_w=None, lat_pad=None)
    else:
        out = {"lattice": Guarded((n_maps, 2, lh, lw, ER.C)), "gmax": Guarded((1,))}
        a = dict(lv, n_maps=n_maps, lattice=out["lattice"], gmax=out["gmax"])
    return getattr(lib, name), a, out


def _c(v):
    """A Python-side argument as ctypes wants it."""
    if isinstance(v, Guarded):
        return abi.ptr(v.view)
    if isinstance(v, torch.Tensor):
        return abi.ptr(v)
    if isinstance(v, list):
        return abi.ptrs(v) if (v and (v[0] is None or isinstance(v[0], torch.Tensor))) else abi.ints(v)
    return v


BIG = (65536, 32768)                                                     # 2^31 texels: no such buffer is ever addressed, the entry refuses from the sizes
_NULLS = lambda names, msg: [(k, None, msg) for k in names]
_LATTICE = [("lat_pad", 1, "bad lattice"), ("lat_h", 20, "bad lattice"), ("lat_w", 18, "bad lattice"), ("lat_h", 5, "bad lattice"),
                        ("lat_w", 7, "bad lattice"), ("n_maps", 7000000, "too many lattice nodes")]
_LEVELS = [("n_levels", 0, "bad level/channel count"), ("n_levels", 5, "bad level/channel count"), ("Cg", 0, "bad level/channel count"),
           ("Cg", 6, "bad level/channel count"), ("gmaps[1]", None, "bad level 1"), ("level_h[0]", 0, "bad level 0"), ("level_w[1]", -1, "bad level 1"),
           ("level[1]", BIG, "bad level 1")]
_LD = [("ld_out", ER.C - 4, "ld_out"), ("ld_out", ER.C + 2, "ld_out")]
_MERGE = _NULLS(("gmaps", "level_h", "level_w"), "bad arguments") + [
    ("n_levels", 0, "bad arguments"), ("n_levels", 5, "bad arguments"), ("n_maps", 0, "bad arguments"), ("gmaps[0]", None, "level 0 is null"),
    ("gmaps[1]", None, "level 1 is null"), ("level[0]", (3, 3), "integer factor"), ("level[0]", (2, 1), "integer factor"), ("level[0]", (1, 2), "integer factor"),
    ("level_h[0]", 0, "integer factor"), ("level_w[1]", 0, "integer factor")]
REFUSALS = {
    "car_gather_encode": _NULLS(("gmaps", "level_h", "level_w", "pixel_val", "grid_in", "ptenc", "wpt", "out"), "null pointer") + _LEVELS + [
        ("V", 1, "needs V == 2"), ("V", 3, "needs V == 2"), ("n_maps", 0, "needs V == 2"), ("n_maps", 3, "needs V == 2"), ("pts", 0, "needs V == 2")] + _LD,
    "car_gather_encode_rows": _NULLS(("gmaps", "level_h", "level_w", "row_src", "row_grid", "row_pe", "wpt", "out"), "null pointer") + _LEVELS + [
        ("n_maps", 0, "bad sizes"), ("rows", 0, "bad sizes")] + _LD,
    "car_lattice_encode_rows": _NULLS(("lattice", "row_src", "row_grid", "row_pe", "wpt", "out"), "null pointer") + [
        ("Cg", 0, "bad sizes"), ("Cg", 6, "bad sizes"), ("n_maps", 0, "bad sizes"), ("rows", 0, "bad sizes")] + _LATTICE + _LD,
    "car_lattice_encode_linear": _NULLS(("lattice", "row_src", "row_grid", "row_pe", "wpt", "packed", "Y"), "null pointer") + [
        ("K", 575, "K must be 576"), ("K", 544, "K must be 576"), ("N", 48, "K must be 576"), ("N", 0, "K must be 576"), ("n_maps", 0, "K must be 576"),
        ("rows", 0, "K must be 576")] + _LATTICE + [("ldy", 28, "ldy"), ("ldy", 34, "ldy"), ("Y+4", None, "ldy"), ("bias+4", None, "ldy"),
                                                              ("lattice+4", None, "ldy"), ("wpt+4", None, "ldy"), ("flags", ER.RELU_IN, "already rectified")],
    "car_merge_lattice": _MERGE,
    "car_merge_lattice_max": _NULLS(("lattice", "gmax"), "car_merge_lattice_max: bad arguments") + _MERGE,
}
REFUSAL_CASES = [(e, f, v, msg) for e, cases in REFUSALS.items() for f, v, msg in cases]


@pytest.mark.parametrize("entry,field,value,message", REFUSAL_CASES, ids=[f"{e}-{f}-{i}" for i, (e, f, v, m) in enumerate(REFUSAL_CASES)])
def test_refusals(entry, field, value, message):
    """At least one call per CAR_REQUIRE of the six entries, and for the checks with several terms their alternatives one at a time: NULL
    pointers, a NULL element of the level array, Cg % 4, V != 2, odd n_maps, ld_out below Cg or no multiple of 4, lat - 2 pad even, pad
    below 2, a lattice too small for its pad, 2^31 lattice nodes, levels that are no common integer factor apart, K != 576, N % 32,
    operands not 16-byte aligned, RELU_IN.  Each returns CAR_E_ARG, leaves the message of the check that fired and writes nothing."""
    lib = abi.lib()
    fn, a, out = _entry(entry)
    if field.endswith("+4"):                                             # the same buffer four bytes on: not 16-byte aligned
        k = field[:-2]
        a[k] = P_((a[k].view if isinstance(a[k], Guarded) else a[k]).data_ptr() + 4)
    elif field.startswith("level["):
        l = int(field[6])
        a["level_h"], a["level_w"] = list(a["level_h"]), list(a["level_w"])
        a["level_h"][l], a["level_w"][l] = value
    elif "[" in field:
        k, l = field[:-3], int(field[-2])
        a[k] = list(a[k])
        a[k][l] = value
    else:
        a[field] = value
    if entry.startswith("car_lattice") and field == "n_maps" and value > 0:
        assert value * 2 * a["lat_h"] * a["lat_w"] >= 2 ** 31
    rc = fn(*[_c(v) for v in a.values()], abi.stream())
    assert rc == CAR_E_ARG, (entry, field, value, rc)
    msg = lib.car_last_error().decode()
    assert message in msg and msg.startswith(entry + ":"), msg
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values()), "a refused call wrote"
