"""The per-texel-projected first layer in its five forms through the C ABI against tests/encode_reference.py: car_gather_encode,
car_gather_encode_rows, car_lattice_encode_rows (csrc/car_encode.hip), car_merge_lattice, car_merge_lattice_max (csrc/car_lattice.hip),
car_lattice_encode_linear (csrc/car_linear16.hip), car_fused_rows (csrc/car_fused.hip) on a merged lattice, and the six entries' refusals.

Tolerance, measured against the reference and never against a kernel: every element must satisfy |got - ref64| <= tol x bound, the bound
the float64 sum of magnitudes that goes with the value (encode_reference.py); where the bound is 0 the value must be exactly 0; a
non-finite result fails.  tol = 8 x max(r32, 2^-22), r32 the worst ratio of the reference run in float32, in the kernel's order, on the
same inputs; for the entries that end in the split-fp16 second layer the yardstick is the CPU emulation of one-product fp16 arithmetic
(fused_reference.fp16_linear, fused_reference.tolerance) and the float32 run's ratio is printed beside it.  Every test prints
ratio_kernel / tolerance as a ``[parity]`` line (profiles/encode_parity.md).

Every output lies inside a larger NaN-filled buffer and starts as NaN itself; row padding and a guard row behind the last row must come
back NaN.  test_encode_reference.py (CPU) asserts that the input sets hold the edges they exist for."""
import ctypes
import functools

import pytest
import torch

import encode_reference as ER
import fused_reference as FR

pytestmark = pytest.mark.gpu

NAN = float("nan")
MARGIN = 64
CAR_E_ARG = -1
F32, F64 = torch.float32, torch.float64
P_ = ctypes.c_void_p


def _lib():
    from cross_attention_renderer_amd import _lib as L
    return L.load()


def _dev():
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else P_(t.data_ptr())


def _stream():
    return P_(torch.cuda.current_stream().cuda_stream)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _ptrs(ts):
    return (P_ * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """A contiguous float32 tensor of `shape` filled with `fill`, inside a NaN-filled buffer."""

    def __init__(self, shape, fill=NAN):
        n = 1
        for d in shape:
            n *= d
        self.n = n
        self.full = torch.full((MARGIN + n + MARGIN,), NAN, dtype=F32, device=_dev())
        self.view = self.full[MARGIN:MARGIN + n].view(*shape)
        self.view.fill_(fill)

    def margins_untouched(self):
        return bool(torch.isnan(self.full[:MARGIN]).all()) and bool(torch.isnan(self.full[MARGIN + self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.full).all())


def _rows_out(rows, width, pad=8):
    """`rows` rows of `width` floats at a stride of width + pad, and a guard row behind them, all NaN."""
    return Guarded((rows + 1, width + pad))


def _take_rows(out, rows, width, what):
    """The rows' windows; everything else of the buffer must still be NaN."""
    got = out.view[:rows, :width].clone()
    out.view[:rows, :width] = NAN
    assert out.untouched(), f"{what}: wrote outside the rows' windows (padding columns, the guard row or the margins)"
    return got.cpu()


def _judge(test, case, got, ref, bound, r32, what="fp32", extra=""):
    """Prints the [parity] line and holds the worst ratio to 8 x max(yardstick, 2^-22)."""
    dev = ref.device
    rk = ER.ratio(got.to(dev), ref, bound)
    tol = ER.tolerance(r32)
    print(f"[parity] {test} {case}: {rk / tol:.3f} (kernel {rk:.2e} {what} {r32:.2e} tol {tol:.2e}{extra})" + ("  ABOVE HALF THE TOLERANCE" if rk > tol / 2 else ""))
    assert rk <= tol, (test, case, rk, tol)


def _level_args(levels, sizes):
    dl = [t.to(_dev()) for t in levels]
    return dl, _ptrs(dl), _ints([h for h, _ in sizes]), _ints([w for _, w in sizes])


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
    lib, s = _lib(), ER.level_set(name)
    _, _, ref, bound, r32 = _level_reference(name, "implicit")
    dl, ptrs, hs, ws = _level_args(s["levels"], s["sizes"])
    pv, gi, pe, wpt = (s[k].to(_dev()) for k in ("pixel_val", "grid_in", "pe", "wpt"))
    rows, Cg = s["rows"], s["Cg"]
    out = _rows_out(rows, Cg)
    rc = lib.car_gather_encode(ptrs, hs, ws, len(dl), Cg, _ptr(pv), _ptr(gi), _ptr(pe), _ptr(wpt), s["n_maps"], 2, s["pts"], _ptr(out.view), Cg + 8, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("gather_encode", name, _take_rows(out, rows, Cg, name), ref, bound, r32)


@pytest.mark.parametrize("name", list(ER.LEVEL_SETS))
def test_gather_encode_rows_matches_fp64(name):
    """car_gather_encode_rows on the same levels with an explicit list whose maps and padding modes change within every 16-row block."""
    lib, s = _lib(), ER.level_set(name)
    src, grid, ref, bound, r32 = _level_reference(name, "explicit")
    dl, ptrs, hs, ws = _level_args(s["levels"], s["sizes"])
    dsrc, dgrid, pe, wpt = src.to(_dev()), grid.to(_dev()), s["pe"].to(_dev()), s["wpt"].to(_dev())
    rows, Cg = s["rows"], s["Cg"]
    out = _rows_out(rows, Cg)
    rc = lib.car_gather_encode_rows(ptrs, hs, ws, len(dl), Cg, _ptr(dsrc), _ptr(dgrid), _ptr(pe), _ptr(wpt), s["n_maps"], rows, _ptr(out.view), Cg + 8, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("gather_encode_rows", name, _take_rows(out, rows, Cg, name), ref, bound, r32)


# ---- the merge -------------------------------------------------------------------------------------------------------------------------------------
MERGE_PYRAMIDS = dict(ER.PYRAMIDS, table_free=ER.TABLE_FREE)


def _merge_maps(name):
    return 2 if name == "table_free" else 3


@functools.lru_cache(maxsize=2)
def _merge_reference(name):
    """(levels on the device, ref64, B_lat, r32, dims) of a pyramid, 576 wide: the reference runs on the device in float64 torch (the
    33 x 433 lattice in seconds); the float32 run beside it."""
    sizes = MERGE_PYRAMIDS[name]
    levels = [t.to(_dev()) for t in ER.levels_of(sizes, _merge_maps(name), ER.C, 500 + len(sizes))]
    ref, B, dims = ER.merge(levels, F64)
    f32, _, _ = ER.merge(levels, F32)
    return levels, ref, B, ER.ratio(f32, ref, B), dims


def _run_merge(lib, levels, sizes, n_maps, with_max=None):
    """car_merge_lattice (or car_merge_lattice_max with gmax = with_max) into a NaN-filled lattice."""
    ptrs, hs, ws = _ptrs(levels), _ints([h for h, _ in sizes]), _ints([w for _, w in sizes])
    lh, lw, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.car_merge_lattice(ptrs, hs, ws, len(sizes), n_maps, None, ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(pad), _stream())
    assert rc == 0, lib.car_last_error()
    assert (lh.value, lw.value, pad.value) == ER.lattice_of(sizes)[:3]
    lat = Guarded((n_maps, 2, lh.value, lw.value, ER.C))
    if with_max is None:
        rc = lib.car_merge_lattice(ptrs, hs, ws, len(sizes), n_maps, _ptr(lat.view), None, None, None, _stream())
    else:
        rc = lib.car_merge_lattice_max(ptrs, hs, ws, len(sizes), n_maps, _ptr(lat.view), _ptr(with_max), _stream())
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
    lat, _ = _run_merge(_lib(), levels, sizes, _merge_maps(name))
    _judge("merge_lattice", name, lat, ref, B, r32)


@pytest.mark.parametrize("name", ["p3", "f3", "table_free"])
def test_merge_lattice_max_matches_fp64_and_its_own_lattice(name):
    """car_merge_lattice_max: its lattice against merge and bit-identical to car_merge_lattice's; gmax = the largest magnitude of the
    lattice it wrote, bit for bit, although it held 1e30 before the call (the entry zeroes it)."""
    sizes = MERGE_PYRAMIDS[name]
    levels, ref, B, r32, _ = _merge_reference(name)
    gmax = torch.full((1,), 1e30, device=_dev())
    lat, _ = _run_merge(_lib(), levels, sizes, _merge_maps(name), with_max=gmax)
    _judge("merge_lattice_max", name, lat, ref, B, r32)
    plain, _ = _run_merge(_lib(), levels, sizes, _merge_maps(name))
    assert torch.equal(_bits(lat), _bits(plain)), "the two entries' lattices differ"
    assert torch.equal(_bits(gmax), _bits(ER.lattice_max(lat).reshape(1))), (float(gmax), float(ER.lattice_max(lat)))
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
    return _test_lattice(kind)[0].to(_dev())


@pytest.mark.parametrize("rows", ER.LATTICE_ROWS)
@pytest.mark.parametrize("kind", ["random", "merged"])
def test_lattice_encode_rows_matches_fp64(kind, rows):
    """car_lattice_encode_rows against encode_lattice: three maps, both modes, edge_grid's points, 1, 15, 17 and 148 rows; a dead row
    (zeros mode, on or beyond the outer ring) is exactly relu(point term)."""
    lib = _lib()
    lat, pad = _test_lattice(kind)
    lh, lw = lat.shape[2:4]
    src, grid, pe = ER.edge_rows(3, rows, 50 + rows)
    wpt = ER.point_table(ER.C, 530)
    ref, bound = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F64)
    f32, _ = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F32)
    out = _rows_out(rows, ER.C)
    dsrc, dgrid, dpe, dwpt = src.to(_dev()), grid.to(_dev()), pe.to(_dev()), wpt.to(_dev())
    rc = lib.car_lattice_encode_rows(_ptr(_lattice_dev(kind)), lh, lw, pad, ER.C, _ptr(dsrc), _ptr(dgrid), _ptr(dpe), _ptr(dwpt), 3, rows, _ptr(out.view),
                                     ER.C + 8, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    got = _take_rows(out, rows, ER.C, f"{kind}-{rows}")
    _judge("lattice_encode_rows", f"{kind} rows={rows}", got, ref, bound, ER.ratio(f32, ref, bound))
    _, ring, _ = FR.lattice_taps(grid, lw, lh, pad, F32)
    dead = ring & (ER.split_src(src)[1] == 1)
    assert bool(dead.any())
    point = torch.relu(ER._point_term(pe, wpt, F32)[0])
    assert torch.equal(_bits(got[dead]), _bits(point[dead])), "a dead row is not relu(point term)"


def _packed_layer(lib, W, N):
    tiles = torch.empty(lib.car_linear_x3_packed_floats(ER.C, N), device=_dev())
    dW = W.to(_dev())
    rc = lib.car_linear_x3_pack(_ptr(dW), ER.C, ER.C, N, _ptr(tiles), _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return tiles


def _judge_linear(test, case, got, h32, ref, bound, W2, b2, flags=0, Y0=None):
    """The entries that end in the split-fp16 second layer.  Two yardsticks on the float32 rows: the one-product fp16 emulation of the
    layer (fused_reference.tolerance's rule for this arithmetic) and the float32 layer.  The kernels form three products per term and keep
    22 bits of each operand (csrc/car_split.h; the 4 in fused_reference.FACTOR), so they are held to the float32 yardstick as well, as
    tests/test_fused_hip.py holds car_fused_rows: the tighter of the two decides."""
    nobound = torch.zeros(h32.shape, dtype=F64)                          # the yardsticks' own bounds are not used: they are judged on the reference's
    yard, _ = ER.encode_linear(h32, nobound, W2, b2, flags, F32, linear=ER.fp16_linear, Y0=Y0)
    y32, _ = ER.encode_linear(h32, nobound, W2, b2, flags, F32, Y0=Y0)
    r16, r32 = ER.ratio(yard, ref, bound), ER.ratio(y32, ref, bound)
    rk = ER.ratio(got, ref, bound)
    tol16, tol32 = FR.tolerance(r16), FR.tolerance(r32)
    print(f"[parity] {test} {case}: {rk / tol32:.3f} (kernel {rk:.2e} fp32 {r32:.2e} tol {tol32:.2e}; fp16-emulation {r16:.2e} tol {tol16:.2e}: {rk / tol16:.4f})"
          + ("  ABOVE HALF THE TOLERANCE" if rk > tol32 / 2 else ""))
    assert rk <= tol16 and rk <= tol32, (test, case, rk, tol16, tol32)


@pytest.mark.parametrize("flags", [0, ER.RELU_OUT, ER.ACCUM], ids=["plain", "relu_out", "accum"])
@pytest.mark.parametrize("rows,N", ER.LINEAR_CASES)
def test_lattice_encode_linear_matches_fp64(rows, N, flags):
    """car_lattice_encode_linear against encode_linear(encode_lattice): N 32, 128, 288 on 64, 193 and 4097 rows; no flag, RELU_OUT, and
    ACCUM onto a random Y0 whose magnitude joins the bound."""
    lib = _lib()
    lat, pad = _test_lattice("random")
    lh, lw = lat.shape[2:4]
    src, grid, pe = ER.edge_rows(3, rows, 60 + N)
    wpt = ER.point_table(ER.C, 531)
    W2, b2 = ER.second_layer(N)
    Y0 = torch.randn(rows, N, generator=ER.gen(70 + N)) if flags & ER.ACCUM else None
    h64, Bh = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F64)
    h32, _ = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F32)
    ref, bound = ER.encode_linear(h64, Bh, W2, b2, flags, F64, Y0=Y0)
    out = _rows_out(rows, N)
    if Y0 is not None:
        out.view[:rows, :N] = Y0.to(_dev())
    tiles = _packed_layer(lib, W2, N)
    dsrc, dgrid, dpe, dwpt, db2 = src.to(_dev()), grid.to(_dev()), pe.to(_dev()), wpt.to(_dev()), b2.to(_dev())
    rc = lib.car_lattice_encode_linear(_ptr(_lattice_dev("random")), lh, lw, pad, _ptr(dsrc), _ptr(dgrid), _ptr(dpe), _ptr(dwpt), 3, rows, _ptr(tiles), _ptr(db2),
                                       ER.C, N, _ptr(out.view), N + 8, flags, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge_linear("lattice_encode_linear", f"rows={rows} N={N} flags={flags}", _take_rows(out, rows, N, "Y"), h32, ref, bound, W2, b2, flags, Y0)


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
    lib, s, r = _lib(), ER.forms_set(name), _forms_reference(name)
    rows, Cc, N = s["rows"], ER.C, FR.E
    sizes = s["sizes"]
    dl, ptrs, hs, ws = _level_args(s["levels"], sizes)
    dsrc, dgrid, dpe, dwpt = (s[k].to(_dev()) for k in ("src", "grid", "pe", "wpt"))
    # 1. the per-level rows
    out = _rows_out(rows, Cc)
    rc = lib.car_gather_encode_rows(ptrs, hs, ws, len(dl), Cc, _ptr(dsrc), _ptr(dgrid), _ptr(dpe), _ptr(dwpt), 2, rows, _ptr(out.view), Cc + 8, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("five_forms", f"{name} gather_encode_rows", _take_rows(out, rows, Cc, "levels"), r["h64"], r["Bh"], r["r32_levels"])
    # 2. the lattice rows on the library's own merge
    gmax = torch.full((1,), 1e30, device=_dev())
    lat, pad = _run_merge(lib, dl, sizes, 2, with_max=gmax)
    lh, lw = lat.shape[2:4]
    assert (lh, lw, pad) == r["dims"]
    out = _rows_out(rows, Cc)
    rc = lib.car_lattice_encode_rows(_ptr(lat), lh, lw, pad, Cc, _ptr(dsrc), _ptr(dgrid), _ptr(dpe), _ptr(dwpt), 2, rows, _ptr(out.view), Cc + 8, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge("five_forms", f"{name} lattice_encode_rows", _take_rows(out, rows, Cc, "lattice"), r["h64"], r["Bh_lat"], r["r32_lat"])
    # 3. the gather-fed second layer
    tiles, db2 = _packed_layer(lib, s["W2"], N), s["b2"].to(_dev())
    out = _rows_out(rows, N)
    rc = lib.car_lattice_encode_linear(_ptr(lat), lh, lw, pad, _ptr(dsrc), _ptr(dgrid), _ptr(dpe), _ptr(dwpt), 2, rows, _ptr(tiles), _ptr(db2), Cc, N,
                                       _ptr(out.view), N + 8, 0, _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    _judge_linear("five_forms", f"{name} lattice_encode_linear", _take_rows(out, rows, N, "Y"), r["h32_lat"], r["y64"], r["By_lat"], s["W2"], s["b2"])
    # 4. the fused kernel's source pass: W1's 576 feature columns are inside the lattice, only its point columns and b1 enter
    W1 = torch.cat([torch.randn(Cc, Cc, generator=ER.gen(7)), s["W1pt"]], dim=1).contiguous().to(_dev())
    db1, dW2 = s["b1"].to(_dev()), s["W2"].to(_dev())
    blob = torch.zeros(lib.car_fused_blob_floats(), device=_dev())
    bias = torch.zeros(lib.car_fused_bias_floats(), device=_dev())
    fwpt = torch.zeros(Cc * 4, device=_dev())
    rc = lib.car_fused_pack_rows(_ptr(W1), _ptr(db1), _ptr(dW2), _ptr(db2), _ptr(blob), _ptr(bias), _ptr(fwpt), _stream())
    assert rc == 0, lib.car_last_error()
    e = Guarded((rows, N))
    rc = lib.car_fused_rows(_ptr(lat), lh, lw, pad, _ptr(gmax), _ptr(fwpt), _ptr(blob), _ptr(bias), _ptr(dsrc), _ptr(dgrid), _ptr(dpe), ER.FORMS_SETS, s["R"],
                            s["P"], ER.FORMS_COMP, _ptr(e.view), _stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert e.margins_untouched()
    _judge_linear("five_forms", f"{name} fused_rows", e.view.cpu(), r["h32_lat"], r["y64"], r["By_lat"], s["W2"], s["b2"])


# ---- refusals: all return CAR_E_ARG before any launch, leave the fired check's message and write nothing ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _refusal_inputs():
    """Small valid arguments of every entry: two 576-wide levels of 2 x 2 and 4 x 4 (lattice 13 x 13, pad 3), two maps, 16 rows, N = 32."""
    lib = _lib()
    sizes, n_maps, rows, N = ((2, 2), (4, 4)), 2, 16, 32
    levels = [t.to(_dev()) for t in ER.levels_of(sizes, n_maps, ER.C, 600)]
    lh, lw, pad, _ = ER.lattice_of(sizes)
    z = lambda *shape: torch.zeros(*shape, device=_dev())
    W2, b2 = ER.second_layer(N)
    t = {"levels": levels, "lattice": z(n_maps, 2, lh, lw, ER.C), "src": torch.zeros(rows, dtype=torch.int32, device=_dev()), "grid": z(rows, 2), "pe": z(rows, 4),
         "wpt": z(ER.C, 4), "pixel_val": z(rows // 2, 2), "grid_in": z(rows // 2, 2, 2), "tiles": _packed_layer(lib, W2, N), "bias": b2.to(_dev())}
    return sizes, n_maps, rows, N, (lh, lw, pad), t


def _entry(name):
    """(function, ordered argument dict, outputs) of an entry, valid as it stands; the stream is appended by the caller."""
    lib = _lib()
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
        return _ptr(v.view)
    if isinstance(v, torch.Tensor):
        return _ptr(v)
    if isinstance(v, list):
        return _ptrs(v) if (v and (v[0] is None or isinstance(v[0], torch.Tensor))) else _ints(v)
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
    lib = _lib()
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
    rc = fn(*[_c(v) for v in a.values()], _stream())
    assert rc == CAR_E_ARG, (entry, field, value, rc)
    msg = lib.car_last_error().decode()
    assert message in msg and msg.startswith(entry + ":"), msg
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values()), "a refused call wrote"
