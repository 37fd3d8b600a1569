"""CPU checks of tests/encode_reference.py, the checker of tests/test_encode_hip.py: the merge against float64 grid_sample at the lattice
nodes and, in float32, against the host shim's merged lattice bit for bit; the per-texel projection against the reference's own order of
operations; the lattice identity — four taps of the merged lattice equal the sum over the levels — to a few ulp of float64
on dyadic points and up to the float32 coordinate's cost elsewhere; the implicit row rule against a loop written from the header's
sentence; and every input set of the GPU suite holds the edges it exists for."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encode_reference as ER
import fused_reference as FR
import gather_reference as GR
from test_gather_reference import WEIGHT_ROUNDING, _cell64, _coords
from test_geom_host import _ptr, shim  # noqa: F401  (shim: the fixture that compiles tests/host/car_geom_host.cpp)

F32, F64 = torch.float32, torch.float64
ULP64 = 2.0 ** -53
ALL_PYRAMIDS = dict(ER.PYRAMIDS, table_free=ER.TABLE_FREE)


def _levels(sizes, n_maps, channels, seed, dtype=F32):
    return [t.to(dtype) for t in ER.levels_of(sizes, n_maps, channels, seed)]


def _mixed_src(n_maps, rows, seed):
    g = ER.gen(seed)
    return (torch.randint(0, n_maps, (rows,), generator=g) | (torch.randint(0, 2, (rows,), generator=g) << ER.MODE_BIT)).to(torch.int32)


# ---- the merge -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL_PYRAMIDS))
def test_float64_merge_is_grid_sample_at_the_nodes(name):
    """Every node of both modes against the sum over the levels of float64 grid_sample at the node's grid coordinate (u + 1) / W_max - 1.
    What may differ: that coordinate is rounded once in float64 (a third is no float64), which moves a level's texel coordinate by at most
    three ulp of W_l and a bilinear sample by that times twice the largest texel difference, on each axis; and the sums' own rounding,
    a few ulp of B_lat."""
    sizes = ALL_PYRAMIDS[name]
    n_maps, Cc = 2, 3
    levels = _levels(sizes, n_maps, Cc, 7, F64)
    lat, B, (lh, lw, pad) = ER.merge(levels, F64)
    hm, wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    assert (lh, lw, pad) == ER.lattice_of(sizes)[:3]
    uy, ux = torch.arange(lh, dtype=F64) - pad, torch.arange(lw, dtype=F64) - pad
    gy, gx = torch.meshgrid((uy + 1) / hm - 1, (ux + 1) / wm - 1, indexing="ij")
    grid = torch.stack([gx, gy], dim=-1)[None].expand(n_maps, -1, -1, -1)
    gmax = max(float(t.abs().max()) for t in levels)
    worst = 0.0
    for mode, pname in enumerate(("border", "zeros")):
        want = sum(F.grid_sample(t.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode=pname, align_corners=False) for t in levels)
        err = (lat[:, mode] - want.permute(0, 2, 3, 1)).abs()
        lim = ULP64 * (16 * B[:, mode] + 2 * 3 * 4 * max(hm, wm) * gmax * len(sizes))
        worst = max(worst, float((err / lim).max()))
        assert float(err.max()) < 1e-13 * gmax * len(sizes)
    print(f"[parity] merge64 {name}: error / bound {worst:.3f}")
    assert worst <= 1.0
    assert bool((lat[:, 1, 0] == 0).all() and (lat[:, 1, -1] == 0).all() and (lat[:, 1, :, 0] == 0).all() and (lat[:, 1, :, -1] == 0).all()), \
        "the zeros-mode outer ring is exactly zero"


@pytest.mark.parametrize("name", list(ALL_PYRAMIDS))
def test_float32_merge_is_the_host_shim_bit_for_bit(shim, name):  # noqa: F811
    """merge(float32) == host_lattice_build (tests/host/car_geom_host.cpp: car_bilinear_taps_px at the nodes, levels from the last index
    down, one fmaf per tap), every bit of both modes."""
    sizes = ALL_PYRAMIDS[name]
    n_maps, Cc = 2, 4
    levels = _levels(sizes, n_maps, Cc, 9)
    lat, _, (lh, lw, pad) = ER.merge(levels, F32)
    r = ER.lattice_of(sizes)[3]
    ia = lambda v: (ctypes.c_int * len(v))(*v)
    for m in range(n_maps):
        lv = [np.ascontiguousarray(t[m].numpy()) for t in levels]
        ptrs = (ctypes.c_void_p * len(lv))(*[a.ctypes.data for a in lv])
        want = np.full((2, lh, lw, Cc), np.nan, np.float32)
        shim.host_lattice_build(ptrs, ia([h for h, _ in sizes]), ia([w for _, w in sizes]), ia(r), len(sizes), Cc, lh, lw, pad, _ptr(want))
        got = lat[m].numpy()
        assert np.array_equal(np.abs(got).view(np.int32), np.abs(want).view(np.int32)), (name, m)      # up to the sign of an exact zero


def test_fma32_is_a_single_rounding():
    """Against exact rational arithmetic on operands chosen to sit near float32 midpoints of the sum."""
    from fractions import Fraction
    g = ER.gen(3)
    a, b = torch.randn(4000, generator=g), torch.randn(4000, generator=g)
    c = torch.randn(4000, generator=g) * 2.0 ** torch.randint(-40, 41, (4000,), generator=g).float()
    c[:1000] = (-(a[:1000].double() * b[:1000].double())).float()                                     # cancellation: the product's low bits decide
    got = ER.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = float(got[i])
        lo, hi = np.nextafter(np.float32(near), np.float32(-np.inf)), np.nextafter(np.float32(near), np.float32(np.inf))
        assert abs(exact - Fraction(near)) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi)))), i


# ---- linearity ---------------------------------------------------------------------------------------------------------------------------------
def test_projected_levels_equal_the_literal_order_of_operations():
    """encode_levels(project(F, W1)) == relu(W1 [grid_sample(F_l) ...; tanh(pt / 5)] + b1) in float64, on finite dyadic coordinates (there
    the float32 taps are the float64 taps, asserted below), both padding modes, to a few ulp of the sum of magnitudes."""
    sizes, chans, n_maps, rows = ((16, 16), (5, 3), (1, 7), (1, 1)), (6, 4, 3, 2), 3, 300
    g = ER.gen(21)
    raw = [torch.randn(n_maps, h, w, c, generator=g, dtype=F64) for (h, w), c in zip(sizes, chans)]
    Cout = 10
    W1 = torch.randn(Cout, sum(chans) + 3, generator=g, dtype=F64)
    b1 = torch.randn(Cout, generator=g, dtype=F64)
    grid = (torch.randint(-1536, 1537, (rows, 2), generator=g).double() / 1024).float()
    grid[:5] = torch.tensor([(-1.0, -1.0), (1.0, 1.0), (0.0, 0.0), (-1.5, 1.5), (1.0 - 1 / 16, -1.0 + 1 / 16)])
    src = _mixed_src(n_maps, rows, 22)
    pt = 5 * torch.randn(rows, 3, generator=g, dtype=F64)
    for (h, w) in sizes:
        for gcol, n in ((grid[:, 0], w), (grid[:, 1], h)):
            assert torch.equal(GR.texel_coord32(gcol, n).double(), ((gcol.double() + 1) * n - 1) / 2)
    pe = torch.cat([torch.tanh(pt / 5), torch.full((rows, 1), float("nan"), dtype=F64)], dim=1)
    wpt = torch.cat([W1[:, -3:], b1[:, None]], dim=1)
    got, _ = ER.encode_levels(ER.project(raw, W1), src, grid, pe, wpt, F64)
    mag, _ = ER.encode_levels(ER.project([t.abs() for t in raw], W1.abs()), src, grid, pe.abs(), wpt.abs(), F64)
    want = ER.literal(raw, W1, b1, src, grid, pt)
    worst = float(((got - want).abs() / (ULP64 * mag)).max())
    print(f"[parity] linearity: error / (2^-53 x sum of magnitudes) {worst:.2f}")
    assert worst <= 32


# ---- the lattice identity ----------------------------------------------------------------------------------------------------------------------
def _dyadic_rows(sizes, n_maps, seed):
    lh, lw, pad, _ = ER.lattice_of(sizes)
    rows = 5 + max(lh, lw) + lh + 100
    return ER.dyadic_grid(sizes, rows, seed), _mixed_src(n_maps, rows, seed + 1), ER.point_rows(rows, seed + 2)


def _assert_dyadic_taps_exact(sizes, grid):
    lh, lw, pad, _ = ER.lattice_of(sizes)
    n32, r32, w32 = FR.lattice_taps(grid, lw, lh, pad, F32)
    n64, r64, w64 = FR.lattice_taps(grid, lw, lh, pad, F64)
    assert torch.equal(n32, n64) and torch.equal(r32, r64) and torch.equal(w32.double(), w64)
    for (h, w) in sizes:
        for gcol, n in ((grid[:, 0], w), (grid[:, 1], h)):
            assert torch.equal(GR.texel_coord32(gcol, n).double(), ((gcol.double() + 1) * n - 1) / 2)


@pytest.mark.parametrize("name", list(ER.PYRAMIDS))
def test_lattice_identity_on_dyadic_points(name):
    """encode_lattice(merge(G)) == encode_levels(G) in float64 to a few ulp of the bound: powers of two, factor 3, non-square levels, both
    modes, nodes, ring, +-1 and points beyond the ring."""
    sizes = ER.PYRAMIDS[name]
    n_maps, Cc = 3, 8
    levels = _levels(sizes, n_maps, Cc, 31, F64)
    grid, src, pe = _dyadic_rows(sizes, n_maps, 32)
    _assert_dyadic_taps_exact(sizes, grid)
    wpt = ER.point_table(Cc, 33)
    lat, B_lat, (lh, lw, pad) = ER.merge(levels, F64)
    a, Ba = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F64, mag=B_lat)
    b, Bb = ER.encode_levels(levels, src, grid, pe, wpt, F64)
    worst = float(((a - b).abs() / (ULP64 * torch.maximum(Ba, Bb))).max())
    print(f"[parity] identity dyadic {name}: error / (2^-53 x bound) {worst:.2f}")
    assert worst <= 32
    _, ring, _ = FR.lattice_taps(grid, lw, lh, pad, F32)
    assert bool(ring.any()) and bool((~ring).any())


def _lattice_coords(g, s, n, pad):
    """(u32, u64) of one axis, clamped onto the lattice, as float64."""
    u32 = ((g + 1.0) * float(s) - 1.0).double()
    u64 = (g.double() + 1) * s - 1
    lo, hi = -float(pad), float(n - 1 - pad)
    return u32.clamp(lo, hi), u64.clamp(lo, hi)


def _fd(t, dx, dy):
    """|dx| (|ne - nw| + |se - sw|) + |dy| (|sw - nw| + |se - ne|) of four taps t [rows, 4, C]."""
    return dx[:, None] * ((t[:, 1] - t[:, 0]).abs() + (t[:, 3] - t[:, 2]).abs()) + dy[:, None] * ((t[:, 2] - t[:, 0]).abs() + (t[:, 3] - t[:, 1]).abs())


@pytest.mark.parametrize("name", list(ER.PYRAMIDS))
def test_lattice_identity_up_to_the_float32_coordinate(name):
    """On edge_grid's finite random points the two forms may differ only by what their float32 coordinates cost: each form's texel /
    lattice coordinate is rounded in float32 on its own.  As in profiles/gather_parity.md: moving a point by (dx, dy) inside a cell moves
    a bilinear sample by at most |dx| (|ne - nw| + |se - sw|) + |dy| (|sw - nw| + |se - ne|), taken over the float32 cell and the float64
    cell (a rounding can carry a point over a cell's edge), per level for the per-level form and on the lattice for the lattice form, plus
    3 x 2^-24 of the sum of magnitudes for each form's float32 weights."""
    sizes = ER.PYRAMIDS[name]
    n_maps, Cc, rows = 3, 8, 3000
    levels = _levels(sizes, n_maps, Cc, 41, F64)
    grid = GR.edge_grid(1, rows, 42)[0]
    grid = torch.where(torch.isfinite(grid), grid, torch.rand(rows, 2, generator=ER.gen(43)) * 2.4 - 1.2)
    src, pe, wpt = _mixed_src(n_maps, rows, 44), ER.point_rows(rows, 45), ER.point_table(Cc, 46)
    m, mode = ER.split_src(src)
    lat, B_lat, (lh, lw, pad) = ER.merge(levels, F64)
    a, Ba = ER.encode_lattice(lat, pad, src, grid, pe, wpt, F64, mag=B_lat)
    b, Bb = ER.encode_levels(levels, src, grid, pe, wpt, F64)
    bound = WEIGHT_ROUNDING * (Ba + Bb) + 1e-15
    for t in levels:                                                                     # the per-level form's coordinate
        _, H, W, _ = t.shape
        flat = t.reshape(n_maps, H * W, Cc)
        for md in (0, 1):
            sel = mode == md
            (x32, x64), (y32, y64) = _coords(grid[sel], W, H, md)
            for cx, cy in ((x32, y32), (x64, y64)):
                idx, valid = _cell64(cx, cy, W, H, md)
                bound[sel] += _fd(flat[m[sel, None], idx] * valid[..., None], (x32 - x64).abs(), (y32 - y64).abs())
    sx, sy = FR.lattice_scale(lh, lw, pad)
    (ux32, ux64), (uy32, uy64) = _lattice_coords(grid[:, 0], sx, lw, pad), _lattice_coords(grid[:, 1], sy, lh, pad)
    flat = lat.reshape(n_maps * 2, lh * lw, Cc)
    for ux, uy in ((ux32, uy32), (ux64, uy64)):                                          # the lattice form's coordinate
        x0 = torch.floor(ux).clamp(max=lw - 2 - pad).long() + pad
        y0 = torch.floor(uy).clamp(max=lh - 2 - pad).long() + pad
        node = y0 * lw + x0
        idx = torch.stack([node, node + 1, node + lw, node + lw + 1], dim=-1)
        bound += _fd(flat[(m * 2 + mode)[:, None], idx], (ux32 - ux64).abs(), (uy32 - uy64).abs())
    worst = float(((a - b).abs() / bound).max())
    print(f"[parity] identity float32-coordinate {name}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    assert float((a - b).abs().max()) > 0 or name == "one"


# ---- the implicit row rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_maps,pts", [(2, 37), (4, 5), (6, 3)])
def test_implicit_rows_follow_the_header(n_maps, pts):
    """include/car_hip.h: "For sample i = (n, j), j < pts, and source view s the kernel writes row i*V + s ... (map, grid, padding) =
    (n, pixel_val[i], border) if s is the sample's own view, else ((scene, s), grid_in[i, s], zeros)", maps ordered (scene, view)."""
    V = 2
    g = ER.gen(n_maps)
    pixel_val, grid_in = torch.randn(n_maps * pts, 2, generator=g), torch.randn(n_maps * pts, V, 2, generator=g)
    src, grid = ER.implicit_rows(V, n_maps, pts, pixel_val, grid_in)
    assert src.dtype == torch.int32 and src.shape == (n_maps * pts * V,) and grid.shape == (n_maps * pts * V, 2)
    for scene in range(n_maps // V):
        for view in range(V):
            n = scene * V + view
            for j in range(pts):
                i = n * pts + j
                for s in range(V):
                    row = i * V + s
                    if s == view:
                        assert int(src[row]) == n and torch.equal(grid[row], pixel_val[i])
                    else:
                        assert int(src[row]) == (scene * V + s) + (1 << 30) and torch.equal(grid[row], grid_in[i, s])


# ---- the input sets hold what they claim ---------------------------------------------------------------------------------------------------------
def _all_masked(src, grid, sizes):
    """Rows none of whose taps carries weight on any level."""
    return torch.stack([(ER.level_taps(src, grid, w, h)[1] == 0).all(1) for h, w in sizes]).all(0)


def _edges(grid, sizes):
    """(rows on a lattice node, on the outer ring without being beyond it, with |x| = |y| = 1) of the sizes' lattice."""
    lh, lw, pad, _ = ER.lattice_of(sizes)
    sx, sy = FR.lattice_scale(lh, lw, pad)
    ux, uy = (grid[:, 0].double() + 1) * sx - 1, (grid[:, 1].double() + 1) * sy - 1
    inside = (ux >= -pad) & (ux <= lw - 1 - pad) & (uy >= -pad) & (uy <= lh - 1 - pad)
    on_ring = inside & ((ux == -pad) | (ux == lw - 1 - pad) | (uy == -pad) | (uy == lh - 1 - pad))
    return inside & (ux == ux.round()) & (uy == uy.round()), on_ring, (grid.abs() == 1).all(1)


@pytest.mark.parametrize("name", list(ER.LEVEL_SETS))
def test_level_sets_hold_their_edges(name):
    s = ER.level_set(name)
    assert s["rows"] == s["n_maps"] * s["pts"] * 2 and s["rows"] % ER.ROW_BLOCK != 0
    assert s["Cg"] % 4 == 0 and 1 <= len(s["sizes"]) <= GR.MAX_LEVELS
    lists = {"implicit": ER.implicit_rows(2, s["n_maps"], s["pts"], s["pixel_val"], s["grid_in"]), "explicit": (s["src"], s["grid"])}
    for what, (src, grid) in lists.items():
        m, mode = ER.split_src(src)
        assert src.shape[0] == s["rows"] and int(m.max()) == s["n_maps"] - 1 and int(m.min()) == 0
        masked = _all_masked(src, grid, s["sizes"])
        assert bool((masked & (mode == 1)).any()) and not bool((masked & (mode == 0)).any()), what
        assert bool(torch.isnan(grid).any()) and bool(torch.isinf(grid).any()) and bool((grid.abs() == 1e10).any()), what
        assert bool((grid.abs() == 1).all(1).any()), what
        block = torch.arange(s["rows"]) // ER.ROW_BLOCK
        for k in range(s["rows"] // ER.ROW_BLOCK):                                         # maps and modes change within every whole 16-row block
            assert len(mode[block == k].unique()) == 2 and len(m[block == k].unique()) > 1, (what, k)
    assert bool(torch.isnan(s["pe"][:, 3]).all()) and bool(torch.isfinite(s["pe"][:, :3]).all())
    assert {len(v[0]) for v in ER.LEVEL_SETS.values()} == {1, 2, 3, 4} and {v[1] for v in ER.LEVEL_SETS.values()} == {4, 12, 64, 576}
    assert {v[2] for v in ER.LEVEL_SETS.values()} == {2, 4}


@pytest.mark.parametrize("rows", ER.LATTICE_ROWS)
def test_lattice_rows_hold_their_edges(rows):
    """The rows of the car_lattice_encode_rows cases on the 8 x 8 lattice at pad 2 the GPU test makes."""
    src, grid, pe = ER.edge_rows(3, rows, 50 + rows)
    lh, lw = FR.lattice_dims(8, 8, 2)
    m, mode = ER.split_src(src)
    _, ring, _ = FR.lattice_taps(grid, lw, lh, 2, F32)
    assert src.shape[0] == rows and bool((ring & (mode == 1))[0]), "row 0 is dead"
    if rows > 1:
        assert rows % ER.ROW_BLOCK != 0 and len(mode.unique()) == 2 and len(m.unique()) == 3
        assert bool(torch.isnan(grid).any()) and bool((grid.abs() == 1).all(1).any())
        assert bool((ring & (mode == 0)).any()), "a border row on or beyond the ring (not dead)"
    assert bool(torch.isnan(pe[:, 3]).all())


@pytest.mark.parametrize("rows,N", ER.LINEAR_CASES)
def test_linear_rows_hold_their_edges(rows, N):
    src, grid, _ = ER.edge_rows(3, rows, 60 + N)
    _, mode = ER.split_src(src)
    lh, lw = FR.lattice_dims(8, 8, 2)
    _, ring, _ = FR.lattice_taps(grid, lw, lh, 2, F32)
    assert N % 32 == 0 and bool((ring & (mode == 1)).any()) and bool((~ring).any())


@pytest.mark.parametrize("name", list(ER.FORMS))
def test_forms_sets_hold_their_edges(name):
    s = ER.forms_set(name)
    assert s["rows"] == ER.FORMS_SETS * s["R"] * s["P"] * ER.FORMS_COMP and s["rows"] % ER.ROW_BLOCK != 0
    assert bool((s["grid"] * 1024 == (s["grid"] * 1024).round()).all()) and float(s["grid"].abs().max()) <= 1.5
    _assert_dyadic_taps_exact(s["sizes"], s["grid"])
    node, on_ring, pm1 = _edges(s["grid"], s["sizes"])
    assert int(node.sum()) >= 5 and int(on_ring.sum()) >= 1 and int(pm1.sum()) >= 4
    m, mode = ER.split_src(s["src"])
    lh, lw, pad, _ = ER.lattice_of(s["sizes"])
    _, ring, _ = FR.lattice_taps(s["grid"], lw, lh, pad, F32)
    assert bool((ring & (mode == 1)).any()), "a dead row"
    assert bool(_all_masked(s["src"], s["grid"], s["sizes"]).any()), "a row with every tap masked"
    # one (map, mode) per (set, component), all four of them
    per = (m * 2 + mode).reshape(ER.FORMS_SETS, s["R"] * s["P"], ER.FORMS_COMP)
    assert bool((per == per[:, :1]).all()) and len(per[:, 0].reshape(-1).unique()) == 4
    assert s["levels"][0].shape[-1] == ER.C == 576 and s["n_maps"] == 2


def test_the_table_free_pyramid_follows_the_launch_rule():
    """car_launch_merge keeps the axis tables in LDS while n_levels x 2 x (lw + ny) x 16 bytes <= 52 KB, ny = per / lw + 2 >= 2: with four
    levels that ends above lw + ny = 416.  The widest level of a four-level pyramid of factors 8, 4, 2, 1 is 8 k wide: lw = 16 k + 17."""
    assert ER.takes_table_free_kernel(ER.TABLE_FREE) and ER.lattice_of(ER.TABLE_FREE)[:3] == (33, 433, 9)
    assert not any(ER.takes_table_free_kernel(p) for p in ER.PYRAMIDS.values())
    # the tables of the other pyramids fit with any ny their lattices allow (ny <= lh x n_maps + 2)
    for p in ER.PYRAMIDS.values():
        lh, lw, _, _ = ER.lattice_of(p)
        assert len(p) * 2 * (lw + 3 * lh + 2) * 16 <= ER.TABLE_LDS
