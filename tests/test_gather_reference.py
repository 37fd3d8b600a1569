"""CPU checks of tests/gather_reference.py, the checker of tests/test_gather_hip.py: tier 1 (taps32) against the product's own header
through the host shim, bit for bit; tier 2 against float64 grid_sample and its autograd gradient, up to what the float32 coordinate
costs; and every input set of the GPU suite holds the edges it exists for (counted here, not assumed there)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gather_reference as GR
from test_geom_host import shim  # noqa: F401  (the fixture that compiles tests/host/car_geom_host.cpp)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name", GR.SET_NAMES)
def test_taps32_is_the_header_bit_for_bit(shim, name):  # noqa: F811
    """taps32 == car_bilinear_taps (compiled by g++ from csrc/car_geom.h), indices and weight bits, both padding modes, on every
    coordinate of every set the GPU suite runs, NaN and +-inf included."""
    _, shapes, grids = GR.coordinate_sets(name)
    for grid in grids:
        g = np.ascontiguousarray(grid.reshape(-1, 2).numpy())
        n = g.shape[0]
        for (H, W) in sorted({(s[0], s[1]) for s in shapes}):
            for mode in (0, 1):
                idx = np.zeros((n, 4), np.int32)
                w = np.zeros((n, 4), np.float32)
                shim.host_bilinear_taps(_ptr(g), n, W, H, mode, _ptr(idx), _ptr(w))
                ti, tw = GR.taps32(grid.reshape(-1, 2), W, H, mode)
                assert ti.min() >= 0 and ti.max() < H * W
                assert np.array_equal(ti.numpy().astype(np.int32), idx), (name, H, W, mode)
                assert np.array_equal(tw.numpy().view(np.int32), w.view(np.int32)), (name, H, W, mode)


# --- float64 grid_sample ---------------------------------------------------------------------------------------------------------------
def _cell64(ix, iy, W, H, mode):
    """The cell of (ix, iy) (float64 texel coordinates, already clamped for border padding): clamped indices [n, 4] and validity."""
    x0, y0 = torch.floor(ix).long(), torch.floor(iy).long()
    xs, ys = torch.stack([x0, x0 + 1, x0, x0 + 1], -1), torch.stack([y0, y0, y0 + 1, y0 + 1], -1)
    valid = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    return ys.clamp(0, H - 1) * W + xs.clamp(0, W - 1), valid


def _coords(grid, W, H, mode):
    """Texel coordinates of tier 1 (float32 arithmetic) and of float64 arithmetic on the same float32 grid, both after the border clamp /
    the +-4 guard, as float64."""
    out = []
    for g, n in ((grid[..., 0], W), (grid[..., 1], H)):
        i32, i64 = GR.texel_coord32(g, n).double(), ((g.double() + 1) * n - 1) / 2
        lo, hi = (0.0, n - 1.0) if mode == 0 else (-4.0, n + 4.0)
        out.append((i32.clamp(lo, hi), i64.clamp(lo, hi)))
    return out


WEIGHT_ROUNDING = 3 * 2.0 ** -24        # tier 1 forms 1 - frac and the product of two weights in float32: three roundings of numbers <= 1


@pytest.mark.parametrize("mode", [0, 1])
def test_tier2_is_float64_grid_sample_up_to_the_float32_coordinate(mode):
    """gather_ref / scatter_ref in float64 against F.grid_sample in float64 and its autograd gradient, finite coordinates (1e10 included).
    What may differ: tier 1's coordinate is float32.  Moving a point by (dx, dy) inside a cell changes a bilinear sample by at most
    |dx| (|ne - nw| + |se - sw|) + |dy| (|sw - nw| + |se - ne|); a rounding that carries the point over a cell's edge is covered by adding
    the same expression for the float64 cell.  Tier 1 also rounds its weights (WEIGHT_ROUNDING of sum |w| |texel|).  For the gradient the
    same per record: every weight moves by at most |dx| + |dy| + WEIGHT_ROUNDING, charged to the texels of both cells."""
    g = GR.gen(5)
    n_maps, pts = 3, 4000
    shapes = ((16, 16, 5), (47, 61, 3), (5, 3, 4), (1, 7, 2), (1, 1, 2))
    grid = GR.edge_grid(n_maps, pts, 6)
    grid = torch.where(torch.isfinite(grid), grid, torch.rand(n_maps, pts, 2, generator=g) * 2.4 - 1.2)
    maps = [torch.randn(n_maps, H, W, C, generator=g, dtype=torch.float64).requires_grad_(True) for H, W, C in shapes]
    Ct = sum(s[2] for s in shapes)
    dout = torch.randn(n_maps * pts, Ct, generator=g, dtype=torch.float64)
    want = torch.cat([F.grid_sample(t.permute(0, 3, 1, 2), grid.double()[:, None], mode="bilinear", padding_mode=("border", "zeros")[mode],
                                    align_corners=False)[:, :, 0].permute(0, 2, 1) for t in maps], -1).flatten(0, 1)
    got, mag = GR.gather_ref([t.detach() for t in maps], grid, mode)
    dgot, _ = GR.scatter_ref(shapes, n_maps, [(grid, mode, GR.PLAIN)], 1, dout.float(), 0)
    # the scatter reference reads a float32 dout: hand autograd the same numbers
    grads = torch.autograd.grad((want * dout.float().double()).sum(), maps)
    want = want.detach()
    worst_f, worst_b, c0 = 0.0, 0.0, 0
    for l, (H, W, C) in enumerate(shapes):
        (x32, x64), (y32, y64) = _coords(grid, W, H, mode)
        dx, dy = (x32 - x64).abs(), (y32 - y64).abs()
        flat = maps[l].detach().reshape(n_maps, H * W, C)
        m = torch.arange(n_maps)[:, None, None]
        bound = WEIGHT_ROUNDING * mag[:, c0:c0 + C].view(n_maps, pts, C) + 1e-15
        per_rec = (dx + dy + WEIGHT_ROUNDING)[..., None] * dout[:, c0:c0 + C].float().double().abs().view(n_maps, pts, C)
        bbound = torch.full((n_maps * H * W, C), 1e-15, dtype=torch.float64)
        for (cx, cy) in ((x32, y32), (x64, y64)):
            idx, valid = _cell64(cx, cy, W, H, mode)
            t = flat[m, idx] * valid[..., None]                                      # nw, ne, sw, se; a tap off the map reads zero
            bound = bound + dx[..., None] * ((t[:, :, 1] - t[:, :, 0]).abs() + (t[:, :, 3] - t[:, :, 2]).abs()) \
                + dy[..., None] * ((t[:, :, 2] - t[:, :, 0]).abs() + (t[:, :, 3] - t[:, :, 1]).abs())
            for k in range(4):
                bbound.index_add_(0, (idx[:, :, k] + m[:, :, 0] * H * W).reshape(-1), per_rec.reshape(-1, C))
        err = (got[:, c0:c0 + C].view(n_maps, pts, C) - want[:, c0:c0 + C].view(n_maps, pts, C)).abs()
        berr = (dgot[l] - grads[l]).abs().reshape(-1, C)
        worst_f, worst_b = max(worst_f, float((err / bound).max())), max(worst_b, float((berr / bbound).max()))
        c0 += C
    print(f"[parity] grid_sample64 mode={mode}: forward error / bound {worst_f:.3f}, gradient error / bound {worst_b:.3f}")
    assert worst_f <= 1.0 and worst_b <= 1.0, (worst_f, worst_b)


# --- the input sets hold their edges ---------------------------------------------------------------------------------------------------
def _edge_counts(grid, W, H):
    """How many points of `grid` sit on each edge, judged on the 16 x 16 level's arithmetic where a level matters."""
    g = grid.reshape(-1, 2)
    x, y = GR.texel_coord32(g[:, 0], W), GR.texel_coord32(g[:, 1], H)
    inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    return {"centre": int((inside & (x == x.floor()) & (y == y.floor())).sum()),
            "pm1": int(((g.abs() == 1).all(1)).sum()),
            "half_beyond": int(((x == -1) | (x == W) | (y == -1) | (y == H)).sum()),
            "far": int((g.abs() == 1e10).any(1).sum()),
            "nan": int(torch.isnan(g).any(1).sum()), "inf": int(torch.isinf(g).any(1).sum())}


EDGE_HOLDERS = tuple(GR.EDGE_SETS) + ("odd", "atomic-stride", "forward-stride-wave", "forward-stride-quad", "bin-stride", "mixed")


@pytest.mark.parametrize("name", EDGE_HOLDERS)
def test_edge_sets_hold_their_edges(name):
    s, shapes, grids = GR.coordinate_sets(name)
    if "base_grids" in s:                                                               # a stride set is whole copies of its base points
        for big, base in zip(s.get("grids", [s.get("grid")]), grids):
            assert big.shape[1] % base.shape[1] == 0
            assert torch.equal(big.view(torch.int32), base.repeat(1, big.shape[1] // base.shape[1], 1).view(torch.int32))
    for grid in grids:
        for (H, W, _) in shapes:
            c = _edge_counts(grid, W, H)
            # every level holds a centre; an even-sized level has none at (0, 0), and the bin stride set's 64, 32 and 8 none elsewhere
            assert c["centre"] >= 1 or (name == "bin-stride" and (H, W) in ((64, 64), (32, 32), (8, 8))), (name, H, W, c)
            assert min(c["pm1"], c["far"], c["nan"], c["inf"]) >= 4, (name, c)
            if (H, W) == (16, 16):
                assert c["half_beyond"] >= 3 and c["centre"] >= 2, (name, c)
            for mode in (0, 1):
                idx, w = GR.taps32(grid, W, H, mode)
                bad = ~torch.isfinite(grid).all(-1)
                assert bool(torch.isfinite(w).all())
                if mode == 1:
                    assert bool((w[bad] == 0).all())                     # NaN / inf with zeros padding: no live tap
                else:
                    assert bool((w[bad].sum(-1) == 1).all())             # with border padding: clamped onto the map, weights sum to 1
                on = (w == 1).any(-1)                                    # on a centre: one tap of weight exactly 1, three exactly 0
                assert bool(((w[on] == 0).sum(-1) == 3).all())
    if name in GR.EDGE_SETS:
        # map 2: no point touches it with zeros padding; with border padding every point is clamped onto it
        cnt = GR.record_counts(shapes, s["n_maps"], [(s["grid"], 1, s["place"])])
        T = sum(H * W for H, W, _ in shapes)
        assert int(cnt[2 * T:3 * T].sum()) == 0 and int(cnt[:2 * T].sum()) > 0 and int(cnt[3 * T:].sum()) > 0
        assert int(GR.record_counts(shapes, s["n_maps"], [(s["grid"], 0, s["place"])])[2 * T:3 * T].sum()) >= s["pts"] * len(shapes)
        rays = s["pts"] // s["run"] if s["pts"] % s["run"] == 0 else None
        if name == "wave4":
            assert s["run"] > 1 and rays % 32 != 0 and rays > 32         # a ragged last ray block, more than one block
        if name == "quad3":
            assert rays is None                                          # run is no divisor of pts: the entry ignores it
        assert s["ld"] % 4 == 0 and s["col_out"] % 4 == 0
    assert any(GR.edge_set(n)["col_out"] > 0 and GR.edge_set(n)["ld"] > GR.edge_set(n)["col_out"] + sum(c for _, _, c in GR.edge_set(n)["shapes"])
               for n in GR.FORWARD_SETS)


def test_mixed_set_empties_a_different_map_in_each_gather():
    """Gather k never touches map k with zeros padding and is clamped onto it with border padding; one, two and four gathers are prefixes
    of the same four; the placements cover all three and every gather reads the one dout inside its window."""
    four = GR.mixed_set(4)
    shapes, n_maps, pts = four["shapes"], four["n_maps"], four["pts"]
    T = sum(H * W for H, W, _ in shapes)
    assert len(four["grids"]) == GR.MAX_GATHERS and set(four["places"]) == {GR.PLAIN, GR.OWN, GR.OTHER2} and set(four["modes"]) == {0, 1}
    for n in (1, 2):
        s = GR.mixed_set(n)
        assert (s["modes"], s["places"]) == (four["modes"][:n], four["places"][:n]) and torch.equal(s["dout"], four["dout"])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(s["grids"], four["grids"]))
    for k, grid in enumerate(four["grids"]):
        zeros = GR.record_counts(shapes, n_maps, [(grid, 1, GR.PLAIN)])
        assert int(zeros[k * T:(k + 1) * T].sum()) == 0 and all(int(zeros[m * T:(m + 1) * T].sum()) > 0 for m in range(n_maps) if m != k)
        assert int(GR.record_counts(shapes, n_maps, [(grid, 0, GR.PLAIN)])[k * T:(k + 1) * T].sum()) >= pts * len(shapes)
    assert four["col_out"] > 0 and four["ld"] > four["col_out"] + sum(c for _, _, c in shapes)
    assert four["dout"].shape[0] == GR.n_rows(GR.OWN, four["V"], n_maps, pts)


def test_forward_sets_reach_both_kernels():
    """Which forward kernel a set runs (launch_gather's rule, restated): three edge sets and one stride set the wave-task kernel, two edge
    sets and the other stride set the per-float4 kernel."""
    chans = lambda s: [c for _, _, c in s["shapes"]]
    assert {n: GR.takes_wave_kernel(chans(GR.edge_set(n))) for n in GR.FORWARD_SETS} == {"wave4": True, "wave3": True, "wave2": True, "quad3": False,
                                                                                         "quad1": False}
    assert max(chans(GR.edge_set("wave4"))) // 4 == 128                                  # two segments of 64 lanes
    assert GR.takes_wave_kernel(chans(GR.forward_stride_set("wave"))) and not GR.takes_wave_kernel(chans(GR.forward_stride_set("quad")))


def test_stride_sets_exceed_their_grids():
    a, b = GR.atomic_stride_set(), GR.bin_stride_set()
    assert a["n_maps"] * a["pts"] * 256 > 65536 * 256                                    # gather_bwd_kernel: one thread per (point, channel)
    assert len(b["grids"]) * b["n_maps"] * b["pts"] * len(b["shapes"]) > 65536 * 256     # bin_kernel: one thread per (gather, point, level)
    assert len(b["grids"]) == GR.MAX_GATHERS and len(b["shapes"]) == GR.MAX_LEVELS
    for kernel in ("wave", "quad"):                                                      # groups of 32 rows, one forward kernel each
        f = GR.forward_stride_set(kernel)
        assert f["n_maps"] * f["pts"] == 2200000 and GR.forward_groups(f["n_maps"], f["pts"], f["run"]) > GR.FORWARD_GRID
    w, q = GR.forward_stride_set("wave"), GR.forward_stride_set("quad")
    assert w["run"] == 1 and GR.forward_groups(w["n_maps"], w["pts"], 1) == 68750
    rays = q["pts"] // q["run"]
    assert q["run"] > 1 and q["pts"] % q["run"] == 0 and rays % GR.FORWARD_ROWS != 0     # steps of rays, a ragged last ray block
    assert GR.forward_groups(q["n_maps"], q["pts"], q["run"]) == 68752


def test_deep_set_holds_every_record_count():
    s = GR.deep_set()
    cnt = GR.record_counts(s["shapes"], s["n_maps"], [(s["grid"], s["mode"], s["place"])])
    T = 256
    for k in range(10):
        assert int(cnt[2 * 16 + k]) == k, (k, int(cnt[2 * 16 + k]))       # texel (2, k): exactly k records (the 4-wide loop and remainders 0..3)
    assert int(cnt[8 * 16 + 8]) >= 50000 and int(cnt.max()) == int(cnt[8 * 16 + 8])
    assert int(cnt[:6 * 16].sum()) == 45                                   # nothing else in rows 0 .. 5
    assert int(cnt[T:].sum()) == 0                                         # map 1: no point touches it
    assert {int(v) for v in cnt[:T]} >= set(range(10))


@pytest.mark.parametrize("name", list(GR.SCAN_SETS))
def test_scan_sets_put_records_on_the_scan_edges(name):
    s = GR.scan_set(name)
    n, blocks, per = GR.scan_geometry(name)
    assert (n, n % 1024, per) == GR.SCAN_EXPECT[name]
    cnt = GR.record_counts(s["shapes"], s["n_maps"], [(s["grid"], s["mode"], s["place"])])
    assert cnt.numel() == n and int(cnt[-1]) == 0
    live = torch.nonzero(cnt).flatten()
    run = 1024 * per
    assert int(cnt[0]) > 0 and int(cnt[n - 2]) > 0                         # the first counter and the last texel
    for unit in (1024, run):                                               # a scan block; a scan thread's run of `per` blocks
        first, last = live[live % unit == 0], live[live % unit == unit - 1]
        assert first.numel() >= 1 and (last.numel() >= 1 or unit - 1 > n - 2), (name, unit)      # n = 1024: counter 1023 is the closing one
        if n - 2 >= 2 * unit:
            assert (first // unit).unique().numel() >= 2 and (last // unit).unique().numel() >= 2 and int((first // unit).max()) >= 1
    for c in s["targets"]:
        assert int(cnt[c]) > 0, (name, c)
    # clustered: most scan blocks are empty, so a wrong block offset moves every later record
    occupied = (live // 1024).unique().numel()
    assert occupied <= max(2, blocks // 4) or blocks <= 2, (occupied, blocks)
    if per > 1:                                                            # records in a block that is not the first of its thread's run
        assert bool(((live // 1024) % per != 0).any())


def test_integer_set_is_exact_in_fp32():
    s = GR.integer_set()
    shapes, n_maps, grid = s["shapes"], s["n_maps"], s["grid"]
    assert all(H & (H - 1) == 0 and W & (W - 1) == 0 for H, W, _ in shapes)
    assert bool((s["dout"] == s["dout"].round()).all()) and float(s["dout"].abs().max()) <= 8
    assert bool((s["q"] * 4 == (s["q"] * 4).round()).all())
    for (H, W, _) in shapes:
        assert torch.equal(GR.texel_coord32(grid[..., 0], W), s["q"][..., 0]) and torch.equal(GR.texel_coord32(grid[..., 1], H), s["q"][..., 1])
        for mode in (0, 1):
            w16 = GR.taps32(grid, W, H, mode)[1] * 16
            assert bool((w16 == w16.round()).all())
    gathers = [(grid, mode, place) for mode, place in s["gathers"]]
    assert int(GR.record_counts(shapes, n_maps, gathers).max()) <= 4096
    ref, bound = GR.scatter_ref(shapes, n_maps, gathers, s["V"], s["dout"], 0)
    f32, _ = GR.scatter_ref(shapes, n_maps, gathers, s["V"], s["dout"], 0, torch.float32)
    for a, b_, c in zip(ref, bound, f32):
        assert float(b_.max()) * 16 < 2 ** 24                              # no partial sum leaves fp32's 24 bits
        assert bool((a * 16 == (a * 16).round()).all()) and torch.equal(c.double(), a)
