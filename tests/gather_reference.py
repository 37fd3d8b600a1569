"""Plain-torch restatement of the pyramid gather and its two scatters (csrc/car_gather.hip, car_gather_bilinear_backward in
csrc/car_backward.hip, csrc/car_scatter.hip), and the input sets both test files use.  Test infrastructure: only ever the checker.

Two tiers, because the kernels' coordinate arithmetic is fp32 by contract (csrc/car_geom.h) and must not be charged to the sums:

  tier 1  taps32        car_bilinear_taps in float32 torch operations, one rounding per operation, in the header's order.  Its indices
                        and weights ARE "the taps" for everything below (tests/test_gather_reference.py holds it to the header bit for
                        bit, and to float64 grid_sample up to the float32 rounding of the coordinate).
  tier 2  gather_ref    out[row, c0_l + c]     = sum_t w_t map_l[m, idx_t, c]
          scatter_ref   dmap_l[m, idx_t, c]    = sum over gathers, points and taps with w_t != 0 of w_t dout[row, col_out + c0_l + c]
                        in `dtype` on tier 1's taps, with the bounds  sum |w| |texel|  per output element and  sum |w| |dout|  per
                        texel-channel, always in float64.  With float32 they restate the kernels' arithmetic: the forward's
                        ((nw + ne) + sw) + se of individually rounded products; the scatter adds rounded products one record at a time,
                        in row order on the CPU (index_add_ walks its index in order there; on a device the order is the device's).

A comparison divides an error by the bound (test_gather_hip.py):  ratio = max |x - ref64| / bound,  tolerance = 8 max(r32, 2^-22)."""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import torch

import parity_rule as PR

PLAIN, OWN, OTHER2 = 0, 1, 2                      # CAR_PLACE_* of include/car_hip.h
MAX_LEVELS, MAX_GATHERS = 4, 4
SCAN_BLOCK, SCAN_THREADS = 1024, 1024             # csrc/car_scatter.hip: counters per scan block, threads of the block-sum scan
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------------------------------
# tier 1
# ---------------------------------------------------------------------------------------------------------------------------------------
def texel_coord32(g: torch.Tensor, n: int) -> torch.Tensor:
    """((g + 1) n - 1) / 2 in float32, every operation rounded on its own."""
    assert g.dtype == torch.float32
    return ((g + 1.0) * float(n) - 1.0) / 2.0


def _axis32(i: torch.Tensor, n: int, mode: int):
    """One axis of car_bilinear_taps_px: texel coordinate -> (clamped index 0, clamped index 1, weight 0, weight 1, valid 0, valid 1)."""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=i.device)
    if mode == 0:
        i = torch.fmin(torch.fmax(i, f(0)), f(n - 1))                    # fmaxf / fminf: a NaN gives way to the other operand
    i = torch.where(i > -4.0, i, f(-4))                                  # !(i > -4): also NaN
    i = torch.where(i > float(n) + 4.0, f(n + 4), i)
    i0f = torch.floor(i)
    i1f = i0f + 1.0
    w0, w1 = i1f - i, i - i0f
    i0 = i0f.to(torch.int64)
    i1 = i0 + 1
    v0, v1 = (i0 >= 0) & (i0 < n), (i1 >= 0) & (i1 < n)
    return i0.clamp(0, n - 1), i1.clamp(0, n - 1), w0, w1, v0, v1


def taps32(grid: torch.Tensor, W: int, H: int, mode: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """grid [..., 2] float32 (x, y in grid_sample's [-1, 1]) -> idx [..., 4] int64 (y W + x, always addressable) and w [..., 4] float32,
    taps in the order nw, ne, sw, se.  mode 0 border, 1 zeros."""
    assert grid.dtype == torch.float32 and mode in (0, 1)
    x0, x1, wx0, wx1, vx0, vx1 = _axis32(texel_coord32(grid[..., 0], W), W, mode)
    y0, y1, wy0, wy1, vy0, vy1 = _axis32(texel_coord32(grid[..., 1], H), H, mode)
    zero = torch.zeros((), dtype=torch.float32, device=grid.device)
    idx = torch.stack([y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1], dim=-1)
    w = torch.stack([torch.where(vx0 & vy0, wx0 * wy0, zero), torch.where(vx1 & vy0, wx1 * wy0, zero),
                     torch.where(vx0 & vy1, wx0 * wy1, zero), torch.where(vx1 & vy1, wx1 * wy1, zero)], dim=-1)
    return idx, w


# ---------------------------------------------------------------------------------------------------------------------------------------
# tier 2
# ---------------------------------------------------------------------------------------------------------------------------------------
def place_row(place: int, V: int, m, i, pts: int):
    """Row of `out` / `dout` that point i of map m owns (car_gather_bilinear's rule); m, i: ints or int64 tensors."""
    if place == PLAIN:
        return m * pts + i
    if place == OWN:
        return (m * pts + i) * V + m % V
    assert place == OTHER2 and V == 2
    sc, s = m // 2, m % 2
    return ((sc * 2 + (1 - s)) * pts + i) * 2 + s


def rows_of(place: int, V: int, n_maps: int, pts: int) -> torch.Tensor:
    """[n_maps, pts] int64: place_row of every point."""
    m = torch.arange(n_maps)[:, None].expand(n_maps, pts)
    i = torch.arange(pts)[None, :].expand(n_maps, pts)
    return place_row(place, V, m, i, pts)


def n_rows(place: int, V: int, n_maps: int, pts: int) -> int:
    return n_maps * pts * (1 if place == PLAIN else V)


def gather_ref(maps: Sequence[torch.Tensor], grid: torch.Tensor, mode: int, dtype=torch.float64, device=None):
    """maps[l] [n_maps, H_l, W_l, C_l], grid [n_maps, pts, 2] float32 (on the CPU: tier 1 always runs there) -> (val [n_maps pts, sum C]
    in `dtype`, bound [same] float64), rows in (map, point) order: row m pts + i belongs at place_row(place, V, m, i, pts)."""
    device = device or maps[0].device
    n_maps, pts = grid.shape[:2]
    vals, bounds = [], []
    m = torch.arange(n_maps, device=device)[:, None, None]
    for t in maps:
        _, H, W, C = t.shape
        idx, w = taps32(grid.cpu(), W, H, mode)
        idx, w = idx.to(device), w.to(device)
        tex = t.to(device).reshape(n_maps, H * W, C)[m, idx]                         # [n_maps, pts, 4, C]
        p = tex.to(dtype) * w.to(dtype)[..., None]
        vals.append(((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3])
        bounds.append((tex.double().abs() * w.double()[..., None]).sum(2))
    return torch.cat(vals, -1).flatten(0, 1), torch.cat(bounds, -1).flatten(0, 1)


def scatter_runs(shapes: Sequence[Tuple[int, int, int]], n_maps: int, gathers, V: int, dout: torch.Tensor, col_out: int, dtypes, device=None):
    """shapes[l] = (H, W, C); gathers = [(grid [n_maps, pts, 2] float32 on the CPU, mode, place)]; dout [rows, ld] float32 ->
    ([dmaps[l] [n_maps, H, W, C] in dtype for dtype in dtypes], bounds[l] float64): the same records summed in each of `dtypes`."""
    device = device or dout.device
    d = dout.to(device)
    outs, bounds = [[] for _ in dtypes], []
    c0 = 0
    for (H, W, C) in shapes:
        accs = [torch.zeros(n_maps * H * W, C, dtype=dt, device=device) for dt in dtypes]
        bnd = torch.zeros(n_maps * H * W, C, dtype=torch.float64, device=device)
        for grid, mode, place in gathers:
            pts = grid.shape[1]
            idx, w = taps32(grid, W, H, mode)
            live = (w != 0).reshape(-1).to(device)
            flat = (idx + torch.arange(n_maps)[:, None, None] * (H * W)).reshape(-1).to(device)[live]         # (map, point, tap) order
            w = w.reshape(-1).to(device)[live]
            rows = rows_of(place, V, n_maps, pts)[:, :, None].expand(n_maps, pts, 4).reshape(-1).to(device)[live]
            g = d[:, col_out + c0:col_out + c0 + C][rows]                            # [records, C]
            for acc, dt in zip(accs, dtypes):
                acc.index_add_(0, flat, g.to(dt) * w.to(dt)[:, None])
            bnd.index_add_(0, flat, g.double().abs() * w.double()[:, None])
        for o, acc in zip(outs, accs):
            o.append(acc.view(n_maps, H, W, C))
        bounds.append(bnd.view(n_maps, H, W, C))
        c0 += C
    return outs, bounds


def scatter_ref(shapes, n_maps: int, gathers, V: int, dout: torch.Tensor, col_out: int, dtype=torch.float64, device=None):
    """(dmaps[l] in `dtype`, bounds[l] float64)."""
    outs, bounds = scatter_runs(shapes, n_maps, gathers, V, dout, col_out, (dtype,), device)
    return outs[0], bounds


def scatter_ref_r32(shapes, n_maps: int, gathers, V: int, dout: torch.Tensor, col_out: int, device=None):
    """(ref64[l], bounds[l], r32): the float64 run, its bounds, and the worst ratio of the float32 run of the same records."""
    (ref, f32), bounds = scatter_runs(shapes, n_maps, gathers, V, dout, col_out, (torch.float64, torch.float32), device)
    return ref, bounds, max(ratio(a, r, b) for a, r, b in zip(f32, ref, bounds))


def record_counts(shapes, n_maps: int, gathers) -> torch.Tensor:
    """Records per counter of the binned scatter: [n_maps T + 1] int64 (T = texels of all levels of a map; the closing counter is 0)."""
    T = sum(H * W for H, W, _ in shapes)
    cnt = torch.zeros(n_maps * T + 1, dtype=torch.int64)
    t0 = 0
    for (H, W, _) in shapes:
        for grid, mode, _place in gathers:
            idx, w = taps32(grid, W, H, mode)
            flat = idx + torch.arange(n_maps)[:, None, None] * T + t0
            cnt.index_add_(0, flat[w != 0], torch.ones(int((w != 0).sum()), dtype=torch.int64))
        t0 += H * W
    return cnt


# max |x - ref| / bound over the elements with a bound, every non-zero bound one; where the bound is 0 the value must be exactly 0, and a
# non-finite x anywhere fails the whole comparison
ratio = functools.partial(PR.ratio, bound_ok="nonzero", all_finite=True)
tolerance = PR.tolerance


# ---------------------------------------------------------------------------------------------------------------------------------------
# input sets (shared by test_gather_reference.py, which asserts the edges they exist for, and test_gather_hip.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
gen = PR.gen


def centre(x: int, W: int) -> float:
    """Grid coordinate of the centre of texel x of a W-wide axis."""
    return (2 * x + 1) / W - 1


SPECIALS = [(0.0, 0.0),                                      # the centre of every odd-sized level
            (centre(8, 16), centre(3, 16)), (centre(0, 16), centre(15, 16)),          # centres of the 16 x 16 level
            (-1.0, -1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0),                       # on +-1
            (-1.0 - 1 / 16, 0.3), (0.3, 1.0 + 1 / 16), (-1.0 - 1 / 16, 1.0 + 1 / 16),  # half a texel of the 16 x 16 level beyond the edge
            (1e10, -1e10), (-1e10, 0.2), (0.2, 1e10),                                 # far outside (geometry.project's scrub value)
            (NAN, 0.1), (0.1, NAN), (NAN, NAN), (INF, 0.1), (0.1, -INF), (-INF, INF), (INF, NAN)]
OUTSIDE = [(1e10, -1e10), (-1e10, 1e10), (NAN, NAN), (INF, -INF), (-3.0, 0.0), (0.0, 2.5), (NAN, 0.0), (1e10, 0.0)]


def edge_grid(n_maps: int, pts: int, seed: int, empty_map: int = -1) -> torch.Tensor:
    """[n_maps, pts, 2] float32: uniform in [-1.5, 1.5]^2, SPECIALS at the start of every map (rotated by the map's number, so that each
    lands in a different place of a ray block), and every point of map `empty_map` off the maps (no live tap with zeros padding)."""
    assert pts >= len(SPECIALS)
    grid = torch.rand(n_maps, pts, 2, generator=gen(seed)) * 3 - 1.5
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    for m in range(n_maps):
        grid[m, :len(SPECIALS)] = sp.roll(m, 0)
    if empty_map >= 0:
        out = torch.tensor(OUTSIDE, dtype=torch.float32)
        grid[empty_map] = out[torch.arange(pts) % len(OUTSIDE)]
    return grid


# name -> (levels (H, W, C), n_maps, pts, place, V, run, ld padding, col_out).  Every channel set, level size, placement and `run` of the
# forward's table; the same sets feed the scatters (which ignore run).  37 rays x 4 steps: the second ray block of 32 is ragged.
EDGE_SETS = {
    "wave4": (((16, 16, 512), (5, 3, 256), (1, 7, 64), (1, 1, 8)), 4, 148, PLAIN, 1, 4, 8, 4),
    "wave3": (((5, 3, 256), (16, 16, 64), (1, 7, 8)), 4, 148, OWN, 2, 1, 0, 0),
    "quad3": (((1, 1, 8), (1, 7, 12), (16, 16, 4)), 6, 148, OWN, 3, 5, 4, 0),           # 148 % 5 != 0: run is ignored
    "quad1": (((5, 3, 4),), 4, 148, OTHER2, 2, 2, 12, 8),
    "wave2": (((16, 16, 64), (5, 3, 8)), 4, 148, OTHER2, 2, 1, 4, 0),                     # other2 through the wave-task kernel
    "lanes": (((16, 16, 12), (5, 3, 20), (1, 7, 36)), 4, 148, PLAIN, 1, 1, 4, 4),        # 3, 5 and 9 quads: the reduce's lanes loop
}
FORWARD_SETS = ("wave4", "wave3", "wave2", "quad3", "quad1")


def _values(shape, seed):
    return torch.randn(*shape, generator=gen(seed))


@functools.lru_cache(maxsize=None)
def edge_set(name: str):
    shapes, n_maps, pts, place, V, run, pad, col_out = EDGE_SETS[name]
    C = sum(s[2] for s in shapes)
    rows = n_rows(place, V, n_maps, pts)
    return {"shapes": shapes, "n_maps": n_maps, "pts": pts, "place": place, "V": V, "run": run, "ld": col_out + C + pad, "col_out": col_out,
            "grid": edge_grid(n_maps, pts, 11, empty_map=2), "maps": [_values((n_maps, H, W, Cc), 12 + l) for l, (H, W, Cc) in enumerate(shapes)],
            "dout": _values((rows, C), 17)}


@functools.lru_cache(maxsize=None)
def deep_set():
    """One 16 x 16 level of 8 channels, zeros padding: texel (2, k) of map 0 holds exactly k records for k = 0 .. 9 (points on its centre: one
    live tap of weight 1), texel (8, 8) at least 50 000 (points within half a texel of its centre), every other texel of rows 0 .. 5 none,
    and map 1 nothing at all (every point off the map)."""
    W = 16
    on = [(centre(k, W), centre(2, W)) for k in range(10) for _ in range(k)]
    n_deep = 50000
    jit = (torch.rand(n_deep, 2, generator=gen(21)) - 0.5) * (2.0 / W) * 0.999
    deep = torch.tensor([centre(8, W), centre(8, W)]) + jit
    g0 = torch.cat([torch.tensor(on, dtype=torch.float32), deep.float()])
    pts = g0.shape[0]
    g1 = torch.tensor(OUTSIDE, dtype=torch.float32)[torch.arange(pts) % len(OUTSIDE)]
    grid = torch.stack([g0, g1])
    return {"shapes": ((16, 16, 8),), "n_maps": 2, "pts": pts, "place": PLAIN, "V": 1, "ld": 12, "col_out": 4, "mode": 1, "grid": grid,
            "dout": _values((2 * pts, 8), 22)}


@functools.lru_cache(maxsize=None)
def integer_set():
    """Exact in fp32 whatever the order: two 16 x 16 levels, coordinates on quarter texels from two texels outside to two texels outside (the
    weights are multiples of 1/16), dout integers in [-8, 8], at most 4096 records per texel: every partial sum is a multiple of 1/16 below
    4096 x 8 = 2^15, 19 bits of fp32's 24."""
    W, n_maps, pts = 16, 2, 6000
    q = torch.randint(-8, 4 * W + 5, (n_maps, pts, 2), generator=gen(31)).float() / 4.0            # ix in quarter texels, [-2, W + 1]
    grid = (2 * q + 1) / W - 1
    C = 12
    rows = n_rows(OWN, 2, n_maps, pts)
    return {"shapes": ((16, 16, 8), (16, 16, 4)), "n_maps": n_maps, "pts": pts, "V": 2, "ld": C + 4, "col_out": 0, "grid": grid, "q": q,
            "gathers": ((0, OWN), (1, OTHER2)), "dout": torch.randint(-8, 9, (rows, C), generator=gen(32)).float()}


@functools.lru_cache(maxsize=None)
def odd_set():
    """61 x 47 texels (W = 61: (gx + 1) W - 1 rounds differently fused and unfused), 64 channels."""
    n_maps, pts = 2, 3000
    return {"shapes": ((47, 61, 64),), "n_maps": n_maps, "pts": pts, "place": OWN, "V": 2, "ld": 72, "col_out": 8,
            "grid": edge_grid(n_maps, pts, 41), "dout": _values((n_rows(OWN, 2, n_maps, pts), 64), 42)}


@functools.lru_cache(maxsize=None)
def atomic_stride_set():
    """2 x 33 000 points x 256 channels = 16.9 M items, more than gather_bwd_kernel's 65536 x 256 threads: its grid-stride loop loops."""
    n_maps, pts = 2, 33000
    return {"shapes": ((16, 16, 256),), "n_maps": n_maps, "pts": pts, "place": PLAIN, "V": 1, "ld": 256, "col_out": 0,
            "grid": edge_grid(n_maps, pts, 51), "dout": _values((n_maps * pts, 256), 52)}


@functools.lru_cache(maxsize=None)
def bin_stride_set():
    """Four plain gathers x 2 maps x 530 000 points x four levels = 16.96 M items, more than bin_kernel's 65536 x 256 threads."""
    n_maps, pts = 2, 530000
    shapes = ((64, 64, 4), (32, 32, 4), (16, 16, 4), (8, 8, 4))
    base = [edge_grid(n_maps, 10000, 61 + j) for j in range(4)]                         # 53 copies of 10 000 points per map
    return {"shapes": shapes, "n_maps": n_maps, "pts": pts, "V": 1, "ld": 16, "col_out": 0,
            "base_grids": base, "grids": [b.repeat(1, 53, 1) for b in base], "modes": (0, 1, 1, 0), "dout": _values((n_maps * pts, 16), 66)}


FORWARD_ROWS, FORWARD_GRID = 32, 65536             # csrc/car_gather.hip: rows of a work group (both forward kernels), the grid's cap


def takes_wave_kernel(channels: Sequence[int]) -> bool:
    """launch_gather's choice, restated: the wave-task kernel when every level's float4 count is a power of two, at most 64 or a multiple
    of 64, and the rows one 64-lane task covers fit the group's 32 (so not a 4-channel level); the per-float4 kernel otherwise."""
    for c in channels:
        quads = c // 4
        if quads <= 0 or quads & (quads - 1) or not (quads <= 64 or quads % 64 == 0) or 64 // min(quads, 64) > FORWARD_ROWS:
            return False
    return True


def forward_groups(n_maps: int, pts: int, run: int) -> int:
    """Work groups of 32 rows the forward kernels walk: per (map, block of 32 rays, step) when run divides pts, per 32 rows otherwise."""
    if run > 1 and pts % run == 0:
        return n_maps * (-(-(pts // run) // FORWARD_ROWS)) * run
    return -(-(n_maps * pts) // FORWARD_ROWS)


# which forward kernel -> (level, run, seed): 2 x 1 100 000 rows each
FORWARD_STRIDE = {"wave": ((16, 16, 8), 1, 71),         # the issue's set: 68 750 groups of 32 rows, wave tasks (2 float4s per row)
                  "quad": ((16, 16, 12), 4, 73)}        # 3 float4s per row: the per-float4 kernel; 275 000 rays x 4 steps, 2 x 8594 x 4 = 68 752 groups


@functools.lru_cache(maxsize=None)
def forward_stride_set(kernel: str):
    """More groups of 32 rows than the 65536 work groups of the grid, for each of the two forward kernels: the group loop takes a second
    trip (its tap tables are rewritten behind the closing barrier)."""
    level, run, seed = FORWARD_STRIDE[kernel]
    n_maps, pts = 2, 1100000
    base = edge_grid(n_maps, 10000, seed)                                               # 110 copies of 10 000 points per map
    return {"shapes": (level,), "n_maps": n_maps, "pts": pts, "place": PLAIN, "V": 1, "run": run, "ld": level[2] + 8, "col_out": 4,
            "base_grids": [base], "grid": base.repeat(1, 110, 1), "maps": [_values((n_maps,) + level, seed + 1)]}


MIXED = ((1, OWN), (0, OTHER2), (1, PLAIN), (0, OTHER2))          # (mode, placement) of the binned scatter's gathers 0 .. 3


@functools.lru_cache(maxsize=None)
def mixed_set(n_gathers: int):
    """The first n_gathers of four gathers on wave3's levels, each with its own points, padding mode and placement, all reading one dout;
    gather k leaves map k alone (every point of that map off the maps: no record with zeros padding)."""
    base = edge_set("wave3")
    n_maps, pts, V = base["n_maps"], base["pts"], 2
    return {"shapes": base["shapes"], "n_maps": n_maps, "pts": pts, "V": V, "ld": base["ld"] + 8, "col_out": 4,
            "grids": [edge_grid(n_maps, pts, 90 + k, empty_map=k) for k in range(n_gathers)], "modes": tuple(m for m, _ in MIXED[:n_gathers]),
            "places": tuple(p for _, p in MIXED[:n_gathers]), "dout": _values((n_maps * pts * V, sum(c for _, _, c in base["shapes"])), 95)}


# the binned scatter's scan: n_maps, (H, W, C); n = n_maps H W + 1 counters, per = ceil(ceil(n / 1024) / 1024) block sums per scan thread
SCAN_SETS = {"n=1024": (1, (31, 33, 4)), "n=1025": (1, (32, 32, 4)), "per=2": (2, (725, 725, 4)), "per=4": (3, (1024, 1024, 4))}
SCAN_EXPECT = {"n=1024": (1024, 0, 1), "n=1025": (1025, 1, 1), "per=2": (1051251, 627, 2), "per=4": (3145729, 1, 4)}      # n, n mod 1024, per


def scan_geometry(name: str):
    n_maps, (H, W, _) = SCAN_SETS[name]
    n = n_maps * H * W + 1
    blocks = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    per = (blocks + SCAN_THREADS - 1) // SCAN_THREADS
    return n, blocks, per


def scan_targets(name: str) -> List[int]:
    """Counters that must hold a record: the first and last of a scan block and of a scan thread's run, at the start, in the middle and at the
    end of the counters, and the last texel (the one before the closing counter)."""
    n, blocks, per = scan_geometry(name)
    run = SCAN_BLOCK * per
    want = {0, n - 2}
    for unit in (SCAN_BLOCK, run):
        k_last = (n - 2) // unit
        for k in {0, 1, k_last // 2, k_last - 1, k_last}:
            for c in (k * unit, k * unit + unit - 1):
                if 0 <= c <= n - 2:
                    want.add(c)
    return sorted(want)


@functools.lru_cache(maxsize=None)
def scan_set(name: str):
    """Points clustered on the target counters' texels (their centres, and a few points within two texels of each), zeros padding: most scan
    blocks hold no record at all, the targets' blocks many."""
    n_maps, (H, W, C) = SCAN_SETS[name]
    targets = scan_targets(name)
    g = gen(81)
    per_map = [[] for _ in range(n_maps)]
    for c in targets:
        m, t = divmod(c, H * W)
        y, x = divmod(t, W)
        per_map[m].append((centre(x, W), centre(y, H)))
        for _ in range(6):
            dx, dy = (torch.rand(2, generator=g) * 4 - 2).tolist()
            per_map[m].append((centre(x, W) + dx * 2 / W, centre(y, H) + dy * 2 / H))
    pts = max(len(p) for p in per_map)
    grid = torch.full((n_maps, pts, 2), 1e10)                                          # a shorter map's tail: off the map
    for m, p in enumerate(per_map):
        grid[m, :len(p)] = torch.tensor(p, dtype=torch.float32)
    return {"shapes": ((H, W, C),), "n_maps": n_maps, "pts": pts, "place": PLAIN, "V": 1, "ld": 8, "col_out": 4, "mode": 1, "grid": grid,
            "dout": _values((n_maps * pts, C), 82), "targets": targets}


# ---------------------------------------------------------------------------------------------------------------------------------------
# every set by name (test_gather_reference.py builds one per test, not at import)
# ---------------------------------------------------------------------------------------------------------------------------------------
_BUILDERS = {"deep": deep_set, "integer": integer_set, "odd": odd_set, "atomic-stride": atomic_stride_set, "bin-stride": bin_stride_set,
             "forward-stride-wave": lambda: forward_stride_set("wave"), "forward-stride-quad": lambda: forward_stride_set("quad"),
             "mixed": lambda: mixed_set(MAX_GATHERS)}
SET_NAMES = tuple(EDGE_SETS) + tuple(_BUILDERS) + tuple(SCAN_SETS)


def named_set(name: str):
    return edge_set(name) if name in EDGE_SETS else scan_set(name) if name in SCAN_SETS else _BUILDERS[name]()


def coordinate_sets(name: str):
    """(set, levels, the distinct coordinate tensors of the set: a stride set repeats its base points; a set of several gathers has one per
    gather)."""
    s = named_set(name)
    return s, s["shapes"], s.get("base_grids") or s.get("grids") or [s["grid"]]
