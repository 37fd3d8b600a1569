"""Plain-torch restatement of the per-texel-projected first layer  h = relu(sum_t w_t G[tap_t] + W1pt pe + b1)  in its five forms
(csrc/car_encode.hip: car_gather_encode, car_gather_encode_rows, car_lattice_encode_rows; csrc/car_lattice.hip: car_merge_lattice,
car_merge_lattice_max; csrc/car_linear16.hip: car_lattice_encode_linear; and car_fused_rows of csrc/car_fused.hip on a merged lattice),
the dtype a parameter, plus the input sets test_encode_reference.py (CPU) and test_encode_hip.py (GPU, through the C ABI) share.  Test
infrastructure: only ever the checker; no GPU code, no ctypes.

The taps are float32 by contract (csrc/car_geom.h) and are not charged to the sums: the per-level forms take gather_reference.taps32,
the lattice forms fused_reference.lattice_taps run in float32 (fused_reference._gather ties the taps' dtype to the sums', so the four
lattice taps are summed here), the merge gather_reference's axis rule at the nodes' texel coordinates (formed in `dtype`: the one division there
is exact for powers of two and rounds for a factor of 3, which the float32 run therefore carries).  On those taps every function sums
in `dtype`; with float32 it restates the kernels' order with one fused multiply-add per tap (fma32: exact, single rounding).  Every
value comes with its sum of magnitudes, always float64:

    B_lat = sum_l sum_t |w| |G_l|                      B_h = sum |w| |G| (or sum |w| B_lat) + |wpt[:, :3]| |pe| + |wpt[:, 3]|
    B_y   = |W2| B_h + |b2|   (h's magnitudes carried through, as fused_reference does)

A comparison divides an error by that bound (parity_rule.ratio); tolerance = 8 max(r32, 2^-22)."""
from __future__ import annotations

import functools
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F

import fused_reference as FR
import gather_reference as GR
import parity_rule as PR

F32, F64 = torch.float32, torch.float64
MODE_BIT = 30
RELU_IN, RELU_OUT, ACCUM = 1, 2, 4                  # CAR_LIN_* of include/car_hip.h
ROW_BLOCK = 16                                      # rows of a workgroup of csrc/car_encode.hip
TABLE_LDS = 52 * 1024                               # csrc/car_lattice.hip car_launch_merge: larger axis tables take the table-free kernel

ratio, tolerance, fp16_linear = PR.ratio, PR.tolerance, FR.fp16_linear


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf(a, b, c) on float32 tensors, rounded once: the product of two float32 is exact in float64; the float64 sum is made
    round-to-odd from its exact error (two-sum), so that the closing rounding to float32 is the only one."""
    p, cc = a.double() * b.double(), c.double()
    s = p + cc
    bb = s - p
    err = (p - (s - bb)) + (cc - bb)
    bits = s.contiguous().view(torch.int64)
    fix = torch.isfinite(s) & (err != 0) & ((bits & 1) == 0)
    step = torch.where((err > 0) == (s > 0), 1, -1)
    return torch.where(fix, bits + step, bits).view(F64).float()


def _acc(acc, w, g, dtype):
    """acc + w g per channel: w [...], g [..., C]."""
    if dtype == F32:
        return fma32(w[..., None].expand_as(g), g, acc)
    return acc + w.to(dtype)[..., None] * g.to(dtype)


def split_src(src: torch.Tensor):
    s = src.long()
    return s & ((1 << MODE_BIT) - 1), (s >> MODE_BIT) & 1


# ---- the implicit two-view row rule ----------------------------------------------------------------------------------------------------------
def implicit_rows(V: int, n_maps: int, pts: int, pixel_val: torch.Tensor, grid_in: torch.Tensor):
    """car_gather_encode's rows as an explicit list: pixel_val [n_maps pts, 2], grid_in [n_maps pts, V, 2] -> (src [n_maps pts V] int32 =
    map | padding mode << 30, grid [n_maps pts V, 2]).  Sample i = (n, j) of map n = (scene, own view); row i V + s is its source view s:
    the own view reads map n at pixel_val[i] with border padding, another view map (scene, s) at grid_in[i, s] with zeros padding."""
    assert V == 2 and n_maps % V == 0
    n = torch.arange(n_maps).repeat_interleave(pts)                                       # map of sample i
    scene, own_view = n // V, n % V
    src = torch.empty(n_maps * pts, V, dtype=torch.int64)
    grid = torch.empty(n_maps * pts, V, 2, dtype=pixel_val.dtype)
    for s in range(V):
        own = own_view == s
        src[:, s] = torch.where(own, n, (scene * V + s) | (1 << MODE_BIT))
        grid[:, s] = torch.where(own[:, None], pixel_val, grid_in[:, s])
    return src.reshape(-1).to(torch.int32), grid.reshape(-1, 2).contiguous()


# ---- the per-level form ----------------------------------------------------------------------------------------------------------------------
def _point_term(pe, wpt, dtype):
    """(wpt[:, :3] . pe[:3] + wpt[:, 3]  [rows, C] in `dtype`: float32 as fmaf(wz, pz, fmaf(wy, py, wx px)) + b; its magnitudes, float64)."""
    p = pe[:, :3]
    mag = p.double().abs() @ wpt[:, :3].double().abs().T + wpt[:, 3].double().abs()
    if dtype == F32:
        rows, Cc = pe.shape[0], wpt.shape[0]
        col = lambda k: wpt[None, :, k].expand(rows, Cc)
        pk = lambda k: p[:, k, None].expand(rows, Cc)
        t = fma32(col(2), pk(2), fma32(col(1), pk(1), col(0) * pk(0)))
        return t + col(3), mag
    return p.to(dtype) @ wpt[:, :3].to(dtype).T + wpt[:, 3].to(dtype), mag


def level_taps(src, grid, W: int, H: int):
    """Tier-1 taps of explicit rows on one level: (idx [rows, 4] into the level's n_maps H W texels, w [rows, 4] float32)."""
    m, mode = split_src(src)
    i0, w0 = GR.taps32(grid, W, H, 0)
    i1, w1 = GR.taps32(grid, W, H, 1)
    zeros = (mode == 1)[:, None]
    return torch.where(zeros, i1, i0) + m[:, None] * (H * W), torch.where(zeros, w1, w0)


def encode_levels(G_levels: Sequence[torch.Tensor], src, grid, pe, wpt, dtype=F64):
    """G_levels[l] [n_maps, H_l, W_l, C]; src [rows] int32; grid [rows, 2] float32; pe [rows, 4] (the fourth float unused); wpt [C, 4] =
    (w0, w1, w2, b) -> (h [rows, C] in `dtype`, B_h float64).  float32: levels ascending, taps nw ne sw se, one fma each from zero, then
    acc + point term, relu — csrc/car_encode.hip."""
    rows, Cc = grid.shape[0], wpt.shape[0]
    acc = torch.zeros(rows, Cc, dtype=dtype)
    mag = torch.zeros(rows, Cc, dtype=F64)
    for t in G_levels:
        _, H, W, _ = t.shape
        idx, w = level_taps(src, grid, W, H)
        flat = t.reshape(-1, Cc)
        for k in range(4):
            g = flat[idx[:, k]]
            acc = _acc(acc, w[:, k], g, dtype)
            mag += w[:, k].double()[:, None] * g.double().abs()
    pt, pmag = _point_term(pe, wpt, dtype)
    return F.relu(acc + pt), mag + pmag


# ---- the merged lattice ----------------------------------------------------------------------------------------------------------------------
def lattice_of(sizes: Sequence[Sequence[int]]):
    """car_lattice_of: sizes[l] = (H_l, W_l) -> (lh, lw, pad, r_l), or None where a level is not the same integer factor coarser than the
    widest in both directions."""
    hm, wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
    r = []
    for h, w in (s[:2] for s in sizes):
        if h <= 0 or w <= 0 or hm % h or wm % w or hm // h != wm // w:
            return None
        r.append(hm // h)
    rmax = max(r)
    return 2 * hm + 2 * rmax + 1, 2 * wm + 2 * rmax + 1, rmax + 1, tuple(r)


def takes_table_free_kernel(sizes) -> bool:
    """car_launch_merge's choice: axis tables of n_levels x 2 modes x (lw + ny) entries of 16 bytes, ny >= 2 whatever the device."""
    _, lw, _, _ = lattice_of(sizes)
    return len(sizes) * 2 * (lw + 2) * 16 > TABLE_LDS


def _node_axis(n_nodes: int, pad: int, r: int, n: int, mode: int, dtype, device):
    """One axis of every node of a level r times coarser: texel coordinate (j - pad + 1 - r) / (2 r), one division of two exact integers
    in `dtype` (float32: the kernel's; a factor of 3 rounds there), through gather_reference's axis rule, which keeps its operand's dtype."""
    j = torch.arange(n_nodes, device=device)
    num = (j - pad + 1 - r).to(dtype)
    i = num / torch.full_like(num, float(2 * r))          # a tensor divisor: a device divides by a scalar as a product with its rounded inverse
    return GR._axis32(i, n, mode)


def merge(G_levels: Sequence[torch.Tensor], dtype=F64, device=None):
    """G_levels[l] [n_maps, H_l, W_l, C] -> (lattice [n_maps, 2, lh, lw, C] in `dtype`, B_lat float64, (lh, lw, pad)): node j of map
    (m, mode) = sum over the levels, from the last index down, of the level's bilinear interpolation at the node, with the level's own
    padding rule; float32: taps nw ne sw se, one fma each from zero — csrc/car_lattice.hip merge_kernel."""
    device = device or G_levels[0].device
    n_maps, Cc = G_levels[0].shape[0], G_levels[0].shape[-1]
    lh, lw, pad, r = lattice_of([t.shape[1:3] for t in G_levels])
    lat = torch.zeros(n_maps, 2, lh, lw, Cc, dtype=dtype, device=device)
    mag = torch.zeros(n_maps, 2, lh, lw, Cc, dtype=F64, device=device)
    zero = torch.zeros((), dtype=dtype, device=device)
    for mode in (0, 1):
        for l in range(len(G_levels) - 1, -1, -1):
            t = G_levels[l].to(device)
            _, H, W, _ = t.shape
            x0, x1, wx0, wx1, vx0, vx1 = _node_axis(lw, pad, r[l], W, mode, dtype, device)
            y0, y1, wy0, wy1, vy0, vy1 = _node_axis(lh, pad, r[l], H, mode, dtype, device)
            for ys, wy, vy, xs, wx, vx in ((y0, wy0, vy0, x0, wx0, vx0), (y0, wy0, vy0, x1, wx1, vx1),
                                           (y1, wy1, vy1, x0, wx0, vx0), (y1, wy1, vy1, x1, wx1, vx1)):
                w = torch.where(vy[:, None] & vx[None, :], wy[:, None] * wx[None, :], zero)             # [lh, lw] in dtype
                g = t[:, ys][:, :, xs]                                                             # [n_maps, lh, lw, C]
                lat[:, mode] = _acc(lat[:, mode], w[None].expand(n_maps, lh, lw), g, dtype)
                mag[:, mode] += w.double()[None, :, :, None] * g.double().abs()
    return lat, mag, (lh, lw, pad)


def lattice_max(lattice: torch.Tensor) -> torch.Tensor:
    """What car_merge_lattice_max leaves in gmax: the largest magnitude of the lattice."""
    return lattice.abs().max()


def encode_lattice(lattice, pad: int, src, grid, pe, wpt, dtype=F64, mag=None):
    """lattice [n_maps, 2, lh, lw, C] -> (h [rows, C] in `dtype`, B_h float64): four taps of the row's (map, mode) lattice on
    fused_reference.lattice_taps run in float32; a zeros-mode row on or beyond the outer ring reads exact zeros (h = relu(point term)).
    `mag` (B_lat of merge) replaces |lattice| in the bound: the merge's rounding is then the form's own."""
    lh, lw, Cc = lattice.shape[2], lattice.shape[3], lattice.shape[4]
    m, mode = split_src(src)
    node, ring, w = FR.lattice_taps(grid, lw, lh, pad, F32)
    dead = ring & (mode == 1)
    w = torch.where(dead[:, None], torch.zeros_like(w), w)
    base = torch.where(dead, torch.zeros_like(node), (m * 2 + mode) * (lh * lw) + node)
    flat = lattice.reshape(-1, Cc)
    fmag = flat.double().abs() if mag is None else mag.reshape(-1, Cc)
    acc = torch.zeros(grid.shape[0], Cc, dtype=dtype)
    bound = torch.zeros(grid.shape[0], Cc, dtype=F64)
    for k, off in enumerate((0, 1, lw, lw + 1)):
        acc = _acc(acc, w[:, k], flat[base + off], dtype)
        bound += w[:, k].double()[:, None] * fmag[base + off]
    pt, pmag = _point_term(pe, wpt, dtype)
    return F.relu(acc + pt), bound + pmag


def encode_linear(h, B_h, W2, b2, flags: int = 0, dtype=F64, linear: Optional[Callable] = None, Y0=None):
    """(y = act(h W2^T + b2 (+ Y0)) in `dtype`, B_y = |W2| B_h + |b2| (+ |Y0|) float64).  `linear(x, W, b)` replaces the layer's arithmetic
    (the fp16 emulation); the bound never uses it."""
    assert not flags & RELU_IN
    y = FR._lin(linear, h.to(dtype) if linear is None else h, W2, b2, dtype)
    B = B_h @ W2.double().abs().T + (0 if b2 is None else b2.double().abs())
    if flags & ACCUM:
        y, B = y + Y0.to(dtype), B + Y0.double().abs()
    return (F.relu(y) if flags & RELU_OUT else y), B


# ---- the reference's own order of operations (models.py:278, 317, 330-341) ---------------------------------------------------------------------
def project(F_levels: Sequence[torch.Tensor], W1: torch.Tensor):
    """G_l = F_l W1[:, ch_l]^T: every raw level [n_maps, H, W, c_l] through its columns of W1 [C, sum c_l + 3]."""
    out, c0 = [], 0
    for t in F_levels:
        c = t.shape[-1]
        out.append(t @ W1[:, c0:c0 + c].to(t.dtype).T)
        c0 += c
    return out


def literal(F_levels, W1, b1, src, grid, pt, dtype=F64):
    """grid_sample every raw level at the rows' points (its own padding mode per row), concatenate, append tanh(pt / 5), one
    W1 [f; pe] + b1, relu."""
    m, mode = split_src(src)
    feats = []
    for t in F_levels:
        maps = t.to(dtype).permute(0, 3, 1, 2)[m]                                             # [rows, c, H, W]
        g = grid.to(dtype)[:, None, None, :]
        s = [F.grid_sample(maps, g, mode="bilinear", padding_mode=name, align_corners=False)[:, :, 0, 0] for name in ("border", "zeros")]
        feats.append(torch.where((mode == 1)[:, None], s[1], s[0]))
    x = torch.cat(feats + [torch.tanh(pt.to(dtype) / 5)], dim=-1)
    return F.relu(x @ W1.to(dtype).T + b1.to(dtype))


# ---- input sets (shared by test_encode_reference.py, which asserts what they hold, and test_encode_hip.py) ------------------------------------
gen = GR.gen
PTS = 37                                            # n_maps x 37 x 2 rows: 148 and 296, neither a multiple of 16
# name -> (levels (H, W), Cg, n_maps): 1 to 4 levels, every Cg, one and two scenes
LEVEL_SETS = {"L1-C4": (((5, 3),), 4, 2), "L2-C12": (((16, 16), (5, 3)), 12, 4), "L3-C64": (((5, 3), (16, 16), (1, 7)), 64, 2),
              "L4-C576": (((16, 16), (5, 3), (1, 7), (1, 1)), 576, 4)}
PYRAMIDS = {"p3": ((4, 4), (8, 8), (16, 16)), "f3": ((2, 3), (6, 9)), "one": ((16, 16),), "p4": ((2, 4), (4, 8), (8, 16), (16, 32))}
TABLE_FREE = ((1, 26), (2, 52), (4, 104), (8, 208))  # 33 x 433 nodes: 4 levels x 2 modes x (433 + ny) x 16 bytes > 52 KB
LATTICE_ROWS = (1, 15, 17, 148)
LINEAR_CASES = ((64, 32), (193, 128), (4097, 288))  # (rows, N)
C = FR.C


def levels_of(sizes, n_maps: int, channels: int, seed: int):
    return [torch.randn(n_maps, h, w, channels, generator=gen(seed + l)) for l, (h, w) in enumerate(sizes)]


def point_table(channels: int, seed: int):
    """wpt [C, 4] = (w0, w1, w2, b)."""
    return (0.3 * torch.randn(channels, 4, generator=gen(seed))).contiguous()


def point_rows(rows: int, seed: int):
    """pe [rows, 4]: tanh of a Gaussian, the unused fourth float NaN."""
    pe = torch.tanh(torch.randn(rows, 4, generator=gen(seed)))
    pe[:, 3] = float("nan")
    return pe.contiguous()


@functools.lru_cache(maxsize=None)
def level_set(name: str):
    """A per-level input set: levels, the implicit form's pixel_val / grid_in / ptenc, and an explicit list over the same number of rows
    whose maps and padding modes change from row to row."""
    sizes, Cg, n_maps = LEVEL_SETS[name]
    S, rows = n_maps * PTS, n_maps * PTS * 2
    seed = 100 + 10 * len(sizes)
    g = gen(seed + 9)
    src = torch.randint(0, n_maps, (rows,), generator=g) | (torch.randint(0, 2, (rows,), generator=g) << MODE_BIT)
    return {"sizes": sizes, "Cg": Cg, "n_maps": n_maps, "pts": PTS, "rows": rows, "levels": levels_of(sizes, n_maps, Cg, seed),
            "pixel_val": GR.edge_grid(n_maps, PTS, seed + 5).reshape(S, 2).contiguous(),
            "grid_in": GR.edge_grid(n_maps, 2 * PTS, seed + 6).reshape(S, 2, 2).contiguous(),
            "pe": point_rows(rows, seed + 7), "wpt": point_table(Cg, seed + 8),
            "src": src.to(torch.int32), "grid": GR.edge_grid(1, rows, seed + 4)[0].contiguous()}


def edge_rows(n_maps: int, rows: int, seed: int):
    """(src, grid, pe) of `rows` explicit rows on gather_reference.edge_grid's points (SPECIALS first, as far as they fit), maps and modes
    changing from row to row; row 0 is a zeros-mode row far outside."""
    g = gen(seed)
    n = max(rows, len(GR.SPECIALS))
    src = torch.randint(0, n_maps, (n,), generator=g) | (torch.randint(0, 2, (n,), generator=g) << MODE_BIT)
    grid = GR.edge_grid(1, n, seed + 1)[0].roll(1, 0)
    grid[0] = torch.tensor([1e10, -1e10])
    src[0] = (n_maps - 1) | (1 << MODE_BIT)
    return src[:rows].to(torch.int32).contiguous(), grid[:rows].contiguous(), point_rows(rows, seed + 2)


def dyadic_grid(sizes, n: int, seed: int):
    """[n, 2] float32, every coordinate a multiple of 2^-10 in [-1.5, 1.5]: random ones, then (+-1, +-1), the centre, and every pair of
    lattice-node coordinates (x = (u + 1) / W - 1, u an integer from ring to ring) that is such a multiple — the ring itself included where
    it is one."""
    lh, lw, pad, _ = lattice_of(sizes)
    hm, wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
    q = torch.randint(-1536, 1537, (n, 2), generator=gen(seed)).double() / 1024

    def nodes(count, width):
        x = (torch.arange(count, dtype=F64) - pad + 1) / width - 1
        return x[(x * 1024 == (x * 1024).round()) & (x.abs() <= 1.5)]
    nx, ny = nodes(lw, wm), nodes(lh, hm)
    k = max(len(nx), len(ny))
    on = torch.stack([nx[torch.arange(k) % len(nx)], ny[(torch.arange(k) * 3) % len(ny)]], dim=1)
    ring = torch.stack([nx[:1].expand(len(ny)), ny], dim=1)                                      # the first node column: the ring where representable
    fixed = torch.cat([torch.tensor([(-1.0, -1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (0.0, 0.0)], dtype=F64), on, ring])
    assert len(fixed) <= n
    q[:len(fixed)] = fixed
    return q.float().contiguous()


# the five-forms sets: name -> (pyramid, R, P) of car_fused_rows' [n_sets = 2][R][P] samples x 2 components = 140 and 132 rows
FORMS = {"p3": (5, 7), "f3": (11, 3)}
FORMS_SETS, FORMS_COMP = 2, 2


@functools.lru_cache(maxsize=None)
def forms_set(name: str):
    """Dyadic rows over a pyramid, 576 wide, two maps; row = sample * 2 + comp, every (set, comp) its own (map, padding mode) — all four —
    as car_fused_rows requires; weights of both layers."""
    sizes, (R, P) = PYRAMIDS[name], FORMS[name]
    rows = FORMS_SETS * R * P * FORMS_COMP
    seed = 300 + len(sizes)
    st = torch.arange(FORMS_SETS).repeat_interleave(R * P)[:, None].expand(-1, FORMS_COMP)
    comp = torch.arange(FORMS_COMP)[None, :].expand(FORMS_SETS * R * P, -1)
    src = (((st + comp) % 2) | (comp << MODE_BIT)).reshape(-1).to(torch.int32)
    g = gen(seed + 9)
    W1pt, b1 = 0.3 * torch.randn(C, 3, generator=g), 0.3 * torch.randn(C, generator=g)
    W2, b2 = torch.randn(FR.E, C, generator=g) / C ** 0.5, 0.1 * torch.randn(FR.E, generator=g)
    return {"sizes": sizes, "n_maps": 2, "R": R, "P": P, "rows": rows, "levels": levels_of(sizes, 2, C, seed), "src": src.contiguous(),
            "grid": dyadic_grid(sizes, rows, seed + 5), "pe": point_rows(rows, seed + 6), "W1pt": W1pt, "b1": b1,
            "wpt": torch.cat([W1pt, b1[:, None]], dim=1).contiguous(), "W2": W2.contiguous(), "b2": b2}


def second_layer(N: int, seed: int = 400):
    g = gen(seed + N)
    return (torch.randn(N, C, generator=g) / C ** 0.5).contiguous(), 0.1 * torch.randn(N, generator=g)
