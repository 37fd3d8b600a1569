"""Plain-torch restatement of the fused per-sample kernel (csrc/car_fused.hip: car_fused_samples, car_fused_samples_parts,
car_fused_samples_f16, car_fused_rows), the dtype a parameter, plus the input sets both test_fused_reference.py (CPU) and
test_fused_hip.py (GPU, through the C ABI) build from.  Test infrastructure: only ever the checker; no GPU, no ctypes.

    h_sv  = relu( four taps of the (view, padding mode) lattice + W1[:, C:C+3] tanh(pt_in[sv] / 5) + b1 )        sv = 0, 1
            source sv == own view v: border lattice of view v at `grid`;  sv != v: zeros lattice of view sv at grid_in[sv], and a
            sample on or beyond the lattice's outer ring there contributes exact zeros (car_lattice_taps flag 4)
    e     = [W2 h_0 + b2 ; W2 h_1 + b2]
    k1    = key_map(e) ;  x = relu(query_embed(g)) ;  logit = <key_map_2(relu(k1)), query_embed_2(x)> / 16      (UNFOLDED: the fold M, v,
            u, c of csrc/car_fused_layout.h is the kernel's business)
    part  = sum over the live steps j of a group of car_fused_tile_steps() steps of exp(logit_j - max_j logit) e_j

Weights come raw under the names of models.py (`query_encode_latent`: only its point columns and bias enter — the 576 feature columns
are already inside the lattice).  Every output comes with the sum of magnitudes that goes with it, always computed in float64 from the
float64 run:  B_h = sum_t w_t |lat_t| + |W1pt| |tanh| + |b1|,  B_e = |W2| B_h + |b2| (h's magnitudes carried through: the
gather's error goes with B_h, not with what is left of h after cancellation and the ReLU),  B_k1 = |Wk1| |e| + |bk1|,
B_x = |Wq1| |g| + |bq1|,  B_logit = (|r|^T (|M| |x| + |v|) + |u|^T |x| + |c|) / 16 with r = relu(k1), M = Wk2^T Wq2, v = Wk2^T bq2,
u = Wq2^T bk2, c = <bk2, bq2>.  A comparison divides an error by that bound (test_fused_hip.py)."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F

from cross_attention_renderer_amd import synthetic as S
from parity_rule import FACTOR, FLOOR, gen, ratio, tolerance  # noqa: F401  (the suites' rule: max |got - ref64| / bound, 8 x max(r, 2^-22))

C, E, D, G = 576, 288, 128, 16
TILE_RAYS, TILE_STEPS = 24, 8                            # a workgroup of csrc/car_fused.hip: 24 rays x 8 steps
SHAPES = {"query_encode_latent": (C, C + 3), "query_encode_latent_2": (E, C), "key_map": (D, C), "key_map_2": (D, D),
          "query_embed": (D, G), "query_embed_2": (D, D)}
F64 = torch.float64
FMAX = 3.4028234663852886e38


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def lattice_scale(lh: int, lw: int, pad: int):
    """(sx, sy): width and height of the finest level, as launch_fused derives them."""
    return float((lw - 2 * pad + 1) // 2), float((lh - 2 * pad + 1) // 2)


def lattice_taps(grid, lw: int, lh: int, pad: int, dtype=F64):
    """csrc/car_geom.h car_lattice_taps, operation for operation, in `dtype`: grid [..., 2] -> north-west node [...] (long), on-or-beyond
    the-outer-ring flag [...] (bool), weights [..., 4] (nw, ne, sw, se)."""
    sx, sy = lattice_scale(lh, lw, pad)
    g = grid.to(dtype)
    one = torch.ones((), dtype=dtype)

    def axis(x, s, n):
        u = (x + one) * s - one
        lo, hi = torch.tensor(-float(pad), dtype=dtype), torch.tensor(float(n - 1 - pad), dtype=dtype)
        u = torch.where(u > lo, u, lo)                                        # also NaN
        u = torch.where(u > hi, hi, u)
        f = torch.minimum(torch.floor(u), hi - one)
        return f, (f + one) - u, u - f, (u <= lo) | (u >= hi)
    x0, wx0, wx1, rx = axis(g[..., 0], sx, lw)
    y0, wy0, wy1, ry = axis(g[..., 1], sy, lh)
    node = (y0.long() + pad) * lw + (x0.long() + pad)
    return node, rx | ry, torch.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], dim=-1)


def _gather(lattice, lw, lh, pad, which, mode, grid, dtype, chunk=2048):
    """Four taps of lattice[which, mode] ([n_maps][2][lh][lw][C]) at grid [S, 2]: (value [S, C] in `dtype`, sum of magnitudes [S, C] in
    `dtype`, dead [S]).  A zeros-mode sample on or beyond the outer ring reads exact zeros."""
    Cc = lattice.shape[-1]
    flat = lattice.reshape(-1, lh * lw, Cc)
    node, ring, w = lattice_taps(grid, lw, lh, pad, dtype)
    dead = ring & (mode == 1)
    w = torch.where(dead[:, None], torch.zeros_like(w), w)
    idx = torch.stack([node, node + 1, node + lw, node + lw + 1], dim=-1)
    val = torch.empty(grid.shape[0], Cc, dtype=dtype)
    mag = torch.empty(grid.shape[0], Cc, dtype=dtype)
    mm = which * 2 + mode
    for a in range(0, grid.shape[0], chunk):
        t = flat[mm[a:a + chunk, None], idx[a:a + chunk]].to(dtype)            # [s, 4, C]
        ww = w[a:a + chunk, :, None]
        val[a:a + chunk] = (ww * t).sum(dim=1)
        mag[a:a + chunk] = (ww * t.abs()).sum(dim=1)
    return val, mag, dead


def _lin(linear, x, W, b, dtype):
    if linear is not None:
        return linear(x, W, b).to(dtype)
    return F.linear(x, W.to(dtype), None if b is None else b.to(dtype))


def _samples(params, lattice, pad, rec, n_sets, V, dtype, linear):
    lh, lw = lattice.shape[2:4]
    Cc = lattice.shape[-1]
    Sn = rec["grid"].shape[0]
    assert V == 2 and Sn % n_sets == 0 and lattice.shape[0] == n_sets and lattice.shape[1] == 2
    n = torch.arange(Sn) // (Sn // n_sets)
    v, sc = n % V, n // V
    W1 = params["query_encode_latent.weight"].reshape(Cc, -1)
    Wp, b1 = W1[:, Cc:Cc + 3].to(dtype), params["query_encode_latent.bias"].to(dtype)
    W2, b2 = params["query_encode_latent_2.weight"].reshape(-1, Cc), params["query_encode_latent_2.bias"]
    hs, Bh, dead = [], [], []
    for sv in range(V):
        own = v == sv
        grid = torch.where(own[:, None], rec["grid"], rec["grid_in"][:, sv])
        tap, tmag, dd = _gather(lattice, lw, lh, pad, sc * V + sv, (~own).long(), grid, dtype)
        t = torch.tanh(rec["pt_in"][:, sv].to(dtype) / 5)
        hs.append(F.relu(tap + t @ Wp.T + b1))
        Bh.append(tmag + t.abs() @ Wp.abs().T + b1.abs())
        dead.append(dd)
    e = torch.cat([_lin(linear, h, W2, b2, dtype) for h in hs], dim=-1)
    Be = torch.cat([m @ W2.to(dtype).abs().T + b2.to(dtype).abs() for m in Bh], dim=-1)
    Wk1, bk1 = params["key_map.weight"].reshape(-1, e.shape[-1]), params["key_map.bias"]
    Wk2, bk2 = params["key_map_2.weight"].reshape(Wk1.shape[0], -1), params["key_map_2.bias"]
    Wq1, bq1 = params["query_embed.weight"].reshape(-1, G), params["query_embed.bias"]
    Wq2, bq2 = params["query_embed_2.weight"].reshape(Wq1.shape[0], -1), params["query_embed_2.bias"]
    k1 = _lin(linear, e, Wk1, bk1, dtype)
    g = rec["g"].to(dtype)
    x = F.relu(_lin(linear, g, Wq1, bq1, dtype))
    key = _lin(linear, F.relu(k1), Wk2, bk2, dtype)
    qry = _lin(linear, x, Wq2, bq2, dtype)
    logit = (key * qry).sum(dim=-1) / 16
    Bk1 = e.abs() @ Wk1.to(dtype).abs().T + bk1.to(dtype).abs()
    Bx = g.abs() @ Wq1.to(dtype).abs().T + bq1.to(dtype).abs()
    M, fv, fu, fc = fold(Wk2, bk2, Wq2, bq2, dtype)
    Blogit = ((F.relu(k1) * (x @ M.abs().T + fv.abs())).sum(dim=-1) + x @ fu.abs() + fc.abs()) / 16
    return {"h": torch.stack(hs, dim=1), "e": e, "k1": k1, "x": x, "logit": logit, "dead": torch.stack(dead, dim=1),
            "B_h": torch.stack(Bh, dim=1), "B_e": Be, "B_k1": Bk1, "B_x": Bx, "B_logit": Blogit}


def fold(Wk2, bk2, Wq2, bq2, dtype=F64):
    """M = Wk2^T Wq2 (index: [r's channel][x's channel]), v = Wk2^T bq2, u = Wq2^T bk2, c = <bk2, bq2> in `dtype`."""
    a, b_ = Wk2.to(dtype), Wq2.to(dtype)
    return a.T @ b_, a.T @ bq2.to(dtype), b_.T @ bk2.to(dtype), (bk2.to(dtype) * bq2.to(dtype)).sum()


def folded_logit(params, k1, x, dtype=F64, folded=None):
    """The logit as the kernel forms it: (r^T (M x + v) + u^T x + c) / 16, r = relu(k1); `folded` = (M, v, u, c) to use (default: fold())."""
    Dd = k1.shape[-1]
    M, fv, fu, fc = folded or fold(params["key_map_2.weight"].reshape(Dd, -1), params["key_map_2.bias"],
                                   params["query_embed_2.weight"].reshape(Dd, -1), params["query_embed_2.bias"], dtype)
    r, xx = F.relu(k1.to(dtype)), x.to(dtype)
    return ((r * (xx @ M.to(dtype).T + fv.to(dtype))).sum(dim=-1) + xx @ fu.to(dtype) + fc.to(dtype)) / 16


BOUNDS = ("B_h", "B_e", "B_k1", "B_x", "B_logit")


def samples(params, lattice, pad: int, rec: Dict[str, torch.Tensor], n_sets: int, V: int = 2, dtype=F64,
            linear: Optional[Callable] = None):
    """lattice [n_sets][2][lh][lw][C]; rec: car_sample_setup's records over S = n_sets R P samples — grid [S, 2], pt_in [S, V, 3],
    grid_in [S, V, 2], g [S, 16] -> dict(h [S, 2, C], e [S, C], k1, x [S, 128], logit [S], dead [S, 2]) in `dtype` and the bounds B_* in
    float64.  `linear(x, W, b)`: replaces the layers' arithmetic (the fp16 emulation); the bounds never use it."""
    out = _samples(params, lattice, pad, rec, n_sets, V, dtype, linear)
    ref = out if (dtype == F64 and linear is None) else _samples(params, lattice, pad, rec, n_sets, V, F64, None)
    for k in BOUNDS:
        out[k] = ref[k]
    return out


def part(e, logit, n_sets: int, R: int, P: int, tile_steps: int = TILE_STEPS, dtype=F64):
    """e [S, C], logit [S] -> (part [n_sets, R, ceil(P / tile_steps), C] computed in `dtype`, its bound sum_j exp(logit_j - m_g) |e_j| in
    float64): the sums run over the LIVE steps of a group only."""
    Cc = e.shape[-1]
    pgs = -(-P // tile_steps)

    def run(dt):
        ee = torch.zeros(n_sets, R, pgs * tile_steps, Cc, dtype=dt)
        ll = torch.full((n_sets, R, pgs * tile_steps), -float("inf"), dtype=dt)
        ee[:, :, :P] = e.to(dt).reshape(n_sets, R, P, Cc)
        ll[:, :, :P] = logit.to(dt).reshape(n_sets, R, P)
        ee, ll = ee.reshape(n_sets, R, pgs, tile_steps, Cc), ll.reshape(n_sets, R, pgs, tile_steps)
        w = torch.exp(ll - ll.amax(dim=-1, keepdim=True))
        return (w[..., None] * ee).sum(dim=3), (w[..., None] * ee.abs()).sum(dim=3)
    val, mag = run(dtype)
    return val, (mag if dtype == F64 else run(F64)[1])


def _rows(params, lattice, pad, row_src, row_grid, row_pe, dtype, linear):
    lh, lw = lattice.shape[2:4]
    Cc = lattice.shape[-1]
    W1 = params["query_encode_latent.weight"].reshape(Cc, -1)
    Wp, b1 = W1[:, Cc:Cc + 3].to(dtype), params["query_encode_latent.bias"].to(dtype)
    W2, b2 = params["query_encode_latent_2.weight"].reshape(-1, Cc), params["query_encode_latent_2.bias"]
    src = row_src.long()
    tap, tmag, dead = _gather(lattice, lw, lh, pad, src & 0x3fffffff, (src >> 30) & 1, row_grid, dtype)
    t = row_pe[:, :3].to(dtype)
    h = F.relu(tap + t @ Wp.T + b1)
    Bh = tmag + t.abs() @ Wp.abs().T + b1.abs()
    return {"h": h, "e": _lin(linear, h, W2, b2, dtype), "dead": dead, "B_h": Bh, "B_e": Bh @ W2.to(dtype).abs().T + b2.to(dtype).abs()}


def rows(params, lattice, pad: int, row_src, row_grid, row_pe, dtype=F64, linear: Optional[Callable] = None):
    """car_fused_rows: row_src [rows] (map | padding mode << 30), row_grid [rows, 2], row_pe [rows, 4] (the point term as it enters the
    layer: no tanh here; the fourth float unused) -> dict(h [rows, C], e [rows, 288], dead) in `dtype`, B_h and B_e in float64."""
    out = _rows(params, lattice, pad, row_src, row_grid, row_pe, dtype, linear)
    ref = out if (dtype == F64 and linear is None) else _rows(params, lattice, pad, row_src, row_grid, row_pe, F64, None)
    out["B_h"], out["B_e"] = ref["B_h"], ref["B_e"]
    return out


# ---- one-product fp16 arithmetic: the emulation of tests/test_render_fp16_cpu.py applied to this chain --------------------------------------
def fp16_linear(x, W, b):
    """A layer as the fp16 instance runs it, emulated on the CPU (tests/test_render_fp16_cpu.py _conv1x1_fp16: operands moved into fp16's
    window by powers of two — activations per row, weights per layer — rounded to nearest fp16, one product per term, wide accumulation)."""
    from test_render_fp16_cpu import _conv1x1_fp16
    return _conv1x1_fp16(x.float(), W.float(), b.float() if b is not None else torch.zeros(W.shape[0]))


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
def gaussian_params(seed: int = 1) -> Dict[str, torch.Tensor]:
    """N(0, 1 / fan_in) weights and 0.1 N(0, 1) biases in float32, drawn in sorted-name order from one generator."""
    g = gen(seed)
    out = {}
    for name in sorted(SHAPES):
        n, k = SHAPES[name]
        out[name + ".weight"] = torch.randn(n, k, generator=g) / k ** 0.5
        out[name + ".bias"] = 0.1 * torch.randn(n, generator=g)
    return out


def rescaled(params, s: float):
    """The `_rescale` pairs of tests/test_hip_parity.py: a layer feeding a ReLU times s (weights and bias), its consumer by 1 / s."""
    p = {k: v.clone() for k, v in params.items()}
    for first, second in (("query_encode_latent", "query_encode_latent_2"), ("key_map", "key_map_2"), ("query_embed", "query_embed_2")):
        p[first + ".weight"] *= s
        p[first + ".bias"] *= s
        p[second + ".weight"] /= s
    return p


def weights(kind: str = "gauss") -> Dict[str, torch.Tensor]:
    p = gaussian_params(1)
    if kind == "gauss":
        return p
    if kind in ("rescale-4", "rescale+4"):
        return rescaled(p, 1e-4 if kind == "rescale-4" else 1e4)
    if kind == "w2zero":
        p["query_encode_latent_2.weight"].zero_()
    elif kind == "kbias":
        p["key_map.bias"].fill_(-1e3)                                           # relu(k1) = 0: logit = u^T x + c, from the fold alone
    elif kind == "qbias":
        p["query_embed.bias"].fill_(-1e3)                                       # x = 0: logit = r^T v + c
    elif kind == "nopoint":
        p["query_encode_latent.weight"][:, C:].zero_()                          # with an all-zero lattice: hp from the 1e-30 clamp
        p["query_encode_latent.bias"].zero_()
    elif kind == "int":
        return integer_params()
    else:
        raise KeyError(kind)
    return p


# ---- lattices -----------------------------------------------------------------------------------------------------------------------------
def lattice_dims(fh: int, fw: int, pad: int):
    """(lh, lw) of the lattice over a finest level of fh x fw texels."""
    return 2 * fh + 2 * pad - 1, 2 * fw + 2 * pad - 1


def random_lattice(kind: str, n_maps: int, fh: int, fw: int, pad: int, seed: int = 7, channels: int = C):
    """[n_maps][2][lh][lw][C] seeded values, every (map, mode) its own; the zeros-mode outer ring is exactly zero (the lattice's contract).
    kinds: gauss | x1e-4 | x1e4 | outliers (a dozen 1e5 entries in N(0, 1)) | zero | int (integers in [-8, 8] times 4)."""
    lh, lw = lattice_dims(fh, fw, pad)
    g = gen(seed)
    if kind == "int":
        lat = 4.0 * torch.randint(-8, 9, (n_maps, 2, lh, lw, channels), generator=g).float()
    else:
        lat = torch.randn(n_maps, 2, lh, lw, channels, generator=g)
    if kind == "x1e-4":
        lat *= 1e-4
    elif kind == "x1e4":
        lat *= 1e4
    elif kind == "outliers":
        at = torch.randint(0, lat.numel(), (12,), generator=g)
        lat.view(-1)[at] = 1e5 * torch.where(torch.rand(12, generator=g) < 0.5, -1.0, 1.0)
    elif kind == "zero":
        lat.zero_()
    elif kind not in ("gauss", "int"):
        raise KeyError(kind)
    lat[:, 1, 0], lat[:, 1, -1], lat[:, 1, :, 0], lat[:, 1, :, -1] = 0.0, 0.0, 0.0, 0.0
    return lat.contiguous()


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def spread_uv(R: int, H: int, W: int, seed: int):
    """R pixel coordinates, a fifth of them up to half an image outside it (their epipolar segments miss or graze the views)."""
    g = gen(seed)
    uv = torch.rand(R, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    out = torch.arange(R) % 5 == 4
    uv[out] = (torch.rand(int(out.sum()), 2, generator=g) * 2 - 0.5) * torch.tensor([W - 1.0, H - 1.0])
    return uv.contiguous()


def patch_rays(rays):
    """Edits CarRay records [n_sets, R, 12] (any device) in place so that the edges of car_sample_setup and car_lattice_taps are met: ray 1
    of the first set gets a NaN moment (non-finite pt, scrubbed to 0), ray 2 of the last set a moment of (3e38, 0, 0) (pt beyond fp32:
    pt_in saturated by nan_to_num), ray 0 of the last set a segment from x = -2.5 to 2.5 (its ends beyond the lattice in its own view:
    clamped onto the ring).  Sets with fewer than 3 rays stay as they are."""
    if rays.shape[1] >= 3:
        rays[0, 1, 3:6] = float("nan")
        rays[-1, 2, 3] = 3e38
        rays[-1, 2, 4:6] = 0.0
        rays[-1, 0, 6] = -2.5
        rays[-1, 0, 8] = 2.5
    return rays


# (R, P, b) of the tile-edge cases: 2, 2, 2, 8, 16, 18 and 6 workgroups
TILE_EDGES = ((24, 8, 1), (1, 1, 1), (23, 7, 1), (25, 9, 1), (37, 13, 2), (49, 17, 1), (24, 8, 3))
BASE = dict(H=16, W=16, fh=8, fw=8, pad=2, alpha=0.5, at=None, no_sample=0, lat="gauss", wts="gauss", rows_comp=0)
CASES: Dict[str, dict] = {f"edge-{R}-{P}-{b}": dict(BASE, R=R, P=P, b=b) for R, P, b in TILE_EDGES}
CASES.update({
    "ctx0": dict(BASE, R=37, P=13, b=1, at=0),                                           # the query camera on context camera 0
    "depths": dict(BASE, R=37, P=13, b=1, no_sample=1),                                   # `steps` holds depths
    "wide": dict(BASE, R=37, P=13, b=2, H=12, W=20, fh=6, fw=10, pad=5),                  # H != W, non-square lattice, the larger pad
})
for _k, _lat, _w in (("lat-4", "x1e-4", "gauss"), ("lat+4", "x1e4", "gauss"), ("outliers", "outliers", "gauss"), ("allzero", "zero", "nopoint"),
                     ("rescale-4", "gauss", "rescale-4"), ("rescale+4", "gauss", "rescale+4"), ("w2zero", "gauss", "w2zero"),
                     ("kbias", "gauss", "kbias"), ("qbias", "gauss", "qbias")):
    CASES["mag-" + _k] = dict(BASE, R=37, P=13, b=1, lat=_lat, wts=_w)
ROWS_CASES = {f"rows-{R}-{P}-{nc}": dict(BASE, R=R, P=P, b=2, rows_comp=nc) for R, P in ((37, 13), (24, 8)) for nc in (1, 3)}
RAGGED = tuple(t for t, c in CASES.items() if c["R"] % TILE_RAYS and c["P"] % TILE_STEPS and c["R"] > 1)


def scene(c: dict):
    """(input dict of synthetic.stereo_scene, uv [R, 2], steps [P]) of a case."""
    uv = spread_uv(c["R"], c["H"], c["W"], 100 + c["R"])
    inp = S.stereo_scene(c["H"], b=c["b"], alpha=c["alpha"], uv=uv, seed=5 + c["P"], query_at_context=c["at"])
    steps = torch.linspace(0.1, 10.0, c["P"]) if c["no_sample"] else torch.linspace(0.0, 1.0, c["P"])
    return inp, uv, steps.contiguous()


def case_lattice(c: dict):
    return random_lattice(c["lat"], 2 * c["b"], c["fh"], c["fw"], c["pad"], seed=7 + c["R"])


def rows_lists(c: dict, rec: Dict[str, torch.Tensor]):
    """Explicit rows for car_fused_rows over the samples of `rec` ([n_sets][R][P], n_sets = 2 b): row = sample * ncomp + comp; every
    (set, component) has its own (map, padding mode) — map = (set + comp) % n_sets, mode = (set // 2 + comp) % 2: all eight of them with
    three components — grid = the sample's own grid point where the mode is border and its landing point in the other view where it is
    zeros (so mode-1 rows lie on and beyond the ring); the point term is tanh(pt_in / 5) of view comp % 2."""
    nc, n_sets = c["rows_comp"], 2 * c["b"]
    Sn = rec["grid"].shape[0]
    n = torch.arange(Sn) // (Sn // n_sets)
    src = torch.empty(Sn, nc, dtype=torch.int32)
    grid = torch.empty(Sn, nc, 2)
    pe = torch.zeros(Sn, nc, 4)
    for k in range(nc):
        mode = (n // 2 + k) % 2
        src[:, k] = (((n + k) % n_sets) | (mode << 30)).int()
        other = rec["grid_in"][torch.arange(Sn), 1 - n % 2]
        grid[:, k] = torch.where((mode == 0)[:, None], rec["grid"], other)
        pe[:, k, :3] = torch.tanh(rec["pt_in"][:, k % 2] / 5)
        pe[:, k, 3] = float("nan")                                              # the fourth float is unused
    return src.reshape(-1).contiguous(), grid.reshape(-1, 2).contiguous(), pe.reshape(-1, 4).contiguous()


# ---- the exact-integer case ---------------------------------------------------------------------------------------------------------------
def integer_params(seed: int = 11):
    """W2: two non-zeros of +-1 per row; b1, b2 small integers; the point columns of the first layer zero (tanh is no integer).  The closing
    layers stay Gaussian: the exactness claim covers h and e only — the fold M = Wk2^T Wq2 of integer layers 128 wide, its per-sample
    powers of two and the 16-wide geometric query (unit vectors, tanh) cannot be joined inside fp16's 11 bits."""
    g = gen(seed)
    p = gaussian_params(1)
    W2 = torch.zeros(E, C)
    for r in range(E):
        cols = torch.randperm(C, generator=g)[:2]
        W2[r, cols] = torch.randint(0, 2, (2,), generator=g).float() * 2 - 1
    p["query_encode_latent_2.weight"] = W2
    p["query_encode_latent_2.bias"] = torch.randint(-3, 4, (E,), generator=g).float()
    p["query_encode_latent.weight"] = torch.zeros(C, C + 3)
    p["query_encode_latent.bias"] = torch.randint(-3, 4, (C,), generator=g).float()
    return p


INT_CASE = dict(BASE, R=37, P=13, b=1, lat="int", wts="int")


def integer_rays(rays, c: dict):
    """Every ray's segment collapsed onto a point whose lattice coordinate is a half-integer in both axes (tap weights 1/4 each) — exact in
    fp32: grid = (u + 1) / s - 1 with s a power of two — varying with the ray; the cross-view landing points stay what the geometry makes
    them, which is why the integer lattice's zeros-mode maps are all zero."""
    n_sets, R = rays.shape[:2]
    r = torch.arange(R, device=rays.device)
    ux = (r % (2 * c["fw"] - 2)).float() + 0.5
    uy = ((r // 3) % (2 * c["fh"] - 2)).float() + 0.5
    rays[:, :, 6] = rays[:, :, 8] = ((ux + 1) / c["fw"] - 1)[None]
    rays[:, :, 7] = rays[:, :, 9] = ((uy + 1) / c["fh"] - 1)[None]
    return rays


def integer_lattice(c: dict):
    lat = random_lattice("int", 2 * c["b"], c["fh"], c["fw"], c["pad"], seed=13)
    lat[:, 1] = 0.0
    return lat
