"""Plain-torch restatement of the geometry header (csrc/car_geom.h) and of the stage kernels built on it (csrc/car_geometry.hip:
car_pose_setup, car_ray_setup, car_sample_setup, car_project_points, car_exchange_rows), the dtype a parameter, plus the input sets that
test_geometry_reference.py (CPU, against the host shim) and test_geometry_hip.py (GPU, through the C ABI) share.  Test infrastructure:
only ever the checker; no GPU, no ctypes.

It works STAGE BY STAGE.  Every stage takes the fp32 records of the stage before it as inputs,

    cameras -> CarPose -> (d, m) -> start / end / overlaps -> pixel_val -> pt -> pt_in / grid_in / g / xenc

so each tolerance belongs to one function of fp32 inputs and the ill-conditioning of one stage is never charged to the next: in float64
`rays` takes the direction record `d32` whose clipping it judges, `samples` the `grid32` and `pt32` records.

  float64   the truth: the header's formulas and definitions (the +1e-12 / +1e-8 terms, the 1e-6 epsilons as the fp32 literals they
            are, k01 / H on BOTH rows, (W - 1) / (H - 1), first-index ties, nan_to_num, the scrub values) in plain double arithmetic;
            pose records from torch.linalg.inv and fp64 products.
  float32   the header's own operation order: fmaf emulated in double as oracle/car_oracle.py does (the product is exact, the one extra
            rounding a 2^-29 event), torch.cross' fma(a, b, -(c d)) pattern, left-to-right sums, everything else one IEEE operation at
            a time; the closest-point island in double with a true fma (error-free product and sum); car_inverse4 as the Gauss-Jordan
            it is.  It must equal the host shim bit for bit — tanhf apart.

With every output come (from the float64 run, whatever `dtype` is)
  M_<name>  the summed magnitudes of its last operations, with the conditioning inside (for pt: (sum |m1 x (l2 x n)| + sum |m2 . n| |l1|)
            / den, built from sum-of-magnitude cross products, so the 1 / sin^2 of a near-parallel pair is in it).  A comparison divides
            an error by it;
  D_<name>  the decided mask: true where every discrete decision behind the output lies further than MARGIN x (the summed magnitudes
            of the compared quantity) from its threshold — the four frame hits' in-bounds and z tests, the gap between the two smallest
            / two largest valid t, ok0 / oki, at_camera (|o| exactly zero, or its norm clear of 1e-6; depth_zero and the p_z tests
            compare stored fp32 inputs and are always decided), any_in of the no_sample branch, isfinite before a scrub (decided where
            every intermediate stays below 1e30 or is non-finite in double as well), fp32 overflow of pt."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional

import torch

import parity_rule as PR

F32, F64 = torch.float32, torch.float64
POSE_FLOATS, RAY_FLOATS, G_DIM, MAX_VIEWS = 96, 12, 16, 3
FMAX = 3.4028234663852886e38
INF = float("inf")

MARGIN = 2.0 ** -14     # decided: further than this x the summed magnitudes from a threshold: 1024 x fp32's unit roundoff
BIG = 1e30              # a finite intermediate below this cannot overflow fp32 in the header's one or two further operations
CAP_UNDECIDED = 0.02    # the share of a set's rays or samples that may lie outside a decided mask
# No sample is left out of the pt comparison as parallel (the issue allows 1 %): M_pt carries 1 / sin^2 and, with the + 1e-12 of den, holds
# down to sin^2 = 0; test_geometry_reference.py asserts r32 of pt on the samples below sin^2 = 1e-6 by themselves.
R32_CEILING = {"pt": 2e-5}          # every other output: R32_CEILING_OTHER.  A summed-magnitude term that is too small would inflate r32 and
R32_CEILING_OTHER = 1e-6            # with it the GPU tolerance 8 x max(r32, 2^-22): the float32 mode must stay below these (measured: 2.6e-7, 7e-6)

# CarPose offsets
Q_REL, C_REL, T0, KC, K01, KQ, INV_Q, PAD = 0, 12, 24, 60, 64, 73, 77, 89


# max over the masked entries of |got - ref64| / bound; equal infinities agree; a bound that is zero or not finite demands a zero error
ratio = functools.partial(PR.ratio, equal_inf=True, bound_ok="finite")
tolerance, gen = PR.tolerance, PR.gen


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------------
def lit(x: float, dt):
    """An fp32 literal of the header (1e-6f, 1e-12f, ...) in `dt`."""
    return torch.tensor(x, dtype=F32).to(dt)


def fma(a, b, c):
    """fmaf in float32 (emulated in double), a * b + c in float64."""
    if a.dtype == F32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma64(a, b, c):
    """A true double fma: the product's error term (Dekker) and the sum's (Knuth) folded into one last rounding."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    r = s + (t + e)
    return torch.where(torch.isfinite(r) & (r != 0), r, p + c)                 # a zero keeps the sign IEEE gives it


def _cross(a, b, island=False):
    """car_cross_f / car_cross_d: fma(a_j, b_k, -(a_k b_j)); plain in the float64 truth."""
    f = fma64 if island else fma
    idx = ((1, 2), (2, 0), (0, 1))
    if a.dtype == F64 and not island:
        return torch.stack([a[..., j] * b[..., k] - a[..., k] * b[..., j] for j, k in idx], dim=-1)
    return torch.stack([f(a[..., j], b[..., k], -(a[..., k] * b[..., j])) for j, k in idx], dim=-1)


def _cross_mag(a, b):
    return torch.stack([a[..., j] * b[..., k] + a[..., k] * b[..., j] for j, k in ((1, 2), (2, 0), (0, 1))], dim=-1)


def _norm3(v, island=False):
    """car_norm3_f / car_norm3_d.  torch's float32 sqrt is not correctly rounded on every CPU build: taken in double and rounded once more
    (innocuous for a square root: 53 >= 2 x 24 + 2)."""
    f = fma64 if island else fma
    s = f(v[..., 2], v[..., 2], f(v[..., 1], v[..., 1], v[..., 0] * v[..., 0]))
    return torch.sqrt(s.double()).to(v.dtype)


def _scrub(x, v):
    return torch.where(torch.isfinite(x), x, torch.full_like(x, v))


def _far(v, thr, mag):
    """Is v decidedly on its side of thr?  NaN never is."""
    return (v - thr).abs() > MARGIN * mag


# ---- poses -------------------------------------------------------------------------------------------------------------------------------
def _inverse4_gj(A):
    """car_inverse4: partial-pivot Gauss-Jordan in double (python floats), rounded once to fp32 by the caller."""
    a = [[float(A[i][j]) for j in range(4)] + [1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for c in range(4):
        piv, best = c, abs(a[c][c])
        for r in range(c + 1, 4):
            if abs(a[r][c]) > best:
                best, piv = abs(a[r][c]), r
        if piv != c:
            a[c], a[piv] = a[piv], a[c]
        inv = 1.0 / a[c][c]
        a[c] = [x * inv for x in a[c]]
        for r in range(4):
            if r != c:
                f = a[r][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return [row[4:] for row in a]


def _matmul_top3(A, B):
    """Rows 0..2 of A @ B as the header's FMA chain over k (float32) / the plain product (float64)."""
    acc = A[..., :3, 0:1] * B[..., 0:1, :]
    for k in (1, 2, 3):
        acc = fma(A[..., :3, k:k + 1].expand_as(acc), B[..., k:k + 1, :].expand_as(acc), acc)
    return acc


def poses(c2w_ctx, c2w_q, K_ctx, K_q, H: int, dtype=F64):
    """car_pose_setup.  c2w_ctx, K_ctx [b, V, 4, 4]; c2w_q, K_q [b, 1, 4, 4] -> dict(rec [b V, 96] in `dtype`, M_rec [b V, 96]).
    float64: torch.linalg.inv and fp64 products, M = (|inv| |c2w|) for the products, |inv| for inv_q, |K / H| for k01."""
    b, V = c2w_ctx.shape[:2]
    cq = c2w_q.reshape(b, 1, 4, 4)

    def run(dt):
        cc, q, Kc, Kq = c2w_ctx.to(dt), cq.to(dt), K_ctx.to(dt), K_q.reshape(b, 1, 4, 4).to(dt)
        if dt == F64:
            inv_c, inv_q = torch.linalg.inv(cc), torch.linalg.inv(q)
        else:
            inv_c = torch.tensor([[_inverse4_gj(cc[i, v].tolist()) for v in range(V)] for i in range(b)], dtype=F64).float()
            inv_q = torch.tensor([[_inverse4_gj(q[i, 0].tolist())] for i in range(b)], dtype=F64).float()
        rec = torch.zeros(b, V, POSE_FLOATS, dtype=dt)
        mag = torch.zeros(b, V, POSE_FLOATS, dtype=F64)
        prod = lambda A, B: _matmul_top3(A, B).reshape(b, V, 12)
        pmag = lambda A, B: (A.abs().double() @ B.abs().double())[..., :3, :].reshape(b, V, 12)
        rec[..., Q_REL:Q_REL + 12], mag[..., Q_REL:Q_REL + 12] = prod(inv_c, q.expand(b, V, 4, 4)), pmag(inv_c, q.expand(b, V, 4, 4))
        rec[..., C_REL:C_REL + 12], mag[..., C_REL:C_REL + 12] = prod(inv_c, cc), pmag(inv_c, cc)
        for s in range(V):
            a = inv_c[:, s:s + 1].expand(b, V, 4, 4)
            rec[..., T0 + 12 * s:T0 + 12 * s + 12], mag[..., T0 + 12 * s:T0 + 12 * s + 12] = prod(a, cc), pmag(a, cc)
        for o, K in ((KC, Kc), (KQ, Kq.expand(b, V, 4, 4))):
            rec[..., o], rec[..., o + 1], rec[..., o + 2], rec[..., o + 3] = K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]
        k01 = Kc[..., :3, :3].clone()
        k01[..., :2, :] = k01[..., :2, :] / float(H)                          # BOTH rows by H: the reference's quirk
        rec[..., K01:K01 + 9] = k01.reshape(b, V, 9)
        rec[..., INV_Q:INV_Q + 12] = inv_q[:, :, :3, :].reshape(b, 1, 12)
        mag[..., KC:KC + 4] = rec[..., KC:KC + 4].abs().double()
        mag[..., KQ:KQ + 4] = rec[..., KQ:KQ + 4].abs().double()
        mag[..., K01:K01 + 9] = rec[..., K01:K01 + 9].abs().double()
        mag[..., INV_Q:INV_Q + 12] = rec[..., INV_Q:INV_Q + 12].abs().double()
        return rec.reshape(b * V, POSE_FLOATS), mag.reshape(b * V, POSE_FLOATS)
    rec, mag = run(dtype)
    return {"rec": rec, "M_rec": mag if dtype == F64 else run(F64)[1]}


# ---- shared pieces of the ray and sample stages ---------------------------------------------------------------------------------------------
def _pixel_ray(M, k4, u, v):
    """car_pixel_ray: M [..., 12], k4 [..., 4], u, v [...] -> d, m, M_d (all [..., 3])."""
    dt = u.dtype
    one = torch.ones_like(u)
    x = (u - k4[..., 2]) / k4[..., 0]
    y = (v - k4[..., 3]) / k4[..., 1]
    w, wm = [], []
    for i in range(3):
        acc = x * M[..., 4 * i]
        acc = fma(y, M[..., 4 * i + 1].expand_as(acc), acc)
        acc = fma(one, M[..., 4 * i + 2].expand_as(acc), acc)
        w.append(fma(one, M[..., 4 * i + 3].expand_as(acc), acc))
        wm.append((x * M[..., 4 * i]).abs() + (y * M[..., 4 * i + 1]).abs() + M[..., 4 * i + 2].abs() + M[..., 4 * i + 3].abs())
    o = torch.stack([M[..., 3], M[..., 7], M[..., 11]], dim=-1).expand(*u.shape, 3)
    d = torch.stack(w, dim=-1) - o
    n = _norm3(d)
    tiny = lit(1e-12, dt)
    n = torch.where(n > tiny, n, tiny)
    d = d / n[..., None]
    return d, o, (torch.stack(wm, dim=-1) + o.abs()) / n[..., None]


def _in_bounds(x, y, dt):
    e = lit(1e-6, dt)
    hi = (torch.tensor(1.0, dtype=F32) + torch.tensor(1e-6, dtype=F32)).to(dt)
    return (x >= -e) & (y >= -e) & (x <= hi) & (y <= hi)


def _bounds_far(x, y, mx, my, dt):
    e = lit(1e-6, dt)
    hi = (torch.tensor(1.0, dtype=F32) + torch.tensor(1e-6, dtype=F32)).to(dt)
    return _far(x, -e, mx) & _far(x, hi, mx) & _far(y, -e, my) & _far(y, hi, my)


def _frame_hit(K, o, d, dim, value):
    """car_frame_hit -> dict(t, x, y, valid, M_t, M_x, M_y, D: validity decided)."""
    dt = d.dtype
    od = 1 - dim
    fs, fo, cs, co = K[..., 3 * dim + dim], K[..., 3 * od + od], K[..., 3 * dim + 2], K[..., 3 * od + 2]
    o_s, o_o, o_z, d_s, d_o, d_z = o[..., dim], o[..., od], o[..., 2], d[..., dim], d[..., od], d[..., 2]
    val = torch.full_like(d_z, value)
    c = (val - cs) / fs
    A, B = c * o_z - o_s, d_s - c * d_z
    t = A / B
    num = fo * (o_o * (c * d_z - d_s) + d_o * (o_s - c * o_z))
    den = d_z * o_s - d_s * o_z
    other = co + num / den
    z = o_z + t * d_z
    x, y = (val, other) if dim == 0 else (other, val)
    valid = _in_bounds(x, y, dt) & (z > -lit(1e-6, dt))
    mA, mB = (c * o_z).abs() + o_s.abs(), d_s.abs() + (c * d_z).abs()
    mt = mA / B.abs() + A.abs() * mB / (B * B)
    mnum = fo.abs() * (o_o.abs() * ((c * d_z).abs() + d_s.abs()) + d_o.abs() * (o_s.abs() + (c * o_z).abs()))
    mden = (d_z * o_s).abs() + (d_s * o_z).abs()
    mo = co.abs() + mnum / den.abs() + num.abs() * mden / (den * den)
    mz = o_z.abs() + mt * d_z.abs()
    mv = torch.zeros_like(val)                 # the coordinate the frame line fixes is exact
    mx, my = (mv, mo) if dim == 0 else (mo, mv)
    exact = (o == 0).all(dim=-1)                # the query ON the camera: 0 / 0 in every precision, every hit invalid
    dec = exact | (_bounds_far(x, y, mx, my, dt) & _far(z, -lit(1e-6, dt), mz))
    return {"t": t, "x": x, "y": y, "valid": valid, "M_t": mt, "M_x": mx, "M_y": my, "D": dec}


def _pinhole01(K, p):
    s = p[..., 2] + lit(1e-8, p.dtype)
    q = [p[..., i] / s for i in range(3)]
    xy, mag = [], []
    ms = (p[..., 2].abs() + 1e-8) / s.abs()
    for r in (0, 1):
        xy.append(fma(K[..., 3 * r + 2].expand_as(q[2]), q[2], fma(K[..., 3 * r + 1].expand_as(q[1]), q[1], K[..., 3 * r] * q[0])))
        mag.append(sum((K[..., 3 * r + j] * q[j]).abs() for j in range(3)) * (1 + ms))
    return xy, mag


def _pick(stack, idx):
    return torch.gather(torch.stack(stack), 0, idx[None])[0]


def _project_ray(K, o, d):
    """car_project_ray -> dict(a [.., 2], b [.., 2], ov, M_a, M_b, D, and the decisions for the edge census)."""
    dt = d.dtype
    hits = [_frame_hit(K, o, d, 0, 0.0), _frame_hit(K, o, d, 0, 1.0), _frame_hit(K, o, d, 1, 0.0), _frame_hit(K, o, d, 1, 1.0)]
    pinf = torch.full_like(hits[0]["t"], INF)
    tmin, tmax = torch.where(hits[0]["valid"], hits[0]["t"], pinf), torch.where(hits[0]["valid"], hits[0]["t"], -pinf)
    imin, imax = torch.zeros_like(tmin, dtype=torch.long), torch.zeros_like(tmin, dtype=torch.long)
    for i in (1, 2, 3):
        a, b_ = torch.where(hits[i]["valid"], hits[i]["t"], pinf), torch.where(hits[i]["valid"], hits[i]["t"], -pinf)
        up, dn = a < tmin, b_ > tmax                                           # strict: the first index wins ties
        tmin, imin = torch.where(up, a, tmin), torch.where(up, torch.full_like(imin, i), imin)
        tmax, imax = torch.where(dn, b_, tmax), torch.where(dn, torch.full_like(imax, i), imax)
    eps = lit(1e-6, dt)
    depth_zero = o[..., 2] < eps
    no = _norm3(o)
    at_camera = no < eps
    p0 = torch.where(at_camera[..., None], d, o)
    xy0, m0 = _pinhole01(K, p0)
    ok0 = _in_bounds(xy0[0], xy0[1], dt) & (p0[..., 2] > -eps)
    ok0 = ok0 & ~(depth_zero & ~at_camera)
    xyi, mi = _pinhole01(K, d)
    oki = _in_bounds(xyi[0], xyi[1], dt) & (d[..., 2] > -eps)
    sel = lambda k, idx: _pick([h[k] for h in hits], idx)
    a = [torch.where(ok0, xy0[0], sel("x", imin)), torch.where(ok0, xy0[1], sel("y", imin))]
    b = [torch.where(oki, xyi[0], sel("x", imax)), torch.where(oki, xyi[1], sel("y", imax))]
    ma = [torch.where(ok0, m0[0], sel("M_x", imin)), torch.where(ok0, m0[1], sel("M_y", imin))]
    mb = [torch.where(oki, mi[0], sel("M_x", imax)), torch.where(oki, mi[1], sel("M_y", imax))]
    vmin, vmax = sel("valid", imin), sel("valid", imax)
    ov = (ok0 | vmin) & (oki | vmax)
    # decided
    exact = (o == 0).all(dim=-1)
    hits_dec = hits[0]["D"] & hits[1]["D"] & hits[2]["D"] & hits[3]["D"]
    ts = torch.stack([torch.where(h["valid"], h["t"], pinf) for h in hits])
    mts = torch.stack([torch.where(h["valid"], h["M_t"], torch.zeros_like(h["M_t"])) for h in hits])
    nvalid = torch.stack([h["valid"] for h in hits]).sum(dim=0)

    def gap_ok(sign):
        v, order = torch.sort(torch.where(torch.isfinite(ts), sign * ts, ts), dim=0)                                 # ascending: the two smallest (largest for sign = -1) first
        m = torch.gather(mts, 0, order)
        return (nvalid <= 1) | ((v[1] - v[0]) > MARGIN * (m[0] + m[1])) | (exact & (nvalid == 0))
    cam_dec = exact | _far(no, eps, no)
    ok0_dec = cam_dec & ((depth_zero & ~at_camera) | ~(p0[..., 2] > -eps) | _bounds_far(xy0[0], xy0[1], m0[0], m0[1], dt))
    oki_dec = ~(d[..., 2] > -eps) | _bounds_far(xyi[0], xyi[1], mi[0], mi[1], dt)
    dec = ok0_dec & oki_dec & (ok0 | (hits_dec & gap_ok(1.0))) & (oki | (hits_dec & gap_ok(-1.0)))
    return {"a": torch.stack(a, -1), "b": torch.stack(b, -1), "ov": ov, "M_a": torch.stack(ma, -1), "M_b": torch.stack(mb, -1), "D": dec,
            "ok0": ok0, "oki": oki, "imin": imin, "imax": imax, "depth_zero": depth_zero, "at_camera": at_camera, "vmin": vmin, "vmax": vmax}


def _project_grid(k4, p, mp, pdec, H: int, W: int):
    """car_project_grid: k4 [..., 4], p [..., 3] with summed magnitudes mp and per-component `pdec` (the component is the same finite or
    non-finite thing in every precision) -> g [..., 2], M_g, D_g."""
    dt = p.dtype
    zz = p[..., 2] + lit(1e-12, dt)
    mzz = mp[..., 2] + 1e-12
    g, mg, dg = [], [], []
    for i, n in ((0, W), (1, H)):
        kp = k4[..., i] * p[..., i]
        x = kp / zz + k4[..., 2 + i]
        fin = torch.isfinite(x)
        mx = k4[..., i].abs() * (mp[..., i] / zz.abs() + p[..., i].abs() * mzz / (zz * zz)) + k4[..., 2 + i].abs()
        x = torch.where(fin, x, lit(1e10, dt).expand_as(x))
        gi = x / float(n - 1) * 2.0 - 1.0
        mi = torch.where(fin, mx / float(n - 1) * 2.0 + 1.0, gi.abs())
        small = (kp.abs() < BIG) & (x.abs() < BIG) & (zz.abs() > 1e-30)
        nonfin_in = ~torch.isfinite(p[..., i]) | ~torch.isfinite(p[..., 2])
        g.append(gi), mg.append(mi), dg.append(pdec[..., i] & pdec[..., 2] & torch.where(fin, small, nonfin_in))
    return torch.stack(g, -1), torch.stack(mg, -1), torch.stack(dg, -1)


# ---- rays --------------------------------------------------------------------------------------------------------------------------------
def _rays(P32, uv, b, V, R, H, W, no_sample, steps, dt, d32):
    Pz = P32.to(dt).reshape(b, V, 1, POSE_FLOATS)
    u, v = uv.to(dt)[:, None, :, 0].expand(b, V, R), uv.to(dt)[:, None, :, 1].expand(b, V, R)
    d, o, md = _pixel_ray(Pz[..., Q_REL:Q_REL + 12], Pz[..., KQ:KQ + 4], u, v)
    du = d if d32 is None else d32.to(dt).reshape(b, V, R, 3)                   # the record whose clipping is judged
    m = _cross(o, du)
    mm = _cross_mag(o.abs(), du.abs())
    rec = torch.zeros(b, V, R, RAY_FLOATS, dtype=dt)
    mag = torch.zeros(b, V, R, RAY_FLOATS, dtype=dt)
    rec[..., 0:3], rec[..., 3:6], mag[..., 0:3], mag[..., 3:6] = d, m, md, mm
    info = {}
    if not no_sample:
        pr = _project_ray(Pz[..., K01:K01 + 9], o, du)
        for k, (xy, mxy) in enumerate(((pr["a"], pr["M_a"]), (pr["b"], pr["M_b"]))):
            raw = (xy - 0.5) * 2.0
            fin = torch.isfinite(raw)
            rec[..., 6 + 2 * k:8 + 2 * k] = torch.where(fin, raw, torch.zeros_like(raw))
            mag[..., 6 + 2 * k:8 + 2 * k] = torch.where(fin, 2.0 * (mxy + 0.5), torch.zeros_like(raw))
            info["scrubbed"] = info.get("scrubbed", False) | ~fin.all(dim=-1)
        rec[..., 10] = pr["ov"].to(dt)
        dec = pr["D"]
        info.update({k: pr[k] for k in ("ok0", "oki", "imin", "imax", "depth_zero", "at_camera", "vmin", "vmax")})
    else:
        kc = Pz[..., KC:KC + 4]
        st = steps.to(dt)
        inside_sure = torch.zeros(b, V, R, dtype=torch.bool)
        outside_sure = torch.ones(b, V, R, dtype=torch.bool)
        any_in = torch.zeros(b, V, R, dtype=torch.bool)
        one = torch.ones((), dtype=dt)
        for p in range(st.numel()):
            s = st[p]
            q = o + s * du
            mq = o.abs() + s.abs() * du.abs()
            g, mg, dg = _project_grid(kc, q, mq, torch.isfinite(q) & (mq < BIG) | ~torch.isfinite(q), H, W)
            cmp = torch.stack([g[..., 0] < one, g[..., 0] > -one, g[..., 1] < one, g[..., 1] > -one])
            far = torch.stack([_far(g[..., 0], one, mg[..., 0]), _far(g[..., 0], -one, mg[..., 0]), _far(g[..., 1], one, mg[..., 1]),
                               _far(g[..., 1], -one, mg[..., 1])]) & torch.stack([dg[..., 0], dg[..., 0], dg[..., 1], dg[..., 1]])
            any_in = any_in | cmp.all(dim=0)
            inside_sure = inside_sure | (cmp & far).all(dim=0)
            outside_sure = outside_sure & (~cmp & far).any(dim=0)
            if p == 0:
                rec[..., 6:8], mag[..., 6:8], d0 = g, mg, dg.all(dim=-1)
            if p == st.numel() - 1:
                rec[..., 8:10], mag[..., 8:10], d1 = g, mg, dg.all(dim=-1)
        rec[..., 10] = any_in.to(dt)
        dec = (inside_sure | outside_sure) & d0 & d1
    n = b * V
    return {"rec": rec.reshape(n, R, RAY_FLOATS), "M_rec": mag.reshape(n, R, RAY_FLOATS).double(), "D": dec.reshape(n, R),
            "info": {k: v.reshape(n, R) for k, v in info.items()}, "o": o.reshape(n, R, 3)}


def rays(P32, uv, b: int, V: int, R: int, H: int, W: int, no_sample: int = 0, steps=None, dtype=F64, d32=None):
    """car_ray_setup.  P32 [b V, 96] fp32 pose records, uv [b, R, 2] -> dict(rec [b V, R, 12] in `dtype`, M_rec, D [b V, R], info).
    float64: d and m's own truth come from the pose and uv; start / end / overlaps (and m = o x d) are judged from `d32`, the direction
    record under test ([b V, R, 3]); without it from the float64 d."""
    out = _rays(P32, uv, b, V, R, H, W, no_sample, steps, dtype, d32 if dtype == F64 else None)
    if dtype != F64:
        ref = _rays(P32, uv, b, V, R, H, W, no_sample, steps, F64, out["rec"][..., 0:3])
        out["M_rec"], out["D"], out["info64"] = ref["M_rec"], ref["D"], ref["info"]
    return out


def coords9(rec, P32, V: int):
    """What ray_kernel writes to coords9 / phi_x: [d, m, o] per (set, ray), bits of the records."""
    n, R = rec.shape[:2]
    o = P32.reshape(n, 1, POSE_FLOATS)[..., [3, 7, 11]].expand(n, R, 3)
    return torch.cat([rec[..., 0:6], o.to(rec.dtype)], dim=-1)


# ---- samples -----------------------------------------------------------------------------------------------------------------------------
def _tanh_mag(x, mx):
    t = torch.tanh(x.double())
    return t.abs() + (1 - t * t) * mx.double()


def _samples(P32, R32, steps, b, V, R, P, H, W, no_sample, dt, grid32, pt32):
    n = b * V
    Pz = P32.to(dt).reshape(n, 1, 1, POSE_FLOATS)
    ray = R32.to(dt).reshape(n, R, 1, RAY_FLOATS)
    st = steps.to(dt).reshape(1, 1, P)
    kc = Pz[..., KC:KC + 4]
    oq = Pz[..., [3, 7, 11]].expand(n, R, P, 3)
    out = {}
    # pixel_val
    if not no_sample:
        s0, s1 = ray[..., 6:8], ray[..., 8:10]
        grid = s0 + (s1 - s0) * st[..., None]
        mgrid = s0.abs() + (s1.abs() + s0.abs()) * st[..., None].abs()
        dgrid = torch.ones_like(grid, dtype=torch.bool)
    else:
        du = ray[..., 0:3]
        q = oq + st[..., None] * du
        mq = oq.abs() + st[..., None].abs() * du.abs()
        grid, mgrid, dgrid = _project_grid(kc, q, mq, torch.isfinite(q) & (mq < BIG) | ~torch.isfinite(q), H, W)
    out.update(grid=grid, M_grid=mgrid, D_grid=dgrid)
    gu = grid if grid32 is None else grid32.to(dt).reshape(n, R, P, 2)
    # pt: the closest point on the query line to the sample's pixel ray
    px = (gu[..., 0] + 1.0) / 2.0 * float(W - 1)
    py = (gu[..., 1] + 1.0) / 2.0 * float(H - 1)
    l2f, oc, _ = _pixel_ray(Pz[..., C_REL:C_REL + 12], kc, px, py)
    m2f = _cross(oc, l2f)
    isl = dt == F32
    l1, m1 = ray[..., 0:3].double().expand(n, R, P, 3), ray[..., 3:6].double().expand(n, R, P, 3)
    l2, m2 = l2f.double(), m2f.double()
    nv = _cross(l1, l2, isl)
    l2xn = _cross(l2, nv, isl)
    first = _cross(m1, l2xn, isl)
    dotm = (m2[..., 0] * nv[..., 0] + m2[..., 1] * nv[..., 1]) + m2[..., 2] * nv[..., 2]
    nn = _norm3(nv, isl)
    den = nn * nn + 1e-12
    p1 = (-first + dotm[..., None] * l1) / den[..., None]
    fin = torch.isfinite(p1)
    if isl:
        pt = torch.where(fin, p1, torch.zeros_like(p1)).float()
    else:
        pt = torch.where(fin, torch.where(p1.abs() > FMAX, torch.sign(p1) * INF, p1), torch.zeros_like(p1))
    mn = _cross_mag(l1.abs(), l2.abs())
    mfirst = _cross_mag(m1.abs(), _cross_mag(l2.abs(), mn))
    mdot = (m2.abs() * mn).sum(dim=-1)
    mpt = torch.where(fin, (mfirst + mdot[..., None] * l1.abs()) / den[..., None], torch.zeros_like(p1))
    mpt = torch.where(torch.isfinite(mpt), mpt, torch.zeros_like(mpt))          # a NaN moment: pt is the scrub's exact 0
    dpt = ~fin | ((p1.abs() - FMAX).abs() > 1e-3 * FMAX)
    out.update(pt=pt, M_pt=mpt, D_pt=dpt, sin2=(nn * nn))
    pu = (pt if pt32 is None else pt32.reshape(n, R, P, 3)).to(dt)
    # the point in every context frame, and where it lands there
    pin, mpin, dpin, gin, mgin, dgin, qraw = [], [], [], [], [], [], []
    for s in range(V):
        T = Pz[..., T0 + 12 * s:T0 + 12 * s + 12]
        q, mq, dq = [], [], []
        for i in range(3):
            terms = [pu[..., 0] * T[..., 4 * i], pu[..., 1] * T[..., 4 * i + 1], pu[..., 2] * T[..., 4 * i + 2]]
            q.append(((terms[0] + terms[1]) + terms[2]) + T[..., 4 * i + 3])
            mq.append(sum(t.abs() for t in terms) + T[..., 4 * i + 3].abs())
            dq.append(torch.stack([~torch.isfinite(t) | (t.abs() < BIG) for t in terms]).all(dim=0))
        q, mq, dq = torch.stack(q, -1), torch.stack(mq, -1), torch.stack(dq, -1)
        ks = P32.to(dt).reshape(b, V, POSE_FLOATS)[:, s, KC:KC + 4].reshape(b, 1, 1, 1, 4).expand(b, V, 1, 1, 4).reshape(n, 1, 1, 4)
        g, mg, dg = _project_grid(ks, q, torch.where(torch.isfinite(mq), mq, torch.zeros_like(mq)), dq, H, W)
        t = torch.where(q != q, torch.zeros_like(q), torch.where(q == INF, torch.full_like(q, FMAX), torch.where(q == -INF, torch.full_like(q, -FMAX), q)))
        pin.append(t), mpin.append(torch.where(torch.isfinite(q), mq, t.abs())), dpin.append(dq)
        qraw.append(q)
        gin.append(g), mgin.append(mg), dgin.append(dg)
    out["q"] = torch.stack(qraw, -2)                                            # T[s] pt before nan_to_num
    out.update(pt_in=torch.stack(pin, -2), M_pt_in=torch.stack(mpin, -2), D_pt_in=torch.stack(dpin, -2),
               grid_in=torch.stack(gin, -2), M_grid_in=torch.stack(mgin, -2), D_grid_in=torch.stack(dgin, -2))
    # the geometric query
    vx, vy = (px - kc[..., 2]) / kc[..., 0], (py - kc[..., 3]) / kc[..., 1]
    cr = torch.stack([vx, vy, torch.ones_like(vx)], -1)
    ncr = _norm3(cr)
    ncr = torch.where(ncr > lit(1e-12, dt), ncr, lit(1e-12, dt))
    mpx, mpy = (gu[..., 0].abs() + 1.0) / 2.0 * float(W - 1), (gu[..., 1].abs() + 1.0) / 2.0 * float(H - 1)
    mcr = torch.stack([(mpx + kc[..., 2].abs()) / kc[..., 0].abs(), (mpy + kc[..., 3].abs()) / kc[..., 1].abs(), torch.ones_like(vx)], -1) / ncr[..., None]
    dv = pu - oq
    depth = _norm3(dv)
    mdepth = ((dv.abs() * (pu.abs() + oq.abs())).sum(dim=-1) / depth)
    mdepth = torch.where(torch.isfinite(mdepth), mdepth, torch.zeros_like(mdepth))
    ddepth = ~torch.isfinite(dv).all(dim=-1) | (dv.abs().amax(dim=-1) < 1e18)
    depth = torch.where(torch.isfinite(depth), depth, lit(1000000.0, dt).expand_as(depth))
    g16 = torch.zeros(n, R, P, G_DIM, dtype=dt)
    mg16 = torch.zeros(n, R, P, G_DIM, dtype=F64)
    dg16 = torch.ones(n, R, P, G_DIM, dtype=torch.bool)
    g16[..., 0:3], mg16[..., 0:3] = cr / ncr[..., None], mcr.double()
    g16[..., 6:9], mg16[..., 6:9] = ray[..., 0:3], ray[..., 0:3].abs().double()
    g16[..., 13:16], mg16[..., 13:16] = oq, oq.abs().double()
    for k, div in enumerate((None, 10.0, 100.0, 1000.0)):
        x = depth if div is None else depth / div
        g16[..., 9 + k] = torch.tanh(x)
        mg16[..., 9 + k] = _tanh_mag(x, mdepth if div is None else mdepth / div)
        dg16[..., 9 + k] = ddepth
    out.update(g=g16, M_g=mg16, D_g=dg16)
    # xenc
    if V == 1:
        xe = torch.cat([torch.tanh(pu / 5.0), torch.tanh(pu / 100.0)], dim=-1)
        mxe = torch.cat([_tanh_mag(pu / 5.0, _scrub(pu.abs() / 5.0, 0.0)), _tanh_mag(pu / 100.0, _scrub(pu.abs() / 100.0, 0.0))], dim=-1)
        dxe = torch.ones_like(xe, dtype=torch.bool)
    else:
        xe = torch.tanh(out["pt_in"] / 5.0)
        mxe = _tanh_mag(out["pt_in"] / 5.0, _scrub(out["M_pt_in"] / 5.0, 0.0))
        dxe = out["D_pt_in"]
    out.update(xenc=xe, M_xenc=mxe, D_xenc=dxe)
    S = n * R * P
    flat = {}
    for k, t in out.items():
        t = t.expand(n, R, P, *t.shape[3:]) if t.dim() >= 3 else t
        flat[k] = t.reshape(S, *t.shape[3:])
    return flat


FIELDS = ("grid", "pt", "g", "pt_in", "grid_in", "xenc")


def samples(P32, R32, steps, b: int, V: int, R: int, P: int, H: int, W: int, no_sample: int = 0, dtype=F64, grid32=None, pt32=None):
    """car_sample_setup over S = b V R P samples -> dict(grid [S, 2], pt [S, 3], g [S, 16], pt_in [S, V, 3], grid_in [S, V, 2],
    xenc [S, 6] (V = 1: tanh(pt / 5), tanh(pt / 100)) or [S, V, 3] (tanh(pt_in / 5)), sin2 [S]) in `dtype`, M_* and D_* from float64.
    float64: pt is judged from `grid32`, everything after it from `grid32` and `pt32` (the records under test); without them from the
    float64 values."""
    out = _samples(P32, R32, steps, b, V, R, P, H, W, no_sample, dtype, grid32 if dtype == F64 else None, pt32 if dtype == F64 else None)
    if dtype != F64:
        ref = _samples(P32, R32, steps, b, V, R, P, H, W, no_sample, F64, out["grid"], out["pt"])
        for k in ref:
            if k[:2] in ("M_", "D_") or k == "sin2":
                out[k] = ref[k]
    return out


# ---- car_project_points / car_exchange_rows -------------------------------------------------------------------------------------------------
def project_points(P32, pts, n_scenes: int, V: int, view: int, H: int, W: int, dtype=F64):
    """pts [n_scenes, npts, 3] through the intrinsics of view `view` of their scene -> dict(grid [n_scenes, npts, 2], M_grid, D_grid)."""
    def run(dt):
        k4 = P32.to(dt).reshape(n_scenes, V, POSE_FLOATS)[:, view, None, KC:KC + 4]
        p = pts.to(dt)
        return _project_grid(k4, p, _scrub(p.abs(), 0.0), torch.ones_like(p, dtype=torch.bool), H, W)
    g, mg, dg = run(dtype)
    if dtype != F64:
        _, mg, dg = run(F64)
    return {"grid": g, "M_grid": mg.double(), "D_grid": dg}


def exchange_rows(P32, pixel_val, pt_in, ptenc, n_scenes: int, V: int, pts: int, H: int, W: int, dtype=F64):
    """car_exchange_rows.  pixel_val [n_scenes V pts, 2], pt_in [n_scenes V pts, V, 3], ptenc [n_scenes V pts, V, 4] -> dict(row_src
    [rows] int32, row_grid [rows, 2], row_pe [rows, 4], M_row_grid, D_row_grid), rows = n_scenes V pts V ordered (scene, context c,
    sample j, component k): k = 0 is c's own sample; k >= 1 the other views o in ascending order — context o's sample j moved into
    frame c (pt_in[o's sample][c]), projected with view o's intrinsics, flagged 1 << 30."""
    sc, c, j, k = torch.meshgrid(torch.arange(n_scenes), torch.arange(V), torch.arange(pts), torch.arange(V), indexing="ij")
    o = torch.where(k == 0, c, torch.where(k - 1 < c, k - 1, k))
    so = (sc * V + o) * pts + j
    src = ((sc * V + o) | torch.where(k == 0, 0, 1 << 30)).to(torch.int32)

    def run(dt):
        k4 = P32.to(dt).reshape(n_scenes * V, POSE_FLOATS)[sc * V + o][..., KC:KC + 4]
        q = pt_in.to(dt)[so, c]
        g, mg, dg = _project_grid(k4, q, _scrub(q.abs(), 0.0), torch.ones_like(q, dtype=torch.bool), H, W)
        own = (k == 0)[..., None]
        pv = pixel_val.to(dt)[so]
        return torch.where(own, pv, g), torch.where(own, pv.abs(), mg), dg | own
    g, mg, dg = run(dtype)
    if dtype != F64:
        _, mg, dg = run(F64)
    pe = ptenc[so, c].clone()
    pe[..., 3] = 0.0
    return {"row_src": src.reshape(-1), "row_grid": g.reshape(-1, 2), "row_pe": pe.reshape(-1, 4), "M_row_grid": mg.reshape(-1, 2).double(),
            "D_row_grid": dg.reshape(-1, 2)}


# ---- input sets: built inside functions, never at import ---------------------------------------------------------------------------------
def _rot(yaw=0.0, pitch=0.0, roll=0.0):
    y, p, r = math.radians(yaw), math.radians(pitch), math.radians(roll)
    Ry = torch.tensor([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]], dtype=F64)
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]], dtype=F64)
    Rz = torch.tensor([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]], dtype=F64)
    return Ry @ Rx @ Rz


def _pose(Rm, t):
    T = torch.eye(4, dtype=F64)
    T[:3, :3], T[:3, 3] = Rm, torch.tensor(list(t), dtype=F64)
    return T


def _K(fx, fy, cx, cy):
    K = torch.eye(4, dtype=F64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return K


def set_uv(b: int, R: int, H: int, W: int, seed: int):
    """[b, R, 2] pixel coordinates: the four corners first, then the four edge midpoints, every fifth of the rest up to half an image
    outside the frame, the others inside; each scene its own."""
    g = gen(seed)
    wh = torch.tensor([W - 1.0, H - 1.0])
    uv = torch.rand(b, R, 2, generator=g) * wh
    out = torch.arange(R) % 5 == 4
    uv[:, out] = (torch.rand(b, int(out.sum()), 2, generator=g) * 2 - 0.5) * wh
    fixed = torch.tensor([[0, 0], [1, 0], [0, 1], [1, 1], [0.5, 0], [0.5, 1], [0, 0.5], [1, 0.5]]) * wh
    uv[:, :8] = fixed
    return uv.contiguous()


R_SET = 301             # two 256-thread blocks per (scene, view) pair and a ragged tail

# name: H, W, V, P, no_sample, world (yaw, pitch, t), view 1 and 2 relative to view 0, the query (a context index or a relative pose)
SETS = {
    "square":    dict(H=16, W=16, V=2, P=9, rel=(-12.0, 0.6), q="between"),
    "wide":      dict(H=12, W=20, V=2, P=7, rel=(-12.0, 0.6), q="between", wide=True),
    "diverging": dict(H=64, W=64, V=2, P=5, rel=(38.0, 0.9), q="between"),
    "v1":        dict(H=16, W=16, V=1, P=5, rel=(-12.0, 0.6), q=(-6.0, [0.3, 0.02, 0.03])),
    "v3":        dict(H=16, W=16, V=3, P=6, rel=(-12.0, 0.6), q="between"),
    "on-ctx0":   dict(H=16, W=16, V=2, P=9, rel=(-12.0, 0.6), q=0, identity=True),
    "on-ctx1":   dict(H=16, W=16, V=2, P=8, rel=(-12.0, 0.6), q=1),
    "behind":    dict(H=16, W=16, V=2, P=7, rel=(-12.0, 0.6), q=(3.0, [0.1, 0.05, -0.8])),
    # the query 1.03e-6 from context 0's centre and 9.9e-7 in front of its plane: depth_zero without at_camera while o itself projects
    # inside the frame — the one place where the `depth_zero && !at_camera` rule decides ok0
    "near":      dict(H=16, W=16, V=2, P=5, rel=(-12.0, 0.6), q=(2.0, [3e-7, 0.0, 9.9e-7]), identity=True),
    "backward":  dict(H=16, W=16, V=2, P=6, rel=(-12.0, 0.6), q=(95.0, [0.2, -0.05, 0.3])),
    "depths":    dict(H=16, W=16, V=2, P=8, rel=(-12.0, 0.6), q=(4.0, [0.25, 0.02, -0.5]), no_sample=1),
    # no_sample with the query exactly on context 0 and the principal point on the last pixel column: ray 8 (uv = the principal point) is
    # d = (0, 0, 1) exactly and every one of its samples lands on grid x = 1.0 exactly, which any_in's strict `< 1` leaves outside
    "rim":       dict(H=16, W=16, V=2, P=6, rel=(-12.0, 0.6), q=0, identity=True, no_sample=1, rim=True),
}
DEPTH_STEPS = (0.1, -0.7, 0.45, 0.55, INF, 2.5, 6.0, 10.0)      # `rim` (P = 6) ends on 2.5


def cameras(name: str, b: int = 2):
    """dict(c2w_ctx [b, V, 4, 4], c2w_q [b, 1, 4, 4], K_ctx, K_q, uv [b, R, 2], steps [P]) of a set, all float32, and its sizes."""
    c = dict(SETS[name])
    H, W, V, P = c["H"], c["W"], c["V"], c["P"]
    g = gen(1000 + sorted(SETS).index(name))
    ctx, qs = [], []
    for i in range(b):
        jit = torch.rand(6, generator=g, dtype=F64) - 0.5
        world = torch.eye(4, dtype=F64) if c.get("identity") else _pose(_rot(20.0 + 10 * jit[0].item(), -8.0 + 6 * jit[1].item()), [0.3 + jit[2].item(), -0.2, 1.5])
        yaw, base = c["rel"]
        cams = [world, world @ _pose(_rot(yaw + 4 * jit[3].item(), 2.0 * jit[4].item()), [base, 0.03 + 0.05 * jit[5].item(), 0.05]),
                world @ _pose(_rot(-0.6 * yaw, 3.0), [-0.5 * base, -0.04, 0.08])][:V]
        if c["q"] == "between":
            q = cams[0] @ _pose(_rot(0.5 * yaw, 1.5, 1.0), [0.5 * base, 0.04, -0.03])
        elif isinstance(c["q"], int):
            q = cams[c["q"]].clone()
        else:
            q = cams[0] @ _pose(_rot(c["q"][0], 1.0), c["q"][1])
        ctx.append(torch.stack(cams)), qs.append(q[None])
    if c.get("wide"):
        Kc = torch.stack([_K(17.3, 11.9, 9.1, 6.7), _K(18.4, 10.6, 10.4, 5.2)])[None].expand(b, V, 4, 4)
        Kq = _K(16.1, 12.4, 10.3, 5.6)[None, None].expand(b, 1, 4, 4)
    else:
        Kc = _K(0.879 * H, 0.879 * H, H / 2.0, H / 2.0)[None, None].expand(b, V, 4, 4)
        Kq = _K(0.879 * H, 0.879 * H, H / 2.0, H / 2.0)[None, None].expand(b, 1, 4, 4)
    if c.get("rim"):
        Kc = _K(14.1, 14.1, W - 1.0, 7.5)[None, None].expand(b, V, 4, 4)
        Kq = _K(14.1, 14.1, W - 1.0, 7.5)[None, None].expand(b, 1, 4, 4)
    steps = torch.tensor(DEPTH_STEPS[:P]) if c.get("no_sample") else torch.linspace(0.0, 1.0, P)
    f = lambda t: t.float().contiguous()
    uv = set_uv(b, R_SET, H, W, 77 + P)
    uv[:, 8] = f(Kq)[0, 0, :2, 2]                                              # ray 8: through the query camera's principal point
    return dict(name=name, b=b, V=V, R=R_SET, P=P, H=H, W=W, no_sample=int(c.get("no_sample", 0)), c2w_ctx=f(torch.stack(ctx)), c2w_q=f(torch.stack(qs)),
                K_ctx=f(Kc), K_q=f(Kq), uv=uv, steps=f(steps))


def pose_set(b: int = 65, V: int = 3):
    """The pose-kernel set: b = 65 (a second 64-thread block with one live thread), V = 3; translations up to 1e3; scene 7 mildly
    non-orthonormal (a 2 % shear and scale on its rotations)."""
    g = gen(4242)
    ctx = torch.zeros(b, V, 4, 4, dtype=F64)
    q = torch.zeros(b, 1, 4, 4, dtype=F64)
    for i in range(b):
        r = torch.rand(V + 1, 6, generator=g, dtype=F64) - 0.5
        scale = 1e3 if i % 8 == 3 else (30.0 if i % 8 == 5 else 1.0)
        for v in range(V + 1):
            M = _pose(_rot(120 * r[v, 0].item(), 60 * r[v, 1].item(), 40 * r[v, 2].item()), (2 * scale * r[v, 3:6]).tolist())
            if i == 7:
                M[:3, :3] = M[:3, :3] @ (torch.eye(3, dtype=F64) + 0.02 * torch.tensor([[1.0, 0.5, 0.0], [0.0, -1.0, 0.3], [0.2, 0.0, 0.5]], dtype=F64))
            if v < V:
                ctx[i, v] = M
            else:
                q[i, 0] = M
    H = 12
    Kc = torch.stack([_K(17.3, 11.9, 9.1, 6.7), _K(18.4, 10.6, 10.4, 5.2), _K(15.0, 15.0, 9.5, 5.5)])[None].expand(b, V, 4, 4)
    Kq = _K(16.1, 12.4, 10.3, 5.6)[None, None].expand(b, 1, 4, 4)
    f = lambda t: t.float().contiguous()
    return dict(b=b, V=V, H=H, c2w_ctx=f(ctx), c2w_q=f(q), K_ctx=f(Kc), K_q=f(Kq))


def edit_rays(rec):
    """Edits CarRay records [n, R, 12] in place for the sample stage (the rays a sample stage is fed are inputs like any other): ray 9 of
    set 0 a NaN moment (p1 not finite: pt the scrub's 0); rays 10..13 of the last set moments of +-3e38 (p1 beyond fp32: pt +-inf, T pt
    of all three nan_to_num kinds, landing points scrubbed to 1e10)."""
    rec[0, 9, 3:6] = float("nan")
    for r, m in ((10, (3e38, 0.0, 0.0)), (11, (0.0, -3e38, 3e38)), (12, (3e38, 3e38, -3e38)), (13, (-3e38, 0.0, 3e38))):
        rec[-1, r, 3:6] = torch.tensor(m)
    return rec


def exchange_inputs(V: int, n_scenes: int = 2, pts: int = 151, seed: int = 31):
    """pixel_val, pt_in, ptenc for car_exchange_rows: points around the cameras, some on the camera plane (z = -1e-12f: zz exactly 0),
    some at +-inf / NaN; ptenc's fourth float NaN (the kernel must write 0 there)."""
    g = gen(seed)
    S = n_scenes * V * pts
    pv = torch.rand(S, 2, generator=g) * 2.4 - 1.2
    pin = torch.randn(S, V, 3, generator=g) * torch.tensor([1.0, 1.0, 2.0]) + torch.tensor([0.0, 0.0, 1.5])
    pin[3, :, 2] = -torch.tensor(1e-12)
    pin[5, :, 0], pin[6, :, 2], pin[7, :, 1] = INF, -INF, float("nan")
    pin[8, :, 2] = 1e-20
    pe = torch.randn(S, V, 4, generator=g)
    pe[..., 3] = float("nan")
    return pv.contiguous(), pin.contiguous(), pe.contiguous()


def project_inputs(n_scenes: int = 2, npts: int = 301, seed: int = 37):
    g = gen(seed)
    p = torch.randn(n_scenes, npts, 3, generator=g) * torch.tensor([1.0, 1.0, 2.0]) + torch.tensor([0.0, 0.0, 1.0])
    p[0, 3, 2] = -torch.tensor(1e-12)
    p[0, 5, 0], p[1, 6, 2], p[1, 7, 1], p[0, 8, 2] = INF, -INF, float("nan"), 1e-20
    return p.contiguous()


@functools.lru_cache(maxsize=None)
def stage(name: str):
    """A set through every stage, once, shared by both suites (never modified): the float32 pose records P32 of its cameras, the
    float32 rays and their float64 judgement, the ray records R32 the sample stage is fed (edit_rays applied), the float32 samples and
    their float64 judgement."""
    c = cameras(name)
    P32 = poses(c["c2w_ctx"], c["c2w_q"], c["K_ctx"], c["K_q"], c["H"], dtype=F32)["rec"]
    dims = (c["b"], c["V"], c["R"], c["H"], c["W"])
    r32 = rays(P32, c["uv"], *dims, c["no_sample"], c["steps"], dtype=F32)
    r64 = rays(P32, c["uv"], *dims, c["no_sample"], c["steps"], dtype=F64, d32=r32["rec"][..., 0:3])
    R32 = edit_rays(r32["rec"].clone())
    sd = (c["b"], c["V"], c["R"], c["P"], c["H"], c["W"], c["no_sample"])
    s32 = samples(P32, R32, c["steps"], *sd, dtype=F32)
    s64 = samples(P32, R32, c["steps"], *sd, dtype=F64, grid32=s32["grid"], pt32=s32["pt"])
    return dict(c=c, P32=P32, r32=r32, r64=r64, R32=R32, s32=s32, s64=s64)


RAY_FIELDS = {"d": (0, 3), "m": (3, 6), "start": (6, 8), "end": (8, 10)}


def ray_ratios(rec, r64):
    """Worst ratio of each CarRay field of `rec` against the float64 judgement r64 (made from rec's own d), on the decided rays."""
    return {f: ratio(rec[..., a:z], r64["rec"][..., a:z], r64["M_rec"][..., a:z], r64["D"][..., None]) for f, (a, z) in RAY_FIELDS.items()}


def sample_ratios(s, s64):
    return {f: ratio(s[f], s64[f], s64["M_" + f], s64["D_" + f]) for f in FIELDS}
