"""Float64 numpy restatement of the relative-pose estimator (csrc/car_pose.hip, harness.estimate_pose) and
the seeded two-view scenes its tests run on.  Test infrastructure: the product never imports this file.

What is independent of the product and what is not:
  * COPIES.  ``sample_table`` and ``recover_pose`` are ``harness.pose_sample_table`` and ``harness.recover_pose`` line for line; the
    tests that compare each pair only guard against one side drifting.  What checks them is the table's properties (range, five
    distinct indices) and the ground-truth pose that recover_pose must return.
  * THE DEVICE'S FORMULATION IN NUMPY.  Null space (complete pivoting), the ten cubics, their elimination, B(z), the choice of rows for
    x and y and the Gauss-Newton polishing follow csrc/car_pose.hip step for step, vectorised over hypotheses, so that the
    candidates come in the device's order and a winner can be compared index for index.  A mistake in the formulation would be
    in both.
  * INDEPENDENT.  The roots of the degree-10 polynomial are the eigenvalues of its companion matrix (``numpy.linalg.eigvals``), where
    the device brackets them through the chain of derivatives; ``residuals`` evaluates the constraints on E itself with numpy's
    det and matrix products; the scenes carry their true (R, t).
What makes it a reference and not a copy is therefore tests/test_pose_reference.py: on seeded scenes the true essential matrix is
among its candidates and the true pose comes back, which no shared mistake in the formulation would survive.

  sample_table        H rows of five distinct indices (harness.pose_sample_table restated)
  solve               the five-point solver: cand [H,10,9], nsol [H]
  sampson / score     cv2's error for the model, and the inlier counts
  select              the winner under the tie rule (largest count, lowest hypothesis, lowest candidate)
  recover_pose        OpenCV's documented recoverPose (four combinations, linear triangulation, cheirality count)
  estimate            the whole estimator
  decided / spread    stability of a hypothesis / a result under relative perturbations of 2^-40
"""
from __future__ import annotations

import numpy as np

# ---- monomial tables (the device's constexpr tables are the same lists, csrc/car_pose.hip) -------------------------------------------
LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]                                                    # x y z 1
QUAD = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
# Nister's column order: the ten monomials eliminated first, then x (z^2 z 1), y (z^2 z 1), (z^3 z^2 z 1)
CUBIC = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


Q2 = [[QUAD.index(_add(a, b)) for b in LIN] for a in LIN]            # linear x linear -> quadratic slot
C3 = [[CUBIC.index(_add(q, l)) for l in LIN] for q in QUAD]          # quadratic x linear -> cubic column

PIVOT_EPS = 1e-13                                                    # a pivot at or below this share of its matrix's scale is zero
MAX_BOUND = 2.0 ** 70                                                # a Cauchy bound on the roots at or above this refuses the hypothesis


def sample_table(n: int, hypotheses: int, seed: int = 0) -> np.ndarray:
    """``hypotheses`` rows of five distinct indices below ``n``, uniform over ordered 5-tuples: the k-th index is drawn among the
    n - k values not yet taken (one ``integers`` call for the whole table)."""
    g = np.random.default_rng(seed)
    out = np.empty((hypotheses, 5), dtype=np.int64)
    draws = g.integers(0, np.array([n, n - 1, n - 2, n - 3, n - 4]), size=(hypotheses, 5))
    for k in range(5):
        idx = draws[:, k].copy()
        prev = np.sort(out[:, :k], axis=1)
        for j in range(k):
            idx += idx >= prev[:, j]
        out[:, k] = idx
    return out.astype(np.int32)


def _mul_ll(a, b):
    out = np.zeros(a.shape[:-1] + (10,))
    for i in range(4):
        for j in range(4):
            out[..., Q2[i][j]] += a[..., i] * b[..., j]
    return out


def _mul_ql(q, l):
    out = np.zeros(q.shape[:-1] + (20,))
    for i in range(10):
        for j in range(4):
            out[..., C3[i][j]] += q[..., i] * l[..., j]
    return out


def _nullspace(A):
    """A [H,5,9] -> basis [H,4,9] (rows X Y Z W), ok [H]: Gauss-Jordan with complete pivoting (first maximum in row-major order)."""
    A = A.copy()
    H = A.shape[0]
    rows = np.arange(H)
    perm = np.tile(np.arange(9), (H, 1))
    scale = np.abs(A).reshape(H, -1).max(axis=1)
    ok = np.isfinite(scale) & (scale > 0)
    for k in range(5):
        sub = np.abs(A[:, k:, k:]).reshape(H, -1)
        sub = np.where(np.isnan(sub), -1.0, sub)
        at = sub.argmax(axis=1)
        pr, pc = k + at // (9 - k), k + at % (9 - k)
        ok &= sub[rows, at] > PIVOT_EPS * scale
        tmp = A[rows, k].copy(); A[rows, k] = A[rows, pr]; A[rows, pr] = tmp
        tmp = A[rows, :, k].copy(); A[rows, :, k] = A[rows, :, pc]; A[rows, :, pc] = tmp
        tmp = perm[rows, k].copy(); perm[rows, k] = perm[rows, pc]; perm[rows, pc] = tmp
        with np.errstate(all="ignore"):
            A[:, k] = A[:, k] / A[:, k, k][:, None]
            for r in range(5):
                if r != k:
                    A[:, r] = A[:, r] - A[:, r, k][:, None] * A[:, k]
    basis = np.zeros((H, 4, 9))
    for f in range(4):
        v = np.zeros((H, 9))
        v[:, 5 + f] = 1.0
        v[:, :5] = -A[:, :, 5 + f]
        basis[rows[:, None], f, perm] = v
    return basis, ok


def _constraints(basis):
    """basis [H,4,9] -> M [H,10,20]: rows 0-8 the entries of (E E^T - tr(E E^T) / 2) E row-major, row 9 det E."""
    H = basis.shape[0]
    E = [[basis[:, :, 3 * r + c] for c in range(3)] for r in range(3)]                      # linear polynomials [H,4]
    EEt = [[sum(_mul_ll(E[i][k], E[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    half_tr = 0.5 * (EEt[0][0] + EEt[1][1] + EEt[2][2])
    L = [[EEt[i][j] - (half_tr if i == j else 0.0) for j in range(3)] for i in range(3)]
    M = np.zeros((H, 10, 20))
    for i in range(3):
        for j in range(3):
            M[:, 3 * i + j] = sum(_mul_ql(L[i][k], E[k][j]) for k in range(3))
    M[:, 9] = (_mul_ql(_mul_ll(E[1][1], E[2][2]) - _mul_ll(E[1][2], E[2][1]), E[0][0])
               - _mul_ql(_mul_ll(E[1][0], E[2][2]) - _mul_ll(E[1][2], E[2][0]), E[0][1])
               + _mul_ql(_mul_ll(E[1][0], E[2][1]) - _mul_ll(E[1][1], E[2][0]), E[0][2]))
    return M


def _eliminate(M):
    """Gauss-Jordan on the first ten columns, rows scaled to unit maximum first, partial pivoting (first maximum).  Returns the right
    half [H,10,10] and ok."""
    M = M.copy()
    H = M.shape[0]
    rows = np.arange(H)
    with np.errstate(all="ignore"):
        rmax = np.abs(M).max(axis=2)
        ok = np.isfinite(rmax).all(axis=1) & (rmax > 0).all(axis=1)
        M = M / rmax[:, :, None]
        for k in range(10):
            col = np.abs(M[:, k:, k])
            col = np.where(np.isnan(col), -1.0, col)
            at = col.argmax(axis=1)
            ok &= col[rows, at] > PIVOT_EPS
            pr = k + at
            tmp = M[rows, k].copy(); M[rows, k] = M[rows, pr]; M[rows, pr] = tmp
            M[:, k] = M[:, k] / M[:, k, k][:, None]
            for r in range(10):
                if r != k:
                    M[:, r] = M[:, r] - M[:, r, k][:, None] * M[:, k]
    return M[:, :, 10:], ok


def _conv(a, b):
    out = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            out[:, i + j] += a[:, i] * b[:, j]
    return out


def _bz(R):
    """The 3 x 3 polynomial matrix B(z) with B (x, y, 1)^T = 0: rows <4> - z <5>, <6> - z <7>, <8> - z <9>; coefficients ascending."""
    B = []
    for ra, rb in ((4, 5), (6, 7), (8, 9)):
        a, b = R[:, ra], R[:, rb]
        bx = np.stack([a[:, 2], a[:, 1] - b[:, 2], a[:, 0] - b[:, 1], -b[:, 0]], axis=1)
        by = np.stack([a[:, 5], a[:, 4] - b[:, 5], a[:, 3] - b[:, 4], -b[:, 3]], axis=1)
        bc = np.stack([a[:, 9], a[:, 8] - b[:, 9], a[:, 7] - b[:, 8], a[:, 6] - b[:, 7], -b[:, 6]], axis=1)
        B.append((bx, by, bc))
    return B


def _polyval(c, z):
    out = np.zeros_like(z)
    for k in range(c.shape[1] - 1, -1, -1):
        out = out * z + c[:, k][:, None]
    return out


def _constraints_at(E):
    """E [...,3,3] -> f [...,10] = (2 E E^T E - tr(E E^T) E, det E), G = E E^T, tr."""
    G = E @ np.swapaxes(E, -1, -2)
    tr = np.trace(G, axis1=-2, axis2=-1)
    f = 2 * G @ E - tr[..., None, None] * E
    return np.concatenate([f.reshape(E.shape[:-2] + (9,)), np.linalg.det(E)[..., None]], axis=-1), G, tr


def _polish(basis, u, steps: int = 3):
    """Gauss-Newton on the ten constraints in (x, y, z) of E = x X + y Y + z Z + W; basis [H,4,9], u [H,10,3].  A step is kept only
    where it lowers |f|^2."""
    Bm = basis.reshape(basis.shape[0], 1, 4, 3, 3)
    make = lambda u: (u[..., None, None] * Bm[:, :, :3]).sum(axis=2) + Bm[:, :, 3]
    u = u.copy()
    live = np.isfinite(u).all(axis=2)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            E = make(u)
            f, G, tr = _constraints_at(E)
            ss = (f * f).sum(axis=-1)
            J = []
            Et = np.swapaxes(E, -1, -2)
            # cofactor matrix without an inverse: rows are cross products of the other two rows
            C = np.stack([np.cross(E[..., 1, :], E[..., 2, :]), np.cross(E[..., 2, :], E[..., 0, :]), np.cross(E[..., 0, :], E[..., 1, :])], axis=-2)
            for d in range(3):
                D = np.broadcast_to(Bm[:, :, d], E.shape)
                S = D @ Et
                df = 2 * (S @ E + np.swapaxes(S, -1, -2) @ E + G @ D) - 2 * np.trace(S, axis1=-2, axis2=-1)[..., None, None] * E - tr[..., None, None] * D
                J.append(np.concatenate([df.reshape(E.shape[:-2] + (9,)), (C * D).sum(axis=(-1, -2))[..., None]], axis=-1))
            J = np.stack(J, axis=-1)                                                        # [H,10,10,3]
            A = np.swapaxes(J, -1, -2) @ J
            b = -(np.swapaxes(J, -1, -2) @ f[..., None])[..., 0]
            adj = np.stack([np.cross(A[..., 1, :], A[..., 2, :]), np.cross(A[..., 2, :], A[..., 0, :]), np.cross(A[..., 0, :], A[..., 1, :])], axis=-1)
            det = (A[..., 0, :] * adj[..., :, 0]).sum(axis=-1)
            v = u + (adj @ b[..., None])[..., 0] / det[..., None]
            f2, _, _ = _constraints_at(make(v))
            live = live & ((f2 * f2).sum(axis=-1) < ss)
            u = np.where(live[..., None], v, u)
    return u


def solve(x0, x1, samples):
    """cand [H,10,9] float64 (unit Frobenius norm, row-major, ascending z; unused slots zero), nsol [H] int32."""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    samples = np.asarray(samples)
    H, N = samples.shape[0], x0.shape[0]
    valid = ((samples >= 0) & (samples < N)).all(axis=1)
    s = np.sort(samples, axis=1)
    valid &= (s[:, 1:] != s[:, :-1]).all(axis=1)
    idx = np.where(valid[:, None], samples, 0)
    p0, p1 = x0[idx], x1[idx]                                                              # [H,5,2]
    valid &= np.isfinite(p0).all(axis=(1, 2)) & np.isfinite(p1).all(axis=(1, 2))
    p0, p1 = np.where(valid[:, None, None], p0, 0.0), np.where(valid[:, None, None], p1, 0.0)
    h0 = np.concatenate([p0, np.ones((H, 5, 1))], axis=2)
    h1 = np.concatenate([p1, np.ones((H, 5, 1))], axis=2)
    A = (h1[:, :, :, None] * h0[:, :, None, :]).reshape(H, 5, 9)                           # x1^T E x0, E row-major
    basis, ok = _nullspace(A)
    valid &= ok
    basis = np.where(valid[:, None, None], basis, 0.0)
    R, ok = _eliminate(_constraints(basis))
    valid &= ok
    R = np.where(valid[:, None, None], R, 0.0)
    B = _bz(R)
    (a0, a1, a2), (b0, b1, b2), (c0, c1, c2) = B
    poly = _conv(a0, _conv(b1, c2) - _conv(b2, c1)) - _conv(a1, _conv(b0, c2) - _conv(b2, c0)) + _conv(a2, _conv(b0, c1) - _conv(b1, c0))
    with np.errstate(all="ignore"):
        pmax = np.abs(poly).max(axis=1)
        valid &= np.isfinite(pmax) & (pmax > 0)
        poly = poly / np.where(valid, pmax, 1.0)[:, None]
        lead = poly[:, 10]
        valid &= np.isfinite(1.0 / lead) & (1.0 + np.abs(poly[:, :10]).max(axis=1) / np.abs(lead) < MAX_BOUND)
        monic = np.where(valid[:, None], poly[:, :10] / np.where(valid, lead, 1.0)[:, None], 0.0)
    comp = np.zeros((H, 10, 10))
    comp[:, np.arange(1, 10), np.arange(0, 9)] = 1.0
    comp[:, :, 9] = -monic
    ev = np.linalg.eigvals(comp)
    real = (np.imag(ev) == 0) & valid[:, None]
    z = np.where(real, np.real(ev), np.inf)
    order = np.argsort(z, axis=1, kind="stable")
    z = np.take_along_axis(z, order, axis=1)
    real = np.isfinite(z)
    z = np.where(real, z, 0.0)
    with np.errstate(all="ignore"):
        rows = [np.stack([_polyval(p, z) for p in B[r]], axis=2) for r in range(3)]        # [H,10,3] each
        crosses = [np.cross(rows[0], rows[1]), np.cross(rows[0], rows[2]), np.cross(rows[1], rows[2])]
        w = np.stack([np.abs(c[:, :, 2]) for c in crosses], axis=2)
        w = np.where(np.isnan(w), -1.0, w)
        pick = w.argmax(axis=2)
        c = np.take_along_axis(np.stack(crosses, axis=2), pick[:, :, None, None], axis=2)[:, :, 0]
        x, y = c[:, :, 0] / c[:, :, 2], c[:, :, 1] / c[:, :, 2]
        u = _polish(basis, np.stack([x, y, z], axis=2))
        x, y, z = u[:, :, 0], u[:, :, 1], u[:, :, 2]
        E = (x[:, :, None] * basis[:, None, 0] + y[:, :, None] * basis[:, None, 1] + z[:, :, None] * basis[:, None, 2] + basis[:, None, 3])
        nrm = np.sqrt((E * E).sum(axis=2))
        E = E / nrm[:, :, None]
        good = real & np.isfinite(E).all(axis=2) & (nrm > 0)
    cand = np.zeros((H, 10, 9))
    nsol = good.sum(axis=1).astype(np.int32)
    slot = np.cumsum(good, axis=1) - 1
    hh, cc = np.nonzero(good)
    cand[hh, slot[hh, cc]] = E[hh, cc]
    return cand, nsol


def sampson(E, x0, x1):
    """(x1^T E x0)^2 / ((E x0)_1^2 + (E x0)_2^2 + (E^T x1)_1^2 + (E^T x1)_2^2); E [...,9] against every match: [..., N]."""
    E = np.asarray(E, dtype=np.float64)[..., None]
    x, y, u, v = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    with np.errstate(all="ignore"):
        a = E[..., 0, :] * x + E[..., 1, :] * y + E[..., 2, :]
        b = E[..., 3, :] * x + E[..., 4, :] * y + E[..., 5, :]
        c = E[..., 6, :] * x + E[..., 7, :] * y + E[..., 8, :]
        ta = E[..., 0, :] * u + E[..., 3, :] * v + E[..., 6, :]
        tb = E[..., 1, :] * u + E[..., 4, :] * v + E[..., 7, :]
        r = u * a + v * b + c
        return (r * r) / (a * a + b * b + ta * ta + tb * tb)


def score(cand, nsol, x0, x1, thresh, chunk: int = 256):
    """counts [H,10] int32 (0 for unused slots; a non-finite error is no inlier), hyp_best [H] int32."""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    H = cand.shape[0]
    counts = np.zeros((H, 10), dtype=np.int32)
    for h0 in range(0, H, chunk):
        err = sampson(cand[h0:h0 + chunk], x0, x1)
        with np.errstate(invalid="ignore"):
            counts[h0:h0 + chunk] = (err < thresh * thresh).sum(axis=2)
    counts[np.arange(10)[None, :] >= np.asarray(nsol)[:, None]] = 0
    return counts, counts.max(axis=1).astype(np.int32)


def select(cand, nsol, counts, x0, x1, thresh):
    """E [9], best (count, hypothesis, candidate), inliers [N] uint8; (zeros, (0, -1, -1), zeros) when no hypothesis has a candidate."""
    used = np.arange(10)[None, :] < np.asarray(nsol)[:, None]
    N = np.asarray(x0).shape[0]
    if not used.any():
        return np.zeros(9), (0, -1, -1), np.zeros(N, dtype=np.uint8)
    key = np.where(used, counts.astype(np.int64), -1).reshape(-1)
    at = int(key.argmax())                                                                 # first maximum: lowest hypothesis, lowest candidate
    h, c = at // 10, at % 10
    with np.errstate(invalid="ignore"):
        inl = (sampson(cand[h, c], np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)) < thresh * thresh).astype(np.uint8)
    return cand[h, c].copy(), (int(counts[h, c]), h, c), inl


def ransac(x0, x1, samples, thresh):
    cand, nsol = solve(x0, x1, samples)
    counts, hyp_best = score(cand, nsol, x0, x1, thresh)
    E, best, inl = select(cand, nsol, counts, x0, x1, thresh)
    return dict(cand=cand, nsol=nsol, counts=counts, hyp_best=hyp_best, E=E, best=best, inliers=inl)


def recover_pose(E, x0, x1, mask, dist: float = 1e9):
    """OpenCV's recoverPose from its documentation: SVD with det(U) = det(V^T) = +1, R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]; of
    (R1, t), (R2, t), (R1, -t), (R2, -t) the first with the most inliers triangulated (linear, P0 = [I | 0], P1 = [R | t]) to
    0 < z < dist in both cameras.  Returns n, R, t, mask (the inliers that pass for the winner)."""
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    sel = np.nonzero(np.asarray(mask).astype(bool))[0]
    a, b = np.asarray(x0, dtype=np.float64)[sel], np.asarray(x1, dtype=np.float64)[sel]
    best = None
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P1 = np.concatenate([R, tt[:, None]], axis=1)
        A = np.zeros((len(sel), 4, 4))
        A[:, 0, 0], A[:, 0, 2] = -1.0, a[:, 0]
        A[:, 1, 1], A[:, 1, 2] = -1.0, a[:, 1]
        A[:, 2] = b[:, 0, None] * P1[2][None] - P1[0][None]
        A[:, 3] = b[:, 1, None] * P1[2][None] - P1[1][None]
        Q = np.linalg.svd(A)[2][:, 3] if len(sel) else np.zeros((0, 4))
        with np.errstate(all="ignore"):
            X = Q[:, :3] / Q[:, 3:4]
            z0 = X[:, 2]
            z1 = (X @ R.T + tt)[:, 2]
            good = (z0 > 0) & (z0 < dist) & (z1 > 0) & (z1 < dist)
        if best is None or good.sum() > best[0]:
            best = (int(good.sum()), R, tt, good)
    out = np.zeros(len(np.asarray(mask)), dtype=bool)
    out[sel] = best[3]
    return best[0], best[1], best[2], out


def normalise(kpts0, kpts1, K0, K1, thresh):
    K0, K1 = np.asarray(K0, dtype=np.float64), np.asarray(K1, dtype=np.float64)
    f_mean = np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])
    x0 = (np.asarray(kpts0, dtype=np.float64) - K0[[0, 1], [2, 2]][None]) / K0[[0, 1], [0, 1]][None]
    x1 = (np.asarray(kpts1, dtype=np.float64) - K1[[0, 1], [2, 2]][None]) / K1[[0, 1], [0, 1]][None]
    return x0, x1, thresh / f_mean


def estimate(kpts0, kpts1, K0, K1, thresh, hypotheses=8192, seed=0, samples=None):
    """The whole estimator: (R, t, mask, ransac dict) or None."""
    if len(kpts0) < 5:
        return None
    x0, x1, nt = normalise(kpts0, kpts1, K0, K1, thresh)
    samples = sample_table(len(x0), hypotheses, seed) if samples is None else samples
    r = ransac(x0, x1, samples, nt)
    if r["best"][0] < 1:
        return None
    n, R, t, mask = recover_pose(r["E"], x0, x1, r["inliers"])
    if n < 1:
        return None
    return R, t, mask, r


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
K = np.array([[225.0, 0.0, 128.0], [0.0, 225.0, 128.0], [0.0, 0.0, 1.0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(n: int, seed: int, noise: float = 0.0, outliers: float = 0.0, angle: float = 0.25):
    """n matches in pixels of two 256 x 256 views with K: a rotation of ``angle`` rad about a random axis, a unit baseline, points in
    the first camera's frustum at depth 2..8 that also project inside the second image; Gaussian pixel noise of ``noise`` on both
    views; the LAST round(outliers * n) matches replaced by uniform pixels in the second view.  Returns kpts0, kpts1, R, t, is_inlier."""
    g = np.random.default_rng(seed)
    axis = g.normal(size=3)
    R = rodrigues(angle * axis / np.linalg.norm(axis))
    t = g.normal(size=3)
    t /= np.linalg.norm(t)
    pts0, pts1 = [], []
    while len(pts0) < n:
        uv = g.uniform(8.0, 248.0, size=(4 * n, 2))
        d = g.uniform(2.0, 8.0, size=4 * n)
        X = np.concatenate([(uv - 128.0) / 225.0, np.ones((4 * n, 1))], axis=1) * d[:, None]
        Y = X @ R.T + t
        p = Y[:, :2] / Y[:, 2:3] * 225.0 + 128.0
        keep = (Y[:, 2] > 0.5) & (p > 8.0).all(axis=1) & (p < 248.0).all(axis=1)
        pts0.extend(uv[keep]); pts1.extend(p[keep])
    k0, k1 = np.array(pts0[:n]), np.array(pts1[:n])
    if noise > 0:
        k0 = k0 + g.normal(scale=noise, size=k0.shape)
        k1 = k1 + g.normal(scale=noise, size=k1.shape)
    n_out = int(round(outliers * n))
    good = np.ones(n, dtype=bool)
    if n_out:
        k1[n - n_out:] = g.uniform(0.0, 256.0, size=(n_out, 2))
        good[n - n_out:] = False
    return k0, k1, R, t, good


def true_E(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return (E / np.linalg.norm(E)).reshape(9)


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def dir_angle(ta, tb):
    c = np.dot(ta, tb) / (np.linalg.norm(ta) * np.linalg.norm(tb))
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


# ---- decidedness and spread ----------------------------------------------------------------------------------------------------------------
PERTURB = 2.0 ** -40


def perturbed(x0, x1, k: int):
    """Run k of the perturbation: every coordinate times 1 + 2^-40 u, u uniform in [-1, 1], seeded by k."""
    g = np.random.default_rng(1000 + k)
    return x0 * (1 + PERTURB * g.uniform(-1, 1, size=x0.shape)), x1 * (1 + PERTURB * g.uniform(-1, 1, size=x1.shape))


def _winner(counts, nsol):
    used = np.arange(10)[None, :] < nsol[:, None]
    return np.where(used, counts, -1).argmax(axis=1)


def decided(x0, x1, samples, thresh, base=None, runs: int = 2):
    """[H] bool: the hypothesis's nsol, hyp_best and winning candidate are those of ``base`` in every perturbed run.  Only the five
    sample points of each hypothesis are perturbed (the matches it is scored on stay), as the definition says."""
    base = ransac(x0, x1, samples, thresh) if base is None else base
    ok = np.ones(len(samples), dtype=bool)
    win = _winner(base["counts"], base["nsol"])
    for k in range(runs):
        p0, p1 = perturbed(x0, x1, k)
        cand, nsol = solve(p0, p1, samples)
        counts, hb = score(cand, nsol, x0, x1, thresh)
        ok &= (nsol == base["nsol"]) & (hb == base["hyp_best"]) & (_winner(counts, nsol) == win)
    return ok


def spread(fn, x0, x1, runs: int = 8):
    """The largest change of fn(x0, x1) (an array) over ``runs`` perturbed inputs."""
    ref = np.asarray(fn(x0, x1), dtype=np.float64)
    worst = 0.0
    for k in range(runs):
        worst = max(worst, float(np.abs(np.asarray(fn(*perturbed(x0, x1, k)), dtype=np.float64) - ref).max()))
    return worst


def residuals(cand, nsol, x0, x1, samples):
    """[H,10,3]: per candidate the largest |x1^T E x0| over its five sample points, |det E| and max |2 E E^T E - tr(E E^T) E|
    (E has unit Frobenius norm, so the three are relative); 0 for unused slots and refused rows."""
    H, N = cand.shape[0], np.asarray(x0).shape[0]
    E = cand.reshape(H, 10, 3, 3)
    ok = ((samples >= 0) & (samples < N)).all(axis=1)
    idx = np.where(ok[:, None], samples, 0)
    h0 = np.concatenate([np.asarray(x0)[idx], np.ones((H, 5, 1))], axis=2)
    h1 = np.concatenate([np.asarray(x1)[idx], np.ones((H, 5, 1))], axis=2)
    with np.errstate(all="ignore"):
        epi = np.abs(np.einsum("hpr,hcrs,hps->hcp", h1, E, h0)).max(axis=2)
        det = np.abs(np.linalg.det(E))
        EEt = E @ np.swapaxes(E, 2, 3)
        tr = np.abs(2 * EEt @ E - np.trace(EEt, axis1=2, axis2=3)[:, :, None, None] * E).reshape(H, 10, 9).max(axis=2)
    out = np.stack([epi, det, tr], axis=2)
    out[np.arange(10)[None, :] >= np.asarray(nsol)[:, None]] = 0.0
    return np.where(np.isfinite(out), out, np.inf)


def winner_spread(x0, x1, row, c, fn=lambda E, a, b: E):
    """The spread of fn(candidate c of the sample ``row``, x0, x1) over the 8 perturbed runs: how far the restatement's own result
    moves when its input moves by 2^-40, the yardstick for "equal up to conditioning"."""
    def one(a, b):
        cand, nsol = solve(a, b, np.asarray(row)[None])
        assert nsol[0] > c, "the candidate vanished under the perturbation: the hypothesis is not decided"
        return fn(cand[0, c], a, b)
    return spread(one, x0, x1)


def pose_of(E, x0, x1, thresh):
    """R (9) and t (3) of recover_pose on E's own inliers, as one vector."""
    with np.errstate(invalid="ignore"):
        inl = sampson(E, x0, x1) < thresh * thresh
    _, R, t, _ = recover_pose(E, x0, x1, inl)
    return np.concatenate([R.reshape(9), t])
