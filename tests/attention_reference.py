"""One attention round and its backward, restated in plain torch float64 from the comments of
include/car_hip.h and the oracle's lines (oracle/car_oracle.py: ``ray_softmax``, a14-a16) — the checker of
tests/test_attention_hip.py.  No GPU, no project imports; tests/test_attention_reference.py checks this file itself.

Layout, as the C ABI has it: sample rows are ``[b*V, R, P]`` (scene-view, ray, step); a ray's softmax runs over its ``S = V * P`` samples
ordered view by view; per-ray results are ``[b, R]``.  ``inv_q`` is ``[b, 3, 4]``: floats 77:89 of the pose record of every scene's FIRST
view (cross_attention_renderer_amd/poses.py); only its last row is read.

Every result comes with the magnitude its rounding error scales with (the sum of the absolute values of the terms of the sum it is):
    Bz      = sum_s w_s |val_s|  (+ |zprev_scale zprev|)
    Bdepth  = sum_s w_s sum_k |m_k| |clamp(pt_sk)| + |m_3|                       m = inv_q[2, :]
    Ba_s    = sum_k |dz_k| |val_sk| + |ddepth| sum_k |m_k| |clamp(pt_sk)|
    Bl_s    = w_s (Ba_s + sum_t w_t Ba_t)
    L1_s    = sum_k |qa_sk| |qb_sk| / 16
"""
import torch

from parity_rule import gen  # noqa: F401

F64 = torch.float64
PT_CLAMP = 100.0
DEPTH_MAX = 10.0


def ray_major(x, b, V):
    """[b*V, R, P, ...] -> [b, R, V*P, ...]: a ray's samples side by side, view by view."""
    R, P = x.shape[1], x.shape[2]
    return x.reshape(b, V, R, P, *x.shape[3:]).transpose(1, 2).reshape(b, R, V * P, *x.shape[3:])


def view_major(x, b, V):
    """[b, R, V*P, ...] -> [b*V, R, P, ...] (the inverse of ray_major)."""
    R, P = x.shape[1], x.shape[2] // V
    return x.reshape(b, R, V, P, *x.shape[3:]).transpose(1, 2).reshape(b * V, R, P, *x.shape[3:])


def first_argmax(x):
    """argmax over the last dim, the LOWEST index on exact ties (torch.argmax does not promise which one it returns)."""
    n = x.shape[-1]
    idx = torch.arange(n).expand(x.shape)
    return torch.where(x == x.amax(dim=-1, keepdim=True), idx, torch.full_like(idx, n)).amin(dim=-1)


def _depth_terms(wr, pt, inv_q, b, V):
    """wr [b, R, S] -> pre-clamp depth zc [b, R], its magnitude bound, and per sample m[:3] . clamp(pt_s) and sum_k |m_k| |clamp(pt_sk)|."""
    m = inv_q.to(F64)[:, 2, :]                                                    # [b, 4]
    pc = ray_major(pt.to(F64), b, V).clamp(-PT_CLAMP, PT_CLAMP)                  # [b, R, S, 3]
    mp = (pc * m[:, None, None, :3]).sum(-1)                                      # [b, R, S]
    mp_abs = (pc.abs() * m[:, None, None, :3].abs()).sum(-1)
    zc = (wr * mp).sum(-1) + m[:, None, 3]
    bound = (wr * mp_abs).sum(-1) + m[:, None, 3].abs()
    return zc, bound, mp, mp_abs


def forward(logit, val, V, zprev=None, zprev_scale=0.0, reps=1, pt=None, inv_q=None):
    """car_attend.  ``logit``: [b*V, R, P], or a pair (qa, qb) of [b*V, R, P, dq] with logit = <qa, qb> / 16.  val [b*V, R, P, D].
    Returns a dict: w [b*V, R, P]; z [b, R, reps * D] = sum_s w_s val_s (+ zprev_scale zprev [b, R, D]), `reps` copies side by side; Bz;
    with pt [b*V, R, P, 3] and inv_q [b, 3, 4] also zc, depth = clamp(zc, 0, 10), Bdepth [b, R]; argmax [b*V, R] (per view, lowest index
    on ties); logit (fp64) and, for a pair, L1 [b*V, R, P]."""
    out = {}
    if isinstance(logit, (tuple, list)):
        qa, qb = (t.to(F64) for t in logit)
        out["L1"] = (qa.abs() * qb.abs()).sum(-1) / 16.0
        logit = (qa * qb).sum(-1) / 16.0
    logit = logit.to(F64)
    val = val.to(F64)
    bV, R, P = logit.shape
    b = bV // V
    lr = ray_major(logit, b, V)
    e = torch.exp(lr - lr.amax(dim=-1, keepdim=True))
    wr = e / e.sum(dim=-1, keepdim=True)                                          # [b, R, S]
    vr = ray_major(val, b, V)                                                     # [b, R, S, D]
    z = (wr[..., None] * vr).sum(dim=2)
    Bz = (wr[..., None] * vr.abs()).sum(dim=2)
    if zprev is not None:
        z = z + float(zprev_scale) * zprev.to(F64)
        Bz = Bz + (float(zprev_scale) * zprev.to(F64)).abs()
    w = view_major(wr, b, V)
    out.update(logit=logit, w=w, z=z.repeat(1, 1, reps), Bz=Bz.repeat(1, 1, reps), argmax=first_argmax(w))
    if pt is not None:
        zc, bound, _, _ = _depth_terms(wr, pt, inv_q, b, V)
        out.update(zc=zc, depth=zc.clamp(0.0, DEPTH_MAX), Bdepth=bound)
    return out


def _groups(x, tile_steps, fill):
    """[b*V, R, P, ...] -> [b*V, R, ceil(P / tile_steps), tile_steps, ...], the tail of the last group filled with `fill`."""
    P = x.shape[2]
    pgs = (P + tile_steps - 1) // tile_steps
    pad = pgs * tile_steps - P
    if pad:
        x = torch.cat([x, torch.full((*x.shape[:2], pad, *x.shape[3:]), fill, dtype=x.dtype)], dim=2)
    return x.reshape(*x.shape[:2], pgs, tile_steps, *x.shape[3:])


def parts(logit, val, tile_steps):
    """The input car_attend_parts expects: part [b*V, R, ceil(P / tile_steps), D] = sum_j exp(l_j - m_g) val_j over the steps j of group g of
    a view, m_g the group's largest logit; fp64 sums rounded once to fp32."""
    lg = _groups(logit.to(F64), tile_steps, float("-inf"))                        # [bV, R, pgs, T]
    vg = _groups(val.to(F64), tile_steps, 0.0)                                    # [bV, R, pgs, T, D]
    e = torch.exp(lg - lg.amax(dim=-1, keepdim=True))
    return (e[..., None] * vg).sum(dim=3).to(torch.float32)


def fold_parts(logit, part, V, tile_steps):
    """z [b, R, D] = sum_g exp(m_g - M) / L part_g  (M the ray's largest logit, L its softmax denominator) — the sum car_attend_parts runs."""
    logit = logit.to(F64)
    b = logit.shape[0] // V
    mg = _groups(logit, tile_steps, float("-inf")).amax(dim=-1)                   # [bV, R, pgs]
    lr = ray_major(logit, b, V)
    M = lr.amax(dim=-1, keepdim=True)                                             # [b, R, 1]
    L = torch.exp(lr - M).sum(dim=-1, keepdim=True)
    f = torch.exp(ray_major(mg, b, V) - M) / L                                    # [b, R, V*pgs]
    return (f[..., None] * ray_major(part.to(F64), b, V)).sum(dim=2)


def backward(w, val, dz, V, ddepth=None, pt=None, inv_q=None):
    """car_attend_backward in closed form, `w` [b*V, R, P] taken as given (the kernel's input):
        a_s = <dz, val_s> + ddepth [0 < zc < 10] m[:3] . clamp(pt_s),   dlogit_s = w_s (a_s - sum_t w_t a_t),   dval_s = w_s dz
    dz [b, R, D], ddepth [b, R].  Returns dlogit, Bl [b*V, R, P], dval [b*V, R, P, D], and zc when ddepth is given."""
    w, val, dz = w.to(F64), val.to(F64), dz.to(F64)
    b = w.shape[0] // V
    wr, vr = ray_major(w, b, V), ray_major(val, b, V)
    a = (vr * dz[:, :, None, :]).sum(-1)                                          # [b, R, S]
    Ba = (vr.abs() * dz[:, :, None, :].abs()).sum(-1)
    out = {}
    if ddepth is not None:
        zc, _, mp, mp_abs = _depth_terms(wr, pt, inv_q, b, V)
        dd = torch.where((zc > 0.0) & (zc < DEPTH_MAX), ddepth.to(F64), torch.zeros_like(zc))
        a = a + dd[..., None] * mp
        Ba = Ba + ddepth.to(F64).abs()[..., None] * mp_abs
        out["zc"] = zc
    t = (wr * a).sum(-1, keepdim=True)
    dl = wr * (a - t)
    Bl = wr * (Ba + (wr * Ba).sum(-1, keepdim=True))
    out.update(dlogit=view_major(dl, b, V), Bl=view_major(Bl, b, V), dval=view_major(wr[..., None] * dz[:, :, None, :], b, V))
    return out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
def make_logits(b, V, R, P, spread, seed):
    """fp32 logits [b*V, R, P] = spread * N(0, 1), with two kinds of planted rays (by ray index r, scene sc):
      (r + sc) % 3 == 0  "planted": in every view v one step gets the ray's largest logit + 1 + v / 2 — the view's argmax, by a margin of
                         at least (1 - 1 / e) of its weight;
      (r + sc) % 3 == 1  "tie" (P >= 2): in every view two steps get the SAME fp32 value, the ray's largest logit + 1.
    Returns logit, planted [b, R], tie [b, R] (bool), winner [b*V, R] (the step the argmax must name on planted / tie rays, else -1)."""
    g = gen(seed)
    logit = (torch.randn(b * V, R, P, generator=g) * spread).to(torch.float32)
    top = ray_major(logit, b, V).amax(dim=-1)                                     # [b, R]
    r_idx = torch.arange(R)[None, :] + torch.arange(b)[:, None]
    planted = (r_idx % 3) == 0
    tie = ((r_idx % 3) == 1) & (P >= 2)
    winner = torch.full((b * V, R), -1, dtype=torch.long)
    for sc in range(b):
        for v in range(V):
            n = sc * V + v
            for r in range(R):
                if planted[sc, r]:
                    p = int(torch.randint(P, (1,), generator=g))
                    logit[n, r, p] = top[sc, r] + 1.0 + 0.5 * v
                    winner[n, r] = p
                elif tie[sc, r]:
                    pq = torch.randperm(P, generator=g)[:2]
                    logit[n, r, pq] = top[sc, r] + 1.0
                    winner[n, r] = int(pq.min())
    return logit, planted, tie, winner


def one_hot_logits(b, V, R, P, seed, gap=1e3):
    """fp32 logits with one sample per ray `gap` above the ray's largest: the softmax is exactly one-hot in fp32 (and in fp64).
    Returns logit [b*V, R, P] and hot [b, R]: the winner's index among the ray's V*P samples."""
    g = gen(seed)
    logit = torch.randn(b * V, R, P, generator=g).to(torch.float32)
    lr = ray_major(logit, b, V).clone()
    hot = torch.randint(V * P, (b, R), generator=g)
    lr.scatter_(2, hot[..., None], lr.amax(dim=-1, keepdim=True) + gap)
    return view_major(lr, b, V).contiguous(), hot


def make_depth_inputs(w, b, V, seed, beyond=0.05):
    """pt [b*V, R, P, 3] and inv_q [b, 3, 4] (fp32) that PLANT the depth class of every ray for the weights `w` [b*V, R, P]:
    class (r + sc) % 3 = 0: pre-clamp zc below 0 (in [-5, -3]); 1: inside (0, 10) (in [2, 8]); 2: above 10 (in [12, 17]).
    pt = U(-1, 1) + shift_r m / |m|^2; a fraction `beyond` of the entries of ONE coordinate per scene (k = sc % 3, where |m_k| = 0.1, so that
    whatever the weights these entries move zc by at most 10) is then replaced by +-1e3, which the read-out clamps to +-100.  zc is linear in
    shift_r as long as the other entries stay inside +-100 (|shift| < 35, |m / |m|^2| < 1.8: they do), and shift_r is solved for the target.
    Returns pt, inv_q, cls [b, R]."""
    g = gen(seed)
    bV, R, P = w.shape
    inv_q = torch.randn(b, 3, 4, generator=g)
    far_axis = torch.arange(b) % 3
    split = 0.2 + 0.5 * torch.rand(b, generator=g)                                # the two other coordinates share 0.9: each at least 0.2
    mag = torch.stack([split, 0.9 - split], dim=1)
    m = torch.zeros(b, 4)
    for sc in range(b):
        others = [k for k in range(3) if k != int(far_axis[sc])]
        m[sc, int(far_axis[sc])] = 0.1
        m[sc, others[0]], m[sc, others[1]] = mag[sc, 0], mag[sc, 1]
    m[:, :3] *= torch.where(torch.rand(b, 3, generator=g) < 0.5, -1.0, 1.0)
    m[:, 3] = torch.rand(b, generator=g) * 4 - 2
    inv_q[:, 2, :] = m
    m = inv_q[:, 2, :].to(F64)
    base = ray_major(torch.rand(bV, R, P, 3, generator=g) * 2 - 1, b, V).to(F64)  # [b, R, S, 3]
    far = ray_major(torch.rand(bV, R, P, 3, generator=g) < beyond, b, V)
    far[:, torch.arange(0, R, 2), torch.arange(0, R, 2) % (V * P), :] = True      # and sample r % S of every second ray, whatever `beyond`
    far = far & (torch.arange(3)[None, :] == far_axis[:, None])[:, None, None, :]
    sign = ray_major(torch.where(torch.rand(bV, R, P, 3, generator=g) < 0.5, -1.0, 1.0), b, V).to(F64)
    u = torch.rand(b, R, generator=g).to(F64)
    cls = (torch.arange(R)[None, :] + torch.arange(b)[:, None]) % 3
    target = torch.where(cls == 0, -5.0 + 2.0 * u, torch.where(cls == 1, 2.0 + 6.0 * u, 12.0 + 5.0 * u))
    wr = ray_major(w.to(F64), b, V)
    m3 = m[:, None, None, :3]
    direction = m3 / (m3 ** 2).sum(-1, keepdim=True)                             # m . direction = 1
    near = (~far).to(F64)
    A = (wr[..., None] * m3 * (near * base + (1 - near) * sign * PT_CLAMP)).sum((-1, -2)) + m[:, None, 3]
    B = (wr[..., None] * m3 * near * direction).sum((-1, -2))
    shift = (target - A) / B
    pt = torch.where(far, sign * 1e3, base + shift[..., None, None] * direction)
    return view_major(pt, b, V).to(torch.float32).contiguous(), inv_q, cls


def make_dot_inputs(b, V, R, P, dq, seed, l1_max=8.0):
    """qa, qb [b*V, R, P, dq] fp32, scaled so that the largest L1_s = sum_k |qa||qb| / 16 is just below l1_max."""
    g = gen(seed)
    qa = torch.randn(b * V, R, P, dq, generator=g)
    qb = torch.randn(b * V, R, P, dq, generator=g)
    l1 = (qa.double().abs() * qb.double().abs()).sum(-1).max().item() / 16.0
    s = (0.98 * l1_max / l1) ** 0.5
    return (qa * s).to(torch.float32).contiguous(), (qb * s).to(torch.float32).contiguous()
