"""SuperPoint and SuperGlue restated from their raw state dicts (estimate_pose/superpoint.py:47-202, superglue.py:51-285), stage by
stage, in the precision the caller names: float64 is the truth of the GPU suite, float32 its yardstick (parity_rule).  The reference's own module cannot run in float64
(superpoint.py:187 casts the keypoints with .float()), so the float64 truth is this file; tests/test_matcher_reference.py holds it to
the reference's float32 outputs in tests/golden/matcher_expected.npz.  Channel-last throughout, like the library.

The bounds are float64 sums of magnitudes.  For a convolution that is m = |W| |a| + |b| on the layer's actual input a: the scale of the
terms that met in the value (what the layers in front amplify is the yardstick's business: the float32 run goes through the same
chain).  Behind a non-linearity the bound is carried to first order: softmax p_c (1 + max_j m_j), a normalised vector
(m_c + |d_c| |m|) / |x|."""
import math

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
BACKBONE = ("conv1a", "conv1b", "pool", "conv2a", "conv2b", "pool", "conv3a", "conv3b", "pool", "conv4a", "conv4b")


def _conv(state, name, x, dtype, relu, mag=False):
    w, b = state[name + ".weight"].to(dtype), state[name + ".bias"].to(dtype)
    if mag:
        w, b = w.abs(), b.abs()
    y = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
    return F.relu(y) if relu and not mag else y


def conv1a(state, gray, dtype=F64):
    """relu(conv1a(gray)) as [n, H, W, 64], and its bound |W| |x| + |b|."""
    x = gray.to(dtype)[:, None]
    y = _conv(state, "conv1a", x, dtype, True)
    m = _conv(state, "conv1a", x.abs().double(), F64, False, mag=True)
    return y.permute(0, 2, 3, 1).contiguous(), m.permute(0, 2, 3, 1).contiguous()


def dense(state, gray, dtype=F64):
    """gray [n, H, W] -> dict of channel-last tensors: logits [n, h, w, 65], raw [n, h, w, 256] (convDb's output), scores [n, H, W]
    (before the suppression), desc [n, h, w, 256] (normalised), and `bound_*` for each in float64."""
    out = {}
    x = gray.to(dtype)[:, None]
    for step in BACKBONE:
        x = F.max_pool2d(x, 2, 2) if step == "pool" else _conv(state, step, x, dtype, True)
    for head, last, what in (("convPa", "convPb", "logits"), ("convDa", "convDb", "raw")):
        a = _conv(state, head, x, dtype, True)
        out[what] = _conv(state, last, a, dtype, False).permute(0, 2, 3, 1).contiguous()
        out["bound_" + what] = _conv(state, last, a.double(), F64, False, mag=True).permute(0, 2, 3, 1).contiguous()
    n, h, w, _ = out["logits"].shape
    p = torch.softmax(out["logits"], -1)[..., :64]
    spread = lambda t: t.reshape(n, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(n, h * 8, w * 8)
    out["scores"] = spread(p)
    out["bound_scores"] = spread(p.double() * (1 + out["bound_logits"].max(-1, keepdim=True).values))
    out["desc"], out["bound_desc"] = normalise(out["raw"], out["bound_raw"])
    return out


def normalise(x, m):
    """x / max(|x|, 1e-12) over the last dimension, and the first-order bound (m_c + |d_c| |m|) / |x| (an all-zero row: m itself)."""
    nrm = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    d = x / nrm
    big = nrm.double() > 1e-12
    bound = torch.where(big, (m + d.double().abs() * m.norm(dim=-1, keepdim=True)) / nrm.double(), m)
    return d, bound


def nms(scores, radius: int):
    """simple_nms on [..., H, W]: comparisons only, so every precision gives the input's own values back."""
    def pooled(x):
        H, W = x.shape[-2:]
        p = F.pad(x, (radius, radius, radius, radius), value=-math.inf)
        m = torch.full_like(x, -math.inf)
        for dy in range(2 * radius + 1):
            for dx in range(2 * radius + 1):
                m = torch.maximum(m, p[..., dy:dy + H, dx:dx + W])
        return m
    zeros = torch.zeros_like(scores)
    keep = scores == pooled(scores)
    for _ in range(2):
        supp = pooled(keep.to(scores.dtype)) > 0
        rest = torch.where(supp, zeros, scores)
        keep = keep | ((rest == pooled(rest)) & ~supp)
    return torch.where(keep, scores, zeros)


def select(nms_map, threshold: float, border: int, max_keypoints: int):
    """One map [H, W] -> keypoints [N, 2] (x, y) float32 and their scores: score > threshold, at least `border` from every edge, the
    max_keypoints largest when more survive; row-major when nothing is cut, else descending score.  Equal scores: the lower
    row-major index first (the library's stated choice; the reference leaves it to torch.topk)."""
    H, W = nms_map.shape
    ys, xs = torch.nonzero(nms_map > threshold, as_tuple=True)
    ok = (ys >= border) & (ys < H - border) & (xs >= border) & (xs < W - border)
    ys, xs = ys[ok], xs[ok]
    s = nms_map[ys, xs]
    if len(s) > max_keypoints:
        order = torch.sort(s, descending=True, stable=True).indices[:max_keypoints]     # stable: ties keep their row-major order
        ys, xs, s = ys[order], xs[order], s[order]
    return torch.stack([xs, ys], -1).to(F32), s


def sample(kpts, desc, bound_desc, dtype=F64):
    """sample_descriptors on one image: kpts [N, 2] (x, y), desc [h, w, 256] -> [N, 256] and its bound.  The coordinate arithmetic runs
    in `dtype` as the reference's runs in float32."""
    h, w, _ = desc.shape
    k = kpts.to(dtype)
    g = (k - 4 + 0.5) / torch.tensor([w * 8 - 4 - 0.5, h * 8 - 4 - 0.5], dtype=dtype) * 2 - 1
    ix, iy = (g[:, 0] + 1) / 2 * (w - 1), (g[:, 1] + 1) / 2 * (h - 1)
    x0, y0 = ix.floor(), iy.floor()
    acc = torch.zeros(len(k), desc.shape[-1], dtype=dtype)
    mag = torch.zeros(len(k), desc.shape[-1], dtype=F64)
    for dy in (0, 1):
        for dx in (0, 1):
            wt = ((x0 + 1 - ix) if dx == 0 else (ix - x0)) * ((y0 + 1 - iy) if dy == 0 else (iy - y0))
            xx, yy = (x0 + dx).long(), (y0 + dy).long()
            inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            xi, yi = xx.clamp(0, w - 1), yy.clamp(0, h - 1)
            wt = torch.where(inside, wt, torch.zeros_like(wt))[:, None]
            acc = acc + wt * desc[yi, xi].to(dtype)
            mag = mag + wt.double().abs() * (bound_desc[yi, xi] + desc[yi, xi].double().abs())
    return normalise(acc, mag)


def superpoint(state, gray, nms_radius=4, keypoint_threshold=0.005, max_keypoints=1024, remove_borders=4, dtype=F64):
    """The whole forward on gray [n, H, W]: per image keypoints [N, 2], scores [N], descriptors [N, 256]; and the dense stage's dict."""
    d = dense(state, gray, dtype)
    kept = nms(d["scores"], nms_radius)
    res = []
    for i in range(len(gray)):
        k, s = select(kept[i], keypoint_threshold, remove_borders, max_keypoints)
        desc, bound = sample(k, d["desc"][i], d["bound_desc"][i], dtype)
        res.append(dict(keypoints=k, scores=s, descriptors=desc, bound_descriptors=bound))
    return res, d


# ---- SuperGlue (estimate_pose/superglue.py:51-285), rows channel-last: a descriptor set is [N, 256] ----------------------------------
KENC = (0, 3, 6, 9, 12)                               # the convolutions of kenc.encoder; a BatchNorm1d behind each of the first four


def _lin(state, name, x, dtype, mag=False):
    W, b = state[name + ".weight"].to(dtype)[:, :, 0], state[name + ".bias"].to(dtype)
    return x.abs() @ W.abs().T + b.abs() if mag else x @ W.T + b


def _bn(state, name, x, dtype):
    g, b, mean, var = (state[f"{name}.{k}"].to(dtype) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - mean) / torch.sqrt(var + 1e-5) * g + b


def encode_keypoints(state, kpts, scores, shape, dtype=F64):
    """normalize_keypoints (centre (W / 2, H / 2), scale 0.7 max(W, H)) and the keypoint encoder on [x, y, score]: [N, 256]."""
    H, W = shape
    size = torch.tensor([W, H], dtype=dtype)
    x = torch.cat([(kpts.to(dtype) - size / 2) / (size.max() * 0.7), scores.to(dtype)[:, None]], 1)
    for i, idx in enumerate(KENC):
        x = _lin(state, f"kenc.encoder.{idx}", x, dtype)
        if i < 4:
            x = F.relu(_bn(state, f"kenc.encoder.{idx + 1}", x, dtype))
    return x


def attention_heads(q, k, v):
    """softmax(q k^T / 8) v for four heads of 64 CONTIGUOUS channels (the device layout): q [N, 256], k, v [M, 256] -> [N, 256], and the
    bound sum_m p_m |v_m| (1 + max_m sum_d |q_d k_md| / 8) in float64."""
    N, M = len(q), len(k)
    qh, kh, vh = q.view(N, 4, 64), k.view(M, 4, 64), v.view(M, 4, 64)
    p = torch.softmax(torch.einsum("nhd,mhd->hnm", qh, kh) / 8, -1)
    out = torch.einsum("hnm,mhd->nhd", p, vh).reshape(N, 256)
    big = torch.einsum("nhd,mhd->hnm", qh.double().abs(), kh.double().abs()).max(-1).values / 8               # [h, n]
    bound = torch.einsum("hnm,mhd->nhd", p.double(), vh.double().abs()) * (1 + big.t()[:, :, None])
    return out, bound.reshape(N, 256)


def _propagate(state, pre, x, src, dtype):
    """AttentionalPropagation: the head split is view(b, 64, 4, n) — torch channel c belongs to head c % 4."""
    q, k, v = (_lin(state, f"{pre}.attn.proj.{j}", t, dtype) for j, t in enumerate((x, src, src)))
    N, M = len(q), len(k)
    p = torch.softmax(torch.einsum("ndh,mdh->hnm", q.view(N, 64, 4), k.view(M, 64, 4)) / 8, -1)
    msg = _lin(state, f"{pre}.attn.merge", torch.einsum("hnm,mdh->ndh", p, v.view(M, 64, 4)).reshape(N, 256), dtype)
    y = F.relu(_bn(state, f"{pre}.mlp.1", _lin(state, f"{pre}.mlp.0", torch.cat([x, msg], 1), dtype), dtype))
    return _lin(state, f"{pre}.mlp.3", y, dtype)


def match_descriptors(state, names, kpts0, scores0, desc0, shape0, kpts1, scores1, desc1, shape1, dtype=F64):
    """The descriptor network: mdesc0 [N0, 256], mdesc1 [N1, 256] and their bounds |W| |x| + |b| of final_proj."""
    d0 = desc0.to(dtype) + encode_keypoints(state, kpts0, scores0, shape0, dtype)
    d1 = desc1.to(dtype) + encode_keypoints(state, kpts1, scores1, shape1, dtype)
    for l, name in enumerate(names):
        s0, s1 = (d1, d0) if name == "cross" else (d0, d1)
        d0, d1 = d0 + _propagate(state, f"gnn.layers.{l}", d0, s0, dtype), d1 + _propagate(state, f"gnn.layers.{l}", d1, s1, dtype)
    return [(_lin(state, "final_proj", d, dtype), _lin(state, "final_proj", d.double(), F64, mag=True)) for d in (d0, d1)]


def transport(mdesc0, mdesc1, bin_score, iters, dtype=F64):
    """log_optimal_transport of mdesc0 mdesc1^T / 16: Z [(m + 1), (n + 1)] and the bound |Z| + 1 + the largest sum_d |a_d b_d| / 16
    of the entry's row and column: u_i and v_j carry the rounding of every coupling of their line into Z_ij (|bin_score| for the dustbin)."""
    a, b = mdesc0.to(dtype), mdesc1.to(dtype)
    m, n = len(a), len(b)
    S = a @ b.T / 16
    bin_ = torch.tensor(float(bin_score), dtype=dtype)
    Zc = torch.cat([torch.cat([S, bin_.expand(m, 1)], 1), bin_.expand(1, n + 1)], 0)
    norm = -torch.tensor(float(m + n), dtype=dtype).log()
    log_mu = torch.cat([norm.expand(m), torch.tensor(float(n), dtype=dtype).log()[None] + norm])
    log_nu = torch.cat([norm.expand(n), torch.tensor(float(m), dtype=dtype).log()[None] + norm])
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Zc + v[None, :], 1)
        v = log_nu - torch.logsumexp(Zc + u[:, None], 0)
    Z = Zc + u[:, None] + v[None, :] - norm
    mag = torch.full((m + 1, n + 1), abs(float(bin_score)), dtype=F64)
    mag[:m, :n] = a.double().abs() @ b.double().abs().T / 16
    return Z, Z.double().abs() + 1 + torch.maximum(mag.max(1, keepdim=True).values, mag.max(0, keepdim=True).values)


def matches(Z, match_threshold):
    """superglue.py:267-285 on one Z: matches0, matches1 (int64, -1 = none), matching_scores0, matching_scores1.  torch's max returns the
    first maximal index, so ties go to the lowest index."""
    inner = Z[:-1, :-1]
    max0, max1 = inner.max(1), inner.max(0)
    i0, i1 = max0.indices, max1.indices
    mutual0 = torch.arange(len(i0)) == i1[i0]
    mutual1 = torch.arange(len(i1)) == i0[i1]
    zero = Z.new_tensor(0)
    s0 = torch.where(mutual0, max0.values.exp(), zero)
    s1 = torch.where(mutual1, s0[i1], zero)
    valid0 = mutual0 & (s0 > match_threshold)
    valid1 = mutual1 & valid0[i1]
    return torch.where(valid0, i0, i0.new_tensor(-1)), torch.where(valid1, i1, i1.new_tensor(-1)), s0, s1


def head_major(c):
    """Device channel -> torch channel: head h = c // 64 owns the torch channels d * 4 + h."""
    return (c % 64) * 4 + c // 64


def folded(state, layers):
    """What car_superglue_pack computes, in float64: every BatchNorm folded into the convolution in front of it, the projections' rows and
    merge's columns permuted head-major.  A state dict of the same names without BatchNorm entries, for match_descriptors_folded."""
    out = {}
    perm = head_major(torch.arange(256))

    def conv(name, bn=None, rows=None, cols=None):
        W, b = state[name + ".weight"].double()[:, :, 0], state[name + ".bias"].double()
        if bn:
            s = state[bn + ".weight"].double() / torch.sqrt(state[bn + ".running_var"].double() + 1e-5)
            W, b = W * s[:, None], (b - state[bn + ".running_mean"].double()) * s + state[bn + ".bias"].double()
        if rows is not None:
            W, b = W[rows], b[rows]
        if cols is not None:
            W = W[:, cols]
        out[name + ".weight"], out[name + ".bias"] = W[:, :, None], b
    for i, idx in enumerate(KENC):
        conv(f"kenc.encoder.{idx}", f"kenc.encoder.{idx + 1}" if i < 4 else None)
    for l in range(layers):
        pre = f"gnn.layers.{l}"
        for j in range(3):
            conv(f"{pre}.attn.proj.{j}", rows=perm)
        conv(f"{pre}.attn.merge", cols=perm)
        conv(f"{pre}.mlp.0", f"{pre}.mlp.1")
        conv(f"{pre}.mlp.3")
    conv("final_proj")
    return out


def match_descriptors_folded(fold, names, kpts0, scores0, desc0, shape0, kpts1, scores1, desc1, shape1):
    """match_descriptors on folded(): no BatchNorm, heads contiguous (attention_heads) — the device's order of operations, in float64."""
    def enc(kpts, scores, shape):
        size = torch.tensor([shape[1], shape[0]], dtype=F64)
        x = torch.cat([(kpts.double() - size / 2) / (size.max() * 0.7), scores.double()[:, None]], 1)
        for i, idx in enumerate(KENC):
            x = _lin(fold, f"kenc.encoder.{idx}", x, F64)
            x = F.relu(x) if i < 4 else x
        return x

    def prop(pre, x, src):
        q, k, v = (_lin(fold, f"{pre}.attn.proj.{j}", t, F64) for j, t in enumerate((x, src, src)))
        msg = _lin(fold, f"{pre}.attn.merge", attention_heads(q, k, v)[0], F64)
        return _lin(fold, f"{pre}.mlp.3", F.relu(_lin(fold, f"{pre}.mlp.0", torch.cat([x, msg], 1), F64)), F64)
    d0, d1 = desc0.double() + enc(kpts0, scores0, shape0), desc1.double() + enc(kpts1, scores1, shape1)
    for l, name in enumerate(names):
        s0, s1 = (d1, d0) if name == "cross" else (d0, d1)
        d0, d1 = d0 + prop(f"gnn.layers.{l}", d0, s0), d1 + prop(f"gnn.layers.{l}", d1, s1)
    return _lin(fold, "final_proj", d0, F64), _lin(fold, "final_proj", d1, F64)


def decided(Z64, tol):
    """Which keypoints' matches a run within `tol` of Z64 must reproduce: the float64 gap between the best and the second-best entry of
    the row (over Z[:-1, :-1]), and of the column its arg-max points to, exceeds twice the tolerance there; likewise from the columns'
    side.  tol: a tensor like Z64 (or a number).  Returns (decided0 [m], decided1 [n])."""
    inner = Z64[:-1, :-1]
    t = (tol[:-1, :-1] if torch.is_tensor(tol) else torch.full_like(inner, float(tol)))

    def gaps(M, T):                                    # per row: best - second best (inf for a single entry), the arg-max, the largest tolerance
        top = M.topk(min(2, M.shape[1]), dim=1).values
        gap = top[:, 0] - top[:, 1] if M.shape[1] > 1 else torch.full_like(top[:, 0], float("inf"))
        return gap, M.argmax(1), T.max(1).values
    g0, i0, t0 = gaps(inner, t)
    g1, i1, t1 = gaps(inner.t(), t.t())
    ok0, ok1 = g0 > 2 * t0, g1 > 2 * t1
    return ok0 & ok1[i0], ok1 & ok0[i1]
