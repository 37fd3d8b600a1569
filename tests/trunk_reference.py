"""Plain-torch restatement of the encoder's front half as the C ABI runs it (include/car_trunk.h, csrc/car_trunk.hip): the weight
standardisation, the 7x7 stem, GroupNorm with residual and ReLU, the SAME max-pool, the SAME 3x3 convolution, the stride-2 pixel copy, the
bottleneck blocks, the trunk and the token rows — from raw weights, on channel-last rows [n][H W][C], in float64 (the reference) or float32
(the yardstick of parity_rule.judge).  Every stage returns its value and the bound that goes with it: the summed magnitudes of its last
contraction; for GroupNorm the magnitude of the normalised value times |gamma| plus |beta| (+ |add|).  Test infrastructure: no GPU, no
ctypes, nothing of encoder.py (tests/test_trunk_reference.py holds this file to encoder.py's own modules)."""
from __future__ import annotations

import functools
import math

import torch

F32, F64 = torch.float32, torch.float64
GROUPS, GN_EPS, STEM_EPS, STAGE_EPS = 32, 1e-5, 1e-6, 1e-8
STAGE_OUT = (256, 512, 1024)
TOK_DIM, TOK_IN = 768, 1024


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- TF "SAME" ----------------------------------------------------------------------------------------------------------------------------
def same_out(i, s):
    return -(-i // s)


def same_pad(i, k, s):
    """(front, behind): total max((ceil(i / s) - 1) s + k - i, 0), the odd pixel behind."""
    total = max((same_out(i, s) - 1) * s + k - i, 0)
    return total // 2, total - total // 2


# ---- weight standardisation ------------------------------------------------------------------------------------------------------------
def weight_standardize(w, eps, dtype=F64):
    """(w - mean) / sqrt(var + eps) per output channel, biased variance; returns (value, bound) in w's shape."""
    flat = w.to(dtype).reshape(w.shape[0], -1)
    mean = flat.mean(dim=1, keepdim=True)
    var = ((flat - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return ((flat - mean) * rstd).reshape(w.shape), ((flat.abs() + mean.abs()) * rstd).double().reshape(w.shape)


# ---- convolutions over channel-last rows ---------------------------------------------------------------------------------------------------
def _conv(x_nchw, w, stride, fill=0.0):
    """The k x k convolution with SAME padding, tap by tap: out[n][oy][ox][o] = sum_taps sum_c x[n][c][oy s + ky - pt][ox s + kx - pl] w[o][c][ky][kx]."""
    n, C, H, W = x_nchw.shape
    k = w.shape[-1]
    (pt, pb), (pl, pr) = same_pad(H, k, stride), same_pad(W, k, stride)
    Ho, Wo = same_out(H, stride), same_out(W, stride)
    xp = torch.full((n, C, H + pt + pb, W + pl + pr), fill, dtype=x_nchw.dtype)
    xp[:, :, pt:pt + H, pl:pl + W] = x_nchw
    out = torch.zeros(n, Ho, Wo, w.shape[0], dtype=x_nchw.dtype)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += torch.einsum("nchw,oc->nhwo", xs, w[:, :, ky, kx])
    return out


def conv_same(x_cl, H, W, w, stride, dtype=F64):
    """x_cl [n][H W][K] channel-last, w [N][K][k][k] (already standardised) -> ([n][Ho Wo][N], bound)."""
    n, _, K = x_cl.shape
    x = x_cl.reshape(n, H, W, K).permute(0, 3, 1, 2)
    y = _conv(x.to(dtype), w.to(dtype), stride)
    b = _conv(x.double().abs(), w.double().abs(), stride)
    return y.reshape(n, -1, w.shape[0]), b.reshape(n, -1, w.shape[0])


def stem(x_nchw, w_std, dtype=F64):
    """x [n][3][H][W], w_std [64][3][7][7] -> ([n][Ho Wo][64], bound); stride 2."""
    y = _conv(x_nchw.to(dtype), w_std.to(dtype), 2)
    b = _conv(x_nchw.double().abs(), w_std.double().abs(), 2)
    return y.reshape(y.shape[0], -1, 64), b.reshape(b.shape[0], -1, 64)


def linear(x, w, dtype=F64, bias=None):
    """x [..., K], w [N][K] -> (x w^T (+ bias), bound)."""
    y, b = x.to(dtype) @ w.to(dtype).T, x.double().abs() @ w.double().abs().T
    if bias is not None:
        y, b = y + bias.to(dtype), b + bias.double().abs()
    return y, b


def pixels_stride2(x_cl, H, W):
    n, _, C = x_cl.shape
    return x_cl.reshape(n, H, W, C)[:, ::2, ::2].reshape(n, -1, C)


def maxpool(x_cl, H, W):
    """3x3, stride 2, SAME with -inf; a NaN in the window gives NaN (torch.maximum propagates it)."""
    n, _, C = x_cl.shape
    (pt, pb), (pl, pr) = same_pad(H, 3, 2), same_pad(W, 3, 2)
    Ho, Wo = same_out(H, 2), same_out(W, 2)
    xp = torch.full((n, H + pt + pb, W + pl + pr, C), -float("inf"), dtype=x_cl.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x_cl.reshape(n, H, W, C)
    out = torch.full((n, Ho, Wo, C), -float("inf"), dtype=x_cl.dtype)
    for ky in range(3):
        for kx in range(3):
            out = torch.maximum(out, xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2])
    return out.reshape(n, -1, C)


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------------------
def groupnorm(x_cl, groups, gamma, beta, eps=GN_EPS, add=None, relu=False, dtype=F64):
    """x_cl [n][HW][C]; statistics per (image, group) over HW C / groups values, biased variance -> (act(gn(x) gamma + beta (+ add)), bound)."""
    n, HW, C = x_cl.shape
    x = x_cl.to(dtype).reshape(n, HW, groups, C // groups)
    mean = x.mean(dim=(1, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    norm = ((x - mean) / torch.sqrt(var + eps)).reshape(n, HW, C)
    y = norm * gamma.to(dtype) + beta.to(dtype)
    b = norm.double().abs() * gamma.double().abs() + beta.double().abs()
    if add is not None:
        y, b = y + add.to(dtype), b + add.double().abs()
    return (torch.relu(y) if relu else y), b


# ---- the trunk -----------------------------------------------------------------------------------------------------------------------------
def block_shapes(depths):
    """[(cin, mid, cout, stride, project)] of every block, in order."""
    out, cin = [], 64
    for s, d in enumerate(depths):
        for i in range(d):
            out.append((cin, STAGE_OUT[s] // 4, STAGE_OUT[s], 2 if (i == 0 and s > 0) else 1, i == 0))
            cin = STAGE_OUT[s]
    return out


def trunk_shapes(depths):
    """The parameters' shapes in state_dict order of ResNetV2Trunk with these depths."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    for cin, mid, cout, _, project in block_shapes(depths):
        if project:
            shapes += [(cout, cin, 1, 1), (cout,), (cout,)]
        shapes += [(mid, cin, 1, 1), (mid,), (mid,), (mid, mid, 3, 3), (mid,), (mid,), (cout, mid, 1, 1), (cout,), (cout,)]
    return shapes


@functools.lru_cache(maxsize=None)
def seeded_trunk(depths, seed=11):
    """Raw weights ~ N(0, 1) + 0.3 (standardisation removes mean and scale; the offset makes a missing one visible), GroupNorm scales
    1 + 0.2 N, biases 0.2 N."""
    g, out, scale_next = gen(seed), [], False
    for shp in trunk_shapes(depths):                                    # behind every convolution: its norm's weight, then its bias
        t = torch.randn(shp, generator=g)
        out.append(t + 0.3 if len(shp) == 4 else (1.0 + 0.2 * t if scale_next else 0.2 * t))
        scale_next = len(shp) == 4
    return tuple(out)


def bottleneck(x, h, w, p, shape, dtype=F64):
    """One block over x [n][h w][cin]; p: its 9 or 12 raw parameters -> (value, bound, ho, wo)."""
    cin, mid, cout, stride, project = shape
    p = list(p)
    ho, wo = same_out(h, stride), same_out(w, stride)
    std = lambda t: weight_standardize(t, STAGE_EPS, dtype)[0]
    shortcut = x.to(dtype)
    if project:
        dw, dg, db = p[:3]
        p = p[3:]
        src = pixels_stride2(x, h, w) if stride == 2 else x
        sc, _ = linear(src, std(dw).reshape(cout, cin), dtype)
        shortcut, _ = groupnorm(sc, GROUPS, dg, db, dtype=dtype)
    w1, g1, b1, w2, g2, b2, w3, g3, b3 = p
    a, _ = linear(x, std(w1).reshape(mid, cin), dtype)
    a, _ = groupnorm(a, GROUPS, g1, b1, relu=True, dtype=dtype)
    a, _ = conv_same(a, h, w, std(w2), stride, dtype)
    a, _ = groupnorm(a, GROUPS, g2, b2, relu=True, dtype=dtype)
    a, _ = linear(a, std(w3).reshape(cout, mid), dtype)
    y, bound = groupnorm(a, GROUPS, g3, b3, add=shortcut, relu=True, dtype=dtype)
    return y, bound, ho, wo


def trunk(x_nchw, params, depths, dtype=F64):
    """-> [(value, bound)] of the three stage ends, [n][h w][C] each."""
    params = list(params)
    n, _, H, W = x_nchw.shape
    y, _ = stem(x_nchw, weight_standardize(params[0], STEM_EPS, dtype)[0], dtype)
    h, w = same_out(H, 2), same_out(W, 2)
    y, _ = groupnorm(y, GROUPS, params[1], params[2], relu=True, dtype=dtype)
    y = maxpool(y, h, w)
    h, w = same_out(h, 2), same_out(w, 2)
    at, outs, shapes, blk = 3, [], block_shapes(depths), 0
    for d in depths:
        for _ in range(d):
            count = 12 if shapes[blk][4] else 9
            y, bound, h, w = bottleneck(y, h, w, params[at:at + count], shapes[blk], dtype)
            at += count
            blk += 1
        outs.append((y, bound))
    assert at == len(params)
    return outs


# ---- the token rows ------------------------------------------------------------------------------------------------------------------------
def resize_pos(pos_embed, grid, gh, gw, dtype=F64):
    """pos_embed [1 + grid grid][768] -> [1 + gh gw][768]: entry 0 kept, the grid entries bilinear with align_corners = False."""
    p = pos_embed.to(dtype)
    g = p[1:].reshape(grid, grid, -1)

    def axis(o, size):
        src = ((torch.arange(o, dtype=dtype) + 0.5) * (grid / size) - 0.5).clamp(min=0)
        i0 = src.floor().long().clamp(max=grid - 1)
        return i0, (i0 + 1).clamp(max=grid - 1), src - i0.to(dtype)
    y0, y1, ly = axis(gh, gh)
    x0, x1, lx = axis(gw, gw)
    ly, lx = ly[:, None, None], lx[None, :, None]
    top = (1 - lx) * g[y0][:, x0] + lx * g[y0][:, x1]
    bot = (1 - lx) * g[y1][:, x0] + lx * g[y1][:, x1]
    return torch.cat([p[:1], ((1 - ly) * top + ly * bot).reshape(gh * gw, -1)], dim=0)


def tokens(feat, pose16, proj_w, proj_b, cls, pos_embed, grid, pose_w, pose_b, gh, gw, dtype=F64):
    """feat [BV][gh gw][1024], pose16 [BV][16] -> (tok [BV][1 + gh gw][768], bound): row 0 = (cls + pos[0]) + pose; row 1 + p =
    ((proj + bias) + pos[1 + p]) + pose."""
    pos = resize_pos(pos_embed, grid, gh, gw, dtype)
    pose, pose_b_ = linear(pose16, pose_w, dtype, bias=pose_b)
    proj, proj_b_ = linear(feat, proj_w, dtype, bias=proj_b)
    BV = feat.shape[0]
    rows = torch.cat([cls.to(dtype).reshape(1, 1, -1).expand(BV, 1, -1), proj], dim=1)
    rows_b = torch.cat([cls.double().abs().reshape(1, 1, -1).expand(BV, 1, -1), proj_b_], dim=1)
    return (rows + pos[None]) + pose[:, None], rows_b + pos.double().abs()[None] + pose_b_[:, None]


@functools.lru_cache(maxsize=None)
def seeded_tokens(grid, seed=5):
    """proj_w, proj_b, cls, pos_embed, pose_w, pose_b."""
    g = gen(seed + grid)
    return (torch.randn(TOK_DIM, TOK_IN, generator=g) / math.sqrt(TOK_IN), 0.1 * torch.randn(TOK_DIM, generator=g), 0.2 * torch.randn(TOK_DIM, generator=g),
            0.2 * torch.randn(1 + grid * grid, TOK_DIM, generator=g), 0.25 * torch.randn(TOK_DIM, 16, generator=g), 0.1 * torch.randn(TOK_DIM, generator=g))
