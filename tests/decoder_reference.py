"""Plain-torch restatement of the encoder's back half as the C ABI runs it (include/car_decoder.h, csrc/car_decoder.hip): the 3x3 convolution
with a padding of 1 and its epilogue, the bilinear 2x upsampling with align_corners = True, the read-out in its split form, conv_map's 7x7
convolution, the image normalisation, the residual unit, the fusion block and the decoder — from raw weights, on channel-last rows
[n][H W][C], in float64 (the reference) or float32 (the yardstick of parity_rule.judge).  Every stage returns its value and the bound that
goes with it: the float64 sum of the magnitudes of the terms of its last contraction and of what is added to it.  Test infrastructure: no
GPU, no ctypes, nothing of encoder.py (tests/test_decoder_reference.py holds this file to encoder.py's own modules)."""
from __future__ import annotations

import functools
import math

import torch

F32, F64 = torch.float32, torch.float64
DIM, FUSE = 768, 256
RN_IN = (256, 512, 768, 768)
RELU_IN, RELU_OUT, ACCUM = 1, 2, 4                   # CAR_LIN_RELU_IN, CAR_LIN_RELU_OUT, CAR_LIN_ACCUM
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def pad1_out(i, s):
    return (i - 1) // s + 1


# ---- convolutions over channel-last rows ---------------------------------------------------------------------------------------------------
def _conv(x_nchw, w, stride, pad):
    """The k x k convolution with a symmetric zero padding, tap by tap."""
    n, C, H, W = x_nchw.shape
    k = w.shape[-1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = torch.zeros(n, C, H + 2 * pad, W + 2 * pad, dtype=x_nchw.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x_nchw
    out = torch.zeros(n, Ho, Wo, w.shape[0], dtype=x_nchw.dtype)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += torch.einsum("nchw,oc->nhwo", xs, w[:, :, ky, kx])
    return out


def conv3x3_pad1(x_cl, H, W, w, stride=1, bias=None, add=None, flags=0, y=None, dtype=F64):
    """x_cl [n][H W][K], w [N][K][3][3] -> (act_out((conv(act_in(x)) + bias) + add) (+ y) as [n][Ho Wo][N], bound)."""
    n, _, K = x_cl.shape
    x = x_cl.reshape(n, H, W, K).permute(0, 3, 1, 2)
    if flags & RELU_IN:
        x = torch.relu(x)
    N = w.shape[0]
    v = _conv(x.to(dtype), w.to(dtype), stride, 1).reshape(n, -1, N)
    b = _conv(x.double().abs(), w.double().abs(), stride, 1).reshape(n, -1, N)
    if bias is not None:
        v, b = v + bias.to(dtype), b + bias.double().abs()
    if add is not None:
        v, b = v + add.to(dtype), b + add.double().abs()
    if flags & RELU_OUT:
        v = torch.relu(v)
    if flags & ACCUM:
        v, b = v + y.to(dtype), b + y.double().abs()
    return v, b


def conv7x7(x_nchw, w, bias, dtype=F64):
    """conv_map: x [n][3][H][W], w [64][3][7][7], bias [64] -> ([n][H W][64], bound); stride 1, padding 3."""
    v = _conv(x_nchw.to(dtype), w.to(dtype), 1, 3) + bias.to(dtype)
    b = _conv(x_nchw.double().abs(), w.double().abs(), 1, 3) + bias.double().abs()
    return v.reshape(v.shape[0], -1, 64), b.reshape(b.shape[0], -1, 64)


# ---- bilinear 2x upsampling, align_corners = True -----------------------------------------------------------------------------------------------
def _axis(E, dtype):
    """Output o of an extent E reads o (E - 1) / (2 E - 1): (i0, i1, fraction), the coordinate taken exactly in integers."""
    o = torch.arange(2 * E)
    num, den = o * (E - 1), 2 * E - 1
    i0 = num // den
    return i0, (i0 + 1).clamp(max=E - 1), ((num % den).to(F64) / den).to(dtype)


def upsample2x(x_cl, H, W, dtype=F64):
    """x_cl [n][H W][C] -> ([n][2H 2W][C], bound): top = v00 + lx (v01 - v00), bot likewise, out = top + ly (bot - top)."""
    n, _, C = x_cl.shape
    x = x_cl.reshape(n, H, W, C)
    y0, y1, ly = _axis(H, dtype)
    x0, x1, lx = _axis(W, dtype)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]

    def mix(v, lx_, ly_, sign):
        v00, v01, v10, v11 = v[:, y0][:, :, x0], v[:, y0][:, :, x1], v[:, y1][:, :, x0], v[:, y1][:, :, x1]
        top = v00 + lx_ * (v01 + sign * v00)
        bot = v10 + lx_ * (v11 + sign * v10)
        return top + ly_ * (bot + sign * top)
    out = mix(x.to(dtype), lx, ly, -1.0)
    bound = mix(x.double().abs(), lx.double(), ly.double(), 1.0)
    return out.reshape(n, -1, C), bound.reshape(n, -1, C)


# ---- the read-out, split: gelu(Wa t[1 + p] + (Wb t[0] + b)) ----------------------------------------------------------------------------------------
def gelu(x):
    return x * torch.special.erfc(-x / math.sqrt(2.0)) / 2


def readout(tok, w, bias, dtype=F64):
    """tok [BV][1 + P][dim], w [dim][2 dim], bias [dim] -> ([BV][P][dim], bound of the GELU's argument, the argument)."""
    dim = tok.shape[-1]
    t, wa, wb = tok.to(dtype), w[:, :dim].to(dtype), w[:, dim:].to(dtype)
    r = t[:, 0] @ wb.T + bias.to(dtype)
    arg = t[:, 1:] @ wa.T + r[:, None]
    ta = tok.double().abs()
    bound = ta[:, 1:] @ w[:, :dim].double().abs().T + (ta[:, 0] @ w[:, dim:].double().abs().T + bias.double().abs())[:, None]
    return gelu(arg), bound, arg


def linear(x, w, bias, dtype=F64):
    y = x.to(dtype) @ w.to(dtype).T + bias.to(dtype)
    return y, x.double().abs() @ w.double().abs().T + bias.double().abs()


# ---- the image normalisation ------------------------------------------------------------------------------------------------------------------
def normalize(rgb_cl, dtype=F32):
    """rgb [n][H][W][3] -> [n][3][H][W]: ((v + 1) / 2 - mean) / std, one rounding per operation, the constants rounded to dtype."""
    x = rgb_cl.to(dtype).permute(0, 3, 1, 2)
    mean, std = torch.tensor(MEAN, dtype=dtype)[None, :, None, None], torch.tensor(STD, dtype=dtype)[None, :, None, None]
    return (((x + 1) / 2.0 - mean) / std).contiguous()


# ---- the fusion ---------------------------------------------------------------------------------------------------------------------------------
def rcu(x, h, w, p, dtype=F64):
    """ResidualConvUnit: conv2(relu(conv1(relu(x)))) + x; p = (w1, b1, w2, b2) -> (value, bound)."""
    w1, b1, w2, b2 = p
    mid, _ = conv3x3_pad1(x, h, w, w1, bias=b1, flags=RELU_IN, dtype=dtype)
    return conv3x3_pad1(mid, h, w, w2, bias=b2, add=x, flags=RELU_IN, dtype=dtype)


def fusion(x, h, w, p, skip=None, dtype=F64):
    """FeatureFusionBlock: p = (out_w, out_b, [rcu1 x 4,] rcu2 x 4) -> (value [n][2h 2w][256], bound)."""
    p = list(p)
    out_w, out_b = p[:2]
    x = x.to(dtype)
    if skip is not None:
        s, _ = rcu(skip, h, w, p[2:6], dtype)
        x = x + s
        p = p[:2] + p[6:]
    x, _ = rcu(x, h, w, p[2:6], dtype)
    x, _ = upsample2x(x, h, w, dtype)
    return linear(x, out_w.reshape(FUSE, FUSE), out_b, dtype)


def decoder_shapes():
    """The 50 parameters' shapes, in car_decoder_pack's order."""
    ro = [(DIM, 2 * DIM), (DIM,), (DIM, DIM, 1, 1), (DIM,)]
    shapes = ro + ro + [(DIM, DIM, 3, 3), (DIM,)] + [(FUSE, c, 3, 3) for c in RN_IN]
    conv = [(FUSE, FUSE, 3, 3), (FUSE,)]
    for i in range(4):
        shapes += [(FUSE, FUSE, 1, 1), (FUSE,)] + conv * (4 if i < 3 else 2)
    return shapes


@functools.lru_cache(maxsize=None)
def seeded_decoder(seed=23):
    """Weights ~ N(0, 1) / sqrt(fan_in), biases 0.1 N."""
    g, out = gen(seed), []
    for shp in decoder_shapes():
        t = torch.randn(shp, generator=g)
        out.append(0.1 * t if len(shp) == 1 else t / math.sqrt(t[0].numel()))
    assert len(out) == 50
    return tuple(out)


def decoder(tap3, tap4, layer1, layer2, gh, gw, params, dtype=F64):
    """tap3, tap4 [BV][1 + gh gw][768], layer1 [BV][4gh 4gw][256], layer2 [BV][2gh 2gw][512] -> [(path_2, bound), (path_1, bound)]."""
    p = list(params)
    BV = tap3.shape[0]
    l3, _ = linear(readout(tap3, p[0], p[1], dtype)[0], p[2].reshape(DIM, DIM), p[3], dtype)
    l4, _ = linear(readout(tap4, p[4], p[5], dtype)[0], p[6].reshape(DIM, DIM), p[7], dtype)
    l4, _ = conv3x3_pad1(l4, gh, gw, p[8], stride=2, bias=p[9], dtype=dtype)
    rn = p[10:14]
    refine = [p[14:24], p[24:34], p[34:44], p[44:50]]
    levels = [layer1, layer2, l3, l4]
    h, w = gh // 2, gw // 2
    path, outs = None, {}
    for i in (3, 2, 1, 0):
        m, _ = conv3x3_pad1(levels[i], h, w, rn[i], dtype=dtype)
        path, bound = fusion(m, h, w, refine[i], dtype=dtype) if i == 3 else fusion(path, h, w, refine[i], skip=m, dtype=dtype)
        h, w = 2 * h, 2 * w
        outs[i] = (path, bound)
    assert path.shape == (BV, 64 * gh * gw, FUSE)
    return [outs[1], outs[0]]
