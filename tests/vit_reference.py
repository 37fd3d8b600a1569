"""Plain-torch restatement of the encoder's transformer stage as the C ABI runs it (include/car_encoder.h, csrc/car_vit.hip: car_layernorm,
car_gelu, car_mha, car_vit_blocks), the dtype a parameter, from RAW weights in car_vit_pack's parameter order — plus the input sets
test_vit_reference.py (CPU) and test_vit_hip.py (GPU, through the C ABI) share.  Test infrastructure: only ever the checker; no GPU code,
no ctypes.  The softmax is written out (maximum subtracted, exp, sum, divide), not scaled_dot_product_attention.

Every item returns (value in `dtype`, bound in float64); the bound is the float64 sum of the magnitudes of the terms of its last contraction:

    layernorm   y_i = (x_i - mean) rstd g_i + b_i                      B_i = (|x_i| + mean|x|) rstd |g_i| + |b_i|
    gelu        y = x (1 + erf(x / sqrt 2)) / 2                        B = |x|
    linear      y = x W^T + bias                                       B = |x| |W|^T + |bias|          (linear_reference.layer's)
    attention   out = sum_j p_j v_j, p = softmax_j(q . k_j / 8)        B = sum_j p_j |v_j|
    block, stage  the residual stream after the block(s)               B = the largest |tok| of the row

A comparison divides an error by its bound (parity_rule.ratio); the same formulas run in float32 are the yardstick, tolerance =
8 max(r_yardstick, 2^-22) (parity_rule.judge)."""
from __future__ import annotations

import functools
import math
from typing import List, Sequence

import torch

from parity_rule import gen

F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
HEAD = 64
EPS = 1e-6                                                            # timm's LayerNorm eps; what car_vit_blocks passes to car_layernorm

# the order of car_vit_pack's `params`, 12 per block (names relative to encoder.Block)
PARAM_ORDER = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _abs64(t):
    return t.double().abs()


def layernorm(x, g, b, eps: float = EPS, dtype=F64):
    """x [M, >= C] (columns beyond C = len(g) are row padding), biased variance over the C channels."""
    C = g.shape[0]
    x = x[:, :C].to(dtype)
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * g.to(dtype) + b.to(dtype)
    x64 = x.double()
    m64 = x64.mean(dim=1, keepdim=True)
    rstd64 = 1.0 / torch.sqrt(((x64 - m64) ** 2).mean(dim=1, keepdim=True) + eps)
    B = (x64.abs() + x64.abs().mean(dim=1, keepdim=True)) * rstd64 * _abs64(g) + _abs64(b)
    return y, B


def gelu(x, dtype=F64):
    x = x.to(dtype)
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))), x.double().abs()


def linear(x, W, b, dtype=F64):
    y = x.to(dtype) @ W.to(dtype).T + b.to(dtype)
    return y, _abs64(x) @ _abs64(W).T + _abs64(b)


def attention(qkv, b: int, S: int, heads: int, dtype=F64):
    """qkv [b S, >= 3 dim] in timm's column order (q | k | v, each [heads][64]); the keys of a query are the S rows of its own scene."""
    dim = heads * HEAD
    x = qkv[:b * S, :3 * dim].to(dtype).reshape(b, S, 3, heads, HEAD).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]                                          # [b, heads, S, 64]
    logit = (q @ k.transpose(-1, -2)) / 8.0
    logit = logit - logit.amax(dim=-1, keepdim=True)
    e = torch.exp(logit)
    p = e / e.sum(dim=-1, keepdim=True)
    out = p @ v
    B = p.double() @ v.double().abs()
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(b * S, dim)
    return flat(out), flat(B)


def _row_bound(tok):
    return tok.double().abs().amax(dim=1, keepdim=True)


def block(tok, P: Sequence[torch.Tensor], b: int, S: int, heads: int, dtype=F64):
    """One pre-norm block on tok [b S, dim]; P = the block's 12 tensors in PARAM_ORDER."""
    x = tok.to(dtype)
    n, _ = layernorm(x, P[0], P[1], EPS, dtype)
    qkv, _ = linear(n, P[2], P[3], dtype)
    a, _ = attention(qkv, b, S, heads, dtype)
    x = x + linear(a, P[4], P[5], dtype)[0]
    n, _ = layernorm(x, P[6], P[7], EPS, dtype)
    h, _ = gelu(linear(n, P[8], P[9], dtype)[0], dtype)
    x = x + linear(h, P[10], P[11], dtype)[0]
    return x, _row_bound(x)


def stage(tok, params: Sequence[torch.Tensor], b: int, S: int, heads: int, taps: Sequence[int] = (), dtype=F64):
    """The blocks one after the other; params = 12 tensors per block.  -> (tok, bound, [(tap value, tap bound), ...])."""
    depth = len(params) // 12
    assert len(params) == 12 * depth and list(taps) == sorted(set(taps)) and all(0 <= t < depth for t in taps)
    x, tapped = tok.to(dtype), []
    for i in range(depth):
        x, B = block(x, params[12 * i:12 * i + 12], b, S, heads, dtype)
        if i in taps:
            tapped.append((x.clone(), B))
    return x, _row_bound(x), tapped


def block_params(m) -> List[torch.Tensor]:
    """The 12 tensors of an encoder.Block, in PARAM_ORDER."""
    sd = dict(m.named_parameters())
    return [sd[n] for n in PARAM_ORDER]


# ---- input sets: every one a named function of a seed ----------------------------------------------------------------------------------------
def seeded_block(dim: int, seed: int) -> List[torch.Tensor]:
    """One block's raw weights, nothing at an initial value: matrices ~ N(0, 1 / fan_in), norm scales 1 + 0.2 N, biases 0.1 N."""
    g = gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    mat = lambda n, k: (r(n, k) / k ** 0.5).contiguous()
    return [1 + 0.2 * r(dim), 0.1 * r(dim), mat(3 * dim, dim), 0.1 * r(3 * dim), mat(dim, dim), 0.1 * r(dim),
            1 + 0.2 * r(dim), 0.1 * r(dim), mat(4 * dim, dim), 0.1 * r(4 * dim), mat(dim, 4 * dim), 0.1 * r(dim)]


@functools.lru_cache(maxsize=None)
def seeded_stage(dim: int, depth: int, seed: int = 11):
    return tuple(t for i in range(depth) for t in seeded_block(dim, seed + i))


# car_mha: (b, S, heads) — the tile edges (31, 32, 33), the ragged last tile, one row, and the three real lengths 257, 514, 771
MHA_SHAPES = ((2, 5, 2), (1, 1, 1), (1, 31, 1), (1, 32, 1), (1, 33, 1), (1, 257, 2), (2, 514, 12), (1, 771, 12), (1, 1024, 1))
MHA_SETS = ("gauss", "peaked", "dominant", "k1e-6", "k1e+4", "uniform")
# where the value sets other than "gauss" run: one small ragged case, the first shape past a tile, two real lengths
MHA_SET_SHAPES = ((2, 5, 2), (1, 33, 1), (1, 257, 2), (2, 514, 12))
MHA_UNIFORM_SHAPES = tuple(s for s in MHA_SHAPES if s[1] & (s[1] - 1) == 0)           # S a power of two: the mean is exactly representable
DOMINANT_BY = 80.0


@functools.lru_cache(maxsize=None)
def mha_input(name: str, b: int, S: int, heads: int, seed: int = 1) -> torch.Tensor:
    """qkv [b S, 3 dim] of a car_mha value set.
    gauss      N(0, 1) throughout: logits ~ N(0, 1).
    peaked     the queries times 8: logits reach about +-30.
    dominant   channel 0 of every head: q = 8, k = DOMINANT_BY at one key per (scene, head) and 0 elsewhere — that key's logit leads by 80
               (the other channels of q are 0.1 N(0, 1): +-0.4 of noise), its weight is 1 and the output its v.
    k1e-6, k1e+4   k and v times that magnitude, q divided by it: the logits are gauss's, the operands' powers of two are not.
    uniform    q = 0, v integers in [-3, 3]: every weight is 1 / S."""
    g = gen(seed + 1000 * S + heads)
    dim = heads * HEAD
    x = torch.randn(b * S, 3, heads, HEAD, generator=g)
    if name == "peaked":
        x[:, 0] *= 8.0
    elif name == "dominant":
        x[:, 0] *= 0.1
        x[:, 0, :, 0] = 8.0
        x[:, 1, :, 0] = 0.0
        star = torch.randint(0, S, (b, heads), generator=g)
        for sc in range(b):
            for h in range(heads):
                x[sc * S + int(star[sc, h]), 1, h, 0] = DOMINANT_BY
    elif name in ("k1e-6", "k1e+4"):
        mag = float(name[1:])
        x[:, 1:] *= mag
        x[:, 0] /= mag
    elif name == "uniform":
        x[:, 0] = 0.0
        x[:, 2] = torch.randint(-3, 4, (b * S, heads, HEAD), generator=g).float()
    elif name != "gauss":
        raise KeyError(name)
    return x.reshape(b * S, 3 * dim).contiguous()


@functools.lru_cache(maxsize=None)
def mha_reference(name: str, b: int, S: int, heads: int):
    """(out float64, bound, out float32) of a value set: computed once, shared, never written to."""
    qkv = mha_input(name, b, S, heads)
    ref, B = attention(qkv, b, S, heads, F64)
    return ref, B, attention(qkv, b, S, heads, F32)[0]


def dominant_rows(qkv: torch.Tensor, b: int, S: int, heads: int) -> torch.Tensor:
    """The v rows of the dominating keys of mha_input("dominant", ...), as the output every query of the (scene, head) must give: [b S, dim]."""
    x = qkv.reshape(b, S, 3, heads, HEAD)
    star = x[:, :, 1, :, 0].argmax(dim=1)                               # [b, heads]
    v = x[:, :, 2]                                                      # [b, S, heads, 64]
    pick = torch.stack([torch.stack([v[sc, star[sc, h], h] for h in range(heads)]) for sc in range(b)])      # [b, heads, 64]
    return pick[:, None].expand(b, S, heads, HEAD).reshape(b * S, heads * HEAD)


# car_layernorm: C x M of the issue, and the row sets
LN_CS, LN_MS = (64, 128, 768), (1, 3, 65, 514)


@functools.lru_cache(maxsize=None)
def ln_input(name: str, M: int, C: int, seed: int = 2):
    """(x [M, C], gamma, beta).  gauss: rows whose scales run over 10^-3 .. 10^3; offset: 1e4 + N(0, 1); const: row m holds one value
    throughout (0.1 (m + 1), not a power of two)."""
    g = gen(seed + C + 7 * M)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    if name == "gauss":
        x = torch.randn(M, C, generator=g) * (torch.logspace(-3, 3, M)[:, None] if M > 1 else 1.0)
    elif name == "offset":
        x = 1e4 + torch.randn(M, C, generator=g)
    elif name == "const":
        x = (0.1 * (torch.arange(M, dtype=F32) + 1))[:, None].expand(M, C).contiguous()
    else:
        raise KeyError(name)
    return x.contiguous(), gamma, beta


def gelu_grid() -> torch.Tensor:
    """[-12, 12] in steps of 1 / 64 (a multiple of 4 values), both ends included."""
    x = torch.arange(-12 * 64, 12 * 64 + 1, dtype=F32) / 64
    return torch.cat([x, x[-3:] * 0 + 0.5])                            # 1537 -> 1540 values: whole float4s
