"""Plain-torch restatement of the BACKWARD of the encoder's transformer stage as the C ABI runs it (include/car_encoder_train.h,
csrc/car_vit_backward.hip: car_layernorm_backward, car_gelu_backward, car_mha_backward, car_vit_blocks_backward), the dtype a parameter,
written out formula by formula — no autograd here; test_vit_backward_reference.py holds the float64 run to float64 autograd of
vit_reference's forward.  Test infrastructure: only ever the checker; no GPU code, no ctypes.

Every item returns (value in `dtype`, bound in float64); the bound is the float64 sum of the magnitudes of the terms of its last contraction:

    layernorm   dx = rstd (a - mean a - xhat mean(a xhat)), a = g dy   B = rstd (|a| + mean|a| + |xhat| mean(|a| |xhat|))
                dgamma = sum_m dy xhat, dbeta = sum_m dy               B = sum_m |dy| |xhat|, sum_m |dy|
    gelu        du = dy (Phi(u) + u phi(u))                            B = |dy| (Phi(u) + |u| phi(u))
    attention   dv_j = sum_i p_ij dout_i                               B = sum_i p_ij |dout_i|
                ds_ij = p_ij (dout_i . v_j - dout_i . out_i)           B(ds) = p_ij (|dout_i| . |v_j| + |dout_i| . |out_i|)
                dq_i = sum_j ds_ij k_j / 8, dk_j = sum_i ds_ij q_i / 8 B = sum_j B(ds_ij) |k_j| / 8, sum_i B(ds_ij) |q_i| / 8
    stage       dtok                                                   B = the largest |dtok| of the row
                every parameter gradient                               B = the largest |g| of the tensor

A comparison divides an error by its bound (parity_rule.ratio); the same formulas run in float32 are the yardstick."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence

import torch

import vit_reference as VR
from parity_rule import gen

F32, F64 = torch.float32, torch.float64
HEAD, EPS = VR.HEAD, VR.EPS
LN_SLAB = 64                                                          # car_layernorm_backward's rows per slab of the column sums


def _abs64(t):
    return t.double().abs()


def _ln_stats(x, eps, dtype):
    x = x.to(dtype)
    mean = x.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    return (x - mean) * rstd, rstd


def layernorm_backward(x, g, dy, eps: float = EPS, dtype=F64):
    """x, dy [M, >= C] (columns beyond C = len(g) are row padding) -> ((dx, B), (dgamma, B), (dbeta, B))."""
    C = g.shape[0]
    xhat, rstd = _ln_stats(x[:, :C], eps, dtype)
    dy = dy[:, :C].to(dtype)
    a = dy * g.to(dtype)
    dx = rstd * (a - a.mean(dim=1, keepdim=True) - xhat * (a * xhat).mean(dim=1, keepdim=True))
    xh64, r64 = _ln_stats(x[:, :C], eps, F64)
    a64 = _abs64(dy) * _abs64(g)
    Bx = r64 * (a64 + a64.mean(dim=1, keepdim=True) + xh64.abs() * (a64 * xh64.abs()).mean(dim=1, keepdim=True))
    return (dx, Bx), ((dy * xhat).sum(dim=0), (_abs64(dy) * xh64.abs()).sum(dim=0)), (dy.sum(dim=0), _abs64(dy).sum(dim=0))


def gelu_grad(u, dtype=F64):
    """Phi(u) + u phi(u), Phi through erfc as the kernel takes it -> (value, its magnitude sum Phi + |u| phi)."""
    u = u.to(dtype)
    Phi = 0.5 * torch.special.erfc(-u / math.sqrt(2.0))
    phi = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    u64 = u.double()
    B = 0.5 * torch.special.erfc(-u64 / math.sqrt(2.0)) + u64.abs() * torch.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi)
    return Phi + u * phi, B


def gelu_backward(u, dy, dtype=F64):
    d, B = gelu_grad(u, dtype)
    return dy.to(dtype) * d, _abs64(dy) * B


def _heads(t, b, S, heads, dtype):
    return t.to(dtype).reshape(b, S, heads, HEAD).permute(0, 2, 1, 3)             # [b, heads, S, 64]


def _split_qkv(qkv, b, S, heads, dtype):
    dim = heads * HEAD
    x = qkv[:b * S, :3 * dim].to(dtype).reshape(b, S, 3, heads, HEAD).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def log_sum_exp(qkv, b: int, S: int, heads: int) -> torch.Tensor:
    """float64 log sum_j exp(q_i . k_j / 8): [b, heads, S] — what car_mha_stats' m + log l is."""
    q, k, _ = _split_qkv(qkv, b, S, heads, F64)
    return torch.logsumexp((q @ k.transpose(-1, -2)) / 8.0, dim=-1)


def attention_backward(qkv, dout, b: int, S: int, heads: int, dtype=F64):
    """qkv [b S, >= 3 dim], dout [b S, >= dim] -> (dqkv [b S, 3 dim], bound [b S, 3 dim]), the formulas of the header written out."""
    dim = heads * HEAD
    q, k, v = _split_qkv(qkv, b, S, heads, dtype)
    do = _heads(dout[:b * S, :dim], b, S, heads, dtype)
    logit = (q @ k.transpose(-1, -2)) / 8.0
    logit = logit - logit.amax(dim=-1, keepdim=True)
    e = torch.exp(logit)
    p = e / e.sum(dim=-1, keepdim=True)
    out = p @ v
    D = (do * out).sum(dim=-1, keepdim=True)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - D)
    dq = (ds @ k) / 8.0
    dk = (ds.transpose(-1, -2) @ q) / 8.0
    p64, do64, q64, k64, v64 = p.double(), _abs64(do), _abs64(q), _abs64(k), _abs64(v)
    Bds = p64 * (do64 @ v64.transpose(-1, -2) + (do64 * _abs64(out)).sum(dim=-1, keepdim=True))
    Bv, Bq, Bk = p64.transpose(-1, -2) @ do64, (Bds @ k64) / 8.0, (Bds.transpose(-1, -2) @ q64) / 8.0
    flat = lambda t3: torch.stack([t.permute(0, 2, 1, 3) for t in t3], dim=2).reshape(b * S, 3 * dim)
    return flat((dq, dk, dv)), flat((Bq, Bk, Bv))


def _linear_backward(dY, X, W, dtype):
    """Y = X W^T + b -> (dX, dW, db)."""
    dY, X = dY.to(dtype), X.to(dtype)
    return dY @ W.to(dtype), dY.T @ X, dY.sum(dim=0)


def block_backward(tok, P: Sequence[torch.Tensor], b: int, S: int, heads: int, g, dtype=F64, ops: Optional[List] = None):
    """One pre-norm block: tok its input, g the gradient of its output -> (gradient of its input, the 12 parameter gradients in
    PARAM_ORDER).  The forward is recomputed in `dtype`.  ops, if given, collects (item, dY, X) of the four weight gradients."""
    x0 = tok.to(dtype)
    n1, _ = VR.layernorm(x0, P[0], P[1], EPS, dtype)
    qkv, _ = VR.linear(n1, P[2], P[3], dtype)
    att, _ = VR.attention(qkv, b, S, heads, dtype)
    x1 = x0 + VR.linear(att, P[4], P[5], dtype)[0]
    n2, _ = VR.layernorm(x1, P[6], P[7], EPS, dtype)
    u, _ = VR.linear(n2, P[8], P[9], dtype)
    h, _ = VR.gelu(u, dtype)
    g = g.to(dtype)
    G: List[Optional[torch.Tensor]] = [None] * 12
    note = (lambda i, dY, X: ops.append((i, dY, X))) if ops is not None else (lambda *a: None)
    dh, G[10], G[11] = _linear_backward(g, h, P[10], dtype)
    note(10, g, h)
    du, _ = gelu_backward(u, dh, dtype)
    dn2, G[8], G[9] = _linear_backward(du, n2, P[8], dtype)
    note(8, du, n2)
    (dx, _), (G[6], _), (G[7], _) = layernorm_backward(x1, P[6], dn2, EPS, dtype)
    g = g + dx
    datt, G[4], G[5] = _linear_backward(g, att, P[4], dtype)
    note(4, g, att)
    dqkv, _ = attention_backward(qkv, datt, b, S, heads, dtype)
    dn1, G[2], G[3] = _linear_backward(dqkv, n1, P[2], dtype)
    note(2, dqkv, n1)
    (dx, _), (G[0], _), (G[1], _) = layernorm_backward(x0, P[0], dn1, EPS, dtype)
    return g + dx, G


def stage_backward(tok, params: Sequence[torch.Tensor], b: int, S: int, heads: int, taps: Sequence[int], dtaps: Sequence[Optional[torch.Tensor]],
                   dout=None, dtype=F64, ops: Optional[Dict] = None):
    """The blocks in reverse.  dout: the gradient of the stage's output (None: zero); dtaps[i]: the gradient of tap i (None: zero).
    -> ((dtok, bound), [(gradient, bound) of the 12 depth parameters])."""
    depth = len(params) // 12
    xs = [tok.to(dtype)]
    for i in range(depth):
        xs.append(VR.block(xs[-1], params[12 * i:12 * i + 12], b, S, heads, dtype)[0])
    g = torch.zeros_like(xs[0]) if dout is None else dout.to(dtype)
    grads: List = [None] * (12 * depth)
    for i in reversed(range(depth)):
        if i in taps and dtaps[list(taps).index(i)] is not None:
            g = g + dtaps[list(taps).index(i)].to(dtype)
        rec = [] if ops is not None else None
        g, G = block_backward(xs[i], params[12 * i:12 * i + 12], b, S, heads, g, dtype, rec)
        grads[12 * i:12 * i + 12] = G
        if ops is not None:
            ops[i] = rec
    bound = lambda t: torch.full((), float(t.double().abs().max()), dtype=F64)
    return (g, g.double().abs().amax(dim=1, keepdim=True)), [(t, bound(t)) for t in grads]


def stage_loss(tok, params, b, S, heads, taps, dtaps, dout=None):
    """sum <dtap_i, tap_i> + <dout, tok_out> in float64, on VR.stage: what float64 autograd differentiates."""
    x, _, tapped = VR.stage(tok, params, b, S, heads, taps, F64)
    loss = x.new_zeros(())
    if dout is not None:
        loss = loss + (x * dout.double()).sum()
    for (t, _), d in zip(tapped, dtaps):
        if d is not None:
            loss = loss + (t * d.double()).sum()
    return loss


@functools.lru_cache(maxsize=None)
def autograd_stage(dim: int, depth: int, taps, b: int, S: int, which: str = "all"):
    """(tok0, dtaps, dout, dtok float64, [parameter gradients float64]) by float64 autograd of VR.stage — computed once, shared, never
    written to.  which: "all" (every tap and the output carry a gradient) or "tap<i>" (that tap alone)."""
    params = VR.seeded_stage(dim, depth)
    tok0 = torch.randn(b * S, dim, generator=gen(dim + S))
    g = gen(7 * dim + S)
    dtaps = [torch.randn(b * S, dim, generator=g) for _ in taps]
    dout = torch.randn(b * S, dim, generator=g)
    if which != "all":
        keep = int(which[3:])
        dtaps, dout = [d if t == keep else None for d, t in zip(dtaps, taps)], None
    leaf = [t.double().requires_grad_(True) for t in (tok0, *params)]
    stage_loss(leaf[0], leaf[1:], b, S, dim // HEAD, taps, dtaps, dout).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return tok0, dtaps, dout, zero(leaf[0]), [zero(t) for t in leaf[1:]]


# ---- input sets ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mha_dout(b: int, S: int, heads: int, seed: int = 5) -> torch.Tensor:
    return torch.randn(b * S, heads * HEAD, generator=gen(seed + 1000 * S + heads))


@functools.lru_cache(maxsize=None)
def mha_backward_reference(name: str, b: int, S: int, heads: int):
    """(dqkv float64, bound, dqkv float32) of a value set of vit_reference.mha_input with mha_dout: computed once, shared."""
    qkv, dout = VR.mha_input(name, b, S, heads), mha_dout(b, S, heads)
    ref, B = attention_backward(qkv, dout, b, S, heads, F64)
    return ref, B, attention_backward(qkv, dout, b, S, heads, F32)[0]


def mha_integers(b: int, S: int, heads: int, seed: int = 6):
    """(qkv, dout) of small integers: every product and sum of the backward is exact in the split arithmetic and in float32, so
    identities hold bit for bit (at S = 1: p = 1, dp = D, ds = 0)."""
    g = gen(seed + S)
    r = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    return r(b * S, 3 * heads * HEAD), r(b * S, heads * HEAD)


@functools.lru_cache(maxsize=None)
def ln_dy(M: int, C: int, seed: int = 8) -> torch.Tensor:
    return torch.randn(M, C, generator=gen(seed + C + 7 * M))


# rows on both sides of the slab of the column sums: one row short of a slab, a whole slab, one over, several slabs and a ragged last one
LN_SLAB_MS = (LN_SLAB - 1, LN_SLAB, LN_SLAB + 1, 3 * LN_SLAB + 5)
