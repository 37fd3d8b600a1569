"""Plain-torch restatement of the two per-ray chain kernels (csrc/car_raychain.hip) and of car_finalize, the dtype a parameter, plus the
helper that lays raw weights out the way the chain entries of include/car_hip.h want them.  Test infrastructure: only ever the checker.

    mid :  z1 = latent_value(ebar) ;  uh = query_repeat_embed.weight[:, :128] encode_latent(z1)                (models.py:487, 548, 552)
    tail:  z = latent_value(ebar) + V z1 ;  x = lin_in(phi_x) ;  3 x { x += lin_z_i([z, z]) ;  x += fc_1(relu(fc_0(relu(x)))) } ;
           rgb = lin_out(relu(x)) valid + (1 - valid)                           (models.py:561-565, 597-617; resnet_block_fc.py:132-168)

Weights come raw and unpacked under the names of models.py.  Every output comes with its LAST layer's bound, always computed in float64
from the float64 run, whatever `dtype` is:  B_z1 = |Wv| |ebar| + |bv|,  B_uh = |Wq| |h| (h = encode_latent(z1)),
B_rgb = |Wo| relu(x) + |bo|.  A comparison divides an error by that bound (test_raychain_hip.py)."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from parity_rule import FACTOR, FLOOR, gen, ratio, tolerance  # noqa: F401  (the suites' rule: max |got - ref64| / bound, 8 x max(r, 2^-22))

C, E, D, PHI = 576, 288, 128, 18                       # ebar / e width, latent width, hidden width, decoder ray input
BLOCKS = 3
SHAPES = {"latent_value": (E, C), "encode_latent": (D, E), "query_repeat_embed": (D, D + 16), "phi.lin_in": (D, PHI), "phi.lin_out": (3, D)}
for _i in range(BLOCKS):
    SHAPES.update({f"phi.lin_z.{_i}": (D, 2 * E), f"phi.blocks.{_i}.fc_0": (D, D), f"phi.blocks.{_i}.fc_1": (D, D)})
MID_LAYERS = ("latent_value", "encode_latent", "query_repeat_embed")
TAIL_LAYERS = ("latent_value", "phi.lin_in") + tuple(n for i in range(BLOCKS) for n in (f"phi.lin_z.{i}", f"phi.blocks.{i}.fc_0", f"phi.blocks.{i}.fc_1")) \
    + ("phi.lin_out",)
PLAN_SLOTS = {"mid": (0, 1, 2), "tail": (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)}      # what car_plan_build / car_render_forward use


def gaussian_params(seed: int) -> Dict[str, torch.Tensor]:
    """N(0, 1 / fan_in) weights and 0.1 N(0, 1) biases in float32, drawn in sorted-name order from one generator."""
    g = gen(seed)
    out = {}
    for name in sorted(SHAPES):
        n, k = SHAPES[name]
        out[name + ".weight"] = torch.randn(n, k, generator=g) / k ** 0.5
        out[name + ".bias"] = 0.1 * torch.randn(n, generator=g)
    return out


def _p(params, name, dtype):
    return params[name + ".weight"].to(dtype), params[name + ".bias"].to(dtype)


def _mid(params, ebar, dtype, trace=None):
    Wv, bv = _p(params, "latent_value", dtype)
    We, be = _p(params, "encode_latent", dtype)
    Wq = params["query_repeat_embed.weight"].to(dtype)[:, :D]
    x = ebar.to(dtype)
    z1 = F.linear(x, Wv, bv)
    h = F.linear(z1, We, be)
    uh = F.linear(h, Wq)
    if trace is not None:
        trace += [("latent_value", x, Wv, bv, None, z1), ("encode_latent", z1, We, be, None, h), ("query_repeat_embed", h, Wq, None, None, uh)]
    return z1, h, uh


def mid(params, ebar, dtype=torch.float64, trace: Optional[list] = None):
    """ebar [M, 576] -> dict(z1 [M, 288], uh [M, 128]) in `dtype`, B_z1 and B_uh in float64.  `trace` (a list) receives, per layer,
    (name, input, weight, bias, what the layer adds to, output)."""
    z1, _, uh = _mid(params, ebar, dtype, trace)
    e64 = ebar.double()
    z64, h64, _ = _mid(params, ebar, torch.float64)
    Wv, bv = _p(params, "latent_value", torch.float64)
    Wq = params["query_repeat_embed.weight"].double()[:, :D]
    return {"z1": z1, "uh": uh, "B_z1": e64.abs() @ Wv.abs().T + bv.abs(), "B_uh": h64.abs() @ Wq.abs().T}


def _valid(overlaps):
    """overlaps [b, V, R] -> valid [b R] (1.0 where any view's entry is non-zero)."""
    return (overlaps != 0).any(dim=1).reshape(-1)


def _tail(params, ebar, phi_x, z1, V, dtype, trace=None):
    Wv, bv = _p(params, "latent_value", dtype)
    e = ebar.to(dtype)
    z1s = float(V) * z1.to(dtype)
    z = F.linear(e, Wv, bv) + z1s
    zz = torch.cat([z, z], dim=-1)
    Wi, bi = _p(params, "phi.lin_in", dtype)
    px = phi_x.to(dtype)
    x = F.linear(px, Wi, bi)
    if trace is not None:
        trace += [("latent_value", e, Wv, bv, z1s, z), ("phi.lin_in", px, Wi, bi, None, x)]
    for i in range(BLOCKS):
        Wz, bz = _p(params, f"phi.lin_z.{i}", dtype)
        W0, b0 = _p(params, f"phi.blocks.{i}.fc_0", dtype)
        W1, b1 = _p(params, f"phi.blocks.{i}.fc_1", dtype)
        x0 = x
        x = x + F.linear(zz, Wz, bz)
        net = F.linear(F.relu(x), W0, b0)
        x1 = x
        x = x + F.linear(F.relu(net), W1, b1)
        if trace is not None:
            trace += [(f"phi.lin_z.{i}", zz, Wz, bz, x0, x1), (f"phi.blocks.{i}.fc_0", F.relu(x1), W0, b0, None, net),
                      (f"phi.blocks.{i}.fc_1", F.relu(net), W1, b1, x1, x)]
    Wo, bo = _p(params, "phi.lin_out", dtype)
    raw = F.linear(F.relu(x), Wo, bo)
    if trace is not None:
        trace += [("phi.lin_out", F.relu(x), Wo, bo, None, raw)]
    return z, x, raw


def tail(params, ebar, phi_x, z1, overlaps, V, dtype=torch.float64, trace: Optional[list] = None):
    """ebar [M, 576], phi_x [M, 18], z1 [M, 288], overlaps [b, V, R] with b R = M -> dict(rgb [M, 3], valid [M], z [M, 288], raw [M, 3]
    (lin_out's output before the blend)) in `dtype`, B_rgb in float64."""
    assert phi_x.shape[-1] == PHI and overlaps.shape[1] == V and overlaps.shape[0] * overlaps.shape[2] == ebar.shape[0]
    z, _, raw = _tail(params, ebar, phi_x, z1, V, dtype, trace)
    valid = _valid(overlaps).to(dtype)
    rgb = raw * valid[:, None] + (1 - valid[:, None])
    _, x64, _ = _tail(params, ebar, phi_x, z1, V, torch.float64)
    Wo, bo = _p(params, "phi.lin_out", torch.float64)
    return {"rgb": rgb, "valid": valid, "z": z, "raw": raw, "B_rgb": F.relu(x64) @ Wo.abs().T + bo.abs()}


def finalize(rgb_in, overlaps):
    """car_finalize: rgb_in [b R, >= 3], overlaps [b, V, R] -> rgb [b R, 3] = rgb_in[:, :3] valid + (1 - valid), valid [b R]."""
    valid = _valid(overlaps).to(rgb_in.dtype)
    return rgb_in[:, :3] * valid[:, None] + (1 - valid[:, None]), valid


def rays_from_overlaps(overlaps, fill=float("nan")):
    """CarRay records [b V, R, 12] that hold `fill` everywhere but in `overlaps` (float 10: csrc/car_geom.h)."""
    b, V, R = overlaps.shape
    rays = torch.full((b * V, R, 12), fill, dtype=torch.float32)
    rays[:, :, 10] = overlaps.reshape(b * V, R).float()
    return rays


# ---- what the C entries need, from raw weights ---------------------------------------------------------------------------------------
def layer_specs(which: str):
    """Per layer of the kernel, in consumption order: (name, ldw, W2 column offset or None, K, N, chained) — the comment above
    car_chain_packed_floats in include/car_hip.h."""
    specs = []
    for name in (MID_LAYERS if which == "mid" else TAIL_LAYERS):
        n, k = SHAPES[name]
        if name == "query_repeat_embed":
            specs.append((name, D + 16, None, D, D, 1))
        elif ".lin_z." in name:
            specs.append((name, 2 * E, E, E, D, 1))                                   # [z, z]: W2 = W + 288, the halves added at pack time
        else:
            specs.append((name, k, None, k, n, 0 if name in ("latent_value", "phi.lin_in") else 1))
    return specs


class ChainTables:
    """Arena, chunk tables, bias block, scale array and slot list of one chain, on the device / as host ctypes arrays."""

    def __init__(self, lib, params, which: str, device, slots: Optional[Sequence[int]] = None, arena_order: Optional[Sequence[int]] = None,
                 gap: int = 0, stream=None):
        """slots: scale slot of every layer, in consumption order (default: the plan's).  arena_order: the order in which the layers lie
        inside the arena (indices into the consumption order; default: consumption order).  gap: floats left between two layers (a
        multiple of 4; they and a margin at either end stay NaN)."""
        assert gap % 4 == 0
        specs = layer_specs(which)
        n = len(specs)
        slots = list(PLAN_SLOTS[which] if slots is None else slots)
        order = list(range(n) if arena_order is None else arena_order)
        assert sorted(order) == list(range(n)) and len(slots) == n and len(set(slots)) == n and all(0 <= s < 16 for s in slots)
        sizes = [int(lib.car_chain_packed_floats(k, nn)) for (_, _, _, k, nn, _) in specs]
        for (_, _, _, k, nn, _), sz in zip(specs, sizes):
            assert sz == -(-k // 32) * -(-nn // 32) * 1024
        at, o = [0] * n, 64
        for i in order:
            at[i] = o
            o += sizes[i] + gap
        self.arena = torch.full((o + 64,), float("nan"), dtype=torch.float32, device=device)
        self.scale = torch.full((32,), float("nan"), dtype=torch.float32, device=device)
        self.weights = {}
        offs, nts = [], []
        for i, (name, ldw, w2, k, nn, chained) in enumerate(specs):
            W = params[name + ".weight"].float().contiguous().to(device)
            assert W.shape[1] == ldw
            self.weights[name] = W
            rc = lib.car_chain_pack(ctypes.c_void_p(W.data_ptr()), ldw, ctypes.c_void_p(W.data_ptr() + 4 * w2) if w2 is not None else None, k, nn,
                                    chained, ctypes.c_void_p(self.arena.data_ptr() + 4 * at[i]), ctypes.c_void_p(self.scale.data_ptr()), slots[i],
                                    stream)
            assert rc == 0, lib.car_last_error()
            chunks, nt = -(-k // 32), -(-nn // 32)
            offs += [at[i] + c * nt * 1024 for c in range(chunks)]
            nts += [nt] * chunks
        assert len(offs) == (31 if which == "mid" else 74) and set(nts) <= {9, 4, 1}
        self.n_chunks = len(offs)
        self.offs = (ctypes.c_uint * len(offs))(*offs)
        self.nts = (ctypes.c_int * len(nts))(*nts)
        self.layers = (ctypes.c_int * n)(*slots)
        self.n_layers = n
        self.layer_at, self.sizes, self.slots = at, sizes, slots
        bias: List[torch.Tensor] = []
        for name in (("latent_value", "encode_latent") if which == "mid" else TAIL_LAYERS):
            bias.append(params[name + ".bias"].float())
        if which == "tail":
            bias.append(torch.zeros(32 - 3))                                          # lin_out.bias padded to 32
        self.bias = torch.cat(bias).contiguous().to(device)
        assert self.bias.numel() == (E + D if which == "mid" else E + D + 3 * BLOCKS * D + 32)


# ---- the cases both test files use -----------------------------------------------------------------------------------------------------
MID_M = (1, 31, 32, 33, 127, 128, 129, 161, 389)
TAIL_SHAPES = ((1, 1, 1), (1, 2, 33), (2, 2, 80), (3, 3, 43), (1, 2, 300))               # (b, V, R); (2, 2, 80): a scene boundary inside a
                                                                                        # workgroup; (3, 3, 43): M = 129
LD_EBAR = (576, 580, 640)
LD_PHI = (20, 24)


def gaussian_inputs(M: int, seed: int):
    g = gen(seed)
    return torch.randn(M, C, generator=g), torch.randn(M, E, generator=g), torch.randn(M, PHI, generator=g)


def random_overlaps(b: int, V: int, R: int, seed: int, p: float = 0.7):
    return (torch.rand(b, V, R, generator=gen(seed)) < p).float()


def magnitude_inputs(M: int, seed: int):
    """Rows of ebar and z1 scaled by logspace(-6, 4) over every 32 consecutive rays (one wave holds both ends); with M >= 8 row 3 of ebar
    all zero, row 5 non-zero only at column 575, row 6 only at column 0.  Returns (ebar, z1, phi_x, special rows)."""
    ebar, z1, phi_x = gaussian_inputs(M, seed)
    s = torch.logspace(-6, 4, 32)[torch.arange(M) % 32]
    ebar, z1 = ebar * s[:, None], z1 * s[:, None]
    special = {}
    if M >= 8:
        ebar[3] = 0.0
        ebar[5, :C - 1] = 0.0
        ebar[6, 1:] = 0.0
        special = {"zero": 3, "last": 5, "first": 6}
    return ebar, z1, phi_x, special


def scaled_params(params, zero_lin_z2: bool, uneven_halves: bool = False):
    """encode_latent's weights x 2^-20, fc_0 of block 1 x 2^10, biases left alone; then lin_z.2's weights all zero.  uneven_halves: also
    lin_z.0's first 288 columns all zero and lin_z.1's last 288 columns x 2^4 — a layer's power of two must come from the largest
    |W + W2|, not from W's half alone (taken from W alone the packed halves leave fp16's range: the first by pow2_scale's clamp, the
    second by four binary orders)."""
    p = {k: v.clone() for k, v in params.items()}
    p["encode_latent.weight"] *= 2.0 ** -20
    p["phi.blocks.1.fc_0.weight"] *= 2.0 ** 10
    if zero_lin_z2:
        p["phi.lin_z.2.weight"].zero_()
    if uneven_halves:
        p["phi.lin_z.0.weight"][:, :E] = 0.0
        p["phi.lin_z.1.weight"][:, E:] *= 2.0 ** 4
    return p


INT_V = 2
INT_WIDE = 2 ** 13                                       # magnitude of the wide rays' entries: (2^12, 2^13]
INT_DEAD = (2, 40, 127)                                  # rays whose x is entirely non-positive in front of fc_0 of block 0


def integer_case(seed: int = 5, M: int = 161):
    """The exact-integer case: every weight row holds two non-zeros of +-1 (lin_z: two per 288-column half, the halves different and
    not cancelling), biases are small integers, and the inputs are integers, so every product and partial sum of either chain is an
    integer that fp32 — and the kernels' 22-bit split operands — hold exactly (test_raychain_reference.py asserts the magnitudes).
      rays with r % 4 != 1: ebar, z1, phi_x integers in [-8, 8];
      rays with r % 4 == 1 ("wide"): integers of magnitude in (2^12, 2^13] with all their low bits, without which no lo half of the
        kernels' operands would be non-zero and the exactness would say nothing about them;
      rays INT_DEAD: ebar = 0, phi_x = 0, z1 = -bv / 2 (bv even) so that z = 0, and lin_in.bias, lin_z.0.bias <= 0: x <= 0 in front of
        fc_0 of block 0, whose output is then its bias exactly.
    Returns (params, ebar, z1, phi_x), all float32 holding integers."""
    g = gen(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def sparse(n, k, width=None):
        W = torch.zeros(n, width or k)
        for r in range(n):
            cols = torch.randperm(k, generator=g)[:2]
            W[r, cols] = ri(0, 1, 2) * 2 - 1
        return W
    params = {}
    for name, (n, k) in SHAPES.items():
        if ".lin_z." in name:
            while True:
                a, b2 = sparse(n, E), sparse(n, E)
                if bool(((a != b2).any(dim=1) & ((a + b2) != 0).any(dim=1)).all()) and bool(((a + b2).abs() == 2).any()):
                    break
            W = torch.cat([a, b2], dim=1)
        elif name == "query_repeat_embed":
            W = torch.cat([sparse(n, D), ri(-1, 1, n, 16)], dim=1)              # the kernel must not read columns 128 and up
        else:
            W = sparse(n, k)
        params[name + ".weight"] = W
        params[name + ".bias"] = ri(-3, 3, n)
    params["latent_value.bias"] = 2 * ri(-2, 2, E)
    params["phi.lin_in.bias"] = ri(-3, 0, D)
    params["phi.lin_z.0.bias"] = ri(-3, 0, D)
    ebar, z1, phi_x = ri(-8, 8, M, C), ri(-8, 8, M, E), ri(-8, 8, M, PHI)
    wide = torch.arange(M) % 4 == 1

    def widen(t):
        big = (ri(2 ** 12 + 1, INT_WIDE, *t.shape)) * (ri(0, 1, *t.shape) * 2 - 1)
        return torch.where(wide[:, None], big, t)
    ebar, z1, phi_x = widen(ebar), widen(z1), widen(phi_x)
    for r in INT_DEAD:
        assert r < M and r % 4 != 1
        ebar[r] = 0.0
        phi_x[r] = 0.0
        z1[r] = -params["latent_value.bias"] / INT_V
    return params, ebar, z1, phi_x


def mid_tags():
    return [f"mid-gauss-{M}" for M in MID_M] + ["mid-mag", "mid-scale0", "mid-scale1"]


def tail_tags():
    return [f"tail-gauss-{b}-{V}-{R}" for b, V, R in TAIL_SHAPES] + ["tail-mag", "tail-scale0", "tail-scale1", "tail-scale2"]


def case(tag: str):
    """The inputs of one tolerance-checked case of test_raychain_hip.py, by name: dict(params, ebar, z1, phi_x, overlaps, V, special)."""
    which, kind, *rest = tag.split("-")
    params = gaussian_params(1)
    special = {}
    if kind == "gauss":
        b, V, R = (1, 1, int(rest[0])) if which == "mid" else map(int, rest)
        ebar, z1, phi_x = gaussian_inputs(b * R, 10 + b * R)
    else:
        b, V, R = (1, 1, 161) if which == "mid" else (2, 2, 80)
        if kind == "mag":
            ebar, z1, phi_x, special = magnitude_inputs(b * R, 20)
        else:
            ebar, z1, phi_x = gaussian_inputs(b * R, 30)
            params = scaled_params(params, zero_lin_z2=kind == "scale1", uneven_halves=kind == "scale2")
    return dict(params=params, ebar=ebar, z1=z1, phi_x=phi_x, overlaps=random_overlaps(b, V, R, 40 + R), V=V, b=b, R=R, special=special)
