"""Plain-torch restatement of the linear layers, forward and weight gradient (csrc/car_linear.hip: car_linear_pack, car_linear;
csrc/car_linear16.hip: car_linear_x3, car_linear_x3_masked, car_key_query_logits; csrc/car_backward.hip: car_linear_wgrad), the dtype a
parameter, plus the launch rules of those entries restated as facts a test can assert, car_linear_pack's layout as an index formula, and
the input sets test_linear_reference.py (CPU) and test_linear_hip.py (GPU, through the C ABI) share.  Test infrastructure: only ever the
checker; no GPU code, no ctypes.

    layer   Y  = relu_out?( relu_in?(X[:, :K]) W^T + b (+ Y0) )       accumulate first, then rectify (include/car_hip.h: "Y[M, N] =
                 act(act_in(X[M, K]) W^T + bias (+ Y))")                    B = |x| |W|^T + |b| (+ |Y0|)
    chain   k1 = relu(Wk1 e + bk1), key = Wk2 k1 + bk2, q1 = relu(Wq1 g + bq1), qry = Wq2 q1 + bq2, logit = <key, qry> / 16 (unfolded)
                 B_k1 = |Wk1| |e| + |bk1|, B_key = |Wk2| B_k1 + |bk2|, B_q1, B_qry likewise, B_logit = (B_key . |qry| + |key| . B_qry) / 16;
                 an entry of k1 / q1 that lies below zero by more than 2^-12 of its own bound is exactly 0 behind the ReLU whatever a
                 float32-class kernel computes (its error is some 2^-20 of that bound), so it carries no magnitude on: for a row whose k1 is
                 negative throughout, B_key is |bk2| alone.  This only ever lowers the bound.
    wgrad   dW = dW0 + dY^T act(X), db = db0 + sum_m dY                     B = |dW0| + |dY|^T |act(X)|,  |db0| + sum |dY|

Every bound is float64.  A comparison divides an error by its bound (parity_rule.ratio); tolerance = 8 max(r, 2^-22), r the worst
ratio of a yardstick on the same inputs (parity_rule.tolerance).  Yardsticks: the float32 run of the same formula (torch float32 on
the CPU); x3_linear, the three-product split-fp16 arithmetic of csrc/car_split.h / car_linear16.hip; wgrad_bf16, the three-product bf16
arithmetic of csrc/car_backward.hip w16_piece.  Both emulations sum in float64: they state which products the kernel forms from which
operand halves, not the order or width of its accumulation."""
from __future__ import annotations

import functools
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F

import pack_reference as PR
from parity_rule import FACTOR, FLOOR, gen, ratio, tolerance  # noqa: F401

F32, F64 = torch.float32, torch.float64
RELU_IN, RELU_OUT, ACCUM, NO_GLDS, WGRAD_FP32 = 1, 2, 4, 8, 16          # CAR_LIN_*, CAR_WGRAD_FP32 of include/car_hip.h
NAN, INF = float("nan"), float("inf")

GATE = 2.0 ** -12                                                      # see the module docstring: the ReLU's dead entries


def _abs64(t):
    return t.double().abs()


# ---- the forward layer ---------------------------------------------------------------------------------------------------------------------------
def layer(X, W, b, Y0, flags: int, dtype=F64, linear: Optional[Callable] = None):
    """X [M, >= K] (columns beyond K are row padding and never read), W [N, K], b [N] or None, Y0 [M, N] (ACCUM) -> (Y in `dtype`, B float64).
    `linear(x, W, b)` replaces the product's arithmetic (an emulation); the bound never uses it."""
    K = W.shape[1]
    x = X[:, :K]
    if flags & RELU_IN:
        x = F.relu(x)
    y = linear(x, W, b).to(dtype) if linear is not None else F.linear(x.to(dtype), W.to(dtype), None if b is None else b.to(dtype))
    B = _abs64(x) @ _abs64(W).T + (0 if b is None else _abs64(b))
    if flags & ACCUM:
        y, B = y + Y0.to(dtype), B + _abs64(Y0)
    return (F.relu(y) if flags & RELU_OUT else y), B


def masked(y, act):
    """car_linear_x3_masked's store rule on a finished layer: the value where act > 0 (false for NaN and for either zero), else +0.0."""
    return torch.where(act > 0, y, torch.zeros_like(y))


# ---- split-fp16, three products (csrc/car_split.h, csrc/car_fused_mma.h mfma_pair, csrc/car_pack.hip) ---------------------------------------------
def fp16_rtz(x: torch.Tensor) -> torch.Tensor:
    """float32 -> fp16 rounded toward zero (v_cvt_pkrtz_f16_f32), returned as float32."""
    h = x.half()
    bits = h.view(torch.int16)
    over = h.float().abs() > x.abs()                                   # rounded away from zero: one step back (sign-magnitude bits)
    return torch.where(over, bits - 1, bits).view(torch.float16).float()


def split_x(xs: torch.Tensor):
    """An activation already multiplied by its power of two: hi toward zero, lo = fp16(x - hi) to nearest (split_pair)."""
    hi = fp16_rtz(xs)
    return hi, (xs - hi).half().float()


def split_w(ws: torch.Tensor):
    """A weight already multiplied by the layer's power of two: both halves to nearest (car_pack_rows16, pack_reference.pack_tiles16)."""
    hi = ws.half().float()
    return hi, (ws - hi).half().float()


def row_pow2(m: torch.Tensor) -> torch.Tensor:
    """csrc/car_split.h pow2_scale on a tensor of magnitudes: 2^k with m 2^k in [2^13, 2^14), the biased exponent of m clamped to
    [97, 230], i.e. 2^k in [2^-90, 2^43]."""
    e = ((m.float().contiguous().view(torch.int32) >> 23) & 0xff).clamp(97, 230)
    return ((267 - e) << 23).to(torch.int32).view(F32)


def x3_linear(x, W, b):
    """The arithmetic of linear16_kernel on float32 operands, float64 sums: the weights carry pack_reference.pow2_scale(max |W|), a row
    of x the power of two of the largest magnitude seen so far along the row, 32 columns at a time (never below 1e-30: the clamp); per
    term hi hi + hi lo(x) + lo(W) hi, the lo lo product dropped; both powers undone exactly; the bias added unsplit."""
    x, W = x.float(), W.float()
    M, K = x.shape
    pW = PR.pow2_scale(W.abs().max().item())
    wh, wl = split_w(W * pW)
    out = torch.zeros(M, W.shape[0], dtype=F64)
    mrun = torch.full((M,), 1e-30)
    for c in range(0, K, 32):
        xc = x[:, c:c + 32]
        mrun = torch.maximum(mrun, xc.abs().amax(dim=1))
        p = row_pow2(mrun)
        xh, xl = split_x(xc * p[:, None])
        whc, wlc = wh[:, c:c + 32].double(), wl[:, c:c + 32].double()
        s = xh.double() @ whc.T + xl.double() @ whc.T + xh.double() @ wlc.T
        out += s / (p.double()[:, None] * pW)
    return out if b is None else out + b.double()


def x3_exact(x, W) -> bool:
    """The condition under which x3_linear (and the kernel, whose float32 partial sums of integers below 2^24 are exact in any order) is
    exact, from csrc/car_split.h: a half keeps fp16's 11 significant bits whatever the power of two (no value here is small enough to be
    subnormal after scaling: integers against a row maximum below 2^14), so hi + lo = x needs no more than 22 significant bits, and the
    dropped lo lo product is zero when, term by term, one of the two operands fits its hi half alone (11 bits, toward zero or to nearest
    alike)."""
    def sig_bits(t):
        t = t.double().abs()
        m, _ = torch.frexp(t)
        m = m * 2 ** 30
        assert bool((m == m.round()).all())
        low = torch.where(t > 0, (m.long() & -m.long()).double().log2(), torch.full_like(t, 29))       # index of the lowest set bit
        return 30 - low
    bx, bw = sig_bits(x), sig_bits(W)
    ok = bool((bx <= 22).all()) and bool((bw <= 22).all())
    wide_x, wide_w = (bx > 11).double(), (bw > 11).double()
    return ok and float((wide_x @ wide_w.T).max()) == 0


# ---- the key / query chain ---------------------------------------------------------------------------------------------------------------------
KQ_NAMES = ("Wk1", "bk1", "Wk2", "bk2", "Wq1", "bq1", "Wq2", "bq2")


def kq_chain(e, g, P: Dict[str, torch.Tensor], dtype=F64, linear: Optional[Callable] = None):
    """e [M, >= Ce], g [M, 16], P the eight tensors of KQ_NAMES -> dict of k1, key, q1, qry [M, 128], logit [M] in `dtype` and, where no
    `linear` replaces the arithmetic, the float64 bounds B_k1, B_key, B_q1, B_qry, B_logit (module docstring)."""
    Ce = P["Wk1"].shape[1]
    lin = (lambda x, W, b: linear(x, W, b).to(dtype)) if linear is not None else (lambda x, W, b: F.linear(x.to(dtype), W.to(dtype), b.to(dtype)))
    ee, gg = e[:, :Ce], g
    k1 = F.relu(lin(ee, P["Wk1"], P["bk1"]))
    key = lin(k1, P["Wk2"], P["bk2"])
    q1 = F.relu(lin(gg, P["Wq1"], P["bq1"]))
    qry = lin(q1, P["Wq2"], P["bq2"])
    out = {"k1": k1, "key": key, "q1": q1, "qry": qry, "logit": (key * qry).sum(dim=-1) / 16}
    if linear is None:
        def carried(x, W, b):
            pre = F.linear(x.double(), W.double(), b.double())
            B = _abs64(x) @ _abs64(W).T + _abs64(b)
            return B, torch.where(pre > -GATE * B, B, torch.zeros_like(B))
        B_k1, live_k1 = carried(ee, P["Wk1"], P["bk1"])
        B_q1, live_q1 = carried(gg, P["Wq1"], P["bq1"])
        B_key = live_k1 @ _abs64(P["Wk2"]).T + _abs64(P["bk2"])
        B_qry = live_q1 @ _abs64(P["Wq2"]).T + _abs64(P["bq2"])
        out.update(B_k1=B_k1, B_key=B_key, B_q1=B_q1, B_qry=B_qry,
                   B_logit=((B_key * qry.double().abs()).sum(-1) + (key.double().abs() * B_qry).sum(-1)) / 16)
    return out


# ---- the weight gradient -------------------------------------------------------------------------------------------------------------------------
def wgrad(dY, X, relu: bool, dW0, db0, dtype=F64):
    """dY [M, >= N], X [M, >= K], dW0 [N, K], db0 [N] or None -> (dW, db or None in `dtype`, B_W, B_b float64)."""
    N, K = dW0.shape
    dy, x = dY[:, :N], X[:, :K]
    if relu:
        x = F.relu(x)
    dW = dW0.to(dtype) + dy.to(dtype).T @ x.to(dtype)
    BW = _abs64(dW0) + _abs64(dy).T @ _abs64(x)
    if db0 is None:
        return dW, None, BW, None
    return dW, db0.to(dtype) + dy.to(dtype).sum(0), BW, _abs64(db0) + _abs64(dy).sum(0)


def bf16_split(x: torch.Tensor):
    """w16_piece: hi = bf16(x), lo = bf16(x - hi), both to nearest; the difference is exact in float32."""
    hi = x.float().bfloat16().float()
    return hi, (x.float() - hi).bfloat16().float()


def wgrad_bf16(dY, X, relu: bool, dW0, db0, products=("hh", "hl", "lh")):
    """wgrad16_kernel's arithmetic, float64 sums: hi hi + hi(dY) lo(X) + lo(dY) hi(X), the lo lo product dropped; the bias column is
    X = 1 (hi = 1, lo = 0).  `products` exists so that a test can drop one and see the exact sets notice."""
    N, K = dW0.shape
    x = F.relu(X[:, :K]) if relu else X[:, :K]
    (yh, yl), (xh, xl) = bf16_split(dY[:, :N]), bf16_split(x)
    yh, yl, xh, xl = yh.double(), yl.double(), xh.double(), xl.double()
    dW, db = dW0.double().clone(), None if db0 is None else db0.double().clone()
    one = torch.ones(X.shape[0], 1, dtype=F64)
    for name, a, bx, bone in (("hh", yh, xh, one), ("hl", yh, xl, None), ("lh", yl, xh, one)):
        if name in products:
            dW += a.T @ bx
            if db is not None and bone is not None:
                db += (a.T @ bone)[:, 0]
    return dW, db


def bf16_exact(dY, X) -> bool:
    """Exact under w16_piece: hi + lo = x needs at most 16 significant bits, and the lo lo product is zero when one of the two operands
    has at most 8 (its lo is zero) — asked of the whole operand, as the issue of this file's tests states it."""
    (yh, yl), (xh, xl) = bf16_split(dY), bf16_split(X)
    whole = torch.equal(yh + yl, dY.float()) and torch.equal(xh + xl, X.float())
    return whole and (not bool(yl.any()) or not bool(xl.any()))


# ---- launch rules, restated --------------------------------------------------------------------------------------------------------------------
def _up(a: int, b: int) -> int:
    return (a + b - 1) // b


def tiles_per_block(tiles: int) -> int:
    return 9 if tiles >= 9 else 4 if tiles >= 3 else 2 if tiles == 2 else 1


def pack_geom(K: int, N: int):
    """csrc/car_linear.hip pack_geom: 32-wide K chunks of K + 1 columns (the bias column), 32-wide tiles, NT tiles per workgroup, the tile
    count rounded up to whole workgroups (phantom tiles: zeros in the pack, masked at the store)."""
    chunks, tiles = _up(K + 1, 32), _up(N, 32)
    nt = tiles_per_block(tiles)
    alloc = _up(tiles, nt) * nt
    return {"chunks": chunks, "tiles": tiles, "nt": nt, "tiles_alloc": alloc, "phantom": alloc - tiles, "floats": chunks * alloc * 1024}


def linear_launch(M: int, K: int, N: int):
    g = pack_geom(K, N)
    return dict(g, grid=(_up(M, 128), g["tiles_alloc"] // g["nt"]), last_block_rows=M - (_up(M, 128) - 1) * 128)


def packed_layout(W, b, K: int, N: int) -> torch.Tensor:
    """pack_kernel as an index formula: float idx = ((chunk tiles_alloc + tile) 4 + j4) 256 + 4 lane + e holds W[n][k] with
    n = 32 tile + lane % 32, k = 32 chunk + 16 (lane / 32) + 4 j4 + e; k == K: the bias (0 without one); k > K or n >= N: 0."""
    g = pack_geom(K, N)
    idx = torch.arange(g["floats"])
    e, lane, j4, ct = idx & 3, (idx >> 2) & 63, (idx >> 8) & 3, idx >> 10
    tile, chunk = ct % g["tiles_alloc"], ct // g["tiles_alloc"]
    n, k = 32 * tile + (lane & 31), 32 * chunk + 16 * (lane >> 5) + 4 * j4 + e
    ext = torch.zeros(32 * g["tiles_alloc"], 32 * g["chunks"] + 1, dtype=F32)
    ext[:N, :K] = W[:, :K]
    if b is not None:
        ext[:N, K] = b
    return ext[n, k]


def x3_launch(M: int, K: int, N: int):
    """linear_x3's NT choice and the kernel's block map: column groups of NT 16-wide tiles; row blocks of 192 in rounds of eight (one per
    XCD), block id -> xcd = id % 8, slot = id / 8, row block (slot / groups) 8 + xcd, group slot % groups; the grid holds whole rounds."""
    tiles = N // 16
    nt = 18 if tiles % 18 == 0 else 8 if tiles % 8 == 0 else 4 if tiles % 4 == 0 else 2
    groups, rblocks = tiles // nt, _up(M, 192)
    rounds = _up(rblocks, 8)
    return {"nt": nt, "groups": groups, "chunks": _up(K, 32), "row_blocks": rblocks, "rounds": rounds, "grid": rounds * 8 * groups,
            "idle_blocks": (rounds * 8 - rblocks) * groups, "last_block_rows": M - (rblocks - 1) * 192}


def wgrad_dispatch(M: int, N: int, K: int, has_db: bool, flags: int = 0) -> str:
    """car_linear_wgrad: "bf16" (wgrad16_kernel), "tile35" (wgrad_tile_kernel<3, 5>, 192 x 320) or "tile22" (<2, 2>, 128 x 128)."""
    wide = N > 128 or K + (1 if has_db else 0) > 128
    if (wide or N * K >= 32 * 32) and M >= 2048 and not flags & WGRAD_FP32:
        return "bf16"
    return "tile35" if wide else "tile22"


def _slabs(M: int, slab: int, block: int, lookahead: int):
    gz = _up(M, slab)
    last = M - (gz - 1) * slab

    def whole(rows):                                                 # iterations m = 0, block, ... with m + lookahead block <= rows
        return (rows - lookahead * block) // block + 1 if rows >= lookahead * block else 0
    return {"slab": slab, "gz": gz, "last_slab_rows": last, "blocks_per_slab": _up(slab, block), "last_slab_blocks": _up(last, block),
            "last_block_rows": last - (_up(last, block) - 1) * block, "whole_iterations": whole(slab) if gz > 1 else whole(last),
            "whole_iterations_last_slab": whole(last)}


def wgrad_tile_launch(M: int, N: int, K: int, has_db: bool, kernel: str):
    """launch_wgrad_tile: ~512 workgroups wanted, slabs of at least four 16-row blocks, whole blocks."""
    WN, WK = (192, 320) if kernel == "tile35" else (128, 128)
    gx, gy = _up(N, WN), _up(K + (1 if has_db else 0), WK)
    want = max(1, 512 // (gx * gy))
    slab = _up(max(_up(M, want), 64), 16) * 16
    return dict(_slabs(M, slab, 16, 1), gx=gx, gy=gy)


def wgrad16_launch(M: int, N: int, K: int, has_db: bool):
    """launch_wgrad16: 256 workgroups wanted, slabs of whole 32-row blocks; an iteration is branch-free ("whole") while two further whole
    blocks follow it inside the slab: m + 3 x 32 <= m_end."""
    gx, gy = _up(N, 192), _up(K + (1 if has_db else 0), 320)
    want = max(1, 256 // (gx * gy))
    slab = _up(_up(M, want), 32) * 32
    return dict(_slabs(M, slab, 32, 3), gx=gx, gy=gy)


def wgrad_launch(M: int, N: int, K: int, has_db: bool, flags: int = 0):
    kernel = wgrad_dispatch(M, N, K, has_db, flags)
    facts = wgrad16_launch(M, N, K, has_db) if kernel == "bf16" else wgrad_tile_launch(M, N, K, has_db, kernel)
    return dict(facts, kernel=kernel)


def smallest_whole_block_rows(N: int, K: int, has_db: bool) -> int:
    """The fewest rows at which wgrad16_kernel runs a branch-free iteration: the slab must reach 96 rows."""
    gx, gy = _up(N, 192), _up(K + (1 if has_db else 0), 320)
    return max(2048, 64 * max(1, 256 // (gx * gy)) + 1)


# ---- input sets: every one a named function of a seed -----------------------------------------------------------------------------------------
def padded(t: torch.Tensor, ld: int) -> torch.Tensor:
    """t [M, K] inside rows of `ld` floats; the padding holds NaN, +inf, -inf in turn."""
    M, K = t.shape
    out = torch.empty(M, ld, dtype=F32)
    out[:, :K] = t
    if ld > K:
        pat = torch.tensor([NAN, INF, -INF])[(torch.arange(M)[:, None] + torch.arange(ld - K)[None, :]) % 3]
        out[:, K:] = pat
    return out.contiguous()


def weights(N: int, K: int, seed: int):
    g = gen(seed)
    return (torch.randn(N, K, generator=g) / max(K, 1) ** 0.5).contiguous(), 0.1 * torch.randn(N, generator=g)


def gauss(M: int, K: int, seed: int):
    return torch.randn(M, K, generator=gen(seed))


def span_rows(M: int, K: int, seed: int, lo: float = -6.0, hi: float = 4.0):
    """Gaussian rows whose scales run from 10^lo to 10^hi (both reached when M > 1)."""
    s = torch.logspace(lo, hi, M) if M > 1 else torch.ones(1)
    return torch.randn(M, K, generator=gen(seed)) * s[:, None]


def along_row(M: int, K: int, seed: int, grow: bool):
    """Magnitudes that grow (or shrink) 10^6-fold along every row."""
    s = torch.logspace(0, 6, K) if K > 1 else torch.ones(1)
    return torch.randn(M, K, generator=gen(seed)) * (s if grow else s.flip(0))[None, :]


def leading_zero(M: int, K: int, seed: int):
    """Row i starts with i % (chunks) all-zero 32-wide chunks, at least one where K > 32 and i > 0."""
    x = torch.randn(M, K, generator=gen(seed))
    chunks = _up(K, 32)
    for i in range(M):
        x[i, :32 * (i % chunks)] = 0
    return x


def zero_rows(M: int, K: int, seed: int):
    """Every other row all zero, the first included."""
    x = torch.randn(M, K, generator=gen(seed))
    x[0::2] = 0
    return x


def tiny_huge(M: int, K: int, seed: int):
    """Gaussian rows; row 0 scaled to largest magnitude 2^-40, row 1 (if any) to 2^40, exactly."""
    x = torch.randn(M, K, generator=gen(seed))
    for i, ex in ((0, -40), (1, 40)):
        if i < M:
            m = x[i].abs().max()
            x[i] = x[i] * (2.0 ** ex / m) if m > 0 else x[i]
            x[i, x[i].abs().argmax()] = 2.0 ** ex
    return x


def cancelling(M: int, K: int, N: int, seed: int):
    """(X, W, b): columns in pairs (x, -x (1 + 2^-10)) against equal weights, an odd last column zero, b = 0: the result is 2^-10 of a pair's
    product where the bound holds both in full."""
    g = gen(seed)
    half = K // 2
    a, w = torch.randn(M, max(half, 1), generator=g), torch.randn(N, max(half, 1), generator=g)
    X, W = torch.zeros(M, K), torch.zeros(N, K)
    if half:
        X[:, 0:2 * half:2], X[:, 1:2 * half:2] = a, -a * (1 + 2.0 ** -10)
        W[:, 0:2 * half:2], W[:, 1:2 * half:2] = w, w
    else:
        X[:, 0], W[:, 0] = a[:, 0], w[:, 0]
    return X, W, torch.zeros(N)


def integers(shape, seed: int, lo: int, hi: int):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def int_layer(M: int, K: int, N: int, seed: int, wide: str = ""):
    """(X, W, b, Y0): integers in [-3, 3]; wide == "x": X's non-zero entries carry 4096 on top (13 bits and more: lo(X) != 0 under the
    fp16 split); wide == "w": W's.  sum |terms| <= 3 x 4099 K + 3 + 7 < 2^24 for K <= 1364."""
    X, W = integers((M, K), seed, -3, 3), integers((N, K), seed + 1, -3, 3)
    if wide == "x":
        X = X + 4096 * X.sign()
    if wide == "w":
        W = W + 4096 * W.sign()
    return X, W, integers((N,), seed + 2, -3, 3), integers((M, N), seed + 3, -7, 7)


def int_wgrad(M: int, N: int, K: int, seed: int, wide: str, live_rows: int = 1024):
    """(dY, X, dW0, db0) of integers: the narrow operand in [-3, 3] (at most 2 significant bits: its lo is zero), the wide one
    +-(256 + 1..3) where not zero (9 bits and more: its bf16 lo is not zero); all but `live_rows` rows, spread evenly, are zero, so
    sum |terms| <= 3 x 259 x 1024 + 7 < 2^24 whatever M."""
    dY, X = integers((M, N), seed, -3, 3), integers((M, K), seed + 1, -3, 3)
    if wide == "dY":
        dY = dY + 256 * dY.sign()
    else:
        X = X + 256 * X.sign()
    if M > live_rows:
        keep = torch.zeros(M, dtype=torch.bool)
        keep[torch.linspace(0, M - 1, live_rows).long()] = True
        dY[~keep] = 0
        X[~keep] = 0
    return dY, X, integers((N, K), seed + 2, -7, 7), integers((N,), seed + 3, -7, 7)


def wgrad_rows(M: int, N: int, K: int, seed: int):
    """The twelve-orders-of-magnitude rows of tests/test_grad_hip.py, with constant columns: dY rows 1e-8 .. 1e4, X rows 1e3 .. 1e-6, the
    first min(8, K) columns of X the constant 1."""
    g = gen(seed)
    dY = torch.randn(M, N, generator=g) * torch.logspace(-8, 4, M)[:, None]
    X = torch.randn(M, K, generator=g) * torch.logspace(3, -6, M)[:, None]
    X[:, :min(8, K)] = 1.0
    return dY, X


def kq_params(Ce: int, seed: int) -> Dict[str, torch.Tensor]:
    """The chain's eight tensors; bk1 is negative throughout, so an all-zero row of e has k1 = relu(bk1) = 0 exactly."""
    g = gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"Wk1": (r(128, Ce) / Ce ** 0.5).contiguous(), "bk1": -0.1 * r(128).abs() - 0.01, "Wk2": (r(128, 128) / 128 ** 0.5).contiguous(), "bk2": 0.1 * r(128),
            "Wq1": (r(128, 16) / 4).contiguous(), "bq1": 0.1 * r(128), "Wq2": (r(128, 128) / 128 ** 0.5).contiguous(), "bq2": 0.1 * r(128)}


def kq_rows(M: int, Ce: int, seed: int):
    """(e [M, Ce], g [M, 16]): Gaussian; row 0 of e all zero (k1 negative throughout before the ReLU: bk1), the last row of g all zero (for M = 1
    both are row 0)."""
    gg = gen(seed)
    e, g = torch.randn(M, Ce, generator=gg), torch.randn(M, 16, generator=gg)
    e[0] = 0
    g[M - 1] = 0
    return e, g


# ---- the shapes the GPU tests run, chosen from the rules above; test_linear_reference.py asserts the path every one is named for -----------------------------
# car_linear: (M, K, N, ldx - K rounded up to 4): every N, K and M of the list once, every NT instance on a ragged M and a ragged K
LINEAR_SHAPES = ((1, 1, 3, 0), (31, 15, 5, 4), (33, 16, 32, 0), (127, 33, 64, 0), (128, 32, 96, 4), (129, 33, 130, 0), (257, 579, 160, 0),
                 (33, 576, 288, 0), (129, 579, 320, 4), (31, 31, 96, 8))
LINEAR_NT = {3: 1, 5: 1, 32: 1, 64: 2, 96: 4, 130: 4, 160: 4, 288: 9, 320: 9}
LINEAR_PHANTOM = {96: 1, 130: 3, 160: 3, 320: 8}
PACK_SHAPES = ((7, 5), (31, 32), (32, 64), (33, 96), (576, 320))        # (K, N)
# car_linear_x3: (M, K, N, extra ldx): the NT choice 2 (96, 160), 4 (64), 8 (128, 256: two groups), 18 (288, 576: two groups), 32 -> 2
X3_SHAPES = ((1, 1, 32, 0), (15, 31, 64, 0), (16, 32, 96, 4), (17, 33, 128, 0), (191, 100, 160, 0), (192, 579, 256, 8), (193, 33, 288, 0),
             (1537, 100, 576, 0), (1537, 31, 96, 4))
X3_NT = {32: (2, 1), 64: (4, 1), 96: (2, 3), 128: (8, 1), 160: (2, 5), 256: (8, 2), 288: (18, 1), 576: (18, 2)}
KQ_SHAPES = ((1, 96, 0), (17, 100, 0), (193, 288, 4), (17, 576, 0), (193, 864, 8), (1, 100, 4))           # (M, Ce, extra lde)
# car_linear_wgrad: name -> (M, N, K, db, relu, flags), the name the path test_linear_reference.py asserts
WGRAD_SHAPES = {
    "tile22-one-row": (1, 3, 16, True, False, 0), "tile22-partial-block": (15, 128, 16, False, True, 0), "tile22-one-block-K128": (16, 128, 128, False, False, 0),
    "tile35-K128-db": (17, 128, 128, True, False, 0), "tile35-N129": (63, 129, 16, True, True, 0), "tile35-bias-last-of-tile": (64, 192, 319, True, False, 0),
    "tile35-bias-alone": (65, 193, 320, True, True, 0), "tile35-tile-exact": (64, 384, 320, False, False, 0), "tile35-K579": (65, 3, 579, True, False, 0),
    "tile22-below-dispatch": (2047, 128, 16, True, False, 0), "bf16-at-dispatch": (2048, 128, 16, True, False, 0),
    "tile22-fp32-flag": (2048, 128, 16, True, False, WGRAD_FP32), "bf16-partial-block": (2049, 128, 16, False, True, 0),
    "bf16-short-last-slab": (2080, 384, 320, True, False, 0), "tile35-fp32-flag": (2080, 384, 320, True, False, WGRAD_FP32),
    "bf16-bias-last-of-tile": (2050, 192, 319, True, True, 0), "bf16-tile-exact": (2048, 192, 320, False, False, 0),
    "bf16-whole-multi-tile": (4130, 384, 579, True, True, 0), "bf16-whole-one-tile": (smallest_whole_block_rows(128, 16, True) + 37, 128, 16, True, False, 0),
}


# ---- the value sets by name, as both test files draw them -------------------------------------------------------------------------------------------
LINEAR_SETS = ("gauss", "span", "cancel", "int")
X3_SETS = ("gauss", "grow", "shrink", "lead0", "zero_rows", "tiny_huge", "int_x", "int_w")
WGRAD_SETS = ("gauss", "rows12", "const", "int_dY", "int_X")
LINEAR_SET_SHAPES = ((129, 33, 130), (257, 579, 160))                  # (M, K, N) the car_linear value sets run at
X3_SET_SHAPE = (193, 100, 128)
WGRAD_SET_SHAPES = ("tile22-below-dispatch", "tile35-bias-alone", "bf16-partial-block", "bf16-whole-multi-tile", "bf16-whole-one-tile")


@functools.lru_cache(maxsize=None)
def linear_set(name: str, M: int, K: int, N: int, seed: int = 1):
    """(X [M, K], W [N, K], b [N], Y0 [M, N]) of a car_linear / car_linear_x3 value set."""
    W, b = weights(N, K, seed + 100)
    Y0 = torch.randn(M, N, generator=gen(seed + 200))
    if name == "gauss":
        return gauss(M, K, seed), W, b, Y0
    if name == "span":
        return span_rows(M, K, seed), W, b, Y0
    if name == "cancel":
        X, W, b = cancelling(M, K, N, seed)
        return X, W, b, torch.zeros(M, N)
    if name == "grow" or name == "shrink":
        return along_row(M, K, seed, name == "grow"), W, b, Y0
    if name == "lead0":
        return leading_zero(M, K, seed), W, b, Y0
    if name == "zero_rows":
        return zero_rows(M, K, seed), W, b, Y0
    if name == "tiny_huge":
        return tiny_huge(M, K, seed), W, b, Y0
    if name in ("int", "int_x", "int_w"):
        return int_layer(M, K, N, seed, name[4:])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def wgrad_set(name: str, M: int, N: int, K: int, seed: int = 1):
    """(dY [M, N], X [M, K], dW0 [N, K], db0 [N]) of a car_linear_wgrad value set."""
    g = gen(seed + 300)
    dW0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    if name == "gauss":
        return gauss(M, N, seed), gauss(M, K, seed + 1), dW0, db0
    if name == "rows12":
        return wgrad_rows(M, N, K, seed) + (dW0, db0)
    if name == "const":
        dY, X = gauss(M, N, seed), gauss(M, K, seed + 1)
        dY[:, :min(4, N)] = 0.5
        X[:, :min(8, K)] = 1.0
        return dY, X, dW0, db0
    if name in ("int_dY", "int_X"):
        return int_wgrad(M, N, K, seed, name[4:])
    raise KeyError(name)
