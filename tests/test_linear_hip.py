"""The linear layers through the C ABI against tests/linear_reference.py: car_linear_packed_floats / car_linear_pack and car_linear
(csrc/car_linear.hip), car_linear_x3, car_linear_x3_masked and car_key_query_logits (csrc/car_linear16.hip), car_linear_wgrad's three
kernels (csrc/car_backward.hip), and the six entries' refusals.  No kernel is the expected value of any test here.

Tolerance, measured against the reference and never against a kernel: every element must be finite and satisfy |got - ref64| <= tol x
bound, the bound the float64 sum of magnitudes that goes with the value (linear_reference.py); where the bound is 0 the value must be
exactly 0.  tol = 8 x max(r, 2^-22) (parity_rule.tolerance), r the worst ratio of the kernel's yardstick on the same inputs: the
float32 run of the same formula for car_linear and the fp32-pipe weight-gradient kernels; for the split-fp16 entries the float32 run
decides and the three-product emulation's ratio is printed beside it; for the bf16 weight-gradient kernel the three-product bf16
emulation decides and the float32 run's ratio is printed beside it.  Integer sets are compared bit for bit.  Every test prints
ratio_kernel / tolerance as a ``[parity]`` line (profiles/linear_parity.md).

Every output lies inside a larger NaN-filled buffer; row padding of Y and dW and a guard row behind the last row must come back NaN,
bit for bit; the row padding of X, dY and e holds NaN and +-inf that must not reach an output.  test_linear_reference.py (CPU) asserts
that the shapes take the paths and the input sets hold the values they exist for."""
import functools

import pytest
import torch

import abi_harness as abi
import linear_reference as LR
from abi_harness import CAR_E_ARG, F32, F64, NAN, P_, Guarded, rows_out, take_rows
from parity_rule import judge

pytestmark = pytest.mark.gpu

FLAGS8 = list(range(8))
FLAG_IDS = ["plain", "relu_in", "relu_out", "relu_in+out", "accum", "relu_in+accum", "accum+relu_out", "all"]


def _judge(test, case, got, ref, bound, r, what="fp32", also=None):
    """One result held to the yardstick `what` of ratio r; `also`: {name: ratio} of a yardstick that is printed and decides nothing."""
    judge(test, case, {"": ((got, ref, bound), r)}, what=what, also=also)


def _exact(test, case, got, ref):
    assert torch.equal(abi.bits(got), abi.bits(ref.float())), (test, case, "not bit for bit", float((got.double() - ref).abs().max()))
    print(f"[parity] {test} {case}: exact")


# ---- car_linear_packed_floats, car_linear_pack ------------------------------------------------------------------------------------------------------
def _pack(lib, W, b, K, N, ldw=None):
    """car_linear_pack of W [N, ldw >= K] into a NaN-guarded buffer of car_linear_packed_floats floats."""
    n = lib.car_linear_packed_floats(K, N)
    assert n == LR.pack_geom(K, N)["floats"]
    packed = Guarded((n,))
    dW, db = W.to(abi.dev()).contiguous(), None if b is None else b.to(abi.dev())
    rc = lib.car_linear_pack(abi.ptr(dW), ldw or W.shape[1], abi.ptr(db), K, N, abi.ptr(packed.view), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return packed


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("K,N", LR.PACK_SHAPES)
def test_linear_pack_is_the_index_formula(K, N, bias):
    """The packed buffer bit for bit against linear_reference.packed_layout, ldw = K + 3 (the columns behind K are NaN and never read),
    with and without a bias; nothing written outside car_linear_packed_floats floats; sizes 0 give 0 floats."""
    lib = abi.lib()
    W, b = LR.weights(N, K, 40 + K)
    Wp = LR.padded(W, K + 3)
    packed = _pack(lib, Wp, b if bias else None, K, N, ldw=K + 3)
    want = LR.packed_layout(W, b if bias else None, K, N)
    got = packed.view.clone().cpu()
    assert torch.equal(abi.bits(got), abi.bits(want))
    packed.view.fill_(NAN)
    assert packed.untouched()
    assert lib.car_linear_packed_floats(0, N) == 0 and lib.car_linear_packed_floats(K, 0) == 0


# ---- car_linear ---------------------------------------------------------------------------------------------------------------------------------------
STORES = {"float4": (4, 0), "odd-ldy": (1, 0), "off-by-4-bytes": (4, 1)}       # name -> (ldy - N made a multiple of 4 or odd, floats off alignment)


def _ldy(N, store):
    step, _ = STORES[store]
    return abi.up4(N) + 4 if step == 4 else (N + 1) | 1


@functools.lru_cache(maxsize=None)
def _linear_reference(name, M, K, N, flags, seed=1):
    """(X, W, b, Y0, ref64, bound, r32) of a value set at a shape, computed once."""
    X, W, b, Y0 = LR.linear_set(name, M, K, N, seed)
    ref, bound = LR.layer(X, W, b, Y0, flags)
    y32, _ = LR.layer(X, W, b, Y0, flags, F32)
    return X, W, b, Y0, ref, bound, LR.ratio(y32, ref, bound)


def _run_linear(lib, X, ldx, W, b, Y0, flags, store):
    M, K, N = X.shape[0], W.shape[1], W.shape[0]
    packed = _pack(lib, W, b, K, N)
    dX = LR.padded(X, ldx).to(abi.dev())
    ldy = _ldy(N, store)
    out = rows_out(M, ldy, offset=STORES[store][1])
    if flags & LR.ACCUM:
        out.view[:M, :N] = Y0.to(abi.dev())
    rc = lib.car_linear(abi.ptr(dX), ldx, abi.ptr(packed.view), K, N, abi.ptr(out.view), ldy, M, flags, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return take_rows(out, M, N, "Y")


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("M,K,N,extra", LR.LINEAR_SHAPES)
def test_linear_shapes_match_fp64(M, K, N, extra, store):
    """car_linear on Gaussian rows at every tile instance (NT 1, 2, 4 with and without phantom tiles, 9), M 1 .. 257, K 1 .. 579 and 576 with
    ldx == K; each through the float4 store, the scalar store of an odd ldy and the scalar store of a Y four bytes off a 16-byte boundary.
    Flags alternate with the shape so that ACCUM | RELU_OUT meets every instance."""
    flags = (LR.ACCUM | LR.RELU_OUT) if (M + N) % 2 else LR.RELU_IN
    X, W, b, Y0, ref, bound, r32 = _linear_reference("gauss", M, K, N, flags)
    got = _run_linear(abi.lib(), X, abi.up4(K) + extra, W, b, Y0, flags, store)
    _judge("linear", f"gauss M={M} K={K} N={N} {store} flags={flags}", got, ref, bound, r32)


@pytest.mark.parametrize("glds", [0, LR.NO_GLDS], ids=["glds", "no_glds"])
@pytest.mark.parametrize("flags", FLAGS8, ids=FLAG_IDS)
@pytest.mark.parametrize("M,K,N", [(129, 33, 130), (33, 576, 288)])
def test_linear_flags_match_fp64(M, K, N, flags, glds):
    """All eight combinations of RELU_IN, RELU_OUT, ACCUM, each with the weights staged by LDS-DMA and through registers (CAR_LIN_NO_GLDS)."""
    X, W, b, Y0, ref, bound, r32 = _linear_reference("gauss", M, K, N, flags)
    got = _run_linear(abi.lib(), X, abi.up4(K), W, b, Y0, flags | glds, "float4")
    _judge("linear", f"flags M={M} K={K} N={N} flags={flags | glds}", got, ref, bound, r32)


@pytest.mark.parametrize("flags", [0, LR.ACCUM | LR.RELU_OUT], ids=["plain", "accum+relu_out"])
@pytest.mark.parametrize("name", LR.LINEAR_SETS)
@pytest.mark.parametrize("M,K,N", LR.LINEAR_SET_SHAPES)
def test_linear_value_sets_match_fp64(M, K, N, name, flags):
    """Gaussian rows, rows spanning 1e-6 .. 1e4, the cancelling set (results 2^-10 of their bound) and integers (bit for bit)."""
    X, W, b, Y0, ref, bound, r32 = _linear_reference(name, M, K, N, flags)
    got = _run_linear(abi.lib(), X, abi.up4(K) + 4, W, b, Y0, flags, "float4" if flags else "odd-ldy")
    if name == "int":
        _exact("linear", f"{name} M={M} K={K} N={N} flags={flags}", got, ref)
    else:
        _judge("linear", f"{name} M={M} K={K} N={N} flags={flags}", got, ref, bound, r32)


# ---- car_linear_x3, car_linear_x3_masked ------------------------------------------------------------------------------------------------------------------
def _pack_x3(lib, W, K, N):
    tiles = torch.empty(lib.car_linear_x3_packed_floats(K, N), device=abi.dev())
    dW = W.to(abi.dev()).contiguous()
    rc = lib.car_linear_x3_pack(abi.ptr(dW), K, K, N, abi.ptr(tiles), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return tiles


@functools.lru_cache(maxsize=None)
def _x3_reference(name, M, K, N, flags, bias, seed=1):
    """(X, W, b, Y0, ref64, bound, r32, r of the three-product emulation) of a value set at a shape, computed once."""
    X, W, b, Y0 = LR.linear_set(name, M, K, N, seed)
    b = b if bias else None
    ref, bound = LR.layer(X, W, b, Y0, flags)
    y32, _ = LR.layer(X, W, b, Y0, flags, F32)
    y3, _ = LR.layer(X, W, b, Y0, flags, F64, linear=LR.x3_linear)
    return X, W, b, Y0, ref, bound, LR.ratio(y32, ref, bound), LR.ratio(y3, ref, bound)


def _run_x3(lib, X, ldx, W, b, Y0, flags, act=None, lda=0):
    M, K, N = X.shape[0], W.shape[1], W.shape[0]
    tiles = _pack_x3(lib, W, K, N)
    dX, db = LR.padded(X, ldx).to(abi.dev()), None if b is None else b.to(abi.dev())
    ldy = N + 8
    out = rows_out(M, ldy)
    if flags & LR.ACCUM:
        out.view[:M, :N] = Y0.to(abi.dev())
    if act is None:
        rc = lib.car_linear_x3(abi.ptr(dX), ldx, abi.ptr(tiles), abi.ptr(db), K, N, abi.ptr(out.view), ldy, M, flags, abi.stream())
    else:
        dact = LR.padded(act, lda).to(abi.dev())
        rc = lib.car_linear_x3_masked(abi.ptr(dX), ldx, abi.ptr(tiles), abi.ptr(db), K, N, abi.ptr(out.view), ldy, M, flags, abi.ptr(dact), lda, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return take_rows(out, M, N, "Y")


def _judge_x3(test, case, got, ref, bound, r32, r3):
    """The float32 yardstick decides; the three-product emulation's ratio and the tolerance it would give are printed beside it."""
    _judge(test, case, got, ref, bound, r32, also={"x3-emulation": r3})


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,K,N,extra", LR.X3_SHAPES)
def test_linear_x3_shapes_match_fp64(M, K, N, extra, bias):
    """car_linear_x3 on Gaussian rows: column groups of NT 2, 4, 8 (one and two groups), 18 (one and two); M 1, 15 / 16 / 17, 191 / 192 / 193
    and 1537 = 8 x 192 + 1 (the second round of row blocks); K 1 .. 579 with ldx exactly K rounded up to 4 (NaN / inf in the one to three
    pad columns) and wider; with a bias and without."""
    flags = (LR.ACCUM | LR.RELU_OUT) if (M + K) % 2 else 0
    X, W, b, Y0, ref, bound, r32, r3 = _x3_reference("gauss", M, K, N, flags, bias)
    got = _run_x3(abi.lib(), X, abi.up4(K) + extra, W, b, Y0, flags)
    _judge_x3("linear_x3", f"gauss M={M} K={K} N={N} ldx={abi.up4(K) + extra} bias={bias} flags={flags}", got, ref, bound, r32, r3)


@pytest.mark.parametrize("flags", FLAGS8, ids=FLAG_IDS)
def test_linear_x3_flags_match_fp64(flags):
    M, K, N = 17, 33, 128
    X, W, b, Y0, ref, bound, r32, r3 = _x3_reference("gauss", M, K, N, flags, True)
    got = _run_x3(abi.lib(), X, abi.up4(K), W, b, Y0, flags)
    _judge_x3("linear_x3", f"flags M={M} K={K} N={N} flags={flags}", got, ref, bound, r32, r3)


@pytest.mark.parametrize("name", LR.X3_SETS)
def test_linear_x3_value_sets_match_fp64(name):
    """193 x 100 -> 128: magnitudes growing and shrinking 1e6-fold along the row (the row's power of two moves under the accumulators),
    rows whose leading chunks are zero (they start from the clamp), all-zero rows (output = the bias bit for bit, and exactly +0.0 without
    one), a row at largest magnitude 2^-40 and one at 2^40 without a bias, and the two integer sets (bit for bit: lo(X) != 0 in one,
    lo(W) != 0 in the other, so that each of the three products carries signal)."""
    M, K, N = LR.X3_SET_SHAPE
    lib = abi.lib()
    bias = name != "tiny_huge"
    for flags in (0, LR.ACCUM) if name.startswith("int") else (0,):
        X, W, b, Y0, ref, bound, r32, r3 = _x3_reference(name, M, K, N, flags, bias)
        got = _run_x3(lib, X, abi.up4(K), W, b, Y0, flags)
        if name.startswith("int"):
            _exact("linear_x3", f"{name} flags={flags}", got, ref)
        else:
            _judge_x3("linear_x3", f"{name} M={M} K={K} N={N}", got, ref, bound, r32, r3)
    if name == "zero_rows":
        assert torch.equal(abi.bits(got[0::2]), abi.bits(b[None, :].expand(len(got[0::2]), N))), "an all-zero row is not the bias bit for bit"
        X, W, _, Y0, ref, bound, r32, r3 = _x3_reference(name, M, K, N, 0, False)
        got = _run_x3(lib, X, abi.up4(K), W, None, Y0, 0)
        _judge_x3("linear_x3", f"{name} nobias", got, ref, bound, r32, r3)
        assert bool((abi.bits(got[0::2]) == 0).all()), "an all-zero row without a bias is not +0.0"


def mask_values(M: int, N: int, seed: int):
    """act [M, N]: Gaussian, with -0.0, +0.0, NaN, -inf, the smallest subnormal and the smallest normal float, 1e-30 and +inf sprinkled over every row."""
    act = torch.randn(M, N, generator=LR.gen(seed))
    special = torch.tensor([-0.0, 0.0, NAN, -float("inf"), 2.0 ** -149, 2.0 ** -126, 1e-30, float("inf")])
    idx = torch.randint(0, N, (M, len(special)), generator=LR.gen(seed + 1))
    act[torch.arange(M)[:, None], idx] = special[None, :].expand(M, -1)
    return act


@pytest.mark.parametrize("flags", [LR.ACCUM, LR.RELU_OUT], ids=["accum", "relu_out"])
@pytest.mark.parametrize("M", [17, 193])
@pytest.mark.parametrize("N", [32, 128, 576])
def test_linear_x3_masked_matches_fp64(N, M, flags):
    """car_linear_x3_masked against the same float64 layer: within tolerance where act > 0, exactly +0.0 elsewhere (act <= 0, -0.0, NaN); the smallest subnormal counts as positive;
    lda > N with poison behind the row."""
    K = 100
    X, W, b, Y0, ref, bound, r32, r3 = _x3_reference("gauss", M, K, N, flags, True)
    act = mask_values(M, N, 50 + N + M)
    keep = act > 0
    assert bool(keep.any()) and bool((~keep).any()) and bool(torch.isnan(act).any()) and bool((act == 2.0 ** -126).any()) and bool((abi.bits(act) == 1).any())
    got = _run_x3(abi.lib(), X, abi.up4(K), W, b, Y0, flags, act=act, lda=N + 4)
    assert bool((abi.bits(got)[~keep] == 0).all()), "a masked column is not +0.0"
    zero = torch.zeros_like(ref)
    _judge_x3("linear_x3_masked", f"M={M} N={N} flags={flags}", got, torch.where(keep, ref, zero), torch.where(keep, bound, zero), r32, r3)


# ---- car_key_query_logits ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kq_reference(M, Ce):
    P = LR.kq_params(Ce, 20 + Ce)
    e, g = LR.kq_rows(M, Ce, 30 + M)
    r64, r32, r3 = LR.kq_chain(e, g, P), LR.kq_chain(e, g, P, F32), LR.kq_chain(e, g, P, F64, linear=LR.x3_linear)
    yard = {k: (LR.ratio(r32[k], r64[k], r64["B_" + k]), LR.ratio(r3[k], r64[k], r64["B_" + k])) for k in ("qry", "logit")}
    return P, e, g, r64, yard


@pytest.mark.parametrize("M,Ce,extra", LR.KQ_SHAPES)
def test_key_query_logits_match_the_unfolded_chain(M, Ce, extra):
    """car_key_query_logits: qry and logit against kq_chain (unfolded, float64) at Ce 96, 100, 288, 576, 864, lde = Ce rounded up to 4 and
    wider (poison behind the row), M 1, 17, 193; row 0 of e is all zero — k1 = relu(bk1) is negative throughout before the ReLU, key must
    be bk2: the logit's bound holds |bk2| alone on the key side — and the last row of g is all zero."""
    lib = abi.lib()
    P, e, g, r64, yard = _kq_reference(M, Ce)
    d = {k: v.to(abi.dev()).contiguous() for k, v in P.items()}
    tiles = _pack_x3(lib, P["Wk1"], Ce, 128)
    tail = torch.empty(lib.car_kq_tail_floats(), device=abi.dev())
    tb = torch.empty(lib.car_kq_bias_floats(), device=abi.dev())
    rc = lib.car_kq_pack(abi.ptr(d["Wk2"]), abi.ptr(d["bk2"]), abi.ptr(d["Wq1"]), abi.ptr(d["bq1"]), abi.ptr(d["Wq2"]), abi.ptr(d["bq2"]), abi.ptr(tail), abi.ptr(tb), abi.stream())
    assert rc == 0, lib.car_last_error()
    lde = abi.up4(Ce) + extra
    de, dg = LR.padded(e, lde).to(abi.dev()), g.to(abi.dev()).contiguous()
    qry, logit = Guarded((M, 128)), Guarded((M,))
    rc = lib.car_key_query_logits(abi.ptr(de), lde, abi.ptr(tiles), abi.ptr(d["bk1"]), Ce, abi.ptr(dg), abi.ptr(tail), abi.ptr(tb), M, abi.ptr(qry.view), abi.ptr(logit.view), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    got = {"qry": qry.view.clone().cpu(), "logit": logit.view.clone().cpu()}
    qry.view.fill_(NAN)
    logit.view.fill_(NAN)
    assert qry.untouched() and logit.untouched(), "wrote outside qry / logit"
    for k in ("qry", "logit"):
        _judge_x3("key_query_logits", f"{k} M={M} Ce={Ce} lde={lde}", got[k], r64[k], r64["B_" + k], *yard[k])
    assert torch.equal(r64["B_key"][0], P["bk2"].double().abs())


# ---- car_linear_wgrad -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _wgrad_reference(name, case, prefill):
    """(dY, X, dW0, db0, refs, bounds, yardstick ratios) of a value set at a named shape, computed once."""
    M, N, K, has_db, relu, flags = LR.WGRAD_SHAPES[case]
    dY, X, dW0, db0 = LR.wgrad_set(name, M, N, K)
    if not prefill:
        dW0, db0 = torch.zeros_like(dW0), torch.zeros_like(db0)
    if not has_db:
        db0 = None
    dW, db, BW, Bb = LR.wgrad(dY, X, relu, dW0, db0)
    w32, b32, _, _ = LR.wgrad(dY, X, relu, dW0, db0, F32)
    r32 = max(LR.ratio(w32, dW, BW), LR.ratio(b32, db, Bb) if has_db else 0.0)
    r16 = None
    if LR.wgrad_dispatch(M, N, K, has_db, flags) == "bf16":
        w16, b16 = LR.wgrad_bf16(dY, X, relu, dW0, db0)
        r16 = max(LR.ratio(w16, dW, BW), LR.ratio(b16, db, Bb) if has_db else 0.0)
    return dY, X, dW0, db0, dW, db, BW, Bb, r32, r16


def _run_wgrad(lib, case, dY, X, dW0, db0):
    M, N, K, has_db, relu, flags = LR.WGRAD_SHAPES[case]
    ldy, ldx, lddw = abi.up4(N) + 4, abi.up4(K) + (4 if K % 4 == 0 else 0), K + 5
    ddY, dX = LR.padded(dY, ldy).to(abi.dev()), LR.padded(X, ldx).to(abi.dev())
    out = rows_out(N, lddw)
    out.view[:N, :K] = dW0.to(abi.dev())
    dbo = Guarded((N,))
    if has_db:
        dbo.view.copy_(db0.to(abi.dev()))
    rc = lib.car_linear_wgrad(abi.ptr(ddY), ldy, abi.ptr(dX), ldx, M, N, K, (LR.RELU_IN if relu else 0) | flags, abi.ptr(out.view), lddw, abi.ptr(dbo.view) if has_db else None, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    gb = dbo.view.clone().cpu() if has_db else None
    dbo.view.fill_(NAN)
    assert dbo.untouched(), "db: wrote outside its N floats" if has_db else "db is NULL and was written"
    return take_rows(out, N, K, "dW"), gb


def _check_wgrad(lib, name, case, prefill):
    M, N, K, has_db, relu, flags = LR.WGRAD_SHAPES[case]
    kernel = LR.wgrad_dispatch(M, N, K, has_db, flags)
    dY, X, dW0, db0, dW, db, BW, Bb, r32, r16 = _wgrad_reference(name, case, prefill)
    gW, gb = _run_wgrad(lib, case, dY, X, dW0, db0)
    tag = f"{name} {case} M={M} N={N} K={K} db={has_db} relu={relu} prefill={prefill}"
    if name.startswith("int"):
        _exact("linear_wgrad dW", tag, gW, dW)
        if has_db:
            _exact("linear_wgrad db", tag, gb, db)
        return
    r, what, also = (r16, "bf16-emulation", {"fp32": r32}) if kernel == "bf16" else (r32, "fp32", None)
    _judge("linear_wgrad dW", tag, gW, dW, BW, r, what, also)
    if has_db:
        _judge("linear_wgrad db", tag, gb, db, Bb, r, what, also)


@pytest.mark.parametrize("prefill", [True, False], ids=["accumulate", "zero"])
@pytest.mark.parametrize("case", list(LR.WGRAD_SHAPES))
def test_linear_wgrad_shapes_match_fp64(case, prefill):
    """car_linear_wgrad on Gaussian operands at every shape of linear_reference.WGRAD_SHAPES — the 128 x 128 and 192 x 320 tiles of the
    fp32 pipe (one row, a partial block, one block, the four-block slab and a row more, tile-exact N and K, the bias column last in a tile
    and alone in a new one, either side of the 2048-row dispatch, CAR_WGRAD_FP32) and the bf16 kernel (a one-block slab, a partial block, a
    short last slab, a whole-block iteration on four tiles with RELU_IN and on one tile without) — onto a pre-filled dW / db and onto zeros.
    dW has a row stride of K + 5: the padding and a guard row come back NaN."""
    M, N, K, has_db, relu, flags = LR.WGRAD_SHAPES[case]
    assert case.startswith(LR.wgrad_dispatch(M, N, K, has_db, flags))
    _check_wgrad(abi.lib(), "gauss", case, prefill)


@pytest.mark.parametrize("name", LR.WGRAD_SETS[1:])
@pytest.mark.parametrize("case", LR.WGRAD_SET_SHAPES)
def test_linear_wgrad_value_sets_match_fp64(case, name):
    """Rows spanning twelve orders of magnitude, constant columns (sums without cancellation) and the two integer sets (bit for bit:
    lo(dY) != 0 in one, lo(X) != 0 in the other; zero rows keep every sum below 2^24) on both fp32-pipe tiles and on the bf16 kernel's
    partial-block, four-tile whole-block and one-tile whole-block shapes."""
    _check_wgrad(abi.lib(), name, case, name != "int_X")


# ---- refusals: all return CAR_E_ARG before any launch, leave a message that starts with the entry's name and write nothing ----------------------------------
@functools.lru_cache(maxsize=None)
def _refusal_inputs():
    """Small valid arguments of every entry: M = 16 rows, K = 32, N = 32 (car_key_query_logits: Ce = 32)."""
    lib = abi.lib()
    M, K, N = 16, 32, 32
    z = lambda *shape: torch.zeros(*shape, device=abi.dev())
    W, b = LR.weights(N, K, 90)
    P = LR.kq_params(K, 91)
    d = {k: v.to(abi.dev()).contiguous() for k, v in P.items()}
    tail, tb = torch.empty(lib.car_kq_tail_floats(), device=abi.dev()), torch.empty(lib.car_kq_bias_floats(), device=abi.dev())
    assert lib.car_kq_pack(abi.ptr(d["Wk2"]), abi.ptr(d["bk2"]), abi.ptr(d["Wq1"]), abi.ptr(d["bq1"]), abi.ptr(d["Wq2"]), abi.ptr(d["bq2"]), abi.ptr(tail), abi.ptr(tb), abi.stream()) == 0
    t = {"W": W.to(abi.dev()), "b": torch.cat([b, torch.zeros(4)]).to(abi.dev()), "X": z(M + 1, K), "dY": z(M + 1, N), "act": z(M + 1, N + 32), "g": z(M + 1, 16),
         "packed": _pack(lib, W, b, K, N).view, "tiles": _pack_x3(lib, W, K, N), "tiles_k1": _pack_x3(lib, P["Wk1"], K, 128), "bk1": torch.cat([d["bk1"], z(4)]),
         "tail": tail, "tb": tb}
    torch.cuda.synchronize()
    return M, K, N, t


def _entry(name):
    """(function, ordered argument dict, outputs) of an entry, valid as it stands; the stream is appended by the caller."""
    lib = abi.lib()
    M, K, N, t = _refusal_inputs()
    if name == "car_linear_pack":
        out = {"packed": Guarded((lib.car_linear_packed_floats(K, N),))}
        a = dict(W=t["W"], ldw=K, bias=t["b"], K=K, N=N, packed=out["packed"])
    elif name == "car_linear":
        out = {"Y": Guarded((M + 1, N))}
        a = dict(X=t["X"], ldx=K, packed=t["packed"], K=K, N=N, Y=out["Y"], ldy=N, M=M, flags=0)
    elif name in ("car_linear_x3", "car_linear_x3_masked"):
        out = {"Y": Guarded((M + 1, N))}
        a = dict(X=t["X"], ldx=K, packed=t["tiles"], bias=t["b"], K=K, N=N, Y=out["Y"], ldy=N, M=M, flags=0)
        if name.endswith("masked"):
            a.update(act=t["act"], lda=N + 32)                              # wide enough for every N the cases pass: the shared checks are reached
    elif name == "car_key_query_logits":
        out = {"qry": Guarded((M + 1, 128)), "logit": Guarded((M,))}
        a = dict(e=t["X"], lde=K, packed_k1=t["tiles_k1"], bias_k1=t["bk1"], Ce=K, g=t["g"], tail=t["tail"], tail_bias=t["tb"], M=M, qry=out["qry"], logit=out["logit"])
    else:
        out = {"dW": Guarded((N + 1, K)), "db": Guarded((N,))}
        a = dict(dY=t["dY"], ldy=N, X=t["X"], ldx=K, M=M, N=N, K=K, flags=0, dW=out["dW"], lddw=K, db=out["db"])
    return getattr(lib, name), a, out


def _c(v):
    if isinstance(v, Guarded):
        return abi.ptr(v.view)
    if isinstance(v, torch.Tensor):
        return abi.ptr(v)
    return v


_NULLS = lambda names, msg: [(k, None, msg) for k in names]
_X3 = _NULLS(("X", "packed", "Y"), "bad arguments") + [("M", 0, "bad arguments"), ("K", 0, "bad arguments"), ("N", 0, "bad arguments"),
      ("N", 48, "multiple of 32"), ("N", 16, "multiple of 32"), ("ldx", 34, "multiple of 32"), ("ldy", 34, "multiple of 32"), ("ldx", 28, "multiple of 32"),
      ("K", 33, "multiple of 32"), ("ldy", 28, "multiple of 32"), ("X+4", None, "16-byte aligned"), ("Y+4", None, "16-byte aligned"), ("bias+4", None, "16-byte aligned")]
REFUSALS = {
    "car_linear_pack": _NULLS(("W", "packed"), "null pointer") + [("K", 0, "bad sizes"), ("N", 0, "bad sizes"), ("K", -1, "bad sizes"), ("ldw", 31, "bad sizes")],
    "car_linear": _NULLS(("X", "packed", "Y"), "null pointer") + [("K", 0, "bad sizes"), ("N", 0, "bad sizes"), ("M", 0, "bad sizes"), ("M", -1, "bad sizes"),
                  ("ldx", 28, "row stride"), ("ldx", 33, "row stride"), ("ldx", 34, "row stride"), ("X+4", None, "row stride"), ("ldy", 31, "ldy")],
    "car_linear_x3": _X3,
    "car_linear_x3_masked": _X3 + [("act", None, "act must be"), ("lda", 28, "act must be"), ("lda", 66, "act must be"), ("act+4", None, "act must be")],
    "car_key_query_logits": _NULLS(("e", "packed_k1", "bias_k1", "g", "tail", "tail_bias", "qry", "logit"), "null pointer") + [
        ("M", 0, "bad sizes"), ("Ce", 0, "bad sizes"), ("lde", 34, "bad sizes"), ("lde", 28, "bad sizes"), ("Ce", 33, "bad sizes"),
        ("e+4", None, "16-byte aligned"), ("g+4", None, "16-byte aligned"), ("qry+4", None, "16-byte aligned"), ("bias_k1+4", None, "16-byte aligned")],
    "car_linear_wgrad": _NULLS(("dY", "X", "dW"), "null pointer") + [("M", 0, "bad sizes"), ("N", 0, "bad sizes"), ("K", 0, "bad sizes"), ("ldy", 28, "bad sizes"),
                        ("ldx", 28, "bad sizes"), ("lddw", 31, "bad sizes"), ("ldy", 34, "multiples of 4"), ("ldx", 34, "multiples of 4"),
                        ("dY+4", None, "16-byte aligned"), ("X+4", None, "16-byte aligned")],
}
REFUSAL_CASES = [(e, f, v, msg) for e, cases in REFUSALS.items() for f, v, msg in cases]


@pytest.mark.parametrize("entry,field,value,message", REFUSAL_CASES, ids=[f"{e}-{f}-{i}" for i, (e, f, v, m) in enumerate(REFUSAL_CASES)])
def test_refusals(entry, field, value, message):
    """At least one call per CAR_REQUIRE the six entries can reach with small arguments, the alternatives of a compound condition one at a
    time: every NULL-able pointer, sizes 0 and below, each stride rule (too short; no multiple of 4), each alignment rule (the same buffer
    four bytes on), N no multiple of 32.  Each returns CAR_E_ARG before any launch, leaves a message that starts with the name of the entry
    that was called and writes nothing.  (Not reachable with arguments a test may pass: car_linear_wgrad's slab count and 32-bit block
    offset checks, profiles/linear_parity.md.)"""
    lib = abi.lib()
    fn, a, out = _entry(entry)
    if field.endswith("+4"):
        k = field[:-2]
        a[k] = P_((a[k].view if isinstance(a[k], Guarded) else a[k]).data_ptr() + 4)
    else:
        a[field] = value
    rc = fn(*[_c(v) for v in a.values()], abi.stream())
    assert rc == CAR_E_ARG, (entry, field, value, rc)
    msg = lib.car_last_error().decode()
    assert message in msg and msg.startswith(entry + ":"), msg
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values()), "a refused call wrote"
