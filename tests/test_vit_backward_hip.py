"""The backward of the encoder's transformer stage on the device, through the C ABI (include/car_encoder_train.h, csrc/car_vit_backward.hip
and the recorded forward of csrc/car_vit.hip): car_layernorm_backward, car_gelu_backward, car_mha_stats, car_mha_backward,
car_vit_pack_train / car_vit_blocks_train / car_vit_blocks_backward against the written-out float64 backward of
tests/vit_backward_reference.py (itself held to float64 autograd on the CPU) and, for the stage, against float64 autograd of
vit_reference.stage.  Every comparison is parity_rule.judge: kernel ratio <= 8 x max(yardstick ratio, 2^-22), the yardstick the same
formulas in float32 (for a weight gradient car_linear_wgrad sends to its bf16 kernel: linear_reference's emulation of that); no other
tolerance.  Buffers are abi_harness.Guarded: NaN in every margin and row padding, and whatever a kernel writes outside its output fails
the test."""
import functools

import pytest
import torch

import abi_harness as AH
import linear_reference as LR
import parity_rule as PRU
import vit_backward_reference as BR
import vit_reference as VR
from abi_harness import CAR_E_ARG, NAN, Guarded, P_, ptr, stream

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
INF = float("inf")
ACCUM, WGRAD_FP32 = 4, 16                                              # CAR_LIN_ACCUM, CAR_WGRAD_FP32


def lib():
    return AH.lib()


def sync():
    torch.cuda.synchronize()


def dev_t(t):
    return t.to(AH.dev()).contiguous()


def ok(rc):
    assert rc == 0, lib().car_last_error()


def nan_work(nbytes):
    return torch.full((max(nbytes, 4) // 4,), NAN, device=AH.dev())


def _yard(y32, ref, B, mask=None):
    return PRU.ratio(y32, ref, B, mask)


# ---- car_layernorm_backward ------------------------------------------------------------------------------------------------------------------
def run_ln_backward(x, g, dy, pad=4, flags=0, dx0=None, params=True, work=None):
    """-> (dx, dgamma, dbeta); x, dy and dx at ld = C + pad with NaN in the padding; the workspace starts as NaN."""
    M, C = x.shape
    X, DY = Guarded((M, C), ld=C + pad, init=x), Guarded((M, C), ld=C + pad, init=dy)
    DX = Guarded((M, C), ld=C + pad, init=dx0) if dx0 is not None else Guarded((M, C), ld=C + pad)
    G, DG, DB = dev_t(g), Guarded((C,)), Guarded((C,))
    nbytes = lib().car_layernorm_backward_workspace_bytes(M, C)
    W = nan_work(nbytes)
    wp, wb = (ptr(W), nbytes) if work is None else work
    ok(lib().car_layernorm_backward(X.ptr, C + pad, ptr(G), C, VR.EPS, DY.ptr, C + pad, DX.ptr, C + pad, M, flags, DG.ptr if params else None,
                                    DB.ptr if params else None, wp if params else None, wb if params else 0, stream()))
    sync()
    if not params:
        assert DG.untouched() and DB.untouched()
        return DX.get("car_layernorm_backward dx"), None, None
    return DX.get("car_layernorm_backward dx"), DG.get("car_layernorm_backward dgamma"), DB.get("car_layernorm_backward dbeta")


def _judge_ln(case, x, g, dy, got):
    (dx, Bx), (dg, Bg), (db, Bb) = BR.layernorm_backward(x, g, dy)
    (x32, _), (g32, _), (b32, _) = BR.layernorm_backward(x, g, dy, dtype=F32)
    PRU.judge("layernorm_backward", case, {"dx": ((got[0], dx, Bx), _yard(x32, dx, Bx)), "dgamma": ((got[1], dg, Bg), _yard(g32, dg, Bg)),
                                           "dbeta": ((got[2], db, Bb), _yard(b32, db, Bb))}, finite=True)


@pytest.mark.parametrize("C", VR.LN_CS)
@pytest.mark.parametrize("M", VR.LN_MS)
def test_layernorm_backward(M, C):
    """Gaussian rows over six orders of magnitude, ld = C + 4 with NaN in the padding; two runs are bit-identical."""
    x, g, _ = VR.ln_input("gauss", M, C)
    dy = BR.ln_dy(M, C)
    got = run_ln_backward(x, g, dy)
    _judge_ln(f"gauss M={M} C={C}", x, g, dy, got)
    again = run_ln_backward(x, g, dy)
    assert all(torch.equal(AH.bits(a), AH.bits(b)) for a, b in zip(got, again))


@pytest.mark.parametrize("M", BR.LN_SLAB_MS)
def test_layernorm_backward_on_both_sides_of_a_slab(M):
    x, g, _ = VR.ln_input("gauss", M, 64)
    dy = BR.ln_dy(M, 64)
    _judge_ln(f"slab M={M} C=64", x, g, dy, run_ln_backward(x, g, dy))


@pytest.mark.parametrize("M,C", [(3, 64), (65, 768)])
def test_layernorm_backward_constant_and_offset_rows(M, C):
    """A constant row has xhat = 0 and rstd = 1000: dx is finite and matches; a row of 1e4 + N(0, 1) does not cancel."""
    dy = BR.ln_dy(M, C)
    for name in ("const", "offset"):
        x, g, _ = VR.ln_input(name, M, C)
        _judge_ln(f"{name} M={M} C={C}", x, g, dy, run_ln_backward(x, g, dy))


def test_layernorm_backward_accumulates_and_skips_the_parameters():
    M, C = 65, 128
    x, g, _ = VR.ln_input("gauss", M, C)
    dy = BR.ln_dy(M, C)
    dx, dg, db = run_ln_backward(x, g, dy)
    dx0 = torch.randn(M, C, generator=PRU.gen(12))
    acc, dg2, db2 = run_ln_backward(x, g, dy, flags=ACCUM, dx0=dx0)
    assert torch.equal(AH.bits(acc), AH.bits(dx + dx0))                # one float32 addition of the written value
    assert torch.equal(AH.bits(dg2), AH.bits(dg)) and torch.equal(AH.bits(db2), AH.bits(db))
    only, none_g, none_b = run_ln_backward(x, g, dy, params=False)
    assert torch.equal(AH.bits(only), AH.bits(dx)) and none_g is None and none_b is None


# ---- car_gelu_backward ---------------------------------------------------------------------------------------------------------------------------
def run_gelu_backward(u, dy, pad=0):
    M, N = u.shape
    U, DY = Guarded((M, N), ld=N + pad, init=u), Guarded((M, N), ld=N + pad, init=dy)
    ok(lib().car_gelu_backward(U.ptr, N + pad, DY.ptr, N + pad, M, N, stream()))
    sync()
    assert torch.equal(AH.bits(U.get("car_gelu_backward u")), AH.bits(u))
    return DY.get("car_gelu_backward")


def test_gelu_backward_grid_and_special_values():
    u = VR.gelu_grid()[None, :]
    dy = torch.randn(u.shape, generator=PRU.gen(3))
    ref, B = BR.gelu_backward(u, dy)
    PRU.judge("gelu_backward", "grid [-12, 12]", {"": ((run_gelu_backward(u, dy), ref, B), _yard(BR.gelu_backward(u, dy, F32)[0], ref, B))}, finite=True)
    us, ds = torch.randn(37, 64, generator=PRU.gen(3)) * 3, torch.randn(37, 64, generator=PRU.gen(4))
    ref, B = BR.gelu_backward(us, ds)
    PRU.judge("gelu_backward", "rows 37 x 64, ld 72", {"": ((run_gelu_backward(us, ds, pad=8), ref, B), _yard(BR.gelu_backward(us, ds, F32)[0], ref, B))},
              finite=True)
    # +-0 give 1/2, a large u gives 1 exactly, a large negative u gives 0, +-inf give NaN (inf times 0), a NaN stays a NaN
    sp = torch.tensor([[0.0, -0.0, 40.0, -40.0, INF, -INF, NAN, 1.0]])
    got = run_gelu_backward(sp, torch.full_like(sp, 2.0))[0]
    assert got[:4].tolist() == [1.0, 1.0, 2.0, 0.0] and bool(torch.isnan(got[4:7]).all())
    assert abs(got[7].item() - 2.0 * BR.gelu_grad(sp)[0][0, 7].item()) < 1e-6


# ---- the recorded forward: car_mha_stats ---------------------------------------------------------------------------------------------------------
def run_mha(qkv, b, S, heads, stats=False, pad=4):
    """car_mha or car_mha_stats -> (out, stats [b, heads, S, 2] or None)."""
    dim = heads * VR.HEAD
    Q, O = Guarded((b * S, 3 * dim), ld=3 * dim + pad, init=qkv), Guarded((b * S, dim), ld=dim + pad)
    nbytes = lib().car_mha_workspace_bytes(b, S, heads)
    W = nan_work(nbytes)
    if not stats:
        ok(lib().car_mha(Q.ptr, 3 * dim + pad, b, S, heads, O.ptr, dim + pad, ptr(W), nbytes, stream()))
        sync()
        return O.get("car_mha"), None
    assert lib().car_mha_stats_floats(b, S, heads) == b * heads * S * 2
    St = Guarded((b, heads, S, 2))
    ok(lib().car_mha_stats(Q.ptr, 3 * dim + pad, b, S, heads, O.ptr, dim + pad, St.ptr, ptr(W), nbytes, stream()))
    sync()
    return O.get("car_mha_stats out"), St.get("car_mha_stats stats")


@pytest.mark.parametrize("b,S,heads", VR.MHA_SHAPES)
def test_mha_stats_leaves_the_output_alone_and_gives_the_log_sum_exp(b, S, heads):
    qkv = VR.mha_input("gauss", b, S, heads)
    plain, _ = run_mha(qkv, b, S, heads)
    out, st = run_mha(qkv, b, S, heads, stats=True)
    assert torch.equal(AH.bits(out), AH.bits(plain))
    assert bool(torch.isfinite(st).all()) and bool((st[..., 1] >= 1.0).all())          # the maximum's own term is exp(0) = 1
    # m + log l against the float64 log-sum-exp; bound: the largest magnitude sum of a row's logits, + 1 for the log of the sum of
    # weights (each in [0, 1], summed over at most 1024 keys); yardstick: the same in float32
    got = st[..., 0].double() + torch.log(st[..., 1].double())
    ref = BR.log_sum_exp(qkv, b, S, heads)
    q, k, _ = BR._split_qkv(qkv, b, S, heads, F64)
    B = (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1) / 8.0 + 1.0
    q32, k32, _ = BR._split_qkv(qkv, b, S, heads, F32)
    y32 = torch.logsumexp((q32 @ k32.transpose(-1, -2)) / 8.0, dim=-1)
    PRU.judge("mha_stats", f"gauss b={b} S={S} heads={heads}", {"lse": ((got, ref, B), _yard(y32, ref, B))})


# ---- car_mha_backward ----------------------------------------------------------------------------------------------------------------------------
def run_mha_backward(qkv, dout, b, S, heads, pad=4, work=None, what="car_mha_backward"):
    """The recorded forward, then the backward: every row buffer at ld = width + pad with NaN in the padding, in front of row 0 and behind
    row b S; dqkv guarded; the workspace starts as NaN.  -> dqkv [b S, 3 dim]"""
    dim = heads * VR.HEAD
    Q, O = Guarded((b * S, 3 * dim), ld=3 * dim + pad, init=qkv), Guarded((b * S, dim), ld=dim + pad)
    D, DQ = Guarded((b * S, dim), ld=dim + pad, init=dout), Guarded((b * S, 3 * dim), ld=3 * dim + pad)
    St = Guarded((b, heads, S, 2))
    fb = lib().car_mha_workspace_bytes(b, S, heads)
    FW = nan_work(fb)
    ok(lib().car_mha_stats(Q.ptr, 3 * dim + pad, b, S, heads, O.ptr, dim + pad, St.ptr, ptr(FW), fb, stream()))
    nbytes = lib().car_mha_backward_workspace_bytes(b, S, heads)
    W = nan_work(nbytes)
    wp, wb = (ptr(W), nbytes) if work is None else work
    ok(lib().car_mha_backward(Q.ptr, 3 * dim + pad, St.ptr, O.ptr, dim + pad, D.ptr, dim + pad, b, S, heads, DQ.ptr, 3 * dim + pad, wp, wb, stream()))
    sync()
    assert Q.margins_untouched() and O.margins_untouched() and D.margins_untouched() and St.margins_untouched()
    return DQ.get(what)


def _judge_mha_backward(name, b, S, heads, got):
    ref, B, y32 = BR.mha_backward_reference(name, b, S, heads)
    dim = heads * VR.HEAD
    part = lambda t, i: t[:, i * dim:(i + 1) * dim]
    PRU.judge("mha_backward", f"{name} b={b} S={S} heads={heads}",
              {n: ((part(got, i), part(ref, i), part(B, i)), _yard(part(y32, i), part(ref, i), part(B, i))) for i, n in enumerate(("dq", "dk", "dv"))},
              finite=True)


@pytest.mark.parametrize("b,S,heads", VR.MHA_SHAPES)
def test_mha_backward_shapes(b, S, heads):
    """N(0, 1) at the tile edges, the ragged last tile, one row and the three real lengths: dq, dk and dv each; two runs are bit-identical."""
    qkv, dout = VR.mha_input("gauss", b, S, heads), BR.mha_dout(b, S, heads)
    got = run_mha_backward(qkv, dout, b, S, heads)
    _judge_mha_backward("gauss", b, S, heads, got)
    assert torch.equal(AH.bits(run_mha_backward(qkv, dout, b, S, heads)), AH.bits(got))


@pytest.mark.parametrize("b,S,heads", VR.MHA_SET_SHAPES)
@pytest.mark.parametrize("name", [n for n in VR.MHA_SETS if n != "gauss"])
def test_mha_backward_value_sets(name, b, S, heads):
    got = run_mha_backward(VR.mha_input(name, b, S, heads), BR.mha_dout(b, S, heads), b, S, heads)
    _judge_mha_backward(name, b, S, heads, got)


def test_mha_backward_of_one_row_is_exact():
    """S = 1: the softmax is the constant 1, so dq = dk = 0 and dv = dout — exactly, on operands whose products the split arithmetic
    holds exactly (small integers, as test_vit_hip's uniform mean: fp16 hi + lo keeps 22 of float32's 24 bits, so dv = dout can not hold
    bit for bit for an arbitrary float32 dout).  The Gaussian row of MHA_SHAPES is judged by the rule in test_mha_backward_shapes."""
    for b, heads in ((1, 1), (3, 2)):
        qkv, dout = BR.mha_integers(b, 1, heads)
        dim = heads * VR.HEAD
        got = run_mha_backward(qkv, dout, b, 1, heads)
        assert not got[:, :2 * dim].any(), "dq, dk"
        assert torch.equal(AH.bits(got[:, 2 * dim:] + 0.0), AH.bits(dout + 0.0)), "dv"


@pytest.mark.parametrize("b,S,heads", [(2, 5, 2), (1, 257, 2)])
def test_mha_backward_of_a_zero_gradient_is_zero(b, S, heads):
    got = run_mha_backward(VR.mha_input("gauss", b, S, heads), torch.zeros(b * S, heads * VR.HEAD), b, S, heads)
    assert not got.any()


@pytest.mark.parametrize("S,heads", [(5, 2), (257, 2)])
def test_mha_backward_scene_is_independent_of_the_other_scenes(S, heads):
    qkv, dout = VR.mha_input("gauss", 2, S, heads), BR.mha_dout(2, S, heads)
    both = run_mha_backward(qkv, dout, 2, S, heads)
    oq, od = qkv.clone(), dout.clone()
    oq[S:] = 1e3 * torch.randn(S, qkv.shape[1], generator=PRU.gen(9))
    od[S:] = 1e-3 * torch.randn(S, dout.shape[1], generator=PRU.gen(10))
    assert torch.equal(AH.bits(run_mha_backward(oq, od, 2, S, heads)[:S]), AH.bits(both[:S]))
    assert torch.equal(AH.bits(run_mha_backward(qkv[:S].contiguous(), dout[:S].contiguous(), 1, S, heads)), AH.bits(both[:S]))
    assert torch.equal(AH.bits(run_mha_backward(qkv[S:].contiguous(), dout[S:].contiguous(), 1, S, heads)), AH.bits(both[S:]))


# ---- car_vit_pack_train / car_vit_blocks_train / car_vit_blocks_backward -------------------------------------------------------------------------
def _at(t, off_floats):
    return P_(t.data_ptr() + 4 * off_floats)


def _pack_train(params, dim, depth):
    dp = [dev_t(t) for t in params]
    packed = Guarded((lib().car_vit_packed_train_floats(dim, depth),), fill=0.0)
    ok(lib().car_vit_pack_train(AH.ptrs(dp), len(dp), dim, depth, packed.ptr, stream()))
    sync()
    assert packed.margins_untouched()
    return packed, dp


def test_vit_pack_train_starts_with_the_forward_pack_and_holds_the_transposes():
    dim, depth = 128, 2
    params = VR.seeded_stage(dim, depth)
    packed, dp = _pack_train(params, dim, depth)
    L, flat = lib(), packed.view
    n = L.car_vit_packed_floats(dim, depth)
    own = torch.zeros(n, device=AH.dev())
    ok(L.car_vit_pack(AH.ptrs(dp), len(dp), dim, depth, ptr(own), stream()))
    sync()
    assert torch.equal(AH.bits(flat[:n]), AH.bits(own))
    # a transposed record runs through car_linear_x3 as dX = dY W
    tr = [L.car_vit_packed_train_offset(dim, depth, i) for i in range(6)]
    for blk in range(depth):
        for t, item in enumerate((2, 4, 8, 10)):
            Wm = params[12 * blk + item]
            N, K = Wm.shape
            dY = torch.randn(37, N, generator=PRU.gen(4 + t))
            out = torch.empty(37, K, device=AH.dev())
            ok(L.car_linear_x3(ptr(dev_t(dY)), N, _at(flat, tr[5] + blk * tr[4] + tr[t]), None, N, K, ptr(out), K, 37, 0, stream()))
            sync()
            want, bound = dY.double() @ Wm.double(), dY.double().abs() @ Wm.double().abs()
            PRU.judge("vit_pack_train", f"block {blk} item {item}", {"": ((out.cpu(), want, bound), _yard(dY @ Wm, want, bound))})


def _blocks_train(tok0, b, S, dim, packed, depth, taps, saved=None, work=None):
    """car_vit_blocks_train -> (tok, [taps], the Guarded saved buffer)."""
    M = b * S
    T, outs = Guarded((M, dim), init=tok0), [Guarded((M, dim)) for _ in taps]
    sb, wb = lib().car_vit_saved_bytes(b, S, dim, depth), lib().car_vit_workspace_bytes(b, S, dim)
    Sv = Guarded((sb // 4,)) if saved is None else saved
    W = Guarded((wb // 4,)) if work is None else work
    ok(lib().car_vit_blocks_train(T.ptr, b, S, dim, packed.ptr, depth, AH.ints(taps), len(taps), AH.ptrs([o.view for o in outs]) if taps else None,
                                  Sv.ptr, Sv.view.numel() * 4, W.ptr, W.view.numel() * 4, stream()))
    sync()
    assert Sv.margins_untouched() and W.margins_untouched() and packed.margins_untouched()
    return T.get("car_vit_blocks_train tok"), [o.get(f"car_vit_blocks_train tap {i}") for i, o in enumerate(outs)], Sv


STAGE_CASES = [(128, 3, (1, 2), 2, 10), (128, 3, (1, 2), 1, 66), (768, 2, (0, 1), 1, 514)]


@pytest.mark.parametrize("dim,depth,taps,b,S", STAGE_CASES)
def test_vit_blocks_train_is_car_vit_blocks_bit_for_bit(dim, depth, taps, b, S):
    M = b * S
    packed, _ = _pack_train(VR.seeded_stage(dim, depth), dim, depth)
    tok0 = torch.randn(M, dim, generator=PRU.gen(dim + S))
    tok, tapped, _ = _blocks_train(tok0, b, S, dim, packed, depth, taps)
    T, outs = Guarded((M, dim), init=tok0), [Guarded((M, dim)) for _ in taps]
    wb = lib().car_vit_workspace_bytes(b, S, dim)
    W = Guarded((wb // 4,))
    ok(lib().car_vit_blocks(T.ptr, b, S, dim, packed.ptr, depth, AH.ints(taps), len(taps), AH.ptrs([o.view for o in outs]), W.ptr, wb, stream()))
    sync()
    assert torch.equal(AH.bits(T.get("car_vit_blocks tok")), AH.bits(tok))
    for i, o in enumerate(outs):
        assert torch.equal(AH.bits(o.get(f"car_vit_blocks tap {i}")), AH.bits(tapped[i])), i


def _grad_offsets(dim):
    return [lib().car_vit_grad_offset(dim, i) for i in range(13)]


def _blocks_backward(dim, depth, taps, b, S, packed, saved, dtaps, dout, flags, work=None):
    """car_vit_blocks_backward over a recorded forward -> (dtok, [the 12 depth parameter gradients in torch shapes])."""
    M, off = b * S, _grad_offsets(dim)
    DT = Guarded((M, dim), init=dout if dout is not None else torch.zeros(M, dim))
    dd = [None if d is None else dev_t(d) for d in dtaps]
    DP = Guarded((depth * off[12],), fill=0.0)
    wb = lib().car_vit_backward_workspace_bytes(b, S, dim)
    W = Guarded((wb // 4,)) if work is None else work
    ok(lib().car_vit_blocks_backward(DT.ptr, b, S, dim, packed.ptr, depth, AH.ints(taps), len(taps), AH.ptrs(dd), saved.ptr, saved.view.numel() * 4,
                                     DP.ptr, flags, W.ptr, W.view.numel() * 4, stream()))
    sync()
    assert W.margins_untouched() and saved.margins_untouched() and packed.margins_untouched()
    flat, params = DP.get("car_vit_blocks_backward dparams"), VR.seeded_stage(dim, depth)
    grads = [flat[(i // 12) * off[12] + off[i % 12]:][:params[i].numel()].reshape(params[i].shape) for i in range(12 * depth)]
    return DT.get("car_vit_blocks_backward dtok"), grads


@functools.lru_cache(maxsize=None)
def _stage_yardstick(dim, depth, taps, b, S):
    """The float32 run of the written-out backward, and the operands of its weight gradients: computed once per shape."""
    tok0, dtaps, dout, _, _ = BR.autograd_stage(dim, depth, taps, b, S)
    ops = {}
    y = BR.stage_backward(tok0, VR.seeded_stage(dim, depth), b, S, dim // VR.HEAD, taps, dtaps, dout, F32, ops)
    return y, ops


@pytest.mark.parametrize("flags", [0, WGRAD_FP32], ids=["wgrad-default", "wgrad-fp32"])
@pytest.mark.parametrize("dim,depth,taps,b,S", STAGE_CASES)
def test_vit_blocks_backward_matches_float64_autograd(dim, depth, taps, b, S, flags):
    """dtok and all 12 depth parameter gradients against float64 autograd of VR.stage, every tap and the output carrying a gradient."""
    params = VR.seeded_stage(dim, depth)
    tok0, dtaps, dout, a_tok, a_params = BR.autograd_stage(dim, depth, taps, b, S)
    packed, _ = _pack_train(params, dim, depth)
    _, _, saved = _blocks_train(tok0, b, S, dim, packed, depth, taps)
    dtok, grads = _blocks_backward(dim, depth, taps, b, S, packed, saved, dtaps, dout, flags)
    ((y_tok, _), y_params), ops = _stage_yardstick(dim, depth, taps, b, S)
    Bt = a_tok.abs().amax(dim=1, keepdim=True)
    entries = {"dtok": ((dtok, a_tok, Bt), _yard(y_tok, a_tok, Bt))}
    for i, (g, a, (y, _)) in enumerate(zip(grads, a_params, y_params)):
        B = torch.full((), float(a.abs().max()), dtype=F64)
        yard = {"fp32": _yard(y, a, B)}
        item, blk = i % 12, i // 12
        if item in (2, 4, 8, 10) and LR.wgrad_dispatch(b * S, a.shape[0], a.shape[1], True, flags) == "bf16":
            dY, X = next((dY, X) for it, dY, X in ops[blk] if it == item)
            yard = {"bf16": _yard(LR.wgrad_bf16(dY, X, False, torch.zeros(a.shape), None)[0], a, B)}
        entries[f"b{blk}.{VR.PARAM_ORDER[item]}"] = ((g, a, B), yard)
    PRU.judge("vit_blocks_backward", f"dim={dim} depth={depth} b={b} S={S} flags={flags}", entries, finite=True)


def _stage_entries_backward(tok0, b, S, dim, packed, depth, taps, dtaps, dout):
    """The sequence car_vit_blocks_backward documents, issued entry by entry over a forward issued entry by entry -> dtok."""
    L, M, heads, st, d = lib(), b * S, dim // VR.HEAD, stream(), AH.dev()
    off = [L.car_vit_packed_offset(dim, i) for i in range(13)]
    tr = [L.car_vit_packed_train_offset(dim, depth, i) for i in range(6)]
    go = _grad_offsets(dim)
    E = lambda *s: torch.empty(*s, device=d)
    fb, bb, lb = L.car_mha_workspace_bytes(b, S, heads), L.car_mha_backward_workspace_bytes(b, S, heads), L.car_layernorm_backward_workspace_bytes(M, dim)
    FW, BW, LW = E(fb // 4), E(bb // 4), E(lb // 4)
    tok, rec = dev_t(tok0), []
    norm, wide = E(M, dim), E(M, 4 * dim)
    pk = packed.view
    for blk in range(depth):
        p = lambda i: _at(pk, blk * off[12] + off[i])
        x0, qkv, att, stt, u = tok.clone(), E(M, 3 * dim), E(M, dim), E(b * heads * S * 2), E(M, 4 * dim)
        ok(L.car_layernorm(ptr(tok), dim, p(0), p(1), dim, VR.EPS, ptr(norm), dim, M, st))
        ok(L.car_linear_x3(ptr(norm), dim, p(2), p(3), dim, 3 * dim, ptr(qkv), 3 * dim, M, 0, st))
        ok(L.car_mha_stats(ptr(qkv), 3 * dim, b, S, heads, ptr(att), dim, ptr(stt), ptr(FW), fb, st))
        ok(L.car_linear_x3(ptr(att), dim, p(4), p(5), dim, dim, ptr(tok), dim, M, ACCUM, st))
        x1 = tok.clone()
        ok(L.car_layernorm(ptr(tok), dim, p(6), p(7), dim, VR.EPS, ptr(norm), dim, M, st))
        ok(L.car_linear_x3(ptr(norm), dim, p(8), p(9), dim, 4 * dim, ptr(u), 4 * dim, M, 0, st))
        wide.copy_(u)
        ok(L.car_gelu(ptr(wide), 4 * dim, M, 4 * dim, st))
        ok(L.car_linear_x3(ptr(wide), 4 * dim, p(10), p(11), 4 * dim, dim, ptr(tok), dim, M, ACCUM, st))
        rec.append((x0, qkv, att, stt, x1, u))
    g = dev_t(dout if dout is not None else torch.zeros(M, dim))
    small, dwide, dp = E(M, dim), E(M, 4 * dim), torch.zeros(go[12], device=d)
    for blk in reversed(range(depth)):
        p = lambda i: _at(pk, blk * off[12] + off[i])
        pt = lambda t: _at(pk, tr[5] + blk * tr[4] + tr[t])
        gp = lambda i: _at(dp, go[i])
        x0, qkv, att, stt, x1, u = rec[blk]
        if blk in taps and dtaps[taps.index(blk)] is not None:
            ok(L.car_add(ptr(g), dim, ptr(g), dim, 1.0, ptr(dev_t(dtaps[taps.index(blk)])), dim, 1.0, M, dim, st))
        ok(L.car_layernorm(ptr(x1), dim, p(6), p(7), dim, VR.EPS, ptr(norm), dim, M, st))
        wide.copy_(u)
        ok(L.car_gelu(ptr(wide), 4 * dim, M, 4 * dim, st))
        ok(L.car_linear_wgrad(ptr(g), dim, ptr(wide), 4 * dim, M, dim, 4 * dim, 0, gp(10), 4 * dim, gp(11), st))
        ok(L.car_linear_x3(ptr(g), dim, pt(3), None, dim, 4 * dim, ptr(dwide), 4 * dim, M, 0, st))
        ok(L.car_gelu_backward(ptr(u), 4 * dim, ptr(dwide), 4 * dim, M, 4 * dim, st))
        ok(L.car_linear_wgrad(ptr(dwide), 4 * dim, ptr(norm), dim, M, 4 * dim, dim, 0, gp(8), dim, gp(9), st))
        ok(L.car_linear_x3(ptr(dwide), 4 * dim, pt(2), None, 4 * dim, dim, ptr(small), dim, M, 0, st))
        ok(L.car_layernorm_backward(ptr(x1), dim, p(6), dim, VR.EPS, ptr(small), dim, ptr(g), dim, M, ACCUM, gp(6), gp(7), ptr(LW), lb, st))
        ok(L.car_linear_wgrad(ptr(g), dim, ptr(att), dim, M, dim, dim, 0, gp(4), dim, gp(5), st))
        ok(L.car_linear_x3(ptr(g), dim, pt(1), None, dim, dim, ptr(small), dim, M, 0, st))
        ok(L.car_mha_backward(ptr(qkv), 3 * dim, ptr(stt), ptr(att), dim, ptr(small), dim, b, S, heads, ptr(dwide), 3 * dim, ptr(BW), bb, st))
        ok(L.car_layernorm(ptr(x0), dim, p(0), p(1), dim, VR.EPS, ptr(norm), dim, M, st))
        ok(L.car_linear_wgrad(ptr(dwide), 3 * dim, ptr(norm), dim, M, 3 * dim, dim, 0, gp(2), dim, gp(3), st))
        ok(L.car_linear_x3(ptr(dwide), 3 * dim, pt(0), None, 3 * dim, dim, ptr(small), dim, M, 0, st))
        ok(L.car_layernorm_backward(ptr(x0), dim, p(0), dim, VR.EPS, ptr(small), dim, ptr(g), dim, M, ACCUM, gp(0), gp(1), ptr(LW), lb, st))
    sync()
    return g.cpu()


@pytest.mark.parametrize("dim,depth,taps,b,S", STAGE_CASES)
def test_vit_blocks_backward_is_the_sequence_of_stage_entries_bit_for_bit(dim, depth, taps, b, S):
    """dtok of the one call against the documented sequence issued entry by entry; and two runs of the one call give the same dtok and
    the same LayerNorm gradients bit for bit (the matrices' gradients go through car_linear_wgrad's atomics and need not)."""
    params = VR.seeded_stage(dim, depth)
    tok0, dtaps, dout, _, _ = BR.autograd_stage(dim, depth, taps, b, S)
    packed, _ = _pack_train(params, dim, depth)
    _, _, saved = _blocks_train(tok0, b, S, dim, packed, depth, taps)
    dtok, grads = _blocks_backward(dim, depth, taps, b, S, packed, saved, dtaps, dout, 0)
    assert torch.equal(AH.bits(_stage_entries_backward(tok0, b, S, dim, packed, depth, taps, dtaps, dout)), AH.bits(dtok))
    again, grads2 = _blocks_backward(dim, depth, taps, b, S, packed, saved, dtaps, dout, 0)
    assert torch.equal(AH.bits(again), AH.bits(dtok))
    for i in range(12 * depth):
        if i % 12 in (0, 1, 6, 7):
            assert torch.equal(AH.bits(grads2[i]), AH.bits(grads[i])), i


def test_a_tap_gradient_joins_the_stream_where_the_tap_was_taken():
    """A gradient at tap 1 alone: block 2's parameter gradients are exactly zero; at tap 2 alone: every block's are non-zero."""
    dim, depth, taps, b, S = 128, 3, (1, 2), 2, 10
    packed, _ = _pack_train(VR.seeded_stage(dim, depth), dim, depth)
    for which in ("tap1", "tap2"):
        tok0, dtaps, dout, a_tok, _ = BR.autograd_stage(dim, depth, taps, b, S, which)
        _, _, saved = _blocks_train(tok0, b, S, dim, packed, depth, taps)
        dtok, grads = _blocks_backward(dim, depth, taps, b, S, packed, saved, dtaps, dout, 0)
        nonzero = [bool(g.any()) for g in grads]
        if which == "tap1":
            assert not any(nonzero[24:]) and all(nonzero[:24])
        else:
            assert all(nonzero)
        Bt = a_tok.abs().amax(dim=1, keepdim=True)
        assert PRU.ratio(dtok, a_tok, Bt) <= 2.0 ** -16                 # the right gradient (its parity is the test above's business)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
def test_the_backward_fits_its_workspaces_and_the_saved_buffer_exactly():
    """Each over a buffer of exactly its size entry's bytes with NaN all around it, then over one twice as large: nothing is written
    outside either, the outputs are the same bytes, and the last float of the exact one was written (the layouts end in a used piece)."""
    last = {}

    def keep(name, fn):
        def run(w, wb):
            out = fn(w, wb)
            sync()
            last.setdefault(name, bool(torch.isfinite(w.view[-1])))
            return out
        return run

    qkv, dout = VR.mha_input("gauss", 2, 33, 1), BR.mha_dout(2, 33, 1)
    AH.exact_then_twice(lib().car_mha_backward_workspace_bytes(2, 33, 1), keep("mha", lambda w, wb: (run_mha_backward(qkv, dout, 2, 33, 1, work=(w.ptr, wb)),)),
                        "car_mha_backward")
    x, g, _ = VR.ln_input("gauss", 65, 64)
    dy = BR.ln_dy(65, 64)
    AH.exact_then_twice(lib().car_layernorm_backward_workspace_bytes(65, 64), keep("ln", lambda w, wb: run_ln_backward(x, g, dy, work=(w.ptr, wb))),
                        "car_layernorm_backward")
    # b S heads 2 = 2112 floats of statistics: whole 64s, so the saved buffer's last float is a statistic
    dim, depth, b, S = 64, 2, 32, 33
    packed, _ = _pack_train(VR.seeded_stage(dim, depth), dim, depth)
    tok0 = torch.randn(b * S, dim, generator=PRU.gen(dim + S))
    dtap = torch.randn(b * S, dim, generator=PRU.gen(5))
    saved_ok = {}

    def forward(sv, sb):
        tok, tapped, _ = _blocks_train(tok0, b, S, dim, packed, depth, (1,), saved=sv)
        saved_ok["sv"] = sv
        return tok, tapped[0]

    AH.exact_then_twice(lib().car_vit_saved_bytes(b, S, dim, depth), keep("saved", forward), "car_vit_blocks_train (saved)")
    saved = saved_ok["sv"]                                              # the larger one: the layout is the same, from its start

    def backward(w, wb):
        dtok, grads = _blocks_backward(dim, depth, (1,), b, S, packed, saved, [dtap], None, WGRAD_FP32, work=w)
        return dtok, grads[0], grads[1], grads[6], grads[7]             # the bit-reproducible ones

    AH.exact_then_twice(lib().car_vit_backward_workspace_bytes(b, S, dim), keep("vit", backward), "car_vit_blocks_backward")
    assert last == {"mha": True, "ln": True, "saved": True, "vit": True}, last


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_car_e_arg_and_launch_nothing():
    L, st = lib(), stream()
    dim, heads, b, S, M = 128, 2, 1, 5, 5
    X, Q, O = Guarded((M, dim), fill=1.0), Guarded((M, 3 * dim), fill=1.0), Guarded((M, dim), fill=1.0)
    St = Guarded((b, heads, S, 2), fill=1.0)
    Y, DQ, DG = Guarded((M, 4 * dim)), Guarded((M, 3 * dim)), Guarded((dim,))
    g = dev_t(torch.ones(dim))
    mb, lb = L.car_mha_backward_workspace_bytes(b, S, heads), L.car_layernorm_backward_workspace_bytes(M, dim)
    vb, fb, sb = L.car_vit_backward_workspace_bytes(b, S, dim), L.car_vit_workspace_bytes(b, S, dim), L.car_vit_saved_bytes(b, S, dim, 3)
    W = Guarded((max(mb, lb, vb, fb, L.car_mha_workspace_bytes(b, S, heads)) // 4,))
    Sv = Guarded((sb // 4,))
    params = [dev_t(t) for t in VR.seeded_stage(dim, 1)]
    packed = Guarded((L.car_vit_packed_train_floats(dim, 3),))
    DP = Guarded((3 * L.car_vit_grad_offset(dim, 12),))
    tap = Guarded((M, dim))
    off16 = lambda G_: P_(G_.view.data_ptr() + 4)                       # 4 bytes off a 16-byte boundary
    ln = lambda x=X.ptr, ldx=dim, C=dim, dy=O.ptr, dx=Y.ptr, lddx=dim, fl=0, dg=DG.ptr, db=DG.ptr, w=W.ptr, wb=lb: \
        L.car_layernorm_backward(x, ldx, ptr(g), C, 1e-6, dy, dim, dx, lddx, M, fl, dg, db, w, wb, st)
    mha = lambda q=Q.ptr, ld=3 * dim, s_=St.ptr, o=O.ptr, d=X.ptr, ldd=dim, S_=S, h=heads, dq=DQ.ptr, lddq=3 * dim, w=W.ptr, wb=mb: \
        L.car_mha_backward(q, ld, s_, o, dim, d, ldd, b, S_, h, dq, lddq, w, wb, st)
    train = lambda t=Y.ptr, S_=S, d_=dim, depth=1, taps=None, n=0, outs=None, sv=Sv.ptr, sb_=sb, w=W.ptr, wb=fb: \
        L.car_vit_blocks_train(t, b, S_, d_, packed.ptr, depth, taps, n, outs, sv, sb_, w, wb, st)
    back = lambda t=Y.ptr, S_=S, d_=dim, depth=1, taps=None, n=0, dts=None, sv=Sv.ptr, sb_=sb, dp=DP.ptr, fl=0, w=W.ptr, wb=vb: \
        L.car_vit_blocks_backward(t, b, S_, d_, packed.ptr, depth, taps, n, dts, sv, sb_, dp, fl, w, wb, st)
    calls = {
        "ln null": lambda: ln(x=None), "ln null dX": lambda: ln(dx=None), "ln one of dgamma, dbeta": lambda: ln(db=None),
        "ln null work": lambda: ln(w=None), "ln C": lambda: ln(C=6), "ln C big": lambda: ln(C=4100), "ln stride below": lambda: ln(lddx=dim - 4),
        "ln stride % 4": lambda: ln(ldx=dim + 2), "ln flags": lambda: ln(fl=1), "ln aligned": lambda: ln(dx=off16(Y)), "ln workspace": lambda: ln(wb=lb - 1),
        "gelu null": lambda: L.car_gelu_backward(None, dim, Y.ptr, dim, M, dim, st),
        "gelu stride below": lambda: L.car_gelu_backward(X.ptr, dim, Y.ptr, dim - 4, M, dim, st),
        "gelu stride % 4": lambda: L.car_gelu_backward(X.ptr, dim + 2, Y.ptr, dim, M, dim, st),
        "gelu N % 4": lambda: L.car_gelu_backward(X.ptr, dim, Y.ptr, dim, M, 6, st),
        "gelu aligned": lambda: L.car_gelu_backward(X.ptr, dim, off16(Y), dim, M, dim, st),
        "stats null": lambda: L.car_mha_stats(Q.ptr, 3 * dim, b, S, heads, Y.ptr, dim, None, W.ptr, mb, st),
        "stats S 0": lambda: L.car_mha_stats(Q.ptr, 3 * dim, b, 0, heads, Y.ptr, dim, DQ.ptr, W.ptr, mb, st),
        "stats aligned": lambda: L.car_mha_stats(Q.ptr, 3 * dim, b, S, heads, Y.ptr, dim, off16(DQ), W.ptr, mb, st),
        "stats workspace": lambda: L.car_mha_stats(Q.ptr, 3 * dim, b, S, heads, Y.ptr, dim, DQ.ptr, W.ptr, 16, st),
        "mha null": lambda: mha(q=None), "mha null stats": lambda: mha(s_=None), "mha null dout": lambda: mha(d=None), "mha null dqkv": lambda: mha(dq=None),
        "mha S 0": lambda: mha(S_=0), "mha S 1025": lambda: mha(S_=1025, wb=1 << 40), "mha heads 0": lambda: mha(h=0),
        "mha heads 17": lambda: mha(h=17, ld=3 * 17 * 64, lddq=3 * 17 * 64, ldd=17 * 64, wb=1 << 40),
        "mha stride below": lambda: mha(ld=3 * dim - 4), "mha stride % 4": lambda: mha(lddq=3 * dim + 2), "mha dout stride below": lambda: mha(ldd=dim - 4),
        "mha aligned": lambda: mha(dq=off16(DQ)), "mha work aligned": lambda: mha(w=off16(W)), "mha workspace": lambda: mha(wb=mb - 1),
        "pack null": lambda: L.car_vit_pack_train(AH.ptrs(params), 12, dim, 1, None, st),
        "pack null parameter": lambda: L.car_vit_pack_train(AH.ptrs(params[:11] + [None]), 12, dim, 1, packed.ptr, st),
        "pack dim": lambda: L.car_vit_pack_train(AH.ptrs(params), 12, 96, 1, packed.ptr, st),
        "pack depth 33": lambda: L.car_vit_pack_train(AH.ptrs(params), 12 * 33, dim, 33, packed.ptr, st),
        "pack count": lambda: L.car_vit_pack_train(AH.ptrs(params), 11, dim, 1, packed.ptr, st),
        "pack aligned": lambda: L.car_vit_pack_train(AH.ptrs(params), 12, dim, 1, off16(packed), st),
        "train null": lambda: train(t=None), "train null saved": lambda: train(sv=None), "train S": lambda: train(S_=1025, wb=1 << 40, sb_=1 << 40),
        "train dim": lambda: train(d_=96), "train depth": lambda: train(depth=0), "train saved short": lambda: train(depth=3, sb_=sb - 1),
        "train tap >= depth": lambda: train(taps=AH.ints([1]), n=1, outs=AH.ptrs([tap.view])),
        "train taps not increasing": lambda: train(depth=3, taps=AH.ints([1, 1]), n=2, outs=AH.ptrs([tap.view, tap.view])),
        "train aligned": lambda: train(sv=off16(Sv)), "train workspace": lambda: train(wb=fb - 1),
        "back null": lambda: back(t=None), "back null saved": lambda: back(sv=None), "back null dparams": lambda: back(dp=None),
        "back null dtaps": lambda: back(taps=AH.ints([0]), n=1, dts=None), "back S": lambda: back(S_=1025, wb=1 << 40, sb_=1 << 40),
        "back dim": lambda: back(d_=96), "back dim big": lambda: back(d_=1088, wb=1 << 40, sb_=1 << 40), "back depth 33": lambda: back(depth=33, sb_=1 << 40),
        "back saved short": lambda: back(depth=3, sb_=sb - 1), "back tap >= depth": lambda: back(taps=AH.ints([1]), n=1, dts=AH.ptrs([tap.view])),
        "back taps not increasing": lambda: back(depth=3, taps=AH.ints([2, 1]), n=2, dts=AH.ptrs([tap.view, tap.view])),
        "back flags": lambda: back(fl=4), "back aligned": lambda: back(dp=off16(DP)), "back work aligned": lambda: back(w=off16(W)),
        "back workspace": lambda: back(wb=vb - 1),
    }
    before = [t.full.clone() for t in (X, Q, O, St)]
    for name, call in calls.items():
        assert call() == CAR_E_ARG, name
        msg = L.car_last_error()
        assert msg and msg.decode().startswith("car_"), (name, msg)
    sync()
    for G_ in (Y, DQ, DG, W, Sv, packed, DP, tap):
        assert G_.untouched(), "a refused call wrote something"
    for t, was in zip((X, Q, O, St), before):
        assert torch.equal(AH.bits(t.full), AH.bits(was))
