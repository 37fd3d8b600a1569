"""The encoder's transformer stage on the device, through the C ABI (include/car_encoder.h, csrc/car_vit.hip): car_layernorm, car_gelu,
car_mha, car_vit_pack / car_vit_blocks against the float64 restatement of tests/vit_reference.py, and get_z with encoder_route = "device"
against the fixtures the reference wrote.  Every comparison of a kernel is parity_rule.judge: kernel ratio <= 8 x max(yardstick ratio,
2^-22), the yardstick the same formulas in float32; no other tolerance.  Buffers are abi_harness.Guarded: NaN in every margin and row
padding, and whatever a kernel writes outside its output fails the test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_harness as AH
import parity_rule as PRU
import vit_reference as VR
from abi_harness import CAR_E_ARG, NAN, Guarded, P_, ptr, stream

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
INF = float("inf")


def lib():
    return AH.lib()


def sync():
    torch.cuda.synchronize()


def dev_t(t):
    return t.to(AH.dev()).contiguous()


def _yard(y32, ref, B):
    return PRU.ratio(y32, ref, B)


# ---- car_layernorm ---------------------------------------------------------------------------------------------------------------------------
def run_layernorm(x, g, b, pad=4, eps=VR.EPS):
    M, C = x.shape
    X, Y = Guarded((M, C), ld=C + pad, init=x), Guarded((M, C), ld=C + pad)
    G, Bt = dev_t(g), dev_t(b)
    assert lib().car_layernorm(X.ptr, C + pad, ptr(G), ptr(Bt), C, eps, Y.ptr, C + pad, M, stream()) == 0, lib().car_last_error()
    sync()
    return Y.get("car_layernorm")


@pytest.mark.parametrize("C", VR.LN_CS)
@pytest.mark.parametrize("M", VR.LN_MS)
def test_layernorm(M, C):
    """Gaussian rows over six orders of magnitude, ld = C + 4 with NaN in the padding, eps 1e-6; the output's padding stays untouched."""
    x, g, b = VR.ln_input("gauss", M, C)
    ref, B = VR.layernorm(x, g, b)
    y32, _ = VR.layernorm(x, g, b, dtype=F32)
    PRU.judge("layernorm", f"gauss M={M} C={C}", {"": ((run_layernorm(x, g, b), ref, B), _yard(y32, ref, B))}, finite=True)


@pytest.mark.parametrize("M,C", [(3, 64), (65, 768)])
def test_layernorm_offset_and_constant_rows(M, C):
    """A row of 1e4 + N(0, 1) does not cancel (the statistics are taken in fp64 over the registers); a constant row gives beta exactly."""
    x, g, b = VR.ln_input("offset", M, C)
    ref, B = VR.layernorm(x, g, b)
    y32, _ = VR.layernorm(x, g, b, dtype=F32)
    got = run_layernorm(x, g, b)
    PRU.judge("layernorm", f"offset M={M} C={C}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
    # the stronger statement the fp64 statistics allow: the error is float32 rounding of the RESULT, not of the mean of 1e4-sized values
    err = float((got.double() - ref).abs().max())
    print(f"[parity] layernorm offset M={M} C={C}: max abs error {err:.2e} on values of size {float(ref.abs().max()):.2f}")
    assert err <= 4 * 2.0 ** -24 * float((ref.abs() + 1).max())
    x, g, b = VR.ln_input("const", M, C)
    got = run_layernorm(x, g, b)
    assert torch.equal(AH.bits(got), AH.bits(b[None, :].expand(M, C)))


# ---- car_gelu --------------------------------------------------------------------------------------------------------------------------------
def run_gelu(x, pad=0):
    M, N = x.shape
    Y = Guarded((M, N), ld=N + pad, init=x)
    assert lib().car_gelu(Y.ptr, N + pad, M, N, stream()) == 0, lib().car_last_error()
    sync()
    return Y.get("car_gelu")


def test_gelu_grid_and_special_values():
    x = VR.gelu_grid()[None, :]
    ref, B = VR.gelu(x)
    y32, _ = VR.gelu(x, F32)
    PRU.judge("gelu", "grid [-12, 12]", {"": ((run_gelu(x), ref, B), _yard(y32, ref, B))}, finite=True)
    # strided rows with guarded padding
    xs = torch.randn(37, 64, generator=PRU.gen(3)) * 3
    ref, B = VR.gelu(xs)
    PRU.judge("gelu", "rows 37 x 64, ld 72", {"": ((run_gelu(xs, pad=8), ref, B), _yard(VR.gelu(xs, F32)[0], ref, B))}, finite=True)
    # +-0 stay +-0, +inf stays +inf, a NaN propagates, -inf gives NaN as the formula does (-inf times 0)
    sp = torch.tensor([[0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, 40.0]])
    got = run_gelu(sp)[0]
    assert torch.equal(AH.bits(got[:2]), AH.bits(sp[0, :2])) and got[2].item() == INF
    assert torch.isnan(got[3]) and torch.isnan(got[4]) and got[7].item() == 40.0
    want = VR.gelu(sp)[0][0]
    assert torch.isnan(want[3]) and abs(got[5].item() - want[5].item()) < 1e-6 and abs(got[6].item() - want[6].item()) < 1e-6


# ---- car_mha ---------------------------------------------------------------------------------------------------------------------------------
def run_mha(qkv, b, S, heads, pad=4, what="car_mha", work=None):
    """qkv rows with NaN in the row padding, in front of row 0 and behind row b S; out guarded; the workspace starts as NaN.
    work: (pointer, bytes) of the caller's own workspace."""
    dim = heads * VR.HEAD
    Q = Guarded((b * S, 3 * dim), ld=3 * dim + pad, init=qkv)
    O = Guarded((b * S, dim), ld=dim + pad)
    nbytes = lib().car_mha_workspace_bytes(b, S, heads)
    W = torch.full((nbytes // 4,), NAN, device=AH.dev())
    wp, wb = (ptr(W), nbytes) if work is None else work
    assert lib().car_mha(Q.ptr, 3 * dim + pad, b, S, heads, O.ptr, dim + pad, wp, wb, stream()) == 0, lib().car_last_error()
    sync()
    return O.get(what)


def _judge_mha(name, b, S, heads, got):
    ref, B, y32 = VR.mha_reference(name, b, S, heads)
    PRU.judge("mha", f"{name} b={b} S={S} heads={heads}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)


@pytest.mark.parametrize("b,S,heads", VR.MHA_SHAPES)
def test_mha_shapes(b, S, heads):
    """N(0, 1) at the tile edges, the ragged last tile and the three real lengths; two runs are bit-identical."""
    qkv = VR.mha_input("gauss", b, S, heads)
    got = run_mha(qkv, b, S, heads)
    _judge_mha("gauss", b, S, heads, got)
    assert torch.equal(AH.bits(run_mha(qkv, b, S, heads)), AH.bits(got))


@pytest.mark.parametrize("b,S,heads", VR.MHA_SET_SHAPES)
@pytest.mark.parametrize("name", [n for n in VR.MHA_SETS if n not in ("gauss", "uniform")])
def test_mha_value_sets(name, b, S, heads):
    qkv = VR.mha_input(name, b, S, heads)
    got = run_mha(qkv, b, S, heads)
    _judge_mha(name, b, S, heads, got)
    if name == "dominant":                                             # weight 1: the output is that key's v, within the rule
        ref, B, y32 = VR.mha_reference(name, b, S, heads)
        PRU.judge("mha", f"dominant-v b={b} S={S} heads={heads}", {"": ((got, VR.dominant_rows(qkv, b, S, heads).double(), B), _yard(y32, ref, B))})


@pytest.mark.parametrize("b,S,heads", VR.MHA_UNIFORM_SHAPES)
def test_mha_uniform_mean_is_exact(b, S, heads):
    """q = 0, small-integer v, S a power of two: every weight is 1 / S and the mean is exactly representable — bit for bit."""
    qkv = VR.mha_input("uniform", b, S, heads)
    ref, _, _ = VR.mha_reference("uniform", b, S, heads)
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(AH.bits(run_mha(qkv, b, S, heads)), AH.bits(ref.float()))


@pytest.mark.parametrize("S,heads", [(5, 2), (257, 2)])
def test_mha_scene_is_independent_of_the_other_scenes(S, heads):
    qkv = VR.mha_input("gauss", 2, S, heads)
    both = run_mha(qkv, 2, S, heads)
    other = qkv.clone()
    other[S:] = 1e3 * torch.randn(S, qkv.shape[1], generator=PRU.gen(9))
    assert torch.equal(AH.bits(run_mha(other, 2, S, heads)[:S]), AH.bits(both[:S]))
    assert torch.equal(AH.bits(run_mha(qkv[:S].contiguous(), 1, S, heads)), AH.bits(both[:S]))
    assert torch.equal(AH.bits(run_mha(qkv[S:].contiguous(), 1, S, heads)), AH.bits(both[S:]))


# ---- car_vit_pack / car_vit_blocks ---------------------------------------------------------------------------------------------------------------
def _offsets(dim):
    return [lib().car_vit_packed_offset(dim, i) for i in range(13)]


def _pack(params, dim, depth):
    dp = [dev_t(t) for t in params]
    n = lib().car_vit_packed_floats(dim, depth)
    packed = Guarded((n,), fill=0.0)
    assert lib().car_vit_pack(AH.ptrs(dp), len(dp), dim, depth, packed.ptr, stream()) == 0, lib().car_last_error()
    sync()
    assert packed.margins_untouched()
    return packed, dp


def _at(t, off_floats):
    return P_(t.data_ptr() + 4 * off_floats)


def _stage_entries(tok, b, S, dim, packed, depth):
    """The sequence car_vit_blocks documents, issued entry by entry; returns tok after every block."""
    L, M, heads, off = lib(), b * S, dim // VR.HEAD, _offsets(dim)
    d = AH.dev()
    norm, att, wide = torch.empty(M, dim, device=d), torch.empty(M, dim, device=d), torch.empty(M, 4 * dim, device=d)
    nbytes = L.car_mha_workspace_bytes(b, S, heads)
    W = torch.empty(nbytes // 4, device=d)
    tok, after, st, ACC = tok.clone(), [], stream(), 4
    for blk in range(depth):
        base = blk * off[12]
        p = lambda i: _at(packed, base + off[i])
        assert L.car_layernorm(ptr(tok), dim, p(0), p(1), dim, VR.EPS, ptr(norm), dim, M, st) == 0
        assert L.car_linear_x3(ptr(norm), dim, p(2), p(3), dim, 3 * dim, ptr(wide), 3 * dim, M, 0, st) == 0
        assert L.car_mha(ptr(wide), 3 * dim, b, S, heads, ptr(att), dim, ptr(W), nbytes, st) == 0
        assert L.car_linear_x3(ptr(att), dim, p(4), p(5), dim, dim, ptr(tok), dim, M, ACC, st) == 0
        assert L.car_layernorm(ptr(tok), dim, p(6), p(7), dim, VR.EPS, ptr(norm), dim, M, st) == 0
        assert L.car_linear_x3(ptr(norm), dim, p(8), p(9), dim, 4 * dim, ptr(wide), 4 * dim, M, 0, st) == 0
        assert L.car_gelu(ptr(wide), 4 * dim, M, 4 * dim, st) == 0
        assert L.car_linear_x3(ptr(wide), 4 * dim, p(10), p(11), 4 * dim, dim, ptr(tok), dim, M, ACC, st) == 0
        after.append(tok.clone())
    sync()
    return after


@pytest.mark.parametrize("dim,depth,taps,b,S", [(128, 3, (1, 2), 2, 10), (128, 3, (1, 2), 1, 66), (768, 2, (0, 1), 1, 514)])
def test_vit_blocks(dim, depth, taps, b, S):
    heads, M = dim // VR.HEAD, b * S
    params = VR.seeded_stage(dim, depth)
    packed, _ = _pack(params, dim, depth)
    tok0 = torch.randn(M, dim, generator=PRU.gen(dim + S))
    T = Guarded((M, dim), init=tok0)
    outs = [Guarded((M, dim)) for _ in taps]
    nbytes = lib().car_vit_workspace_bytes(b, S, dim)
    W = Guarded((nbytes // 4,))
    rc = lib().car_vit_blocks(T.ptr, b, S, dim, packed.ptr, depth, AH.ints(taps), len(taps), AH.ptrs([o.view for o in outs]), W.ptr, nbytes, stream())
    assert rc == 0, lib().car_last_error()
    sync()
    got, tapped = T.get("car_vit_blocks tok"), [o.get(f"car_vit_blocks tap {i}") for i, o in enumerate(outs)]
    assert W.margins_untouched() and packed.margins_untouched()
    # bit-identical to the same sequence through the stage entries; a tap is tok after that block
    after = _stage_entries(dev_t(tok0), b, S, dim, packed.view, depth)
    assert torch.equal(AH.bits(after[-1].cpu()), AH.bits(got))
    for t, o in zip(taps, tapped):
        assert torch.equal(AH.bits(after[t].cpu()), AH.bits(o)), t
    # parity of the whole stage and of every tap
    ref, B, ref_taps = VR.stage(tok0, params, b, S, heads, taps)
    y32, _, y32_taps = VR.stage(tok0, params, b, S, heads, taps, dtype=F32)
    entries = {"tok": ((got, ref, B), _yard(y32, ref, B))}
    for i, t in enumerate(taps):
        entries[f"tap{t}"] = ((tapped[i], ref_taps[i][0], ref_taps[i][1]), _yard(y32_taps[i][0], ref_taps[i][0], ref_taps[i][1]))
    PRU.judge("vit_blocks", f"dim={dim} depth={depth} b={b} S={S}", entries, finite=True)


def test_mha_and_blocks_fit_their_workspaces_exactly():
    """car_mha (b = 2, S = 33, one head: a ragged second key tile) and car_vit_blocks (b = 1, S = 33, dim = 64, one block, whose workspace
    holds car_mha's nested behind its own three maps), each over a workspace of exactly its size entry's bytes with NaN all around it,
    then over one twice as large: nothing is written outside either and the outputs are the same bytes."""
    qkv = VR.mha_input("gauss", 2, 33, 1)
    AH.exact_then_twice(lib().car_mha_workspace_bytes(2, 33, 1), lambda w, wb: (run_mha(qkv, 2, 33, 1, work=(w.ptr, wb)),), "car_mha")
    dim, depth, b, S = 64, 1, 1, 33
    packed, _ = _pack(VR.seeded_stage(dim, depth), dim, depth)
    tok0 = torch.randn(b * S, dim, generator=PRU.gen(dim + S))

    def blocks(work, wb):
        T, tap = Guarded((b * S, dim), init=tok0), Guarded((b * S, dim))
        rc = lib().car_vit_blocks(T.ptr, b, S, dim, packed.ptr, depth, AH.ints((0,)), 1, AH.ptrs([tap.view]), work.ptr, wb, stream())
        assert rc == 0, lib().car_last_error()
        sync()
        return T.get("car_vit_blocks tok"), tap.get("car_vit_blocks tap")

    tok, tap = AH.exact_then_twice(lib().car_vit_workspace_bytes(b, S, dim), blocks, "car_vit_blocks")
    assert torch.equal(AH.bits(tok), AH.bits(tap)) and bool(torch.isfinite(tok).all()) and packed.margins_untouched()


def test_vit_pack_layout():
    """The vectors are copies; each packed matrix is what car_linear_x3_pack makes of the raw one, and runs through car_linear_x3 as it does."""
    dim, depth = 128, 2
    params = VR.seeded_stage(dim, depth)
    packed, dp = _pack(params, dim, depth)
    flat, off, L = packed.view, _offsets(dim), lib()
    X = dev_t(torch.randn(37, 4 * dim, generator=PRU.gen(4)))
    for blk in range(depth):
        for i in range(12):
            raw, at = dp[12 * blk + i], blk * off[12] + off[i]
            if raw.dim() == 1:
                assert torch.equal(flat[at:at + raw.numel()], raw), (blk, i)
                continue
            N, K = raw.shape
            n = L.car_linear_x3_packed_floats(K, N)
            own = torch.zeros(n, device=AH.dev())
            assert L.car_linear_x3_pack(ptr(raw), K, K, N, ptr(own), stream()) == 0
            ya, yb = torch.empty(37, N, device=AH.dev()), torch.empty(37, N, device=AH.dev())
            assert L.car_linear_x3(ptr(X), 4 * dim, _at(flat, at), None, K, N, ptr(ya), N, 37, 0, stream()) == 0
            assert L.car_linear_x3(ptr(X), 4 * dim, ptr(own), None, K, N, ptr(yb), N, 37, 0, stream()) == 0
            sync()
            assert torch.equal(AH.bits(ya), AH.bits(yb)), (blk, i)
            xc, wc = X[:, :K].cpu(), raw.cpu()                            # against the RAW matrix: the right one, in the right layout
            want, bound = xc.double() @ wc.double().T, xc.double().abs() @ wc.double().abs().T
            PRU.judge("vit_pack", f"block {blk} item {i}", {"": ((ya.cpu(), want, bound), _yard(xc @ wc.T, want, bound))})


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_car_e_arg_and_launch_nothing():
    L, st = lib(), stream()
    dim, heads, b, S, M = 128, 2, 1, 5, 5
    X = Guarded((M, dim), fill=1.0)
    Y = Guarded((M, 4 * dim))
    g = dev_t(torch.ones(dim))
    Q = Guarded((M, 3 * dim), fill=1.0)
    nb = L.car_mha_workspace_bytes(b, S, heads)
    W = Guarded((max(nb, L.car_vit_workspace_bytes(b, S, dim)) // 4,))
    params = [dev_t(t) for t in VR.seeded_stage(dim, 1)]
    packed = Guarded((L.car_vit_packed_floats(dim, 1),))
    tap = Guarded((M, dim))
    off16 = lambda G_: P_(G_.view.data_ptr() + 4)                       # 4 bytes off a 16-byte boundary
    vb = L.car_vit_workspace_bytes(b, S, dim)
    calls = {
        "layernorm null": lambda: L.car_layernorm(None, dim, ptr(g), ptr(g), dim, 1e-6, Y.ptr, dim, M, st),
        "layernorm C": lambda: L.car_layernorm(X.ptr, dim, ptr(g), ptr(g), 6, 1e-6, Y.ptr, dim, M, st),
        "layernorm C big": lambda: L.car_layernorm(X.ptr, 4100, ptr(g), ptr(g), 4100, 1e-6, Y.ptr, 4100, 1, st),
        "layernorm stride below": lambda: L.car_layernorm(X.ptr, dim, ptr(g), ptr(g), dim, 1e-6, Y.ptr, dim - 4, M, st),
        "layernorm stride % 4": lambda: L.car_layernorm(X.ptr, dim, ptr(g), ptr(g), dim, 1e-6, Y.ptr, dim + 2, M, st),
        "layernorm aligned": lambda: L.car_layernorm(X.ptr, dim, ptr(g), ptr(g), dim, 1e-6, off16(Y), dim, M, st),
        "gelu null": lambda: L.car_gelu(None, dim, M, dim, st),
        "gelu stride below": lambda: L.car_gelu(Y.ptr, dim - 4, M, dim, st),
        "gelu stride % 4": lambda: L.car_gelu(Y.ptr, dim + 2, M, dim, st),
        "gelu aligned": lambda: L.car_gelu(off16(Y), dim, M, dim, st),
        "mha null": lambda: L.car_mha(Q.ptr, 3 * dim, b, S, heads, None, dim, W.ptr, nb, st),
        "mha S 0": lambda: L.car_mha(Q.ptr, 3 * dim, b, 0, heads, Y.ptr, dim, W.ptr, nb, st),
        "mha S 1025": lambda: L.car_mha(Q.ptr, 3 * dim, b, 1025, heads, Y.ptr, dim, W.ptr, 1 << 40, st),
        "mha heads 0": lambda: L.car_mha(Q.ptr, 3 * dim, b, S, 0, Y.ptr, dim, W.ptr, nb, st),
        "mha heads 17": lambda: L.car_mha(Q.ptr, 3 * 17 * 64, b, S, 17, Y.ptr, 17 * 64, W.ptr, 1 << 40, st),
        "mha stride below": lambda: L.car_mha(Q.ptr, 3 * dim - 4, b, S, heads, Y.ptr, dim, W.ptr, nb, st),
        "mha stride % 4": lambda: L.car_mha(Q.ptr, 3 * dim + 2, b, S, heads, Y.ptr, dim, W.ptr, nb, st),
        "mha out stride below": lambda: L.car_mha(Q.ptr, 3 * dim, b, S, heads, Y.ptr, dim - 4, W.ptr, nb, st),
        "mha aligned": lambda: L.car_mha(off16(Q), 3 * dim, b, S, heads, Y.ptr, dim, W.ptr, nb, st),
        "mha work aligned": lambda: L.car_mha(Q.ptr, 3 * dim, b, S, heads, Y.ptr, dim, off16(W), nb, st),
        "mha workspace": lambda: L.car_mha(Q.ptr, 3 * dim, b, S, heads, Y.ptr, dim, W.ptr, nb - 1, st),
        "pack null": lambda: L.car_vit_pack(AH.ptrs(params), 12, dim, 1, None, st),
        "pack null parameter": lambda: L.car_vit_pack(AH.ptrs(params[:11] + [None]), 12, dim, 1, packed.ptr, st),
        "pack dim": lambda: L.car_vit_pack(AH.ptrs(params), 12, 96, 1, packed.ptr, st),
        "pack dim big": lambda: L.car_vit_pack(AH.ptrs(params), 12, 1088, 1, packed.ptr, st),
        "pack depth": lambda: L.car_vit_pack(AH.ptrs(params), 0, dim, 0, packed.ptr, st),
        "pack depth 33": lambda: L.car_vit_pack(AH.ptrs(params), 12 * 33, dim, 33, packed.ptr, st),
        "pack count": lambda: L.car_vit_pack(AH.ptrs(params), 11, dim, 1, packed.ptr, st),
        "pack aligned": lambda: L.car_vit_pack(AH.ptrs(params), 12, dim, 1, off16(packed), st),
        "blocks null": lambda: L.car_vit_blocks(None, b, S, dim, packed.ptr, 1, None, 0, None, W.ptr, vb, st),
        "blocks null taps": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 1, None, 1, AH.ptrs([tap.view]), W.ptr, vb, st),
        "blocks S": lambda: L.car_vit_blocks(X.ptr, b, 1025, dim, packed.ptr, 1, None, 0, None, W.ptr, 1 << 40, st),
        "blocks dim": lambda: L.car_vit_blocks(X.ptr, b, S, 96, packed.ptr, 1, None, 0, None, W.ptr, vb, st),
        "blocks dim big": lambda: L.car_vit_blocks(X.ptr, b, S, 1088, packed.ptr, 1, None, 0, None, W.ptr, 1 << 40, st),
        "blocks depth": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 0, None, 0, None, W.ptr, vb, st),
        "blocks depth 33": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 33, None, 0, None, W.ptr, vb, st),
        "blocks tap >= depth": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 1, AH.ints([1]), 1, AH.ptrs([tap.view]), W.ptr, vb, st),
        "blocks taps not increasing": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 3, AH.ints([1, 1]), 2, AH.ptrs([tap.view, tap.view]), W.ptr, vb, st),
        "blocks null tap_out": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 1, AH.ints([0]), 1, AH.ptrs([None]), W.ptr, vb, st),
        "blocks aligned": lambda: L.car_vit_blocks(off16(X), b, S, dim, packed.ptr, 1, None, 0, None, W.ptr, vb, st),
        "blocks workspace": lambda: L.car_vit_blocks(X.ptr, b, S, dim, packed.ptr, 1, None, 0, None, W.ptr, vb - 1, st),
    }
    x_before = X.full.clone()
    for name, call in calls.items():
        assert call() == CAR_E_ARG, name
        msg = L.car_last_error()
        assert msg and msg.decode().startswith("car_"), (name, msg)
    sync()
    assert Y.untouched() and W.untouched() and packed.untouched() and tap.untouched(), "a refused call wrote something"
    assert torch.equal(AH.bits(X.full), AH.bits(x_before))


# ---- end to end: get_z on the device route against the reference's fixtures ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _renderer():
    import encoder_cases as EC
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="midas_vit", n_view=2).eval()
    m.load_state_dict(EC.seeded_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    inp = {k: {kk: vv.to(AH.dev()) for kk, vv in v.items()} for k, v in EC.context_pair().items()}
    return m.to(AH.dev()), inp


def _get_z(m, inp, route):
    m.encoder_route = route
    try:
        with torch.no_grad():
            return [t.float().cpu() for t in m.get_z(inp)]
    finally:
        m.encoder_route = "torch"


@pytest.mark.parametrize("variant", ["default", "no_multiview"])
def test_get_z_on_the_device_route_reproduces_the_reference(variant):
    """The fixtures were made by running the reference; the device route is held to the bound test_encoder.py holds the float32 torch route
    to: 1e-3 rms + 1e-6 per level on the stored samples."""
    import encoder_cases as EC
    m, inp = _renderer()
    fx = np.load(EC.fixture_path(variant))
    m.no_multiview = variant == "no_multiview"
    try:
        z_dev, z_torch = _get_z(m, inp, "device"), _get_z(m, inp, "torch")
    finally:
        m.no_multiview = False
    worst = []
    for i, (got, got_t) in enumerate(zip(EC.sample(z_dev), EC.sample(z_torch))):
        want = fx[f"z{i}"]
        rms = max(float(np.sqrt((want ** 2).mean())), 1e-30)
        bound = 1e-3 * rms + 1e-6
        e_dev, e_torch = float(np.abs(got - want).max()), float(np.abs(got_t - want).max())
        print(f"[parity] get_z {variant} level {i}: device {e_dev:.3e} torch {e_torch:.3e} bound {bound:.3e} (rms {rms:.3e})")
        worst.append((i, e_dev, bound))
    assert all(e <= bd for _, e, bd in worst), (variant, worst)


def test_device_route_refuses_instead_of_falling_back():
    m, inp = _renderer()
    enc = m.encoder
    m.encoder_route = "device"
    try:
        with torch.no_grad():
            tok = torch.zeros(1, 514, 768, device=AH.dev(), dtype=F64)
            with pytest.raises(ValueError, match="computes in float32"):
                enc._blocks_on_device(tok, tok, 2, 257)
            with pytest.raises(ValueError, match="CPU tensors run on vit_route = 'torch'"):
                enc._blocks_on_device(tok.float().cpu(), tok, 2, 257)
        assert torch.is_grad_enabled() and any(p.requires_grad for p in enc.parameters())
        with pytest.raises(ValueError, match="keep vit_route = 'torch'"):
            m.get_z(inp)                                                # autograd would record it: the condition models.forward trains on
    finally:
        m.encoder_route = "torch"


def test_a_fused_optimizer_step_reaches_the_device_route_after_eval():
    """torch's fused / foreach updates change a parameter without advancing _version, which the packed cache's key relies on: leaving
    train() mode drops the cache, so the next eval() get_z packs the parameters as they are."""
    m, inp = _renderer()
    p = m.encoder.pretrained.model.blocks[11].mlp.fc2.bias
    z0 = _get_z(m, inp, "device")
    assert m.encoder._vit_packed.value is not None
    saved, version = p.detach().clone(), p._version
    try:
        m.train()
        with torch.no_grad():
            torch._foreach_add_([p.data], 0.5)
        print(f"[stale] _version {version} -> {p._version} after torch._foreach_add_ on .data")
        m.eval()
        assert m.encoder._vit_packed.value is None                      # dropped in the transition
        z1, z1_t = _get_z(m, inp, "device"), _get_z(m, inp, "torch")
    finally:
        with torch.no_grad():
            p.copy_(saved)
        m.eval()
        m.encoder.drop_device_caches()
    moved = float((z1[0] - z0[0]).abs().max())
    rms = float(z1_t[0].double().pow(2).mean().sqrt())
    assert moved > 1e-2 * rms, "get_z did not see the new parameter"
    assert float((z1[0] - z1_t[0]).abs().max()) <= 2 * (1e-3 * rms + 1e-6)          # both routes within the fixture bound of the same function
