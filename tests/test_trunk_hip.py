"""The encoder's front half on the device, through the C ABI (include/car_trunk.h, csrc/car_trunk.hip): car_weight_standardize, car_stem7x7,
car_groupnorm, car_maxpool3x3s2_same, car_conv3x3_same, car_pixels_stride2, car_trunk_pack / car_trunk_forward and car_vit_tokens against the
float64 restatement of tests/trunk_reference.py, and get_z with the trunk on the device against the fixtures the reference wrote.  Every
comparison of a kernel is parity_rule.judge: kernel ratio <= 8 x max(yardstick ratio, 2^-22), the yardstick the same formulas in float32;
no other tolerance.  Buffers are abi_harness.Guarded: NaN in every margin, and whatever a kernel writes outside its output fails the test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import abi_harness as AH
import parity_rule as PRU
import trunk_reference as TR
from abi_harness import CAR_E_ARG, NAN, Guarded, P_, ptr, stream

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
INF = float("inf")
RELU = 1                           # CAR_GN_RELU


def lib():
    return AH.lib()


def sync():
    torch.cuda.synchronize()


def dev_t(t):
    return t.to(AH.dev()).contiguous()


def ok(rc):
    assert rc == 0, lib().car_last_error()


def _yard(y32, ref, B):
    return PRU.ratio(y32, ref, B)


def depths_of(d):
    return AH.ints(d)


# ---- car_weight_standardize ------------------------------------------------------------------------------------------------------------------
def run_std(w, eps):
    N, fan_in = w.shape[0], w[0].numel()
    W, O = dev_t(w), Guarded((N, fan_in))
    ok(lib().car_weight_standardize(ptr(W), N, fan_in, eps, O.ptr, stream()))
    sync()
    return O.get("car_weight_standardize").reshape(w.shape)


@pytest.mark.parametrize("eps", [1e-6, 1e-8])
@pytest.mark.parametrize("fan_in", [64, 147, 2304, 1024])
def test_weight_standardize(fan_in, eps):
    """N(0, 1) filters, filters of 1e3 + noise (the mean does not cancel: fp64 statistics) and a constant filter, which gives exact zeros."""
    g = PRU.gen(fan_in)
    for name, w in (("gauss", torch.randn(37, fan_in, generator=g)), ("offset", 1e3 + torch.randn(37, fan_in, generator=g))):
        ref, B = TR.weight_standardize(w, eps)
        y32, _ = TR.weight_standardize(w, eps, F32)
        got = run_std(w, eps)
        if name == "offset":                                           # the float32 yardstick loses the noise under the mean; the kernel must not
            err = float((got.double() - ref).abs().max())
            print(f"[parity] weight_standardize offset fan_in={fan_in}: max abs error {err:.2e} on values of size {float(ref.abs().max()):.2f}")
            assert err <= 4 * 2.0 ** -24 * float(ref.abs().max())
        PRU.judge("weight_standardize", f"{name} fan_in={fan_in} eps={eps:g}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
    const = torch.full((5, fan_in), 1.0) * torch.tensor([1.0, -3.5, 1e3, 1e-3, 0.0])[:, None]
    assert torch.equal(AH.bits(run_std(const, eps)), AH.bits(torch.zeros(5, fan_in)))


# ---- car_stem7x7 -----------------------------------------------------------------------------------------------------------------------------
def run_stem(x, w):
    n, _, H, W = x.shape
    Ho, Wo = TR.same_out(H, 2), TR.same_out(W, 2)
    X, Wt, Y = Guarded(tuple(x.shape), init=x), dev_t(w), Guarded((n, Ho * Wo, 64))
    ok(lib().car_stem7x7(X.ptr, n, H, W, ptr(Wt), Y.ptr, stream()))
    sync()
    return Y.get("car_stem7x7")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (9, 11), (16, 16), (32, 32)])
def test_stem7x7(n, H, W):
    g = PRU.gen(H * 100 + W + n)
    x = torch.randn(n, 3, H, W, generator=g) * 2
    w = TR.weight_standardize(torch.randn(64, 3, 7, 7, generator=g) + 0.3, TR.STEM_EPS)[0].float()
    ref, B = TR.stem(x, w)
    y32, _ = TR.stem(x, w, F32)
    PRU.judge("stem7x7", f"n={n} {H}x{W}", {"": ((run_stem(x, w), ref, B), _yard(y32, ref, B))}, finite=True)
    xi = torch.randint(-4, 5, (n, 3, H, W), generator=g).float()       # integers: every sum is exact, bit for bit
    wi = torch.randint(-3, 4, (64, 3, 7, 7), generator=g).float()
    assert torch.equal(AH.bits(run_stem(xi, wi)), AH.bits(TR.stem(xi, wi)[0].float()))


# ---- car_groupnorm ---------------------------------------------------------------------------------------------------------------------------
def run_gn(x, groups, gamma, beta, add=None, relu=False, in_place=False, eps=TR.GN_EPS, work=None):
    n, HW, C = x.shape
    X = Guarded((n, HW, C), init=x)
    Y = X if in_place else Guarded((n, HW, C))
    A = None if add is None else Guarded((n, HW, C), init=add)
    G, Bt = dev_t(gamma), dev_t(beta)
    nbytes = lib().car_groupnorm_workspace_bytes(n, HW, C, groups)
    assert nbytes > 0, lib().car_last_error()
    Wk = Guarded((nbytes // 4,))
    wp, wb = (Wk.ptr, nbytes) if work is None else work
    ok(lib().car_groupnorm(X.ptr, n, HW, C, groups, ptr(G), ptr(Bt), eps, None if A is None else A.ptr, RELU if relu else 0, Y.ptr, wp, wb, stream()))
    sync()
    assert Wk.margins_untouched(), "car_groupnorm wrote outside its workspace"
    if not in_place:
        assert torch.equal(AH.bits(X.get("car_groupnorm X")), AH.bits(x)), "car_groupnorm changed its input"
    return Y.get("car_groupnorm")


def gn_input(n, HW, C, seed):
    g = PRU.gen(seed)
    x = torch.randn(n, HW, C, generator=g) * (10.0 ** torch.empty(1, 1, C).uniform_(-2, 2, generator=g)) + torch.randn(1, 1, C, generator=g)
    return x, 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g), torch.randn(n, HW, C, generator=g)


@pytest.mark.parametrize("C", [64, 256, 1024])
@pytest.mark.parametrize("HW", [1, 7, "slab+1", 256, 1000])
def test_groupnorm(C, HW):
    """2, 8 and 32 channels per group; HW below, at the edge of and over several slabs (8192 / C pixels each); one image and three; every
    combination of ReLU and residual; in place."""
    HW = 8192 // C + 1 if HW == "slab+1" else HW
    for n in (1, 3):
        x, gamma, beta, add = gn_input(n, HW, C, C + HW + n)
        for relu in (False, True):
            for a in (None, add):
                ref, B = TR.groupnorm(x, 32, gamma, beta, add=a, relu=relu)
                y32, _ = TR.groupnorm(x, 32, gamma, beta, add=a, relu=relu, dtype=F32)
                got = run_gn(x, 32, gamma, beta, add=a, relu=relu)
                PRU.judge("groupnorm", f"C={C} HW={HW} n={n} relu={int(relu)} add={int(a is not None)}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
                if n == 3:
                    assert torch.equal(AH.bits(run_gn(x, 32, gamma, beta, add=a, relu=relu, in_place=True)), AH.bits(got)), "in place"
        if n == 3:                                                     # an image alone = the same image inside the batch, bit for bit; two runs agree
            both = run_gn(x, 32, gamma, beta, add=add, relu=True)
            assert torch.equal(AH.bits(both), AH.bits(got))
            for i in range(3):
                alone = run_gn(x[i:i + 1].contiguous(), 32, gamma, beta, add=add[i:i + 1].contiguous(), relu=True)
                assert torch.equal(AH.bits(alone[0]), AH.bits(both[i])), i


@pytest.mark.parametrize("C,HW", [(64, 200), (256, 33), (1024, 9)])
@pytest.mark.parametrize("relu", [False, True])
def test_groupnorm_offset_and_constant_groups(C, HW, relu):
    """A group of 1e4 + N(0, 1) comes out with the rounding of the result, not of the mean; constant groups of 1, 1e4 and 1e6 give beta exactly
    (ReLU'd where flagged): the variance can not go below zero into the square root."""
    g = PRU.gen(C + HW)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    x = 1e4 + torch.randn(2, HW, C, generator=g)
    ref, B = TR.groupnorm(x, 32, gamma, beta, relu=relu)
    y32, _ = TR.groupnorm(x, 32, gamma, beta, relu=relu, dtype=F32)
    got = run_gn(x, 32, gamma, beta, relu=relu)
    PRU.judge("groupnorm", f"offset C={C} HW={HW} relu={int(relu)}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
    err = float((got.double() - ref).abs().max())
    print(f"[parity] groupnorm offset C={C} HW={HW}: max abs error {err:.2e} on values of size {float(ref.abs().max()):.2f}")
    assert err <= 4 * 2.0 ** -24 * float((ref.abs() + 1).max())
    cpg = C // 32
    value = torch.tensor([1.0, 1e4, 1e6, -1e6])[torch.arange(32) % 4].repeat_interleave(cpg)      # one constant per group
    got = run_gn(value[None, None, :].expand(2, HW, C).contiguous(), 32, gamma, beta, relu=relu)
    want = (torch.relu(beta) if relu else beta)[None, None, :].expand(2, HW, C)
    assert torch.equal(AH.bits(got), AH.bits(want.contiguous()))


# ---- car_maxpool3x3s2_same, car_pixels_stride2 -------------------------------------------------------------------------------------------------
def run_pool(x, H, W, entry="car_maxpool3x3s2_same"):
    n, _, C = x.shape
    X, Y = Guarded((n, H * W, C), init=x), Guarded((n, TR.same_out(H, 2) * TR.same_out(W, 2), C))
    ok(getattr(lib(), entry)(X.ptr, n, H, W, C, Y.ptr, stream()))
    sync()
    return Y.get(entry)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (16, 16)])
def test_maxpool_and_pixels_stride2(H, W):
    """Bit-equal to the restatement; -inf, +inf and NaN inputs (a NaN in the window gives NaN, a window of -inf gives -inf)."""
    for n, C in ((1, 64), (3, 8)):
        x = torch.randn(n, H * W, C, generator=PRU.gen(H + W + C))
        for k, v in enumerate((-INF, INF, NAN)):
            x.view(-1)[k::7][:11] = v
        x[0, :, 0] = -INF
        got, want = run_pool(x, H, W), TR.maxpool(x, H, W)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(want).any())
        assert torch.equal(AH.bits(torch.nan_to_num(got, nan=0.0)), AH.bits(torch.nan_to_num(want, nan=0.0)))
        assert bool((got[0, :, 0] == -INF).all())
        assert torch.equal(AH.bits(run_pool(x, H, W, "car_pixels_stride2")), AH.bits(TR.pixels_stride2(x, H, W).contiguous()))


# ---- car_conv3x3_same ------------------------------------------------------------------------------------------------------------------------
def pack_same(w):
    N, K = w.shape[:2]
    n = lib().car_conv3x3_same_packed_floats(K, N)
    assert n > 0, lib().car_last_error()
    Wt, packed = dev_t(w), Guarded((n,), fill=0.0)
    ok(lib().car_conv3x3_same_pack(ptr(Wt), K, N, packed.ptr, stream()))
    sync()
    assert packed.margins_untouched()
    return packed


@functools.lru_cache(maxsize=None)
def conv_layer(K, N, integer=False):
    g = PRU.gen(K * 7 + N)
    w = torch.randint(-2, 3, (N, K, 3, 3), generator=g).float() if integer else TR.weight_standardize(torch.randn(N, K, 3, 3, generator=g) + 0.3, TR.STAGE_EPS)[0].float()
    return w, pack_same(w)


def run_conv(x, n, H, W, K, N, stride, packed):
    Ho, Wo = TR.same_out(H, stride), TR.same_out(W, stride)
    X, Y = Guarded((n, H * W, K), init=x), Guarded((n, Ho * Wo, N))
    ok(lib().car_conv3x3_same(X.ptr, n, H, W, K, N, stride, packed.ptr, Y.ptr, stream()))
    sync()
    return Y.get("car_conv3x3_same")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [64, 128, 256])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_conv3x3_same(stride, K, N):
    """Odd and even extents (both SAME cases at stride 2), row blocks that straddle image rows and images, M no multiple of 192; pixels
    whose magnitudes span ten orders; integer weights and inputs bit for bit."""
    w, packed = conv_layer(K, N)
    wi, packed_i = conv_layer(K, N, True)
    for n in (1, 3):
        for H, W in ((1, 1), (2, 2), (5, 7), (15, 16), (17, 9)):
            g = PRU.gen(H * 31 + W + n + stride)
            x = torch.randn(n, H * W, K, generator=g) * 10.0 ** torch.empty(n, H * W, 1).uniform_(-5, 5, generator=g)
            ref, B = TR.conv_same(x, H, W, w, stride)
            y32, _ = TR.conv_same(x, H, W, w, stride, F32)
            got = run_conv(x, n, H, W, K, N, stride, packed)
            PRU.judge("conv3x3_same", f"s={stride} {K}->{N} n={n} {H}x{W}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
            xi = torch.randint(-3, 4, (n, H * W, K), generator=g).float()
            assert torch.equal(AH.bits(run_conv(xi, n, H, W, K, N, stride, packed_i)), AH.bits(TR.conv_same(xi, H, W, wi, stride)[0].float() + 0.0)), (n, H, W)
    assert packed.margins_untouched() and packed_i.margins_untouched()


def test_conv3x3_same_pack_is_car_conv3x3s_tiles_and_an_image_stands_alone():
    """The packed layer is what car_conv3x3_pack writes (tiles and scale) without its bias; at stride 1 the result, ReLU'd, equals car_conv3x3
    with a zero bias; an image alone gives the bits it gives inside a batch, and two runs agree."""
    K, N, n, H, W = 64, 128, 3, 6, 5
    w, packed = conv_layer(K, N)
    L = lib()
    own = Guarded((L.car_conv3x3_packed_floats(K, N),), fill=0.0)
    Wt, zero = dev_t(w), dev_t(torch.zeros(N))
    ok(L.car_conv3x3_pack(ptr(Wt), ptr(zero), K, N, own.ptr, stream()))
    sync()
    tiles = 9 * K * N + 64
    assert torch.equal(AH.bits(own.view[:tiles].cpu()), AH.bits(packed.view[:tiles].cpu()))
    x = torch.randn(n, H * W, K, generator=PRU.gen(2))
    got = run_conv(x, n, H, W, K, N, 1, packed)
    X, Y = Guarded((n, H * W, K), init=x), Guarded((n, H * W, N))
    ok(L.car_conv3x3(X.ptr, n, H, W, K, N, own.ptr, Y.ptr, stream()))
    sync()
    assert torch.equal(torch.relu(got), Y.get("car_conv3x3"))
    for stride in (1, 2):
        both = run_conv(x, n, H, W, K, N, stride, packed)
        assert torch.equal(AH.bits(run_conv(x, n, H, W, K, N, stride, packed)), AH.bits(both))
        for i in range(n):
            assert torch.equal(AH.bits(run_conv(x[i:i + 1].contiguous(), 1, H, W, K, N, stride, packed)[0]), AH.bits(both[i])), (stride, i)


# ---- car_trunk_pack / car_trunk_forward ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packed_trunk(depths):
    params = TR.seeded_trunk(depths)
    dp = [dev_t(t) for t in params]
    n = lib().car_trunk_packed_floats(depths_of(depths))
    assert n > 0, lib().car_last_error()
    packed = Guarded((n,), fill=0.0)
    ok(lib().car_trunk_pack(AH.ptrs(dp), len(dp), depths_of(depths), packed.ptr, stream()))
    sync()
    assert packed.margins_untouched()
    return packed, dp


def run_trunk(x, depths, work=None):
    n, _, H, W = x.shape
    packed, _ = packed_trunk(depths)
    up = lambda v, k: -(-v // k)
    X = Guarded(tuple(x.shape), init=x)
    outs = [Guarded((n, up(H, s) * up(W, s), c)) for s, c in ((4, 256), (8, 512), (16, 1024))]
    nbytes = lib().car_trunk_workspace_bytes(n, H, W, depths_of(depths))
    assert nbytes > 0, lib().car_last_error()
    Wk = Guarded((nbytes // 4,)) if work is None else None
    wp, wb = (Wk.ptr, nbytes) if work is None else work
    ok(lib().car_trunk_forward(X.ptr, n, H, W, packed.ptr, depths_of(depths), outs[0].ptr, outs[1].ptr, outs[2].ptr, wp, wb, stream()))
    sync()
    assert packed.margins_untouched() and (Wk is None or Wk.margins_untouched())
    return [o.get(f"car_trunk_forward output {i}") for i, o in enumerate(outs)]


def _stage_entries(x, depths):
    """The sequence car_trunk_forward documents, issued entry by entry from the raw parameters (every weight standardised and packed here,
    through the exported packers); returns the three stage ends on the host."""
    L, st, d = lib(), stream(), AH.dev()
    _, dp = packed_trunk(depths)
    n, _, H, W = x.shape
    gnw = torch.empty(1 << 16, device=d)

    def std(w, eps):
        out = torch.empty(w.shape[0], w[0].numel(), device=d)
        ok(L.car_weight_standardize(ptr(w), w.shape[0], w[0].numel(), eps, ptr(out), st))
        return out

    def gn(t, HW, g, b, add, flags):
        nb = L.car_groupnorm_workspace_bytes(n, HW, t.shape[-1], 32)
        assert 0 < nb <= gnw.numel() * 4
        ok(L.car_groupnorm(ptr(t), n, HW, t.shape[-1], 32, ptr(g), ptr(b), TR.GN_EPS, ptr(add), flags, ptr(t), ptr(gnw), nb, st))

    def lin(t, w, rows):
        N, K = w.shape[:2]
        packed = torch.zeros(L.car_linear_x3_packed_floats(K, N), device=d)
        ok(L.car_linear_x3_pack(ptr(std(w, TR.STAGE_EPS)), K, K, N, ptr(packed), st))
        out = torch.empty(rows, N, device=d)
        ok(L.car_linear_x3(ptr(t), K, ptr(packed), None, K, N, ptr(out), N, rows, 0, st))
        return out

    X = dev_t(x)
    h, w = TR.same_out(H, 2), TR.same_out(W, 2)
    y = torch.empty(n * h * w, 64, device=d)
    ok(L.car_stem7x7(ptr(X), n, H, W, ptr(std(dp[0], TR.STEM_EPS)), ptr(y), st))
    gn(y, h * w, dp[1], dp[2], None, RELU)
    h2, w2 = TR.same_out(h, 2), TR.same_out(w, 2)
    cur = torch.empty(n * h2 * w2, 64, device=d)
    ok(L.car_maxpool3x3s2_same(ptr(y), n, h, w, 64, ptr(cur), st))
    h, w = h2, w2
    at, outs, shapes, blk = 3, [], TR.block_shapes(depths), 0
    for dd in depths:
        for _ in range(dd):
            cin, mid, cout, stride, project = shapes[blk]
            ho, wo = TR.same_out(h, stride), TR.same_out(w, stride)
            shortcut = cur
            if project:
                src = cur
                if stride == 2:
                    src = torch.empty(n * ho * wo, cin, device=d)
                    ok(L.car_pixels_stride2(ptr(cur), n, h, w, cin, ptr(src), st))
                shortcut = lin(src, dp[at], n * ho * wo)
                gn(shortcut, ho * wo, dp[at + 1], dp[at + 2], None, 0)
                at += 3
            a = lin(cur, dp[at], n * h * w)
            gn(a, h * w, dp[at + 1], dp[at + 2], None, RELU)
            pk = torch.zeros(L.car_conv3x3_same_packed_floats(mid, mid), device=d)
            ok(L.car_conv3x3_same_pack(ptr(std(dp[at + 3], TR.STAGE_EPS)), mid, mid, ptr(pk), st))
            b = torch.empty(n * ho * wo, mid, device=d)
            ok(L.car_conv3x3_same(ptr(a), n, h, w, mid, mid, stride, ptr(pk), ptr(b), st))
            gn(b, ho * wo, dp[at + 4], dp[at + 5], None, RELU)
            c = lin(b, dp[at + 6], n * ho * wo)
            gn(c, ho * wo, dp[at + 7], dp[at + 8], shortcut, RELU)
            at += 9
            blk += 1
            cur, h, w = c, ho, wo
        outs.append(cur.reshape(n, h * w, -1))
    sync()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("depths", [(1, 1, 1), (2, 1, 2)])
@pytest.mark.parametrize("H,W", [(32, 32), (48, 32)])
def test_trunk_forward(depths, H, W):
    """Real widths, two images; the three stage ends against the float64 trunk, and bit-identical to the sequence through the stage entries."""
    x = torch.randn(2, 3, H, W, generator=PRU.gen(H + W))
    got = run_trunk(x, depths)
    for i, (a, b) in enumerate(zip(_stage_entries(x, depths), got)):
        assert torch.equal(AH.bits(a), AH.bits(b)), f"stage {i} differs from the sequence of stage entries"
    ref = TR.trunk(x, TR.seeded_trunk(depths), depths)
    y32 = TR.trunk(x, TR.seeded_trunk(depths), depths, F32)
    entries = {f"stage{i}": ((got[i], ref[i][0], ref[i][1]), _yard(y32[i][0], ref[i][0], ref[i][1])) for i in range(3)}
    PRU.judge("trunk_forward", f"depths={depths} {H}x{W}", entries, finite=True)
    alone = run_trunk(x[1:].contiguous(), depths)                      # an image does not depend on the other images of the call
    for a, b in zip(alone, got):
        assert torch.equal(AH.bits(a[0]), AH.bits(b[1]))


def test_trunk_fits_its_workspace_exactly():
    depths, x = (1, 1, 1), torch.randn(2, 3, 48, 32, generator=PRU.gen(80))
    nbytes = lib().car_trunk_workspace_bytes(2, 48, 32, depths_of(depths))
    outs = AH.exact_then_twice(nbytes, lambda w, wb: run_trunk(x, depths, work=(w.ptr, wb)), "car_trunk_forward")
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    packed, _ = packed_trunk(depths)
    Wk, X = Guarded((nbytes // 4,)), dev_t(x)
    O = [Guarded((2, 12 * 8, 256)), Guarded((2, 6 * 4, 512)), Guarded((2, 3 * 2, 1024))]
    assert lib().car_trunk_forward(ptr(X), 2, 48, 32, packed.ptr, depths_of(depths), O[0].ptr, O[1].ptr, O[2].ptr, Wk.ptr, nbytes - 1, stream()) == CAR_E_ARG
    assert lib().car_last_error().startswith(b"car_trunk_forward: the workspace is too small")
    sync()
    assert Wk.untouched() and all(o.untouched() for o in O)


# ---- car_vit_tokens --------------------------------------------------------------------------------------------------------------------------
def run_tokens(feat, pose16, params, grid, gh, gw, work=None):
    L, BV = lib(), feat.shape[0]
    dp = [dev_t(t) for t in params]
    n = L.car_vit_tokens_packed_floats(gh, gw)
    assert n > 0, L.car_last_error()
    packed = Guarded((n,), fill=0.0)
    ok(L.car_vit_tokens_pack(ptr(dp[0]), ptr(dp[1]), ptr(dp[2]), ptr(dp[3]), grid, ptr(dp[4]), ptr(dp[5]), gh, gw, packed.ptr, stream()))
    Fe, Po, T = Guarded((BV, gh * gw, 1024), init=feat), Guarded((BV, 16), init=pose16), Guarded((BV, 1 + gh * gw, 768))
    nbytes = L.car_vit_tokens_workspace_bytes(BV, gh, gw)
    Wk = Guarded((nbytes // 4,))
    wp, wb = (Wk.ptr, nbytes) if work is None else work
    ok(L.car_vit_tokens(Fe.ptr, BV, gh, gw, Po.ptr, packed.ptr, T.ptr, wp, wb, stream()))
    sync()
    assert packed.margins_untouched() and Wk.margins_untouched()
    return T.get("car_vit_tokens")


@pytest.mark.parametrize("grid", [4, 24])
@pytest.mark.parametrize("gh,gw", [(1, 1), (2, 3), (16, 16)])
def test_vit_tokens(grid, gh, gw):
    L = lib()
    params = TR.seeded_tokens(grid)
    pw, pb, cls, pos, sw, sb = params
    for BV in (1, 3):
        g = PRU.gen(BV + gh + grid)
        feat, pose16 = torch.relu(torch.randn(BV, gh * gw, 1024, generator=g)), torch.randn(BV, 16, generator=g)
        got = run_tokens(feat, pose16, params, grid, gh, gw)
        ref, B = TR.tokens(feat, pose16, pw, pb, cls, pos, grid, sw, sb, gh, gw)
        y32, _ = TR.tokens(feat, pose16, pw, pb, cls, pos, grid, sw, sb, gh, gw, F32)
        PRU.judge("vit_tokens", f"grid={grid} {gh}x{gw} BV={BV}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
        # the stated order of the sums, bit for bit.  The resized position embedding as the pack holds it: every other term zero
        zeros = (pw, torch.zeros_like(pb), torch.zeros_like(cls), pos, torch.zeros_like(sw), torch.zeros_like(sb))      # over features of zero
        pos_k = run_tokens(torch.zeros_like(feat), torch.zeros_like(pose16), zeros, grid, gh, gw)[0]
        want_pos = TR.resize_pos(pos, grid, gh, gw)
        PRU.judge("vit_tokens", f"pos_embed grid={grid} {gh}x{gw}", {"": ((pos_k, want_pos, want_pos.abs()), _yard(TR.resize_pos(pos, grid, gh, gw, F32), want_pos, want_pos.abs()))})
        assert torch.equal(AH.bits(pos_k[0]), AH.bits(pos[0]))
        pose = torch.zeros(BV, 768, dtype=F64)                         # the 16 terms in order, then the bias, in float64; rounded once
        for k in range(16):
            pose += pose16[:, k:k + 1].double() * sw[:, k].double()[None]
        pose = (pose + sb.double()[None]).float()
        assert torch.equal(AH.bits(got[:, 0]), AH.bits((cls[None] + pos_k[0][None]) + pose)), "class row"
        d = AH.dev()
        packed = torch.zeros(L.car_linear_x3_packed_floats(1024, 768), device=d)
        proj, Fd, Bd, Wd = torch.empty(BV * gh * gw, 768, device=d), dev_t(feat), dev_t(pb), dev_t(pw)
        ok(L.car_linear_x3_pack(ptr(Wd), 1024, 1024, 768, ptr(packed), stream()))
        ok(L.car_linear_x3(ptr(Fd), 1024, ptr(packed), ptr(Bd), 1024, 768, ptr(proj), 768, BV * gh * gw, 0, stream()))
        sync()
        want = (proj.cpu().reshape(BV, gh * gw, 768) + pos_k[None, 1:]) + pose[:, None]
        for row in (0, gh * gw - 1):
            assert torch.equal(AH.bits(got[:, 1 + row]), AH.bits(want[:, row].contiguous())), f"patch row {row}"
        assert torch.equal(AH.bits(got[:, 1:]), AH.bits(want))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_car_e_arg_and_launch_nothing():
    L, st = lib(), stream()
    n, H, W, C = 1, 4, 4, 64
    X = Guarded((n, H * W, 256), fill=1.0)
    Y = Guarded((n, H * W, 1024))
    img = Guarded((n, 3, 32, 32), fill=1.0)
    g = dev_t(torch.ones(1024))
    d1 = depths_of((1, 1, 1))
    gb = L.car_groupnorm_workspace_bytes(n, H * W, C, 32)
    tb = L.car_trunk_workspace_bytes(1, 32, 32, d1)
    kb = L.car_vit_tokens_workspace_bytes(1, 2, 2)
    Wk = Guarded((max(gb, tb, kb) // 4,))
    packed = Guarded((max(L.car_trunk_packed_floats(d1), L.car_vit_tokens_packed_floats(2, 2)),))
    params = [dev_t(t) for t in TR.seeded_trunk((1, 1, 1))]
    tp = [dev_t(t) for t in TR.seeded_tokens(4)]
    off16 = lambda G_: P_(G_.view.data_ptr() + 4)                       # 4 bytes off a 16-byte boundary
    gnorm = lambda X_=X.ptr, n_=n, HW=H * W, C_=C, G_=32, g_=ptr(g), Y_=Y.ptr, W_=Wk.ptr, wb=gb, fl=0, add=None: \
        L.car_groupnorm(X_, n_, HW, C_, G_, g_, ptr(g), 1e-5, add, fl, Y_, W_, wb, st)
    conv = lambda X_=X.ptr, n_=n, H_=H, K=64, N=64, s=1, P=packed.ptr, Y_=Y.ptr: L.car_conv3x3_same(X_, n_, H_, W, K, N, s, P, Y_, st)
    trunk = lambda x=img.ptr, n_=1, H_=32, P=packed.ptr, d=d1, l1=Y.ptr, W_=Wk.ptr, wb=tb: L.car_trunk_forward(x, n_, H_, 32, P, d, l1, Y.ptr, Y.ptr, W_, wb, st)
    tpack = lambda pw=ptr(tp[0]), grid=4, gh=2, P=packed.ptr: L.car_vit_tokens_pack(pw, ptr(tp[1]), ptr(tp[2]), ptr(tp[3]), grid, ptr(tp[4]), ptr(tp[5]), gh, 2, P, st)
    toks = lambda f=X.ptr, BV=1, gh=2, T=Y.ptr, W_=Wk.ptr, wb=kb: L.car_vit_tokens(f, BV, gh, 2, ptr(g), packed.ptr, T, W_, wb, st)
    calls = {
        "std null": lambda: L.car_weight_standardize(None, 4, 64, 1e-8, Y.ptr, st),
        "std N": lambda: L.car_weight_standardize(X.ptr, 0, 64, 1e-8, Y.ptr, st),
        "std fan_in": lambda: L.car_weight_standardize(X.ptr, 4, 0, 1e-8, Y.ptr, st),
        "std aligned": lambda: L.car_weight_standardize(X.ptr, 4, 64, 1e-8, off16(Y), st),
        "stem null": lambda: L.car_stem7x7(img.ptr, 1, 32, 32, None, Y.ptr, st),
        "stem n": lambda: L.car_stem7x7(img.ptr, 0, 32, 32, ptr(g), Y.ptr, st),
        "stem H": lambda: L.car_stem7x7(img.ptr, 1, 0, 32, ptr(g), Y.ptr, st),
        "stem cap": lambda: L.car_stem7x7(img.ptr, 1, 1 << 14, 1 << 14, ptr(g), Y.ptr, st),
        "stem aligned": lambda: L.car_stem7x7(off16(img), 1, 32, 32, ptr(g), Y.ptr, st),
        "groupnorm null": lambda: gnorm(Y_=None),
        "groupnorm null work": lambda: gnorm(W_=None),
        "groupnorm groups": lambda: gnorm(G_=3),
        "groupnorm one channel per group": lambda: gnorm(G_=64),
        "groupnorm C": lambda: gnorm(C_=96),
        "groupnorm C big": lambda: gnorm(C_=2048, HW=1),
        "groupnorm n": lambda: gnorm(n_=0),
        "groupnorm n cap": lambda: gnorm(n_=65536, HW=1),
        "groupnorm HW": lambda: gnorm(HW=0),
        "groupnorm flags": lambda: gnorm(fl=2),
        "groupnorm aligned": lambda: gnorm(Y_=off16(Y)),
        "groupnorm add aligned": lambda: gnorm(add=off16(X)),
        "groupnorm work aligned": lambda: gnorm(W_=off16(Wk)),
        "groupnorm workspace": lambda: gnorm(wb=gb - 1),
        "pool null": lambda: L.car_maxpool3x3s2_same(None, n, H, W, C, Y.ptr, st),
        "pool C": lambda: L.car_maxpool3x3s2_same(X.ptr, n, H, W, 6, Y.ptr, st),
        "pool W": lambda: L.car_maxpool3x3s2_same(X.ptr, n, H, 0, C, Y.ptr, st),
        "pool aligned": lambda: L.car_maxpool3x3s2_same(X.ptr, n, H, W, C, off16(Y), st),
        "pixels null": lambda: L.car_pixels_stride2(X.ptr, n, H, W, C, None, st),
        "pixels C": lambda: L.car_pixels_stride2(X.ptr, n, H, W, 0, Y.ptr, st),
        "pixels n": lambda: L.car_pixels_stride2(X.ptr, -1, H, W, C, Y.ptr, st),
        "pixels aligned": lambda: L.car_pixels_stride2(off16(X), n, H, W, C, Y.ptr, st),
        "conv pack null": lambda: L.car_conv3x3_same_pack(None, 64, 64, packed.ptr, st),
        "conv pack K": lambda: L.car_conv3x3_same_pack(X.ptr, 32, 64, packed.ptr, st),
        "conv pack N": lambda: L.car_conv3x3_same_pack(X.ptr, 64, 512, packed.ptr, st),
        "conv pack aligned": lambda: L.car_conv3x3_same_pack(X.ptr, 64, 64, off16(packed), st),
        "conv null": lambda: conv(Y_=None),
        "conv K": lambda: conv(K=96),
        "conv N": lambda: conv(N=512),
        "conv stride 0": lambda: conv(s=0),
        "conv stride 3": lambda: conv(s=3),
        "conv n": lambda: conv(n_=0),
        "conv H": lambda: conv(H_=0),
        "conv aligned": lambda: conv(X_=off16(X)),
        "trunk pack null": lambda: L.car_trunk_pack(AH.ptrs(params), len(params), d1, None, st),
        "trunk pack null depths": lambda: L.car_trunk_pack(AH.ptrs(params), len(params), None, packed.ptr, st),
        "trunk pack null parameter": lambda: L.car_trunk_pack(AH.ptrs(params[:-1] + [None]), len(params), d1, packed.ptr, st),
        "trunk pack depth 0": lambda: L.car_trunk_pack(AH.ptrs(params), len(params), depths_of((0, 1, 1)), packed.ptr, st),
        "trunk pack depth 17": lambda: L.car_trunk_pack(AH.ptrs(params), len(params), depths_of((1, 1, 17)), packed.ptr, st),
        "trunk pack count": lambda: L.car_trunk_pack(AH.ptrs(params), len(params) - 1, d1, packed.ptr, st),
        "trunk pack count of other depths": lambda: L.car_trunk_pack(AH.ptrs(params), len(params), depths_of((2, 1, 1)), packed.ptr, st),
        "trunk pack aligned": lambda: L.car_trunk_pack(AH.ptrs(params), len(params), d1, off16(packed), st),
        "trunk null": lambda: trunk(l1=None),
        "trunk null depths": lambda: trunk(d=None),
        "trunk depth": lambda: trunk(d=depths_of((1, 0, 1))),
        "trunk n": lambda: trunk(n_=0),
        "trunk H": lambda: trunk(H_=0),
        "trunk aligned": lambda: trunk(x=off16(img)),
        "trunk work aligned": lambda: trunk(W_=off16(Wk)),
        "trunk workspace": lambda: trunk(wb=tb - 1),
        "tokens pack null": lambda: tpack(pw=None),
        "tokens pack grid": lambda: tpack(grid=0),
        "tokens pack gh": lambda: tpack(gh=65),
        "tokens pack aligned": lambda: tpack(P=off16(packed)),
        "tokens null": lambda: toks(T=None),
        "tokens BV": lambda: toks(BV=0),
        "tokens gh": lambda: toks(gh=0),
        "tokens aligned": lambda: toks(f=off16(X)),
        "tokens work aligned": lambda: toks(W_=off16(Wk)),
        "tokens workspace": lambda: toks(wb=kb - 1),
    }
    x_before = X.full.clone()
    for name, call in calls.items():
        assert call() == CAR_E_ARG, name
        msg = L.car_last_error()
        assert msg and msg.decode().startswith("car_"), (name, msg)
    sync()
    assert Y.untouched() and Wk.untouched() and packed.untouched(), "a refused call wrote something"
    assert torch.equal(AH.bits(X.full), AH.bits(x_before))


# ---- end to end: get_z with the trunk on the device against the reference's fixtures --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _renderer():
    import encoder_cases as EC
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="midas_vit", n_view=2).eval()
    m.load_state_dict(EC.seeded_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    inp = {k: {kk: vv.to(AH.dev()) for kk, vv in v.items()} for k, v in EC.context_pair().items()}
    return m.to(AH.dev()), inp


def _get_z(m, inp, route):
    """route: a value of encoder_route, or the encoder's own (trunk_route, vit_route)."""
    if isinstance(route, tuple):
        m.encoder.trunk_route, m.encoder.vit_route = route
    else:
        m.encoder_route = route
    try:
        with torch.no_grad():
            return [t.float().cpu() for t in m.get_z(inp)]
    finally:
        m.encoder_route = "torch"


@pytest.mark.parametrize("route", ["device_trunk", ("device", "torch")])
@pytest.mark.parametrize("variant", ["default", "no_multiview", "no_high_freq"])
def test_get_z_with_the_trunk_on_the_device_reproduces_the_reference(variant, route):
    """The fixtures were made by running the reference; the route is held to the bound test_encoder.py holds the float32 torch route to:
    1e-3 rms + 1e-6 per level on the stored samples."""
    import encoder_cases as EC
    m, inp = _renderer()
    fx = np.load(EC.fixture_path(variant))
    for k, v in EC.VARIANTS[variant].items():
        setattr(m, k, v)
    try:
        z_dev, z_torch = _get_z(m, inp, route), _get_z(m, inp, "torch")
    finally:
        for k in EC.VARIANTS[variant]:
            setattr(m, k, False)
    worst = []
    for i, (got, got_t) in enumerate(zip(EC.sample(z_dev), EC.sample(z_torch))):
        want = fx[f"z{i}"]
        rms = max(float(np.sqrt((want ** 2).mean())), 1e-30)
        bound = 1e-3 * rms + 1e-6
        e_dev, e_torch = float(np.abs(got - want).max()), float(np.abs(got_t - want).max())
        print(f"[parity] get_z {variant} route={route} level {i}: device {e_dev:.3e} torch {e_torch:.3e} bound {bound:.3e} (rms {rms:.3e})")
        worst.append((i, e_dev, bound))
    assert all(e <= bd for _, e, bd in worst), (variant, route, worst)


def test_encoder_route_device_leaves_the_trunk_on_torch():
    """encoder_route = "device" is the blocks alone, as before this route existed: the trunk switch stays "torch", the new entries are never
    reached and nothing of theirs is packed.  (Bits can not be compared across two forwards: the torch trunk's MIOpen convolutions are
    not bit-stable from run to run, which the printed line records; the results agree within the fixture bound.)"""
    m, inp = _renderer()
    enc = m.encoder
    enc.drop_device_caches()
    m.encoder_route = "device"
    assert (enc.trunk_route, enc.vit_route) == ("torch", "device")
    m.encoder_route = "torch"

    def never(*a, **k):
        raise AssertionError("encoder_route = 'device' reached the trunk's device route")
    enc._front_on_device = never                                        # an instance attribute over the method
    try:
        z_a, z_b = _get_z(m, inp, "device"), _get_z(m, inp, ("torch", "device"))
    finally:
        del enc._front_on_device
    assert enc._trunk_packed is None or enc._trunk_packed.value is None
    same = all(torch.equal(AH.bits(a), AH.bits(b)) for a, b in zip(z_a, z_b))
    t_a, t_b = _get_z(m, inp, "torch"), _get_z(m, inp, "torch")
    print(f"[info] two forwards bit-equal: encoder_route='device' {same}, encoder_route='torch' {all(torch.equal(AH.bits(a), AH.bits(b)) for a, b in zip(t_a, t_b))}")
    for a, b in zip(z_a, z_b):
        rms = float(b.double().pow(2).mean().sqrt())
        assert float((a - b).abs().max()) <= 1e-3 * rms + 1e-6
    # what CAN be held to bits: the block stage, fed one and the same token tensor, does not see the trunk switch
    tok = torch.randn(1, 2 * 257, 768, generator=PRU.gen(6)).to(AH.dev())
    taps = {}
    try:
        with torch.no_grad():
            for trunk in ("torch", "device"):
                enc.trunk_route = trunk
                taps[trunk] = enc._blocks_on_device(tok.clone(), tok, 2, 257)
    finally:
        enc.trunk_route = "torch"
    for t in enc.VIT_TAPS:
        assert torch.equal(AH.bits(taps["torch"][t].cpu()), AH.bits(taps["device"][t].cpu())), t


def test_trunk_route_refuses_instead_of_falling_back():
    m, inp = _renderer()
    enc = m.encoder
    x, pose = torch.zeros(2, 3, 256, 256, device=AH.dev()), torch.zeros(2, 16, device=AH.dev())
    with torch.no_grad():
        with pytest.raises(ValueError, match="computes in float32"):
            enc._front_on_device(x.double(), pose, 16, 16)
        with pytest.raises(ValueError, match="CPU tensors run on trunk_route = 'torch'"):
            enc._front_on_device(x.cpu(), pose, 16, 16)
    m.encoder_route = "device_trunk"
    try:
        assert torch.is_grad_enabled() and any(p.requires_grad for p in enc.parameters())
        with pytest.raises(ValueError, match="keep trunk_route = 'torch'"):
            m.get_z(inp)                                                # autograd would record it
    finally:
        m.encoder_route = "torch"


def test_a_fused_optimizer_step_on_the_trunk_reaches_the_device_route_after_eval():
    """torch's foreach updates change a parameter without advancing _version, which the packed cache's key relies on: leaving train() mode
    drops the packed trunk, so the next eval() get_z packs the parameters as they are."""
    m, inp = _renderer()
    p = m.encoder.pretrained.model.patch_embed.backbone.stages[2].blocks[8].norm3.bias
    z0 = _get_z(m, inp, "device_trunk")
    assert m.encoder._trunk_packed.value is not None and m.encoder._tokens_packed.value is not None
    saved, version = p.detach().clone(), p._version
    try:
        m.train()
        with torch.no_grad():
            torch._foreach_add_([p.data], 0.5)
        print(f"[stale] _version {version} -> {p._version} after torch._foreach_add_ on .data")
        m.eval()
        assert m.encoder._trunk_packed.value is None and m.encoder._tokens_packed.value is None and m.encoder._trunk_work == {}
        z1, z1_t = _get_z(m, inp, "device_trunk"), _get_z(m, inp, "torch")
    finally:
        with torch.no_grad():
            p.copy_(saved)
        m.eval()
        m.encoder.drop_device_caches()
    moved = float((z1[0] - z0[0]).abs().max())
    rms = float(z1_t[0].double().pow(2).mean().sqrt())
    assert moved > 1e-2 * rms, "get_z did not see the new parameter"
    assert float((z1[0] - z1_t[0]).abs().max()) <= 2 * (1e-3 * rms + 1e-6)          # both routes within the fixture bound of the same function
