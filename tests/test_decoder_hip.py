"""The encoder's back half on the device, through the C ABI (include/car_decoder.h, csrc/car_decoder.hip): car_conv3x3_pad1,
car_upsample2x_bilinear, car_readout, car_conv7x7_pad3, car_normalize_rgb, car_decoder_pack / car_decoder_forward and car_getz against the
float64 restatement of tests/decoder_reference.py, and get_z with the decoder — or everything — on the device against the fixtures the
reference wrote.  Every comparison of a kernel is parity_rule.judge: kernel ratio <= 8 x max(yardstick ratio, 2^-22), the yardstick the same
formulas in float32; no other tolerance.  Buffers are abi_harness.Guarded: NaN in every margin, and whatever a kernel writes outside its
output fails the test."""
import functools

import numpy as np
import pytest
import torch

import abi_harness as AH
import decoder_reference as DR
import parity_rule as PRU
import trunk_reference as TR
import vit_reference as VR
from abi_harness import CAR_E_ARG, NAN, Guarded, P_, ptr, stream

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
RELU_IN, RELU_OUT, ACCUM = DR.RELU_IN, DR.RELU_OUT, DR.ACCUM


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


# ---- car_conv3x3_pad1 --------------------------------------------------------------------------------------------------------------------------
def pack_pad1(w):
    N, K = w.shape[:2]
    n = lib().car_conv3x3_pad1_packed_floats(K, N)
    assert n > 0, lib().car_last_error()
    Wt, packed = dev_t(w), Guarded((n,), fill=0.0)
    ok(lib().car_conv3x3_pad1_pack(ptr(Wt), K, N, packed.ptr, stream()))
    sync()
    assert packed.margins_untouched()
    return packed


@functools.lru_cache(maxsize=None)
def conv_layer(K, N, integer=False):
    g = PRU.gen(K * 7 + N)
    w = torch.randint(-2, 3, (N, K, 3, 3), generator=g).float() if integer else torch.randn(N, K, 3, 3, generator=g) / (9 * K) ** 0.5
    b = torch.randint(-3, 4, (N,), generator=g).float() if integer else 0.1 * torch.randn(N, generator=g)
    return w, b, pack_pad1(w)


def run_conv(x, n, H, W, K, N, stride, packed, bias=None, add=None, flags=0, y=None):
    """Every operand in a guarded buffer of its own; the input must come back unchanged."""
    Ho, Wo = DR.pad1_out(H, stride), DR.pad1_out(W, stride)
    X = Guarded((n, H * W, K), init=x)
    Y = Guarded((n, Ho * Wo, N)) if y is None else Guarded((n, Ho * Wo, N), init=y)
    Bi = None if bias is None else Guarded((N,), init=bias)
    Ad = None if add is None else Guarded((n, Ho * Wo, N), init=add)
    ok(lib().car_conv3x3_pad1(X.ptr, n, H, W, K, N, stride, packed.ptr, None if Bi is None else Bi.ptr, None if Ad is None else Ad.ptr, flags, Y.ptr, stream()))
    sync()
    assert torch.equal(AH.bits(X.get("car_conv3x3_pad1 X")), AH.bits(x)), "car_conv3x3_pad1 changed its input"
    assert (Bi is None or Bi.margins_untouched()) and (Ad is None or torch.equal(AH.bits(Ad.get("add")), AH.bits(add)))
    return Y.get("car_conv3x3_pad1")


def wide_input(n, HW, K, g):
    return torch.randn(n, HW, K, generator=g) * 10.0 ** torch.empty(n, HW, 1).uniform_(-5, 5, generator=g)


@pytest.mark.parametrize("K", [256, 512, 768])
@pytest.mark.parametrize("N", [256, 768])
def test_conv3x3_pad1(K, N):
    """Extents of one pixel, of fewer than a window, odd and even (both halvings at stride 2), pixels whose magnitudes span ten orders, with
    the bias; integer weights, inputs and bias bit for bit."""
    w, b, packed = conv_layer(K, N)
    wi, bi, packed_i = conv_layer(K, N, True)
    for stride, H, W in [(s, h, w_) for s in (1, 2) for h, w_ in ((1, 1), (2, 3), (5, 4), (7, 7))] + [(2, 16, 16)]:
        g = PRU.gen(H * 31 + W + stride)
        x = wide_input(1, H * W, K, g)
        ref, B = DR.conv3x3_pad1(x, H, W, w, stride, bias=b)
        y32, _ = DR.conv3x3_pad1(x, H, W, w, stride, bias=b, dtype=F32)
        got = run_conv(x, 1, H, W, K, N, stride, packed, bias=b)
        assert got.shape[1] == DR.pad1_out(H, stride) * DR.pad1_out(W, stride)
        PRU.judge("conv3x3_pad1", f"s={stride} {K}->{N} {H}x{W}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
        xi = torch.randint(-3, 4, (1, H * W, K), generator=g).float()
        want = DR.conv3x3_pad1(xi, H, W, wi, stride, bias=bi)[0].float() + 0.0
        assert torch.equal(AH.bits(run_conv(xi, 1, H, W, K, N, stride, packed_i, bias=bi)), AH.bits(want)), (stride, H, W)
    assert packed.margins_untouched() and packed_i.margins_untouched()


@pytest.mark.parametrize("stride", [1, 2])
def test_conv3x3_pad1_across_blocks_and_images(stride):
    """n = 2 at 10 x 10: at stride 1 the 200 rows cross the 192-row block and the border between the images lies inside a block.  n = 3 at
    9 x 9 with image 1 all NaN: images 0 and 2 are finite and equal to what each gives alone (nothing is read across an image's border, a
    tap outside is dropped by index), and two runs agree."""
    K, N = 256, 256
    w, b, packed = conv_layer(K, N)
    g = PRU.gen(5 + stride)
    x = wide_input(2, 100, K, g)
    ref, B = DR.conv3x3_pad1(x, 10, 10, w, stride, bias=b)
    y32, _ = DR.conv3x3_pad1(x, 10, 10, w, stride, bias=b, dtype=F32)
    PRU.judge("conv3x3_pad1", f"s={stride} n=2 10x10", {"": ((run_conv(x, 2, 10, 10, K, N, stride, packed, bias=b), ref, B), _yard(y32, ref, B))}, finite=True)
    x = torch.randn(3, 81, K, generator=g)
    x[1] = NAN
    both = run_conv(x, 3, 9, 9, K, N, stride, packed, bias=b, flags=RELU_OUT)
    assert torch.equal(AH.bits(run_conv(x, 3, 9, 9, K, N, stride, packed, bias=b, flags=RELU_OUT)), AH.bits(both))
    assert bool(torch.isnan(both[1]).all()), "RELU_OUT keeps a NaN"
    for i in (0, 2):
        assert bool(torch.isfinite(both[i]).all())
        alone = run_conv(x[i:i + 1].contiguous(), 1, 9, 9, K, N, stride, packed, bias=b, flags=RELU_OUT)
        assert torch.equal(AH.bits(alone[0]), AH.bits(both[i])), i


def test_conv3x3_pad1_flags_and_residual():
    """The bias, the residual, each flag alone and all together, in the order of the formula: act_out((conv(act_in(X)) + bias) + add) + Y."""
    K, N, n, H, W = 512, 256, 2, 5, 4
    w, b, packed = conv_layer(K, N)
    g = PRU.gen(77)
    x = torch.randn(n, H * W, K, generator=g)
    add, y = torch.randn(n, H * W, N, generator=g), torch.randn(n, H * W, N, generator=g)
    cases = {"plain": {}, "bias": {"bias": b}, "add": {"add": add}, "relu_in": {"flags": RELU_IN}, "relu_out": {"flags": RELU_OUT},
             "accum": {"flags": ACCUM, "y": y}, "all": {"bias": b, "add": add, "flags": RELU_IN | RELU_OUT | ACCUM, "y": y}}
    for stride in (1, 2):
        Ho, Wo = DR.pad1_out(H, stride), DR.pad1_out(W, stride)
        rows = lambda t: None if t is None else t[:, :Ho * Wo].contiguous()
        for name, kw in cases.items():
            kw = {**kw, "add": rows(kw.get("add")), "y": rows(kw.get("y"))}
            ref, B = DR.conv3x3_pad1(x, H, W, w, stride, **kw)
            y32, _ = DR.conv3x3_pad1(x, H, W, w, stride, dtype=F32, **kw)
            got = run_conv(x, n, H, W, K, N, stride, packed, **kw)
            PRU.judge("conv3x3_pad1", f"s={stride} {name}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
            if name == "relu_out":
                assert bool((got >= 0).all())
    # act_in leaves the padding zeros and drops the negatives: an input of -1 everywhere gives the bias alone
    got = run_conv(-torch.ones(1, 9, K), 1, 3, 3, K, N, 1, packed, bias=b, flags=RELU_IN)
    assert torch.equal(AH.bits(got), AH.bits(b[None, None].expand(1, 9, N).contiguous()))


def test_conv3x3_pad1_equals_car_conv3x3_where_both_apply():
    """At stride 1, with a zero bias and RELU_OUT, the VALUES of car_conv3x3 at K = N = 256 (torch.equal: bits up to the sign of a zero).  Not
    judge: both are the same row sweep over the same tiles — car_conv3x3_pack's, compared here — with the K steps in the same order and the
    same powers of two per layer and per pixel, so every sum is the same sequence of operations; adding a zero bias behind the sum instead of
    starting from it can change the sign of a zero and nothing else."""
    K, N, n, H, W = 256, 256, 2, 6, 5
    w, _, packed = conv_layer(K, N)
    L = lib()
    own = Guarded((L.car_conv3x3_packed_floats(K, N),), fill=0.0)
    Wt, zero = dev_t(w), dev_t(torch.zeros(N))
    ok(L.car_conv3x3_pack(ptr(Wt), ptr(zero), K, N, own.ptr, stream()))
    sync()
    tiles = 9 * K * N + 64
    assert torch.equal(AH.bits(own.view[:tiles].cpu()), AH.bits(packed.view[:tiles].cpu()))
    x = torch.randn(n, H * W, K, generator=PRU.gen(2))
    got = run_conv(x, n, H, W, K, N, 1, packed, bias=torch.zeros(N), flags=RELU_OUT)
    X, Y = Guarded((n, H * W, K), init=x), Guarded((n, H * W, N))
    ok(L.car_conv3x3(X.ptr, n, H, W, K, N, own.ptr, Y.ptr, stream()))
    sync()
    assert torch.equal(got, Y.get("car_conv3x3"))


def test_conv3x3_same_and_pad1_are_one_convolution():
    """K = N = 256, the one width pair both entries accept, at odd extents, where SAME's padding in front is 1 at either stride and the two
    geometries coincide: car_conv3x3_same and car_conv3x3_pad1 (no bias, no residual, flags 0) give the same BYTES, and so do their packers.
    8 images of 5 x 5 at stride 1 are 200 rows, across the 192-row block; 2 images at stride 2.  The pixels' magnitudes span ten orders, so
    rows move their power of two during the sweep."""
    K = N = 256
    w, _, packed = conv_layer(K, N)
    L = lib()
    floats = L.car_conv3x3_same_packed_floats(K, N)
    assert floats == packed.view.numel() > 0, L.car_last_error()
    own, Wt = Guarded((floats,), fill=0.0), dev_t(w)
    ok(L.car_conv3x3_same_pack(ptr(Wt), K, N, own.ptr, stream()))
    sync()
    assert own.margins_untouched()
    assert torch.equal(AH.bits(own.view.cpu()), AH.bits(packed.view.cpu())) and bool((own.view != 0).any())
    for n, stride in ((8, 1), (2, 2)):
        x = wide_input(n, 25, K, PRU.gen(40 + stride))
        Ho = DR.pad1_out(5, stride)
        assert Ho == TR.same_out(5, stride) and TR.same_pad(5, 3, stride)[0] == 1
        pad1 = run_conv(x, n, 5, 5, K, N, stride, packed)
        X, Y = Guarded((n, 25, K), init=x), Guarded((n, Ho * Ho, N))
        ok(L.car_conv3x3_same(X.ptr, n, 5, 5, K, N, stride, own.ptr, Y.ptr, stream()))
        sync()
        same = Y.get("car_conv3x3_same")
        assert torch.equal(AH.bits(same), AH.bits(pad1)) and bool((same != 0).any()), (n, stride)


# ---- car_upsample2x_bilinear ----------------------------------------------------------------------------------------------------------------------
def run_up(x, H, W):
    n, _, C = x.shape
    X, Y = Guarded((n, H * W, C), init=x), Guarded((n, 4 * H * W, C))
    ok(lib().car_upsample2x_bilinear(X.ptr, n, H, W, C, Y.ptr, stream()))
    sync()
    assert torch.equal(AH.bits(X.get("car_upsample2x_bilinear X")), AH.bits(x))
    return Y.get("car_upsample2x_bilinear")


@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 2), (3, 7), (16, 16)])
def test_upsample2x_bilinear(H, W, C):
    for n in (1, 3):
        x = torch.randn(n, H * W, C, generator=PRU.gen(H * 9 + W + C + n)) * 3 + 1
        ref, B = DR.upsample2x(x, H, W)
        y32, _ = DR.upsample2x(x, H, W, F32)
        got = run_up(x, H, W)
        PRU.judge("upsample2x", f"{H}x{W} C={C} n={n}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
        g4, x4 = got.reshape(n, 2 * H, 2 * W, C), x.reshape(n, H, W, C)
        for oy, iy in ((0, 0), (2 * H - 1, H - 1)):
            for ox, ix in ((0, 0), (2 * W - 1, W - 1)):
                assert torch.equal(AH.bits(g4[:, oy, ox]), AH.bits(x4[:, iy, ix])), "a corner is the input's corner, bit for bit"
    const = torch.full((2, H * W, C), 0.3) * torch.tensor([1.0, -1e5])[:, None, None]
    assert torch.equal(AH.bits(run_up(const, H, W)), AH.bits(const[:, :1].expand(2, 4 * H * W, C).contiguous())), "a constant image comes back exactly"


# ---- car_readout -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def readout_layer(dim):
    g = PRU.gen(dim)
    w, b = torch.randn(dim, 2 * dim, generator=g) / (2 * dim) ** 0.5, 0.1 * torch.randn(dim, generator=g)
    n = lib().car_readout_packed_floats(dim)
    assert n > 0, lib().car_last_error()
    Wt, Bt, packed = dev_t(w), dev_t(b), Guarded((n,), fill=0.0)
    ok(lib().car_readout_pack(ptr(Wt), ptr(Bt), dim, packed.ptr, stream()))
    sync()
    assert packed.margins_untouched()
    return w, b, packed


def run_readout(tok, packed, work=None):
    BV, T, dim = tok.shape
    Tk, Y = Guarded((BV, T, dim), init=tok), Guarded((BV, T - 1, dim))
    nbytes = lib().car_readout_workspace_bytes(BV, T - 1, dim)
    assert nbytes > 0, lib().car_last_error()
    Wk = Guarded((nbytes // 4,))
    wp, wb = (Wk.ptr, nbytes) if work is None else work
    ok(lib().car_readout(Tk.ptr, BV, T - 1, dim, packed.ptr, Y.ptr, wp, wb, stream()))
    sync()
    assert Wk.margins_untouched() and packed.margins_untouched() and torch.equal(AH.bits(Tk.get("car_readout tok")), AH.bits(tok))
    return Y.get("car_readout")


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("P", [1, 4, 256])
def test_readout(dim, P):
    """One view and three; patch rows of size 1 under a class row of size 1e4, whose product must not swallow them."""
    w, b, packed = readout_layer(dim)
    for BV in (1, 3):
        for name, cls_scale in (("gauss", 1.0), ("class row 1e4", 1e4)):
            tok = torch.randn(BV, 1 + P, dim, generator=PRU.gen(dim + P + BV))
            tok[:, 0] *= cls_scale
            ref, B, _ = DR.readout(tok, w, b)
            y32, _, _ = DR.readout(tok, w, b, F32)
            got = run_readout(tok, packed)
            PRU.judge("readout", f"dim={dim} P={P} BV={BV} {name}", {"": ((got, ref, B), _yard(y32, ref, B))}, finite=True)
    if P == 4:
        tok = torch.randn(2, 5, dim, generator=PRU.gen(1))
        outs = AH.exact_then_twice(lib().car_readout_workspace_bytes(2, 4, dim), lambda wk, wb: (run_readout(tok, packed, work=(wk.ptr, wb)),), "car_readout")
        assert bool(torch.isfinite(outs[0]).all())


# ---- car_conv7x7_pad3, car_normalize_rgb -----------------------------------------------------------------------------------------------------------
def run_map(x, w, b):
    n, _, H, W = x.shape
    X, Wt, Bt, Y = Guarded(tuple(x.shape), init=x), Guarded((64 * 147,), init=w.reshape(-1)), Guarded((64,), init=b), Guarded((n, H * W, 64))
    ok(lib().car_conv7x7_pad3(X.ptr, n, H, W, Wt.ptr, Bt.ptr, Y.ptr, stream()))
    sync()
    return Y.get("car_conv7x7_pad3")


def run_normalize(rgb):
    n, H, W, _ = rgb.shape
    X, Y = Guarded(tuple(rgb.shape), init=rgb), Guarded((n, 3, H, W))
    ok(lib().car_normalize_rgb(X.ptr, n, H, W, Y.ptr, stream()))
    sync()
    return Y.get("car_normalize_rgb")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8), (19, 17)])
def test_conv7x7_pad3_and_normalize_rgb(n, H, W):
    """At 1 x 1 and 3 x 5 whole rows of the window lie in the padding.  Integers bit for bit; the normalisation bit for bit against the
    restatement that tests/test_decoder_reference.py holds to get_z's own lines."""
    g = PRU.gen(H * 100 + W + n)
    rgb = torch.rand(n, H, W, 3, generator=g) * 2 - 1
    rgb[0, 0, 0] = torch.tensor([-1.0, 1.0, 0.0])
    x = run_normalize(rgb)
    assert torch.equal(AH.bits(x), AH.bits(DR.normalize(rgb)))
    w, b = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5, 0.1 * torch.randn(64, generator=g)
    ref, B = DR.conv7x7(x, w, b)
    y32, _ = DR.conv7x7(x, w, b, F32)
    PRU.judge("conv7x7_pad3", f"n={n} {H}x{W}", {"": ((run_map(x, w, b), ref, B), _yard(y32, ref, B))}, finite=True)
    xi, wi, bi = torch.randint(-4, 5, (n, 3, H, W), generator=g).float(), torch.randint(-3, 4, (64, 3, 7, 7), generator=g).float(), torch.randint(-9, 10, (64,), generator=g).float()
    assert torch.equal(AH.bits(run_map(xi, wi, bi)), AH.bits(DR.conv7x7(xi, wi, bi)[0].float() + 0.0))


# ---- car_decoder_pack / car_decoder_forward ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packed_decoder():
    dp = [dev_t(t) for t in DR.seeded_decoder()]
    n = lib().car_decoder_packed_floats()
    packed = Guarded((n,), fill=0.0)
    ok(lib().car_decoder_pack(AH.ptrs(dp), len(dp), packed.ptr, stream()))
    sync()
    assert packed.margins_untouched()
    return packed, dp


@functools.lru_cache(maxsize=None)
def decoder_inputs(BV, gh, gw):
    g, P = PRU.gen(BV + gh), gh * gw
    return (torch.randn(BV, 1 + P, 768, generator=g), torch.randn(BV, 1 + P, 768, generator=g), torch.relu(torch.randn(BV, 16 * P, 256, generator=g)),
            torch.relu(torch.randn(BV, 4 * P, 512, generator=g)))


def run_decoder(BV, gh, gw, work=None):
    L, P = lib(), gh * gw
    packed, _ = packed_decoder()
    ins = [Guarded(tuple(t.shape), init=t) for t in decoder_inputs(BV, gh, gw)]
    p2, p1 = Guarded((BV, 16 * P, 256)), Guarded((BV, 64 * P, 256))
    nbytes = L.car_decoder_workspace_bytes(BV, gh, gw)
    assert nbytes > 0, L.car_last_error()
    Wk = Guarded((nbytes // 4,)) if work is None else None
    wp, wb = (Wk.ptr, nbytes) if work is None else work
    ok(L.car_decoder_forward(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, BV, gh, gw, packed.ptr, p2.ptr, p1.ptr, wp, wb, stream()))
    sync()
    assert packed.margins_untouched() and (Wk is None or Wk.margins_untouched())
    return p2.get("car_decoder_forward path_2"), p1.get("car_decoder_forward path_1")


def decoder_by_stage_entries(tap3, tap4, layer1, layer2, BV, gh, gw, dp):
    """The sequence car_decoder_forward documents, issued entry by entry from the RAW parameters (every layer packed here, through the exported
    packers); tensors on the device in, (path_2, path_1) on the device out."""
    L, st, d, P = lib(), stream(), AH.dev(), gh * gw

    def readout(tok, w, b):
        packed = torch.zeros(L.car_readout_packed_floats(768), device=d)
        ok(L.car_readout_pack(ptr(w), ptr(b), 768, ptr(packed), st))
        nb = L.car_readout_workspace_bytes(BV, P, 768)
        work, out = torch.empty(nb // 4, device=d), torch.empty(BV * P, 768, device=d)
        ok(L.car_readout(ptr(tok), BV, P, 768, ptr(packed), ptr(out), ptr(work), nb, st))
        return out

    def lin(x, w, b, rows):
        N, K = w.shape[:2]
        packed, out = torch.zeros(L.car_linear_x3_packed_floats(K, N), device=d), torch.empty(rows, N, device=d)
        ok(L.car_linear_x3_pack(ptr(w), K, K, N, ptr(packed), st))
        ok(L.car_linear_x3(ptr(x), K, ptr(packed), ptr(b), K, N, ptr(out), N, rows, 0, st))
        return out

    def conv(x, h, w_, wt, b, stride=1, add=None, flags=0, out=None):
        N, K = wt.shape[:2]
        packed = torch.zeros(L.car_conv3x3_pad1_packed_floats(K, N), device=d)
        ok(L.car_conv3x3_pad1_pack(ptr(wt), K, N, ptr(packed), st))
        out = torch.empty(BV * DR.pad1_out(h, stride) * DR.pad1_out(w_, stride), N, device=d) if out is None else out
        ok(L.car_conv3x3_pad1(ptr(x), BV, h, w_, K, N, stride, ptr(packed), ptr(b), ptr(add), flags, ptr(out), st))
        return out

    l3 = lin(readout(tap3, dp[0], dp[1]), dp[2], dp[3], BV * P)
    l4 = conv(lin(readout(tap4, dp[4], dp[5]), dp[6], dp[7], BV * P), gh, gw, dp[8], dp[9], stride=2)
    levels, rn = [layer1, layer2, l3, l4], dp[10:14]
    refine = [dp[14:24], dp[24:34], dp[34:44], dp[44:50]]
    h, w_, path, outs = gh // 2, gw // 2, None, {}
    for i in (3, 2, 1, 0):
        r = refine[i]
        m = conv(levels[i], h, w_, rn[i], None)
        if i == 3:
            path, r = m, r[:2] + [None] * 4 + r[2:]
        else:
            path = path.clone()                                         # the forward's own copy of path_2; harmless elsewhere
            mid = conv(m, h, w_, r[2], r[3], flags=RELU_IN)
            conv(mid, h, w_, r[4], r[5], add=m, flags=RELU_IN | ACCUM, out=path)
        mid = conv(path, h, w_, r[6], r[7], flags=RELU_IN)
        u = conv(mid, h, w_, r[8], r[9], add=path, flags=RELU_IN)
        up = torch.empty(BV * 4 * h * w_, 256, device=d)
        ok(L.car_upsample2x_bilinear(ptr(u), BV, h, w_, 256, ptr(up), st))
        h, w_ = 2 * h, 2 * w_
        path = lin(up, r[0], r[1], BV * h * w_)
        outs[i] = path
    sync()
    return outs[1], outs[0]


def test_decoder_forward():
    """gh = gw = 2, two views: both outputs bit-identical to the documented sequence issued through the stage entries from the raw
    parameters, against the float64 decoder, and a view alone gives the bits it gives inside the call."""
    BV, gh, gw = 2, 2, 2
    got = run_decoder(BV, gh, gw)
    _, dp = packed_decoder()
    ins = decoder_inputs(BV, gh, gw)
    staged = decoder_by_stage_entries(*[dev_t(t) for t in ins], BV, gh, gw, dp)
    for name, a, b in zip(("path_2", "path_1"), staged, got):
        assert torch.equal(AH.bits(a.cpu().reshape(b.shape)), AH.bits(b)), f"{name} differs from the sequence of stage entries"
    ref = DR.decoder(*ins, gh, gw, DR.seeded_decoder())
    y32 = DR.decoder(*ins, gh, gw, DR.seeded_decoder(), F32)
    entries = {name: ((got[i], ref[i][0], ref[i][1]), _yard(y32[i][0], ref[i][0], ref[i][1])) for i, name in enumerate(("path_2", "path_1"))}
    PRU.judge("decoder_forward", f"BV={BV} {gh}x{gw}", entries, finite=True)


def test_decoder_fits_its_workspace_exactly():
    BV, gh, gw = 2, 2, 2
    nbytes = lib().car_decoder_workspace_bytes(BV, gh, gw)
    outs = AH.exact_then_twice(nbytes, lambda w, wb: run_decoder(BV, gh, gw, work=(w.ptr, wb)), "car_decoder_forward")
    assert all(bool(torch.isfinite(o).all()) for o in outs)


# ---- car_getz --------------------------------------------------------------------------------------------------------------------------------------
GETZ = dict(BV=2, H=32, W=32, gh=2, gw=2, nviews=2, depths=(1, 1, 1), vit_depth=2, taps=(0, 1), grid=4)


@functools.lru_cache(maxsize=None)
def getz_packs():
    """The four packed arrays of a small get_z (one block per trunk stage, two transformer blocks of the real width) and conv_map's pair."""
    L, c, d = lib(), GETZ, AH.dev()
    depths = AH.ints(c["depths"])
    trunk_p = [dev_t(t) for t in TR.seeded_trunk(c["depths"])]
    trunk = torch.zeros(L.car_trunk_packed_floats(depths), device=d)
    ok(L.car_trunk_pack(AH.ptrs(trunk_p), len(trunk_p), depths, ptr(trunk), stream()))
    tp = [dev_t(t) for t in TR.seeded_tokens(c["grid"])]
    toks = torch.zeros(L.car_vit_tokens_packed_floats(c["gh"], c["gw"]), device=d)
    ok(L.car_vit_tokens_pack(ptr(tp[0]), ptr(tp[1]), ptr(tp[2]), ptr(tp[3]), c["grid"], ptr(tp[4]), ptr(tp[5]), c["gh"], c["gw"], ptr(toks), stream()))
    vp = [dev_t(t) for t in VR.seeded_stage(768, c["vit_depth"])]
    vit = torch.zeros(L.car_vit_packed_floats(768, c["vit_depth"]), device=d)
    ok(L.car_vit_pack(AH.ptrs(vp), len(vp), 768, c["vit_depth"], ptr(vit), stream()))
    g = PRU.gen(64)
    map_w, map_b = dev_t(torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5), dev_t(0.1 * torch.randn(64, generator=g))
    sync()
    return trunk, toks, vit, packed_decoder()[0], map_w, map_b


def getz_inputs():
    g, c = PRU.gen(9), GETZ
    return torch.rand(c["BV"], c["H"], c["W"], 3, generator=g) * 2 - 1, 0.5 * torch.randn(c["BV"], 16, generator=g)


def run_getz(no_high_freq=0, work=None, **over):
    L, c = lib(), {**GETZ, **over}
    trunk, toks, vit, dec, map_w, map_b = getz_packs()
    rgb, pose = getz_inputs()
    BV, H, W, P = c["BV"], c["H"], c["W"], c["gh"] * c["gw"]
    R, Po = Guarded(tuple(rgb.shape), init=rgb), Guarded(tuple(pose.shape), init=pose)
    z = [Guarded((BV, 16 * P, 256)), Guarded((BV, 64 * P, 256)), Guarded((BV, H * W, 64))]
    depths = AH.ints(c["depths"])
    nbytes = L.car_getz_workspace_bytes(BV, H, W, c["gh"], c["gw"], c["nviews"], depths, c["vit_depth"])
    assert nbytes > 0, L.car_last_error()
    Wk = Guarded((nbytes // 4,)) if work is None else None
    wp, wb = (Wk.ptr, nbytes) if work is None else work
    ok(L.car_getz(R.ptr, Po.ptr, BV, H, W, c["gh"], c["gw"], c["nviews"], depths, ptr(trunk), ptr(toks), ptr(vit), c["vit_depth"], AH.ints(c["taps"]), dec.ptr,
                  ptr(map_w), ptr(map_b), no_high_freq, z[0].ptr, z[1].ptr, z[2].ptr, wp, wb, stream()))
    sync()
    assert Wk is None or Wk.margins_untouched()
    return [t.get(f"car_getz z{i}") for i, t in enumerate(z)]


def test_getz_is_its_six_stage_calls():
    """A 32 x 32 pair, one block per trunk stage, two transformer blocks of width 768 tapped at (0, 1) — car_getz takes the taps as arguments,
    as car_vit_blocks does: bit-identical to car_normalize_rgb -> car_trunk_forward -> car_vit_tokens -> car_vit_blocks ->
    car_decoder_forward -> car_conv7x7_pad3 issued by the host over workspaces of their own; zeros under no_high_freq."""
    L, c, d, st = lib(), GETZ, AH.dev(), stream()
    trunk, toks, vit, dec, map_w, map_b = getz_packs()
    rgb, pose = getz_inputs()
    BV, H, W, gh, gw, P = c["BV"], c["H"], c["W"], c["gh"], c["gw"], c["gh"] * c["gw"]
    T, depths = 1 + P, AH.ints(c["depths"])
    got = run_getz()
    work = lambda nbytes: torch.empty(nbytes // 4, device=d)
    R, Po = dev_t(rgb), dev_t(pose)
    x = torch.empty(BV, 3, H, W, device=d)
    ok(L.car_normalize_rgb(ptr(R), BV, H, W, ptr(x), st))
    l1, l2, feat = torch.empty(BV, 16 * P, 256, device=d), torch.empty(BV, 4 * P, 512, device=d), torch.empty(BV, P, 1024, device=d)
    wk = work(L.car_trunk_workspace_bytes(BV, H, W, depths))
    ok(L.car_trunk_forward(ptr(x), BV, H, W, ptr(trunk), depths, ptr(l1), ptr(l2), ptr(feat), ptr(wk), wk.numel() * 4, st))
    tok = torch.empty(BV, T, 768, device=d)
    wk = work(L.car_vit_tokens_workspace_bytes(BV, gh, gw))
    ok(L.car_vit_tokens(ptr(feat), BV, gh, gw, ptr(Po), ptr(toks), ptr(tok), ptr(wk), wk.numel() * 4, st))
    taps = [torch.empty(BV, T, 768, device=d) for _ in range(2)]
    b, S = BV // c["nviews"], c["nviews"] * T
    wk = work(L.car_vit_workspace_bytes(b, S, 768))
    ok(L.car_vit_blocks(ptr(tok), b, S, 768, ptr(vit), c["vit_depth"], AH.ints(c["taps"]), 2, AH.ptrs(taps), ptr(wk), wk.numel() * 4, st))
    z0, z1, z2 = torch.empty(BV, 16 * P, 256, device=d), torch.empty(BV, 64 * P, 256, device=d), torch.empty(BV, H * W, 64, device=d)
    wk = work(L.car_decoder_workspace_bytes(BV, gh, gw))
    ok(L.car_decoder_forward(ptr(taps[0]), ptr(taps[1]), ptr(l1), ptr(l2), BV, gh, gw, dec.ptr, ptr(z0), ptr(z1), ptr(wk), wk.numel() * 4, st))
    ok(L.car_conv7x7_pad3(ptr(x), BV, H, W, ptr(map_w), ptr(map_b), ptr(z2), st))
    sync()
    for i, (a, b_) in enumerate(zip((z0, z1, z2), got)):
        assert bool(torch.isfinite(b_).all()) and torch.equal(AH.bits(a.cpu()), AH.bits(b_)), f"z{i} differs from the six stage calls"
    flagged = run_getz(no_high_freq=1)
    assert torch.equal(AH.bits(flagged[0]), AH.bits(got[0])) and torch.equal(AH.bits(flagged[1]), AH.bits(got[1]))
    assert torch.equal(AH.bits(flagged[2]), AH.bits(torch.zeros_like(got[2])))


def test_getz_fits_its_workspace_exactly():
    c = GETZ
    nbytes = lib().car_getz_workspace_bytes(c["BV"], c["H"], c["W"], c["gh"], c["gw"], c["nviews"], AH.ints(c["depths"]), c["vit_depth"])
    AH.exact_then_twice(nbytes, lambda w, wb: run_getz(work=(w.ptr, wb)), "car_getz")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_car_e_arg_and_launch_nothing():
    L, st, c = lib(), stream(), GETZ
    # every buffer is large enough for the call it stands in at the default arguments: a call that was NOT refused fails the test, it does not fault
    X = Guarded((2, 64, 768), fill=1.0)
    Y = Guarded((2 * 64 * 4 * 256,))
    Y2 = Guarded((2 * 32 * 32 * 64,))
    g = dev_t(torch.ones(9 * 768 * 768 + 64))
    d1 = AH.ints(c["depths"])
    rb, db = L.car_readout_workspace_bytes(2, 4, 768), L.car_decoder_workspace_bytes(2, 2, 2)
    gb = L.car_getz_workspace_bytes(2, 32, 32, 2, 2, 2, d1, 2)
    Wk = Guarded((max(rb, db, gb) // 4,))
    packed = Guarded((L.car_decoder_packed_floats(),))
    params = [dev_t(t) for t in DR.seeded_decoder()]
    trunk, toks, vit, dec, map_w, map_b = getz_packs()
    off16 = lambda G_: P_(G_.view.data_ptr() + 4)                       # 4 bytes off a 16-byte boundary
    conv = lambda X_=X.ptr, n=1, H=4, K=768, N=256, s=1, P=ptr(g), b=None, a=None, fl=0, Y_=Y.ptr: L.car_conv3x3_pad1(X_, n, H, 4, K, N, s, P, b, a, fl, Y_, st)
    up = lambda X_=X.ptr, n=1, H=4, C=768, Y_=Y.ptr: L.car_upsample2x_bilinear(X_, n, H, 4, C, Y_, st)
    ro = lambda t=X.ptr, BV=2, P=4, dim=768, pk=ptr(g), Y_=Y.ptr, W_=Wk.ptr, wb=rb: L.car_readout(t, BV, P, dim, pk, Y_, W_, wb, st)
    cmap = lambda x=X.ptr, n=1, H=4, w=ptr(g), b=ptr(g), Y_=Y.ptr: L.car_conv7x7_pad3(x, n, H, 4, w, b, Y_, st)
    norm = lambda r=X.ptr, n=1, H=4, x=Y.ptr: L.car_normalize_rgb(r, n, H, 4, x, st)
    fwd = lambda t3=X.ptr, l1=X.ptr, BV=2, gh=2, gw=2, pk=dec.ptr, p2=Y.ptr, W_=Wk.ptr, wb=db: \
        L.car_decoder_forward(t3, X.ptr, l1, X.ptr, BV, gh, gw, pk, p2, Y.ptr, W_, wb, st)
    getz = lambda r=X.ptr, BV=2, H=32, gh=2, nv=2, d=d1, vd=2, taps=AH.ints((0, 1)), z0=Y.ptr, W_=Wk.ptr, wb=gb: \
        L.car_getz(r, X.ptr, BV, H, 32, gh, 2, nv, d, ptr(trunk), ptr(toks), ptr(vit), vd, taps, dec.ptr, ptr(map_w), ptr(map_b), 0, z0, Y.ptr, Y2.ptr, W_, wb, st)
    calls = {
        "conv pack null": lambda: L.car_conv3x3_pad1_pack(None, 256, 256, packed.ptr, st),
        "conv pack K": lambda: L.car_conv3x3_pad1_pack(X.ptr, 64, 256, packed.ptr, st),
        "conv pack N": lambda: L.car_conv3x3_pad1_pack(X.ptr, 256, 512, packed.ptr, st),
        "conv pack aligned": lambda: L.car_conv3x3_pad1_pack(X.ptr, 256, 256, off16(packed), st),
        "conv null": lambda: conv(Y_=None), "conv null packed": lambda: conv(P=None),
        "conv K": lambda: conv(K=128), "conv N": lambda: conv(N=512),
        "conv stride 0": lambda: conv(s=0), "conv stride 3": lambda: conv(s=3),
        "conv flags": lambda: conv(fl=8), "conv n": lambda: conv(n=0), "conv n cap": lambda: conv(n=4097), "conv H": lambda: conv(H=0),
        "conv aligned": lambda: conv(X_=off16(X)), "conv bias aligned": lambda: conv(b=off16(X)), "conv add aligned": lambda: conv(a=off16(X)),
        "up null": lambda: up(Y_=None), "up C": lambda: up(C=6), "up C 0": lambda: up(C=0), "up n": lambda: up(n=0), "up H": lambda: up(H=0),
        "up side": lambda: up(H=16385), "up aligned": lambda: up(X_=off16(X)),
        "readout pack null": lambda: L.car_readout_pack(X.ptr, None, 768, packed.ptr, st),
        "readout pack dim": lambda: L.car_readout_pack(X.ptr, X.ptr, 100, packed.ptr, st),
        "readout pack aligned": lambda: L.car_readout_pack(X.ptr, X.ptr, 768, off16(packed), st),
        "readout null": lambda: ro(Y_=None), "readout null work": lambda: ro(W_=None), "readout BV": lambda: ro(BV=0), "readout P": lambda: ro(P=0),
        "readout P cap": lambda: ro(P=4097), "readout dim": lambda: ro(dim=48), "readout aligned": lambda: ro(t=off16(X)),
        "readout work aligned": lambda: ro(W_=off16(Wk)), "readout workspace": lambda: ro(wb=rb - 1),
        "map null": lambda: cmap(b=None), "map n": lambda: cmap(n=0), "map H": lambda: cmap(H=-1), "map aligned": lambda: cmap(w=off16(X)),
        "normalize null": lambda: norm(x=None), "normalize n": lambda: norm(n=0), "normalize H": lambda: norm(H=0), "normalize aligned": lambda: norm(r=off16(X)),
        "decoder pack null": lambda: L.car_decoder_pack(AH.ptrs(params), 50, None, st),
        "decoder pack null parameter": lambda: L.car_decoder_pack(AH.ptrs(params[:-1] + [None]), 50, packed.ptr, st),
        "decoder pack count 49": lambda: L.car_decoder_pack(AH.ptrs(params), 49, packed.ptr, st),
        "decoder pack count 54": lambda: L.car_decoder_pack(AH.ptrs(params + params[:4]), 54, packed.ptr, st),
        "decoder pack aligned": lambda: L.car_decoder_pack(AH.ptrs(params), 50, off16(packed), st),
        "decoder null": lambda: fwd(p2=None), "decoder null work": lambda: fwd(W_=None), "decoder BV": lambda: fwd(BV=0),
        "decoder odd grid": lambda: fwd(gh=3), "decoder grid 0": lambda: fwd(gw=0), "decoder grid 66": lambda: fwd(gh=66),
        "decoder aligned": lambda: fwd(t3=off16(X)), "decoder layer aligned": lambda: fwd(l1=off16(X)), "decoder work aligned": lambda: fwd(W_=off16(Wk)),
        "decoder workspace": lambda: fwd(wb=db - 1),
        "getz null": lambda: getz(z0=None), "getz null depths": lambda: getz(d=None), "getz null taps": lambda: getz(taps=None),
        "getz BV % nviews": lambda: getz(BV=3), "getz nviews 0": lambda: getz(nv=0), "getz grid": lambda: getz(gh=4), "getz image": lambda: getz(H=48),
        "getz depth": lambda: getz(d=AH.ints((1, 0, 1))), "getz blocks": lambda: getz(vd=0), "getz taps order": lambda: getz(taps=AH.ints((1, 1))),
        "getz tap >= depth": lambda: getz(taps=AH.ints((0, 2))), "getz aligned": lambda: getz(r=off16(X)), "getz work aligned": lambda: getz(W_=off16(Wk)),
        "getz workspace": lambda: getz(wb=gb - 1),
    }
    x_before = X.full.clone()
    for name, call in calls.items():
        assert call() == CAR_E_ARG, name
        msg = L.car_last_error()
        assert msg and msg.decode().startswith("car_"), (name, msg)
    sync()
    assert Y.untouched() and Y2.untouched() and Wk.untouched() and packed.untouched(), "a refused call wrote something"
    assert torch.equal(AH.bits(X.full), AH.bits(x_before))


# ---- end to end: get_z with the decoder, or everything, on the device against the reference's fixtures --------------------------------------------
def _renderer():
    from test_trunk_hip import _renderer as shared                      # one encoder on the device for both suites
    return shared()


def _get_z(m, inp, route, keep=False):
    """route: a value of encoder_route, or the encoder's own (trunk_route, vit_route, decoder_route)."""
    if isinstance(route, tuple):
        m.encoder.trunk_route, m.encoder.vit_route, m.encoder.decoder_route = route
    else:
        m.encoder_route = route
    try:
        with torch.no_grad():
            z = m.get_z(inp)
            return z if keep else [t.float().cpu() for t in z]
    finally:
        m.encoder_route = "torch"


@pytest.mark.parametrize("route", ["device_full", ("torch", "torch", "device")])
@pytest.mark.parametrize("variant", ["default", "no_multiview", "no_high_freq"])
def test_get_z_with_the_decoder_on_the_device_reproduces_the_reference(variant, route):
    """The fixtures were made by running the reference; the route is held to the bound test_trunk_hip.py holds the other routes to:
    1e-3 rms + 1e-6 per level on the stored samples."""
    import encoder_cases as EC
    m, inp = _renderer()
    fx = np.load(EC.fixture_path(variant))
    for k, v in EC.VARIANTS[variant].items():
        setattr(m, k, v)
    try:
        z_dev = _get_z(m, inp, route)
    finally:
        for k in EC.VARIANTS[variant]:
            setattr(m, k, False)
    assert [tuple(t.shape) for t in z_dev] == [(2, 256, 64, 64), (2, 256, 128, 128), (2, 64, 256, 256)]
    worst = []
    for i, got in enumerate(EC.sample(z_dev)):
        want = fx[f"z{i}"]
        rms = max(float(np.sqrt((want ** 2).mean())), 1e-30)
        bound = 1e-3 * rms + 1e-6
        e_dev = float(np.abs(got - want).max())
        print(f"[parity] get_z {variant} route={route} level {i}: device {e_dev:.3e} bound {bound:.3e} (rms {rms:.3e})")
        worst.append((i, e_dev, bound))
    assert all(e <= bd for _, e, bd in worst), (variant, route, worst)


def test_device_full_leaves_no_torch_module_in_get_z_and_hands_the_engine_views():
    """Under "device_full" conv_map's forward, every module's under scratch and act_postprocess3 / 4, the trunk's and the blocks' are replaced
    by a function that raises: get_z still succeeds.  Its z are NCHW views of channel-last buffers, and the render from them has the bits
    of the render from their contiguous copies."""
    m, inp = _renderer()
    enc = m.encoder
    mods = [m.conv_map, enc.pretrained.model.patch_embed.backbone, *enc.pretrained.model.blocks]
    mods += [s for top in (enc.scratch, enc.pretrained.act_postprocess3, enc.pretrained.act_postprocess4) for s in top.modules()]

    def never(*a, **k):
        raise AssertionError("encoder_route = 'device_full' reached a torch module")
    for mod in mods:
        mod.forward = never                                             # an instance attribute over the method
    try:
        z = _get_z(m, inp, "device_full", keep=True)
    finally:
        for mod in mods:
            del mod.forward
    assert all(t.permute(0, 2, 3, 1).is_contiguous() for t in z)
    with torch.no_grad():
        out_views = m(inp, z=z)
        out_copies = m(inp, z=[t.contiguous() for t in z])
    sync()
    for k in ("rgb", "depth_ray", "at_wt"):
        assert bool(torch.isfinite(out_views[k]).all()) and torch.equal(AH.bits(out_views[k].float().cpu()), AH.bits(out_copies[k].float().cpu())), k


def test_decoder_route_refuses_instead_of_falling_back():
    m, inp = _renderer()
    enc, d = m.encoder, AH.dev()
    tap, l1, l2 = torch.zeros(2, 257, 768, device=d), torch.zeros(2, 256, 64, 64, device=d), torch.zeros(2, 512, 32, 32, device=d)
    with torch.no_grad():
        with pytest.raises(ValueError, match="computes in float32"):
            enc._back_on_device(tap.double(), tap.double(), l1, l2, l1, 16, 16)
        with pytest.raises(ValueError, match="CPU tensors run on decoder_route = 'torch'"):
            enc._back_on_device(tap.cpu(), tap, l1, l2, l1, 16, 16)
    for route, text in ((("torch", "torch", "device"), "keep decoder_route = 'torch'"), ("device_full", "keep encoder_route = 'torch'")):
        if isinstance(route, tuple):
            enc.trunk_route, enc.vit_route, enc.decoder_route = route
        else:
            m.encoder_route = route
        try:
            assert torch.is_grad_enabled() and any(p.requires_grad for p in enc.parameters())
            with pytest.raises(ValueError, match=text):
                m.get_z(inp)                                            # autograd would record it
        finally:
            m.encoder_route = "torch"


def test_a_fused_optimizer_step_on_the_decoder_reaches_the_device_route_after_eval():
    """torch's foreach updates change a parameter without advancing _version, which the packed cache's key relies on: leaving train() mode
    drops the packed decoder, so the next eval() get_z packs the parameters as they are.  How far z must move is what the torch route moves
    by under the same step (a bias of refinenet2 behind an upsampling and a 1x1 layer: about 1 on values of rms 160), not a fraction of the rms."""
    m, inp = _renderer()
    p = m.encoder.scratch.refinenet2.resConfUnit2.conv2.bias
    z0, z0_t = _get_z(m, inp, "device_full"), _get_z(m, inp, "torch")
    assert m.encoder._decoder_packed.value is not None
    saved, version = p.detach().clone(), p._version
    try:
        m.train()
        with torch.no_grad():
            torch._foreach_add_([p.data], 0.5)
        print(f"[stale] _version {version} -> {p._version} after torch._foreach_add_ on .data")
        m.eval()
        assert m.encoder._decoder_packed.value is None and m.encoder._decoder_work == {}
        z1, z1_t = _get_z(m, inp, "device_full"), _get_z(m, inp, "torch")
    finally:
        with torch.no_grad():
            p.copy_(saved)
        m.eval()
        m.encoder.drop_device_caches()
    moved, moved_t = float((z1[0] - z0[0]).abs().max()), float((z1_t[0] - z0_t[0]).abs().max())
    rms = float(z1_t[0].double().pow(2).mean().sqrt())
    print(f"[stale] z0 moved by {moved:.3f} on the device route, by {moved_t:.3f} on the torch route (rms {rms:.1f})")
    assert moved_t > 4 * (1e-3 * rms + 1e-6), "the step does not stand out from what two routes may differ by"
    assert moved > 0.5 * moved_t, "get_z did not see the new parameter"
    assert float((z1[0] - z1_t[0]).abs().max()) <= 2 * (1e-3 * rms + 1e-6)          # both routes within the fixture bound of the same function
