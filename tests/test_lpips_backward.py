"""The LPIPS training loss (car_lpips_forward_train / car_lpips_backward, harness.lpips_loss, train_realestate10k.py --lpips).

The checker is tests/lpips_backward_reference.py: the float64 vector-Jacobian product of the restatement, linearised at 13 activation maps
it is GIVEN.  On the CPU it is pinned to torch.autograd of the restatement; on the GPU the device's gradient is held against it at the
device's own maps, so no ReLU or pool decision that flips between arithmetics has to be budgeted.  Against plain float64 autograd the
end-to-end test first compares the decisions and lists every unit that differs.

Weights are seeded (LR.seeded_weights), not the pretrained ones: as tests/test_lpips.py, this pins the arithmetic to the restatement, NOT
to the lpips package (tests/golden/make_lpips_golden.py --lpips closes that where the package exists).

Figures measured on an MI355X are in profiles/lpips_backward.md."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import abi_harness as abi
import lpips_backward_reference as LBR
import lpips_restatement as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")

# (B, H, W, seed): the chain's shapes; the first three, with kinds `unrelated` and `noisy`, are also the end-to-end cases (the float32
# restatement itself flips decisions on the `near` kind and at 128 x 128 and above, so those stay with the fixed linearisation point)
CHAIN_SHAPES = ((12, 32, 32, 51), (2, 50, 70, 13), (2, 16, 16, 14), (1, 256, 256, 11))
KINDS = ("unrelated", "noisy", "near")
E2E_CASES = tuple((s, k) for s in CHAIN_SHAPES[:3] for k in KINDS[:2])
# (K, N, side) of the nine distinct layer shapes of the network on a 256 x 256 image (tests/test_lpips.py)
LAYER_SHAPES = ((3, 64, 256), (64, 64, 256), (64, 128, 128), (128, 128, 128), (128, 256, 64), (256, 256, 64), (256, 512, 32), (512, 512, 32),
                (512, 512, 16))
# with and without act / add; the first layer's gradient lands on the image and has neither (car_conv3x3_backward refuses them there)
GRADIENT_CASES = tuple((s, e) for s in LAYER_SHAPES for e in (False, True) if not (s[0] == 3 and e))


def _pair_pm1(kind, b, h, w, seed):
    """tests/test_lpips.py's pairs, mapped to [-1, 1] in harness.lpips's arithmetic: x, and y unrelated / x + 0.05 normal / x + 1e-3 normal."""
    x = LR.make_image(seed, b, h, w)
    if kind == "unrelated":
        y = LR.make_image(seed + 1000, b, h, w)
    else:
        g = torch.Generator().manual_seed(seed + 2000 + KINDS.index(kind))
        y = x + {"noisy": 0.05, "near": 1e-3}[kind] * torch.randn(x.shape, generator=g)
    return tuple(((t.to(torch.float32) - 0.5) * 2).contiguous() for t in (x, y))


def _cotangent(b, seed):
    return 0.5 + torch.rand(b, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.fixture(scope="module")
def weights():
    return LR.seeded_weights(0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    return _lib.load()


# ---- CPU: the checker ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [((2, 16, 16, 14), "unrelated"), ((2, 16, 16, 14), "near"), ((1, 50, 70, 13), "noisy"), ((2, 33, 47, 15), "unrelated")],
                         ids=lambda c: f"B{c[0][0]}_{c[0][1]}x{c[0][2]}_{c[1]}")
def test_checker_equals_autograd_at_the_restatements_own_maps(weights, case):
    """1e-12 of each image's largest gradient entry: float64 rounding over the 13 layers and nothing else (odd sizes included)."""
    (b, h, w, seed), kind = case
    conv_w, conv_b, lin = weights
    x, y = _pair_pm1(kind, b, h, w, seed)
    g = _cotangent(b, seed)
    want_x, want_y = LBR.autograd(x, y, conv_w, conv_b, lin, g)
    acts = LR.layers(torch.cat([x, y]), conv_w, conv_b)
    got_x, got_y = LBR.vjp(acts, conv_w, lin, g)
    assert want_x.abs().max().item() > 0 and want_y.abs().max().item() > 0
    ex, ey = LBR.worst(got_x, want_x), LBR.worst(got_y, want_y)
    print(f"checker vs autograd {case}: {ex:.2e}, {ey:.2e} of the largest entry")
    assert ex <= 1e-12 and ey <= 1e-12


def test_head_backward_formula_equals_autograd_of_the_head(weights):
    conv_w, conv_b, lin = weights
    x, y = _pair_pm1("noisy", 2, 32, 40, 3)
    f0 = [t.clone().requires_grad_(True) for t in LR.taps(x, conv_w, conv_b)]
    f1 = [t.clone().requires_grad_(True) for t in LR.taps(y, conv_w, conv_b)]
    g = _cotangent(2, 3)
    total, _ = LR.head(f0, f1, lin)
    (total * g).sum().backward()
    for k in range(5):
        d0, d1 = LBR.head_backward(f0[k].detach(), f1[k].detach(), lin[k], g)
        assert LBR.worst(d0, f0[k].grad) <= 1e-12 and LBR.worst(d1, f1[k].grad) <= 1e-12, k
    # a pixel without features: the norm's derivative is taken as 0, the result is finite (and, against a pixel with features, not 0)
    z, o = torch.zeros(1, 64, 1, 1), torch.ones(1, 64, 1, 1)
    for a, b_ in ((z, z), (z, o), (o, z)):
        d0, d1 = LBR.head_backward(a, b_, lin[0], torch.ones(1))
        assert torch.isfinite(d0).all() and torch.isfinite(d1).all()
    assert LBR.head_backward(z, o, lin[0], torch.ones(1))[0].abs().max().item() > 0


def test_pool_backward_rule_is_torchs(weights):
    """The routing rule against autograd of max_pool2d on maps with equal positive values and all-zero windows, odd sizes included."""
    g = torch.Generator().manual_seed(5)
    for h, w in ((8, 8), (7, 10), (9, 5)):
        act = (F.relu(torch.randn(2, 6, h, w, generator=g, dtype=torch.float64)) * 2).round() / 2
        assert (act == 0).double().mean() > 0.2
        t = torch.randn(2, 6, h // 2, w // 2, generator=g, dtype=torch.float64)
        a = act.clone().requires_grad_(True)
        (F.max_pool2d(a, 2, 2) * t).sum().backward()
        assert torch.equal(LBR.pool_backward(t, act), a.grad), (h, w)


@pytest.mark.parametrize("case", E2E_CASES, ids=lambda c: f"B{c[0][0]}_{c[0][1]}x{c[0][2]}_{c[1]}")
def test_end_to_end_inputs_are_stable_in_float32(weights, case):
    """The condition on the end-to-end cases: the restatement's gradient in float32 has no entry further than 1e-4 of the image's largest
    from the float64 one (so float32-class arithmetic flips no decision that matters), and every tap pixel's channel norm exceeds 1e-6."""
    (b, h, w, seed), kind = case
    conv_w, conv_b, lin = weights
    x, y = _pair_pm1(kind, b, h, w, seed)
    g = torch.ones(b, dtype=torch.float64)
    w64 = LBR.autograd(x, y, conv_w, conv_b, lin, g)
    w32 = LBR.autograd(x, y, conv_w, conv_b, lin, g, dtype=torch.float32)
    worst = max(LBR.worst(a, b_) for a, b_ in zip(w32, w64))
    l2 = max(((a.double() - b_).norm() / b_.norm()).item() for a, b_ in zip(w32, w64))
    print(f"float32 restatement vs float64 {case}: worst entry {worst:.2e} of the largest, relative L2 {l2:.2e}")
    assert worst <= 1e-4
    for t in LR.taps(torch.cat([x, y]), conv_w, conv_b):
        assert t.pow(2).sum(1).sqrt().min().item() > 1e-6


# ---- CPU: the C entries, the wrapper, the script --------------------------------------------------------------------------------------

def test_backward_sizes(lib):
    pairs = list(zip(LR.WIDTHS[:-1], LR.WIDTHS[1:]))
    assert lib.car_lpips_backward_packed_floats() == sum(9 * k * n + 64 for k, n in pairs)
    assert lib.car_conv3x3_backward_packed_floats(256, 512) == 9 * 256 * 512 + 64 and lib.car_conv3x3_backward_packed_floats(512, 64) == 9 * 512 * 64 + 64
    for bad in ((3, 64), (3, 128), (64, 96), (32, 64), (1024, 64), (0, 0)):
        assert lib.car_conv3x3_backward_packed_floats(*bad) == 0, bad
    # the 13 maps of both images are (128 + 64 + 48 + 24 + 6) H W floats per image; the backward's own buffers come on top
    assert lib.car_lpips_train_workspace_bytes(1, 256, 256) >= 2 * 270 * 256 * 256 * 4
    assert lib.car_lpips_train_workspace_bytes(2, 50, 70) > lib.car_lpips_workspace_bytes(2, 50, 70)
    offs = [lib.car_lpips_train_layer_offset(2, 50, 70, l) for l in range(13)]
    assert offs[0] == 0 and all(o % 16 == 0 for o in offs)
    h, w = 50, 70
    for l in range(12):
        assert offs[l + 1] - offs[l] >= 4 * 4 * h * w * LR.WIDTHS[l], l
        if l + 1 in LR.POOL_BEFORE:
            h, w = h // 2, w // 2
    assert offs[12] + 4 * 4 * h * w * 512 <= lib.car_lpips_train_workspace_bytes(2, 50, 70)
    none = ctypes.c_size_t(-1).value
    assert lib.car_lpips_train_layer_offset(2, 50, 70, 13) == none and lib.car_lpips_train_layer_offset(2, 50, 70, -1) == none
    for bad in ((0, 64, 64), (-1, 64, 64), (1, 15, 64), (1, 64, 15), (1 << 20, 256, 256), (1, 1 << 15, 1 << 15)):
        assert lib.car_lpips_train_workspace_bytes(*bad) == 0, bad
        assert lib.car_lpips_train_layer_offset(*bad, 0) == none, bad


def test_backward_entries_refuse_bad_arguments(lib):
    """Every refusal happens before the device is touched, so host addresses stand in for the buffers (never dereferenced)."""
    buf = (ctypes.c_double * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    odd = p + 4

    def check(fn, name, good, cases):
        for kw, msg in cases:
            a = dict(good, **kw)
            assert fn(*a.values()) == -1, (name, kw)
            err = lib.car_last_error()
            assert err.startswith(name.encode() + b":") and msg in err, (name, kw, err)

    need = lib.car_lpips_train_workspace_bytes(1, 64, 64)
    good = dict(x=p, y=p, B=1, H=64, W=64, packed=p, lpips=p, per_tap=None, work=p, n=need, stream=None)
    check(lib.car_lpips_forward_train, "car_lpips_forward_train", good,
          [(dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(packed=None), b"null pointer"), (dict(lpips=None), b"null pointer"),
           (dict(work=None), b"null pointer"), (dict(B=0), b"B = 0"), (dict(B=-3), b"B = -3"), (dict(H=15), b"H >= 16"), (dict(W=15), b"W >= 16"),
           (dict(n=need - 1), b"workspace"), (dict(n=lib.car_lpips_workspace_bytes(1, 64, 64)), b"workspace"),
           (dict(B=1 << 20, H=256, W=256), b"too large"), (dict(H=1 << 15, W=1 << 15), b"too large"), (dict(packed=odd), b"aligned"),
           (dict(work=odd), b"aligned")])
    good = dict(g=p, gx=p, gy=p, B=1, H=64, W=64, packed=p, packed_backward=p, work=p, n=need, stream=None)
    check(lib.car_lpips_backward, "car_lpips_backward", good,
          [(dict(g=None), b"null pointer"), (dict(gx=None, gy=None), b"neither gx nor gy"), (dict(packed=None), b"null pointer"),
           (dict(packed_backward=None), b"null pointer"), (dict(work=None), b"null pointer"), (dict(B=0), b"B = 0"), (dict(H=15), b"H >= 16"),
           (dict(W=15), b"W >= 16"), (dict(n=need - 1), b"workspace"), (dict(B=1 << 20, H=256, W=256), b"too large"),
           (dict(packed=odd), b"aligned"), (dict(packed_backward=odd), b"aligned"), (dict(work=odd), b"aligned")])

    tables = (ctypes.c_void_p * 13)(*([p] * 13))
    holes = (ctypes.c_void_p * 13)(*([p] * 12 + [None]))
    good = dict(conv_w=tables, packed=p, stream=None)
    check(lib.car_lpips_pack_backward, "car_lpips_pack_backward", good,
          [(dict(conv_w=None), b"null pointer"), (dict(packed=None), b"null pointer"), (dict(conv_w=holes), b"layer 12"), (dict(packed=odd), b"aligned")])

    good = dict(D=p, n=1, H=8, W=8, K=64, N=64, packed=p, act=None, add=None, out=p, stream=None)
    check(lib.car_conv3x3_backward, "car_conv3x3_backward", good,
          [(dict(D=None), b"null pointer"), (dict(packed=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(K=3, N=128), b"3 -> 128"),
           (dict(K=96), b"96 -> 64"), (dict(N=1024), b"64 -> 1024"), (dict(K=3, act=p), b"must be NULL"), (dict(K=3, add=p), b"must be NULL"),
           (dict(n=0), b"0 images"), (dict(H=0), b"at least one pixel"), (dict(n=1 << 20, H=256, W=256), b"too large"), (dict(D=odd), b"aligned"),
           (dict(act=odd), b"aligned"), (dict(add=odd), b"aligned"), (dict(out=odd), b"aligned")])
    good = dict(w=p, K=64, N=128, packed=p, stream=None)
    check(lib.car_conv3x3_backward_pack, "car_conv3x3_backward_pack", good,
          [(dict(w=None), b"null pointer"), (dict(packed=None), b"null pointer"), (dict(K=5), b"5 -> 128"), (dict(K=3, N=64), b"3 -> 64"),
           (dict(packed=odd), b"aligned")])
    good = dict(T=p, act=p, add=None, n=1, H=8, W=8, C=64, out=p, stream=None)
    check(lib.car_maxpool2x2_backward, "car_maxpool2x2_backward", good,
          [(dict(T=None), b"null pointer"), (dict(act=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(H=1), b"H, W >= 2"),
           (dict(C=6), b"multiple of 4"), (dict(n=1 << 20, H=256, W=256), b"too large"), (dict(T=odd), b"aligned"), (dict(add=odd), b"aligned")])

    five, hole = (ctypes.c_void_p * 5)(*([p] * 5)), (ctypes.c_void_p * 5)(p, p, None, p, p)
    good = dict(feats=five, B=1, H=64, W=64, lin=p, g=p, gf0=five, gf1=None, stream=None)
    check(lib.car_lpips_head_backward, "car_lpips_head_backward", good,
          [(dict(feats=None), b"null pointer"), (dict(feats=hole), b"tap 2"), (dict(lin=None), b"null pointer"), (dict(g=None), b"null pointer"),
           (dict(gf0=None), b"neither gf0 nor gf1"), (dict(gf0=hole), b"tap 2"), (dict(gf1=hole), b"tap 2"), (dict(B=0), b"B = 0"),
           (dict(H=15), b"H >= 16"), (dict(W=15), b"W >= 16"), (dict(B=1 << 20, H=256, W=256), b"too large")])


def test_lpips_loss_refuses_cpu_tensors_and_bad_shapes(weights):
    from cross_attention_renderer_amd import harness
    w = harness.LpipsWeights(*weights)
    x = torch.rand(2, 16, 16, 3) * 2 - 1
    with pytest.raises(ValueError, match="no CPU fallback"):
        harness.lpips_loss(x, x, w)
    with pytest.raises(ValueError, match="no CPU fallback"):
        harness.lpips_loss(x.clone().requires_grad_(True), x, w)
    for a, b_ in ((x, x[:1]), (x[0], x[0]), (x.numpy(), x.numpy()), (torch.rand(2, 16, 16, 4), torch.rand(2, 16, 16, 4)), (x.double(), x.double())):
        with pytest.raises(ValueError):
            harness.lpips_loss(a, b_, w)


def test_train_script_refuses_lpips_without_weights_before_any_device(tmp_path):
    base = [sys.executable, TRAIN, "--experiment_name", "t", "--logging_root", str(tmp_path), "--lpips"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")           # a device that is opened anyway fails differently
    out = subprocess.run(base, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "backward" in out.stderr and "--lpips_weights" in out.stderr and "Traceback" not in out.stderr, out.stderr
    out = subprocess.run(base + ["--lpips_weights", "a", "b", "--query_sparsity", "1000"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "multiple of 1024" in out.stderr and "Traceback" not in out.stderr, out.stderr
    out = subprocess.run([sys.executable, TRAIN, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--lpips_coeff" in out.stdout


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def _nhwc(t):
    """[n, C, h, w] CPU -> channel-last float32 on the device."""
    return t.permute(0, 2, 3, 1).contiguous().float().to(abi.dev())


def _nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def _assert_parity(got, want, what):
    """|a - b| <= 1e-4 max(1, |b|) elementwise (tests/test_lpips.py's rule), the outermost rows and columns on their own; channel-last."""
    err = (got.detach().cpu().double() - want).abs() / want.abs().clamp_min(1.0)
    assert torch.isfinite(err).all(), what
    edge = torch.zeros(err.shape[1:3], dtype=torch.bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    worst_edge, worst = err[:, edge].max().item(), err.max().item()
    print(f"{what}: worst |a - b| / max(1, |b|) = {worst:.3e} (outermost rows and columns {worst_edge:.3e}), max |b| = {want.abs().max().item():.3f}")
    assert worst_edge <= 1e-4, (what, "border", worst_edge)
    assert worst <= 1e-4, (what, worst)


def _check_data_gradient(lib, shape, use_act, use_add):
    """D [2, side, side, N] -> [2, side, side, K] against float64 conv_transpose2d of the same float32 inputs with the same mask and
    `add`, scaled so that the largest result is about 5."""
    from cross_attention_renderer_amd import _lib
    K, N, side = shape
    g = torch.Generator().manual_seed(300 + LAYER_SHAPES.index(shape))
    w = (torch.randn(N, K, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * K)) ** 0.5).float()
    d = torch.randn(2, N, side, side, generator=g)
    scale = 1.0 / torch.tensor(LR.SCALE, dtype=torch.float64).view(1, 3, 1, 1) if K == 3 else 1.0

    def ref(dd):
        return F.conv_transpose2d(dd.double(), w.double(), stride=1, padding=1) * scale
    d = (d * (5.0 / ref(d).abs().max().item())).float()
    want = ref(d)
    act = F.relu(torch.randn(2, K, side, side, generator=g)).float()
    add = torch.randn(2, K, side, side, generator=g).float()
    if use_add:
        want = want + add.double()
    if use_act:
        want = want * (act > 0)
        assert 0.3 < (act > 0).double().mean().item() < 0.7
    assert 1.0 <= want.abs().max().item() <= 10.0
    wd = w.to(abi.dev()).contiguous()
    if K == 3:
        packed = torch.empty(lib.car_conv3x3_packed_floats(3, 64), dtype=torch.float32, device=abi.dev())
        bias = torch.zeros(64, device=abi.dev())
        _lib.check(lib.car_conv3x3_pack(wd.data_ptr(), bias.data_ptr(), 3, 64, packed.data_ptr(), abi.stream()), "car_conv3x3_pack")
    else:
        packed = torch.empty(lib.car_conv3x3_backward_packed_floats(K, N), dtype=torch.float32, device=abi.dev())
        _lib.check(lib.car_conv3x3_backward_pack(wd.data_ptr(), K, N, packed.data_ptr(), abi.stream()), "car_conv3x3_backward_pack")
    dd, ad, gd = _nhwc(d), (_nhwc(act) if use_act else None), (_nhwc(add) if use_add else None)
    out = torch.full((2, side, side, K), float("nan"), dtype=torch.float32, device=abi.dev())
    _lib.check(lib.car_conv3x3_backward(dd.data_ptr(), 2, side, side, K, N, packed.data_ptr(), ad.data_ptr() if use_act else None,
                                        gd.data_ptr() if use_add else None, out.data_ptr(), abi.stream()), "car_conv3x3_backward")
    torch.cuda.synchronize()
    what = " with " + " and ".join(n for n, u in (("act", use_act), ("add", use_add)) if u) if use_act or use_add else ""
    _assert_parity(out, want.permute(0, 2, 3, 1).contiguous(), f"data gradient of {K} -> {N} at {side} x {side}{what}")
    if use_act:
        assert (out.cpu()[~(act > 0).permute(0, 2, 3, 1)] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,epilogue", GRADIENT_CASES, ids=lambda v: f"{v[0]}to{v[1]}at{v[2]}" if isinstance(v, tuple) else ("act_add" if v else "plain"))
def test_data_gradient_matches_float64_conv_transpose2d(lib, shape, epilogue):
    """Each layer shape, swapped, with neither `act` nor `add` and with both."""
    _check_data_gradient(lib, shape, epilogue, epilogue)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 128, 128), (128, 256, 64), (256, 512, 32)], ids=lambda v: f"{v[0]}to{v[1]}at{v[2]}")
@pytest.mark.parametrize("which", ["act_only", "add_only"])
def test_data_gradient_epilogue_branches_on_their_own(lib, shape, which):
    """The epilogue's two optional operands one at a time, on one shape of each kernel instance (gradients 64, 128 and 256 wide): the
    chain reaches `act` alone through every non-tap layer, `add` alone never (a tap's `add` always meets its ReLU mask)."""
    _check_data_gradient(lib, shape, which == "act_only", which == "add_only")


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(8, 8), (7, 10), (50, 35)])
def test_pool_backward_is_exact(lib, hw):
    """Bit-exact against the routing rule on maps with equal positive values and all-zero windows, with and without `add`."""
    from cross_attention_renderer_amd import _lib
    h, w = hw
    g = torch.Generator().manual_seed(7)
    act = ((F.relu(torch.randn(3, 64, h, w, generator=g)) * 2).round() / 2).float()
    win = act[:, :, :h // 2 * 2, :w // 2 * 2].reshape(3, 64, h // 2, 2, w // 2, 2)
    top = win.amax((3, 5), keepdim=True)
    assert ((win == top).sum((3, 5)) > 1)[top[:, :, :, 0, :, 0] > 0].any() and (top == 0).any()
    t = torch.randn(3, 64, h // 2, w // 2, generator=g).float()
    add = torch.randn(3, 64, h, w, generator=g).float()
    routed = LBR.pool_backward(t, act)
    td, ad, gd = _nhwc(t), _nhwc(act), _nhwc(add)
    for use_add in (False, True):
        want = ((routed + add) if use_add else routed) * (act > 0)
        out = torch.full((3, h, w, 64), float("nan"), dtype=torch.float32, device=abi.dev())
        _lib.check(lib.car_maxpool2x2_backward(td.data_ptr(), ad.data_ptr(), gd.data_ptr() if use_add else None, 3, h, w, 64, out.data_ptr(), abi.stream()),
                   "car_maxpool2x2_backward")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want.permute(0, 2, 3, 1)), (hw, use_add)


def _gpu_head_backward(lib, f0, f1, lin, g, sides="xy"):
    """car_lpips_head_backward on lists of five [B, C, h, w] float32 CPU maps -> lists of five [B, h, w, C] CPU gradients (or None)."""
    from cross_attention_renderer_amd import _lib
    B, H, W = f0[0].shape[0], f0[0].shape[2], f0[0].shape[3]
    maps = [torch.cat([a, b]).permute(0, 2, 3, 1).contiguous().to(abi.dev()) for a, b in zip(f0, f1)]
    table = (ctypes.c_void_p * 5)(*[m.data_ptr() for m in maps])
    lin_d = torch.cat([w.float() for w in lin]).to(abi.dev())
    gd = g.double().to(abi.dev())
    outs, tabs = [], []
    for s in "xy":
        o = [torch.full((B, *m.shape[1:]), float("nan"), dtype=torch.float32, device=abi.dev()) for m in maps] if s in sides else None
        outs.append(o)
        tabs.append((ctypes.c_void_p * 5)(*[t.data_ptr() for t in o]) if o else None)
    _lib.check(lib.car_lpips_head_backward(table, B, H, W, lin_d.data_ptr(), gd.data_ptr(), tabs[0], tabs[1], abi.stream()), "car_lpips_head_backward")
    torch.cuda.synchronize()
    return [[t.cpu() for t in o] if o else None for o in outs]


@pytest.mark.gpu
def test_head_backward_matches_the_float64_formula(lib, weights):
    """Against the formula on the same float32 maps to one float32 rounding of the stored value (|a - b| <= 2^-23 |b|); bitwise equal
    across runs, between a pair alone and inside a batch, and whichever sides are asked for."""
    conv_w, conv_b, lin = weights
    x, y = _pair_pm1("noisy", 3, 50, 70, 31)
    f0 = [t.float() for t in LR.taps(x, conv_w, conv_b)]
    f1 = [t.float() for t in LR.taps(y, conv_w, conv_b)]
    g = _cotangent(3, 31)
    got = _gpu_head_backward(lib, f0, f1, lin, g)
    for k in range(5):
        want = [t.permute(0, 2, 3, 1) for t in LBR.head_backward(f0[k], f1[k], lin[k], g)]
        for side in range(2):
            a, b_ = got[side][k].double(), want[side]
            excess = ((a - b_).abs() - 2.0 ** -23 * b_.abs()).max().item()
            print(f"head backward tap {k} side {side}: worst |a - b| / |b| {((a - b_).abs() / b_.abs().clamp_min(1e-300)).max().item():.3e}, largest |b| {b_.abs().max().item():.3e}")
            assert b_.abs().max().item() > 0 and excess <= 0.0, (k, side, excess)
    again = _gpu_head_backward(lib, f0, f1, lin, g)
    for side in range(2):
        assert all(torch.equal(a, b_) for a, b_ in zip(got[side], again[side]))
    for i in (0, 2):
        one = _gpu_head_backward(lib, [t[i:i + 1] for t in f0], [t[i:i + 1] for t in f1], lin, g[i:i + 1])
        for side in range(2):
            assert all(torch.equal(a[0], b_[i]) for a, b_ in zip(one[side], got[side])), (i, side)
    only_x, only_y = _gpu_head_backward(lib, f0, f1, lin, g, "x"), _gpu_head_backward(lib, f0, f1, lin, g, "y")
    assert only_x[1] is None and only_y[0] is None
    assert all(torch.equal(a, b_) for a, b_ in zip(only_x[0], got[0])) and all(torch.equal(a, b_) for a, b_ in zip(only_y[1], got[1]))


@pytest.fixture(scope="module")
def dev_weights(weights):
    from cross_attention_renderer_amd import harness
    return harness.LpipsWeights(*weights)


def _chain(lib, dev_weights, x, y, g, sides="xy", maps=True, work=None):
    """car_lpips_forward_train + car_lpips_backward through the C ABI: (lpips [B], gx, gy, the 13 retained maps [2 B, C, h, w] float32 CPU).
    work: the caller's own workspace (a device tensor of bytes) in place of a fresh one of car_lpips_train_workspace_bytes."""
    from cross_attention_renderer_amd import _lib
    B, H, W, _ = x.shape
    xd, yd, gd = x.to(abi.dev()).contiguous(), y.to(abi.dev()).contiguous(), g.double().to(abi.dev())
    packed, packed_b = dev_weights.packed(abi.dev()), dev_weights.packed_backward(abi.dev())
    n = lib.car_lpips_train_workspace_bytes(B, H, W) if work is None else work.numel()
    work = torch.empty(n, dtype=torch.uint8, device=abi.dev()) if work is None else work
    out = torch.empty(B, dtype=torch.float64, device=abi.dev())
    _lib.check(lib.car_lpips_forward_train(xd.data_ptr(), yd.data_ptr(), B, H, W, packed.data_ptr(), out.data_ptr(), None, work.data_ptr(), n, abi.stream()),
               "car_lpips_forward_train")
    gx = torch.full((B, H, W, 3), float("nan"), dtype=torch.float32, device=abi.dev()) if "x" in sides else None
    gy = torch.full((B, H, W, 3), float("nan"), dtype=torch.float32, device=abi.dev()) if "y" in sides else None
    _lib.check(lib.car_lpips_backward(gd.data_ptr(), gx.data_ptr() if gx is not None else None, gy.data_ptr() if gy is not None else None, B, H, W,
                                      packed.data_ptr(), packed_b.data_ptr(), work.data_ptr(), n, abi.stream()), "car_lpips_backward")
    torch.cuda.synchronize()
    acts = []
    if maps:
        h, w = H, W
        for l in range(13):
            if l in LR.POOL_BEFORE:
                h, w = h // 2, w // 2
            off, c = lib.car_lpips_train_layer_offset(B, H, W, l), LR.WIDTHS[l]
            flat = work[off:off + 4 * 2 * B * h * w * c].view(torch.float32)
            acts.append(flat.view(2 * B, h, w, c).permute(0, 3, 1, 2).cpu())
    return out.cpu(), (gx.cpu() if gx is not None else None), (gy.cpu() if gy is not None else None), acts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
def test_chain_matches_the_checker_at_the_devices_own_maps(lib, weights, dev_weights, shape, kind):
    """The whole backward against the float64 vector-Jacobian product linearised at the 13 maps the device retained: every gradient
    entry within 1e-4 of the image's largest entry (the project's parity bar, normalised as tests/golden/grad_cases.py normalises
    gradients).  gx only, gy only and both give the same bits."""
    b, h, w, seed = shape
    conv_w, conv_b, lin = weights
    x, y = _pair_pm1(kind, b, h, w, seed)
    g = _cotangent(b, seed)
    value, gx, gy, acts = _chain(lib, dev_weights, x, y, g)
    want_x, want_y = LBR.vjp(acts, conv_w, lin, g)
    ex, ey = LBR.worst(gx, want_x), LBR.worst(gy, want_y)
    l2 = max(((a.double() - b_).norm() / b_.norm()).item() for a, b_ in ((gx, want_x), (gy, want_y)))
    print(f"chain {kind} B={b} {h}x{w}: worst entry {ex:.3e} (x) {ey:.3e} (y) of the image's largest, relative L2 {l2:.3e}, "
          f"largest entry {want_x.abs().max().item():.3e}")
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
    assert want_x.abs().max().item() > 0 and want_y.abs().max().item() > 0
    assert ex <= 1e-4 and ey <= 1e-4, (shape, kind, ex, ey)
    _, only_x, none_y, _ = _chain(lib, dev_weights, x, y, g, "x", maps=False)
    _, none_x, only_y, _ = _chain(lib, dev_weights, x, y, g, "y", maps=False)
    assert none_x is None and none_y is None
    assert torch.equal(only_x, gx) and torch.equal(only_y, gy)


@pytest.mark.gpu
def test_the_workspaces_are_exactly_as_large_as_their_size_entries_say(lib, dev_weights):
    """B = 1, 16 x 16 (the smallest image: the last tap is one pixel): car_lpips, then car_lpips_forward_train + car_lpips_backward, each
    over a workspace of exactly its size entry's bytes with NaN all around it, then over one twice as large.  Nothing is written outside
    either, and the values, the gradients and the 13 retained maps are the same bytes."""
    B, H, W = 1, 16, 16
    x, y = _pair_pm1("unrelated", B, H, W, 14)
    g = _cotangent(B, 14)
    xd, yd, packed = x.to(abi.dev()).contiguous(), y.to(abi.dev()).contiguous(), dev_weights.packed(abi.dev())

    def forward(work, wb):
        value, taps = abi.Guarded((B,), dtype=torch.float64), abi.Guarded((B, 5), dtype=torch.float64)
        assert lib.car_lpips(xd.data_ptr(), yd.data_ptr(), B, H, W, packed.data_ptr(), value.ptr, taps.ptr, work.ptr, wb, abi.stream()) == 0, lib.car_last_error()
        return value.get("lpips"), taps.get("per_tap")

    def chain(work, wb):
        value, gx, gy, acts = _chain(lib, dev_weights, x, y, g, work=work.view.view(torch.uint8))
        return (value, gx, gy, *acts)

    value, taps = abi.exact_then_twice(lib.car_lpips_workspace_bytes(B, H, W), forward, "car_lpips")
    assert bool((value > 0).all()) and bool(torch.isfinite(taps).all())
    n = lib.car_lpips_train_workspace_bytes(B, H, W)
    out = abi.exact_then_twice(n, chain, "car_lpips_forward_train + car_lpips_backward")
    assert bool((out[0] > 0).all()) and bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[2]).all())


def _decisions_differ(acts_dev, acts64, conv_w, conv_b, limit=20):
    """Lists the units whose ReLU sign or (for a window with a positive maximum) pool choice differs between the device's maps and the
    float64 restatement's: (what, layer, (image, channel, row, column), float64 pre-activation, the device's pre-activation recomputed in
    float64 from its own previous map)."""
    units = []

    def pre(acts, l):
        src = acts[l - 1].double()
        if l in LR.POOL_BEFORE:
            src = F.max_pool2d(src, 2, 2)
        return F.conv2d(src, conv_w[l].double(), conv_b[l].double(), stride=1, padding=1)
    for l in range(13):
        sign = (acts_dev[l] > 0) != (acts64[l] > 0)
        where = sign.nonzero()
        if l + 1 in LR.POOL_BEFORE:
            cd, c64 = LBR.pool_choice(acts_dev[l]), LBR.pool_choice(acts64[l])
            live = F.max_pool2d(acts64[l], 2, 2) > 0
            pw = ((cd != c64) & live).nonzero()
            for i in pw[:limit].tolist():
                n, c, oy, ox = i
                units.append(("pool choice", l, (n, c, oy, ox), acts64[l][n, c, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2].flatten().tolist(),
                              acts_dev[l][n, c, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2].flatten().tolist()))
            if len(pw) > limit:
                units.append(("pool choice", l, f"... {len(pw) - limit} more", None, None))
        if len(where):
            if l == 0:
                units.append(("relu sign", 0, f"{len(where)} units", None, None))
                continue
            p64, pdev = pre(acts64, l), pre(acts_dev, l)
            for i in where[:limit].tolist():
                units.append(("relu sign", l, tuple(i), p64[tuple(i)].item(), pdev[tuple(i)].item()))
            if len(where) > limit:
                units.append(("relu sign", l, f"... {len(where) - limit} more", None, None))
    return units


@pytest.mark.gpu
@pytest.mark.parametrize("case", E2E_CASES, ids=lambda c: f"B{c[0][0]}_{c[0][1]}x{c[0][2]}_{c[1]}")
def test_lpips_loss_backward_matches_float64_autograd(lib, weights, dev_weights, case):
    """harness.lpips_loss(...).backward() against unconstrained float64 autograd of the restatement, on the cases the CPU test above shows
    to be stable in float32.  The device's ReLU signs and pool choices are first compared with the float64 restatement's: where all agree
    the 1e-4 bound applies against plain autograd; where some differ each unit is printed and the bound against the checker at the
    device's own maps stands alone."""
    from cross_attention_renderer_amd import harness
    (b, h, w, seed), kind = case
    conv_w, conv_b, lin = weights
    x, y = _pair_pm1(kind, b, h, w, seed)
    g = torch.ones(b, dtype=torch.float64)
    xd, yd = x.to(abi.dev()).requires_grad_(True), y.to(abi.dev()).requires_grad_(True)
    loss = harness.lpips_loss(xd, yd, dev_weights)
    assert loss.dtype == torch.float64 and loss.shape == (b,)
    loss.sum().backward()
    gx, gy = xd.grad.cpu(), yd.grad.cpu()
    assert gx.dtype == torch.float32 and gx.shape == x.shape and gy.shape == y.shape
    value, cx, cy, acts = _chain(lib, dev_weights, x, y, g)
    assert torch.equal(value, loss.detach().cpu()) and torch.equal(cx, gx) and torch.equal(cy, gy)
    at_own = LBR.vjp(acts, conv_w, lin, g)
    own = max(LBR.worst(gx, at_own[0]), LBR.worst(gy, at_own[1]))
    want = LBR.autograd(x, y, conv_w, conv_b, lin, g)
    free = max(LBR.worst(gx, want[0]), LBR.worst(gy, want[1]))
    l2 = max(((a.double() - b_).norm() / b_.norm()).item() for a, b_ in ((gx, want[0]), (gy, want[1])))
    units = _decisions_differ(acts, LR.layers(torch.cat([x, y]), conv_w, conv_b), conv_w, conv_b)
    print(f"lpips_loss backward {kind} B={b} {h}x{w}: vs float64 autograd worst entry {free:.3e} of the largest, relative L2 {l2:.3e}; "
          f"vs the checker at the device's maps {own:.3e}; {len(units)} differing decisions")
    for u in units:
        print("  differs:", *u)
    assert own <= 1e-4, (case, own)
    if not units:
        assert free <= 1e-4, (case, free)


@pytest.mark.gpu
def test_exact_properties(dev_weights):
    """Identical images: gradient exactly 0.  Two runs: the same bits.  A cotangent scaled by 2^-20 or 2^20 scales every entry exactly
    (the rows' powers of two follow the gradient's magnitude).  The value is harness.lpips's, bit for bit."""
    from cross_attention_renderer_amd import harness
    for b, h, w, seed in ((2, 50, 70, 13), (12, 32, 32, 51)):
        img = ((LR.make_image(seed, b, h, w) - 0.5) * 2).contiguous().to(abi.dev())
        a, c = img.clone().requires_grad_(True), img.clone().requires_grad_(True)
        loss = harness.lpips_loss(a, c, dev_weights)
        loss.sum().backward()
        assert (loss == 0).all() and (a.grad == 0).all() and (c.grad == 0).all(), (b, h, w)

    def run(x, y, scale=1.0, sides=(True, True)):
        a, c = x.clone().requires_grad_(sides[0]), y.clone().requires_grad_(sides[1])
        loss = harness.lpips_loss(a, c, dev_weights)
        (loss * scale).sum().backward()
        return loss.detach(), a.grad, c.grad
    for (b, h, w, seed), kind in (((2, 50, 70, 13), "noisy"), ((12, 32, 32, 51), "unrelated")):
        x, y = (t.to(abi.dev()) for t in _pair_pm1(kind, b, h, w, seed))
        v0, gx0, gy0 = run(x, y)
        v1, gx1, gy1 = run(x, y)
        assert torch.equal(v0, v1) and torch.equal(gx0, gx1) and torch.equal(gy0, gy1)
        assert gx0.abs().max().item() > 0 and gy0.abs().max().item() > 0
        for k in (-20, 20):
            _, sx, sy = run(x, y, 2.0 ** k)
            assert torch.equal(sx, gx0 * 2.0 ** k) and torch.equal(sy, gy0 * 2.0 ** k), k
        # only the prediction needs a gradient in training: the same bits, and nothing for the other image
        _, nx, oy = run(x, y, sides=(False, True))
        assert nx is None and torch.equal(oy, gy0)
        # a pair's gradient does not depend on its place in the batch
        _, px, py = run(x[1:2], y[1:2])
        assert torch.equal(px[0], gx0[1]) and torch.equal(py[0], gy0[1])


@pytest.mark.gpu
def test_loss_value_is_harness_lpips_bit_for_bit(dev_weights):
    from cross_attention_renderer_amd import harness
    for (b, h, w, seed), kind in (((2, 50, 70, 13), "noisy"), ((12, 32, 32, 51), "unrelated"), ((1, 256, 256, 11), "near")):
        img = LR.make_image(seed, b, h, w).to(abi.dev())
        other = LR.make_image(seed + 7, b, h, w).to(abi.dev())
        want = harness.lpips(img, other, dev_weights)
        x, y = ((t.to(torch.float32) - 0.5) * 2 for t in (img, other))          # harness.lpips's own mapping
        got = harness.lpips_loss(x, y, dev_weights)
        assert got.dtype == torch.float64 and torch.equal(got, want), (b, h, w)


def _save_weights(weights, tmp_path):
    vgg, lin = LR.state_dicts(*weights, "split")
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    return [str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")]


@pytest.mark.gpu
def test_train_script_runs_with_the_lpips_term(weights, tmp_path):
    files = _save_weights(weights, tmp_path)
    out = subprocess.run([sys.executable, TRAIN, "--experiment_name", "t", "--views", "2", "--synthetic", "--lpips", "--lpips_weights", *files,
                          "--query_sparsity", "1024", "--batch_size", "2", "--img_sidelength", "64", "--max_steps", "3", "--steps_til_summary", "1",
                          "--logging_root", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("step ")]
    assert len(lines) == 3 and all("lpips" in l for l in lines), out.stdout
    terms = [float(l.split("lpips")[1].split()[0]) for l in lines]
    assert all(t > 0 and t == t for t in terms), terms
    assert os.path.exists(tmp_path / "t" / "checkpoints" / "model_final.pth")


@pytest.mark.gpu
@pytest.mark.parametrize("coeff", (0.1, 5.0))
def test_a_gradient_step_lowers_the_combined_loss_by_the_predicted_amount(dev_weights, coeff):
    """tests/test_grad_hip.py's step test with the reference's second-stage loss (loss_functions.py:100-118): L1 plus coeff x LPIPS of the
    32 x 32 patch each scene's 1024 rays form, through model(inp) in training mode.  One plain gradient step sized for a first-order
    decrease of 1 % must lower the loss by that amount to within the same factor 1.5.
    coeff = 0.1 is the reference's.  With the seeded lin weights (|normal| / C) LPIPS is some 25 times smaller than with the pretrained
    ones, so at 0.1 the term is 0.2 % of this loss and a wrong LPIPS gradient would go unnoticed; coeff = 5 gives it the share of the loss
    the pretrained weights give it at 0.1 (asserted: more than 5 %)."""
    import numpy as np
    from cross_attention_renderer_amd import harness, synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    dev = abi.dev()
    H, P = 64, 32
    torch.manual_seed(0)
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=P, with_encoder=False).train()
    S.perturb_parameters(m, seed=0)
    m.H = m.W = H
    m = m.to(dev)
    g = torch.Generator().manual_seed(3)
    grid = S.pixel_grid(H, H).view(H, H, 2)
    uv = grid[11:43, 20:52].reshape(1024, 2).contiguous()
    inp = S.stereo_scene(H, b=2, uv=uv, seed=5)
    inp = {k: {kk: (vv if kk in ("cam2world", "intrinsics") else vv.to(dev)) for kk, vv in v.items()} for k, v in inp.items()}
    z = [t.to(dev).requires_grad_(True) for t in S.feature_maps(2, 2, H, seed=1)]
    target = torch.tanh(torch.randn(2, 1, 1024, 3, generator=g)).to(dev)
    mask = torch.ones(2, device=dev)

    def loss_of():
        rgb = m(inp, z=z)["rgb"]
        gt_p, pred_p = target.reshape(-1, 32, 32, 3), rgb.reshape(-1, 32, 32, 3)
        term = harness.lpips_loss(gt_p * mask[:, None, None, None], pred_p * mask[:, None, None, None], dev_weights).mean()
        return (rgb - target).abs().mean() + coeff * term.to(rgb.dtype), term
    loss0, term0 = loss_of()
    share = coeff * term0.item() / loss0.item()
    assert term0.item() > 0 and (coeff < 1 or share > 0.05), (term0.item(), loss0.item())
    loss0.backward()
    leaves = [p for p in list(m.parameters()) + z if p.grad is not None]
    gnorm2 = sum((p.grad.double() ** 2).sum().item() for p in leaves)
    predicted = 0.01 * loss0.item()
    eta = predicted / gnorm2
    with torch.no_grad():
        for p in leaves:
            p -= eta * p.grad
    loss1 = loss_of()[0].item()
    drop = loss0.item() - loss1
    print(f"combined loss, coeff {coeff}: {loss0.item():.5f} (LPIPS term {term0.item():.5f}, {100 * share:.1f} % of the loss) -> {loss1:.5f}: "
          f"drop {drop:.3e}, predicted {predicted:.3e}")
    assert np.isfinite(loss1) and predicted / 1.5 <= drop <= predicted * 1.5, (loss0.item(), loss1, predicted)
