"""encoder_route = "device_train" (MultiViewDPTEncoder.vit_route = "device_train"): get_z's transformer blocks recorded through
car_vit_blocks_train and trained through car_vit_blocks_backward (include/car_encoder_train.h; encoder._VitBlocksTrain), on the seeded model
and the context pair of tests/golden/encoder_cases.py (b = 1), and the training script under --encoder_route device_train.

The gradients are judged against the float64 torch route run on the device, with the float32 torch route of the same model as yardstick:
every tensor's error over its largest |g64| is held to parity_rule.tolerance(the yardstick's).  What the figures look like: the seeded
model amplifies a rounding-sized difference (float32 torch against float64: 3e-3 to 3e-2 of a tensor's largest gradient), and torch's
float32 route is not reproducible from run to run on it (two backwards against twice one: 4e-2), so the yardstick is run YARD_RUNS times and
its largest ratio counts; the route's own quotient has a median of 0.12 (the route is as far from float64 as float32 torch is)."""
import contextlib
import functools
import os
import subprocess
import sys

import pytest
import torch

import abi_harness as AH
import parity_rule as PRU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")
F32, F64 = torch.float32, torch.float64
YARD_RUNS = 5


@functools.lru_cache(maxsize=None)
def _renderer():
    import encoder_cases as EC
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    m = CrossAttentionRenderer(model="midas_vit", n_view=2).eval()
    m.load_state_dict(EC.seeded_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}), strict=True)
    inp = {k: {kk: vv.to(AH.dev()) for kk, vv in v.items()} for k, v in EC.context_pair().items()}
    return m.to(AH.dev()), inp


def _names(m):
    """The parameters get_z reaches: the encoder's and conv_map's."""
    return [n for n, _ in m.named_parameters() if n.startswith(("encoder.", "conv_map."))]


def _cotangents(z):
    g = PRU.gen(21)
    return [torch.randn(t.shape, generator=g).to(t.device) for t in z]


@contextlib.contextmanager
def _blocks_input(enc, detached):
    """detached: the token array enters the blocks without its history, on either route — nothing flows back into the trunk."""
    if not detached:
        yield
        return
    hook = enc.pretrained.model.blocks[0].register_forward_pre_hook(lambda mod, args: (args[0].detach(),))
    recorded = enc._blocks_recorded_on_device
    enc._blocks_recorded_on_device = lambda tok, BV, T: recorded(tok.detach(), BV, T)
    try:
        yield
    finally:
        hook.remove()
        del enc._blocks_recorded_on_device


def _gradients(m, inp, route, dtype=F32, detached=False):
    """The gradients of sum_i <w_i, z_i> with respect to every parameter get_z reaches and to the context images -> ({name: grad}, z)."""
    m.encoder_route = route
    try:
        with _blocks_input(m.encoder, detached):
            inp = {k: dict(v) for k, v in inp.items()}
            rgb = inp["context"]["rgb"].to(dtype).requires_grad_(True)
            inp["context"]["rgb"] = rgb
            inp["context"]["cam2world"] = inp["context"]["cam2world"].to(dtype)
            z = m.get_z(inp)
            loss = sum((t * c.to(t.dtype)).sum() for t, c in zip(z, _cotangents(z)))
            named, names = dict(m.named_parameters()), _names(m)
            grads = torch.autograd.grad(loss, [rgb] + [named[n] for n in names], allow_unused=True)
            return dict(zip(["context.rgb"] + names, grads)), [t.detach() for t in z]
    finally:
        m.encoder_route = "torch"


@functools.lru_cache(maxsize=None)
def _reference_gradients(detached=False):
    """(float64 torch route on the device, [float32 torch route, YARD_RUNS times]): computed once.  torch's float32 route is not
    reproducible from run to run on this model (its convolution backwards), and the model amplifies a rounding-sized difference: the
    yardstick's ratio is taken as the largest of its runs."""
    m, inp = _renderer()
    g32 = [_gradients(m, inp, "torch", detached=detached)[0] for _ in range(YARD_RUNS)]
    m.double()
    try:
        g64, _ = _gradients(m, inp, "torch", F64, detached=detached)
    finally:
        m.float()
    host = lambda g: {k: (None if v is None else v.cpu()) for k, v in g.items()}
    return host(g64), [host(g) for g in g32]


def _yardstick(g32, name, ref, B):
    return max(PRU.ratio(g[name], ref, B) for g in g32)


def _get_z(m, inp, route):
    m.encoder_route = route
    try:
        with torch.no_grad():
            return [t.float().cpu() for t in m.get_z(inp)]
    finally:
        m.encoder_route = "torch"


def test_under_no_grad_device_train_is_the_device_route_bit_for_bit():
    """The same call and the same bits.  The blocks: the two routes' taps of one token array, bit for bit.  The whole get_z: bit for bit
    too where the torch stages around the blocks are themselves reproducible from call to call (two torch-route calls are compared
    first and the outcome printed); where they are not, the two routes are held to twice the fixture bound of each other."""
    m, inp = _renderer()
    enc = m.encoder
    tok = torch.randn(1, 514, 768, device=AH.dev(), generator=torch.Generator(device=AH.dev()).manual_seed(2))
    taps = {}
    with torch.no_grad():
        for route in ("device", "device_train"):
            enc.vit_route = route
            try:
                taps[route] = (enc._blocks_on_device if route == "device" else lambda *a: enc._blocks_inference(*a, True))(tok.clone(), tok, 2, 257)
            finally:
                enc.vit_route = "torch"
    for i in enc.VIT_TAPS:
        assert torch.equal(AH.bits(taps["device"][i]), AH.bits(taps["device_train"][i])), i
    t0, t1 = _get_z(m, inp, "torch"), _get_z(m, inp, "torch")
    a, b = _get_z(m, inp, "device_train"), _get_z(m, inp, "device")
    steady = all(torch.equal(AH.bits(x), AH.bits(y)) for x, y in zip(t0, t1))
    same = all(torch.equal(AH.bits(x), AH.bits(y)) for x, y in zip(a, b))
    print(f"[info] two torch-route get_z bit-equal: {steady}; device_train and device bit-equal: {same}")
    if steady:
        assert same
    for x, y in zip(a, b):
        rms = float(y.double().pow(2).mean().sqrt())
        assert float((x - y).abs().max()) <= 2 * (1e-3 * rms + 1e-6)
    m.encoder_route = "device_train"
    assert m.encoder_route == "device_train" and (m.encoder.trunk_route, m.encoder.vit_route, m.encoder.decoder_route) == ("torch", "device_train", "torch")
    m.encoder_route = "torch"


def test_gradients_match_the_float64_torch_route():
    """Every parameter get_z reaches, and the context images.  The recorded forward's z itself stays within the fixture bound of the torch
    route's (1e-3 rms + 1e-6, the bound the device route is held to)."""
    m, inp = _renderer()
    g64, g32 = _reference_gradients()
    got, z = _gradients(m, inp, "device_train")
    z_t = _get_z(m, inp, "torch")
    for i, (a, t) in enumerate(zip(z, z_t)):
        rms = float(t.double().pow(2).mean().sqrt())
        assert float((a.cpu() - t).abs().max()) <= 2 * (1e-3 * rms + 1e-6), i
    assert set(got) == set(g64) and [k for k in got if got[k] is None] == [k for k in g64 if g64[k] is None]
    worst, bad, quot = {}, [], {}
    for name, ref in g64.items():
        if ref is None:
            continue
        B = torch.full((), float(ref.abs().max()), dtype=F64)
        rk, ry = PRU.ratio(got[name].cpu(), ref, B), _yardstick(g32, name, ref, B)
        group = "blocks" if ".model.blocks." in name else "images" if name == "context.rgb" else "trunk" if "patch_embed" in name else "rest"
        quot.setdefault(group, []).append(rk / PRU.tolerance(ry))
        if group not in worst or rk / PRU.tolerance(ry) > worst[group][1] / PRU.tolerance(worst[group][2]):
            worst[group] = (name, rk, ry)
        if not rk <= PRU.tolerance(ry):
            bad.append((name, rk, ry))
    for group, (name, rk, ry) in sorted(worst.items()):
        print(f"[parity] get_z gradients, device_train, {group}: worst {rk / PRU.tolerance(ry):.3f} at {name} (route {rk:.2e} fp32 torch {ry:.2e} "
              f"tol {PRU.tolerance(ry):.2e}); over its {len(quot[group])} tensors the quotient's median is {sorted(quot[group])[len(quot[group]) // 2]:.3f}")
    assert not bad, bad[:8]


def test_the_blocks_own_gradients_with_their_input_detached():
    """The trunk's float32 error (its forward against the float64 trunk's, amplified through some fifty ReLU layers) is most of every
    figure of the test above, on both routes alike.  Here the token array enters the blocks detached, so that the gradient of the blocks'
    144 parameters passes through the decoder and the blocks only; same reference, same yardstick, same rule."""
    m, inp = _renderer()
    g64, g32 = _reference_gradients(True)
    got, _ = _gradients(m, inp, "device_train", detached=True)
    names = [n for n in g64 if ".model.blocks." in n]
    assert len(names) == 144 and all(got[n] is not None for n in names)
    assert got["encoder.pretrained.model.patch_embed.proj.weight"] is None            # nothing flows back through the token array
    quot, bad = [], []
    for n in names:
        B = torch.full((), float(g64[n].abs().max()), dtype=F64)
        rk, ry = PRU.ratio(got[n].cpu(), g64[n], B), _yardstick(g32, n, g64[n], B)
        quot.append((rk / PRU.tolerance(ry), n, rk, ry))
        if not rk <= PRU.tolerance(ry):
            bad.append((n, rk, ry))
    q, n, rk, ry = max(quot)
    print(f"[parity] get_z gradients, device_train, blocks with their input detached: worst {q:.3f} at {n} (route {rk:.2e} fp32 torch {ry:.2e} "
          f"tol {PRU.tolerance(ry):.2e}); median quotient {sorted(quot)[72][0]:.3f}")
    assert not bad, bad[:8]


def test_two_backwards_accumulate_and_a_step_reaches_the_next_forward():
    """Two recorded forwards and backwards without zero_grad give twice the gradient.  At the stage, where nothing but the route's own code
    runs: the gradient of the tokens and of the LayerNorm parameters doubles exactly (g + g, bit for bit — they are bit-reproducible), the
    matrices' and biases' to rounding (car_linear_wgrad's fp32 atomics order M = 514 terms per entry anew on every run: a relative
    2^-24 sqrt(514) of the terms' magnitudes, held at 2^-16 of the tensor's largest gradient).  Through the whole get_z torch's own
    backwards are not reproducible from run to run on this model, so the torch route's own deviation from doubling, measured here, is the
    yardstick there (parity_rule.tolerance of it).  Then an SGD step (torch's foreach update, which does not advance _version) moves the
    parameters and the next recorded forward sees them."""
    m, inp = _renderer()
    enc = m.encoder
    blocks = enc._vit_parameters()
    tok = torch.randn(1, 514, 768, device=AH.dev(), generator=torch.Generator(device=AH.dev()).manual_seed(3)).requires_grad_(True)
    w = [torch.randn(2, 257, 768, device=AH.dev(), generator=torch.Generator(device=AH.dev()).manual_seed(4 + i)) for i in range(2)]
    enc.vit_route = "device_train"
    try:
        m.zero_grad(set_to_none=True)
        for k in range(2):
            taps = enc._blocks_recorded_on_device(tok, 2, 257)
            sum((taps[i] * c).sum() for i, c in zip(enc.VIT_TAPS, w)).backward()
            if k == 0:
                g1 = [tok.grad.clone()] + [p.grad.clone() for p in blocks]
        for i, (p, g) in enumerate(zip([tok] + blocks, g1)):
            if i == 0 or (i - 1) % 12 in (0, 1, 6, 7):
                assert torch.equal(AH.bits(p.grad), AH.bits(g + g)), i
            else:
                assert float((p.grad - 2 * g).abs().max()) <= 2.0 ** -16 * float(g.abs().max()), i
    finally:
        enc.vit_route = "torch"
        m.zero_grad(set_to_none=True)

    names = _names(m)
    named = dict(m.named_parameters())
    params = [named[n] for n in names]
    before = [p.detach().clone() for p in params]

    def once(route):
        m.encoder_route = route
        try:
            z = m.get_z(inp)
            sum((t * c).sum() for t, c in zip(z, _cotangents(z))).backward()
            return [t.detach().float().cpu() for t in z]
        finally:
            m.encoder_route = "torch"

    def doubling(route):
        """max over the tensors of |g after two backwards - 2 g after one| / the largest |g|"""
        m.zero_grad(set_to_none=True)
        once(route)
        first = [None if p.grad is None else p.grad.detach().clone() for p in params]
        once(route)
        return max(float((p.grad - 2 * g).abs().max()) / float(g.abs().max()) for p, g in zip(params, first) if g is not None)
    try:
        d_torch, d_dev = doubling("torch"), doubling("device_train")
        print(f"[parity] get_z, two backwards against twice one: device_train {d_dev:.2e}, torch {d_torch:.2e} tol {PRU.tolerance(d_torch):.2e}")
        assert d_dev <= PRU.tolerance(d_torch)
        m.zero_grad(set_to_none=True)
        z0 = once("device_train")
        used = [p for p in params if p.grad is not None]
        top = max(float(p.grad.abs().max()) for p in used)
        torch.optim.SGD(used, lr=1e-2 / top).step()
        assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before) if p.grad is not None)
        m.zero_grad(set_to_none=True)
        z1 = once("device_train")
        m.zero_grad(set_to_none=True)
        z1_t = _get_z(m, inp, "torch")
        rms = float(z1_t[0].double().pow(2).mean().sqrt())
        assert float((z1[0] - z0[0]).abs().max()) > 1e-3 * rms, "the recorded forward did not see the new parameters"
        assert float((z1[0] - z1_t[0]).abs().max()) <= 2 * (1e-3 * rms + 1e-6)
    finally:
        with torch.no_grad():
            for p, b in zip(params, before):
                p.copy_(b)
        m.zero_grad(set_to_none=True)
        m.encoder.drop_device_caches()


def test_guards():
    m, inp = _renderer()
    enc = m.encoder
    tok = torch.randn(1, 514, 768, device=AH.dev(), generator=torch.Generator(device=AH.dev()).manual_seed(1))
    enc.vit_route = "device_train"
    try:
        # a parameter modified in place between forward and backward
        p = enc.pretrained.model.blocks[3].mlp.fc1.bias
        taps = enc._blocks_recorded_on_device(tok.clone().requires_grad_(True), 2, 257)
        with torch.no_grad():
            p.add_(0.0)                                                 # the values stay, the version moves
        with pytest.raises(RuntimeError, match="modified in place between forward and backward"):
            sum(t.sum() for t in taps.values()).backward()
        # once differentiable
        leaf, c = tok.clone().requires_grad_(True), torch.ones(2, 257, 768, device=AH.dev(), requires_grad=True)
        taps = enc._blocks_recorded_on_device(leaf, 2, 257)
        (g,) = torch.autograd.grad(sum((t * c).sum() for t in taps.values()), leaf, create_graph=True)      # the cotangent itself has a history
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()
        # no fallback
        with pytest.raises(ValueError, match="CPU tensors run on vit_route = 'torch'"):
            enc._blocks_recorded_on_device(tok.cpu().requires_grad_(True), 2, 257)
        with pytest.raises(ValueError, match="computes in float32"):
            enc._blocks_recorded_on_device(tok.double().requires_grad_(True), 2, 257)
    finally:
        enc.vit_route = "torch"
        m.zero_grad(set_to_none=True)
    # the inference routes still refuse a forward that autograd would record
    assert torch.is_grad_enabled()
    for route in ("device", "device_trunk", "device_full"):
        m.encoder_route = route
        try:
            with pytest.raises(ValueError, match="is inference only"):
                m.get_z(inp)
        finally:
            m.encoder_route = "torch"
    with pytest.raises(ValueError, match="vit_route must be"):
        enc.vit_route = "device_training"
    with pytest.raises(ValueError, match="'device_train'"):
        m.encoder_route = "device_training"


def _train(tmp_path, name, route):
    cmd = [sys.executable, TRAIN, "--experiment_name", name, "--views", "2", "--img_sidelength", "256", "--batch_size", "2", "--max_steps", "2",
           "--steps_til_summary", "1", "--logging_root", str(tmp_path), "--query_sparsity", "192", "--with_encoder", "--encoder_route", route]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    losses = [float(l.split("loss ")[1].split()[0]) for l in out.stdout.splitlines() if l.startswith("step ")]
    assert len(losses) == 2, out.stdout
    return losses, torch.load(tmp_path / name / "checkpoints" / "model_final.pth", map_location="cpu")["model"]


def test_the_training_script_trains_through_the_device_route(tmp_path):
    """Two steps on synthetic scenes with the encoder, 2 scenes x 192 rays, under --encoder_route device_train and under torch.  The first
    step's loss is a mean of |gt - rgb| over colours in [-1, 1]; the two routes' z agree within the get_z fixture bound, 1e-3 of a
    level's rms, and the loss is held to the same relative step: |difference| <= 1e-3 (1 + loss).  Both steps finite; the parameters moved."""
    dev_l, dev_ck = _train(tmp_path, "dev", "device_train")
    tor_l, tor_ck = _train(tmp_path, "tor", "torch")
    print(f"[train] first-step loss: device_train {dev_l[0]:.6f} torch {tor_l[0]:.6f}; second step {dev_l[1]:.6f} / {tor_l[1]:.6f}")
    assert all(l == l and abs(l) < float("inf") for l in dev_l)
    assert abs(dev_l[0] - tor_l[0]) <= 1e-3 * (1 + abs(tor_l[0]))
    # the script seeds the model: the torch run started from the same values, so what differs from a fresh model has moved
    sys.path.insert(0, os.path.join(ROOT, "experiment_scripts"))
    import common
    opt = common.parser("t").parse_args(["--experiment_name", "x", "--views", "2", "--img_sidelength", "256", "--with_encoder"])
    fresh = common.build_model(opt, "cpu").state_dict()
    moved = [k for k in fresh if ".model.blocks." in k and not torch.equal(fresh[k], dev_ck[k])]
    assert len(moved) == 144 and all(bool(torch.isfinite(dev_ck[k]).all()) for k in dev_ck)
