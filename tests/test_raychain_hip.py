"""The two per-ray chain kernels (csrc/car_raychain.hip) and car_finalize, each through the C ABI against tests/raychain_reference.py:
car_chain_packed_floats, car_chain_pack, car_ray_mid, car_ray_tail, car_finalize, their refusals, and the tables car_plan_build /
car_render_forward assemble for them.

Tolerance, measured against the reference and never against the kernel: for every output, ratio = max over entries of
|got - ref64| / B_last (the last layer's sum of magnitudes, float64); the same ratio is computed for the restatement run in float32 on
the CPU on the same inputs, and the kernel must satisfy  ratio_kernel <= 8 x max(ratio_fp32, 2^-22)  — 4 because the kernels' operands
keep 22 bits against fp32's 24 (car_split.h), 2 for the spread of a maximum over a few thousand entries.  Every test prints
ratio_kernel / tolerance as a ``[parity]`` line (profiles/raychain_parity.md).  Every output lies inside a larger NaN-filled buffer: the
margins must come back untouched, so rows >= M are never written; row padding of the inputs holds inf (ebar) or NaN (phi_x, rays)."""
import ctypes
import functools

import pytest
import torch

import abi_harness as abi
import raychain_reference as RC
from abi_harness import CAR_E_ARG, NAN, Guarded
from parity_rule import judge

pytestmark = pytest.mark.gpu


def _padded(t, ld, fill):
    """t [M, K] as rows of stride ld on the device, the padding holding `fill`."""
    M, K = t.shape
    out = torch.full((M, ld), fill, dtype=torch.float32)
    out[:, :K] = t
    return out.contiguous().to(abi.dev())


def run_mid(lib, T, ebar, ld_ebar=RC.C):
    M = ebar.shape[0]
    e = _padded(ebar, ld_ebar, float("inf"))
    z1, uh = Guarded((M, RC.E)), Guarded((M, RC.D))
    rc = lib.car_ray_mid(abi.ptr(T.arena), T.offs, T.nts, T.n_chunks, abi.ptr(T.bias), abi.ptr(T.scale), T.layers, T.n_layers, abi.ptr(e), ld_ebar, z1.ptr, uh.ptr, M,
                         abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return {"z1": z1.get("z1"), "uh": uh.get("uh")}


def run_tail(lib, T, ebar, phi_x, z1, overlaps, ld_ebar=RC.C, ld_phi=20):
    b, V, R = overlaps.shape
    M = b * R
    assert ebar.shape[0] == M
    e, px = _padded(ebar, ld_ebar, float("inf")), _padded(phi_x, ld_phi, NAN)
    zin, rays = z1.float().contiguous().to(abi.dev()), RC.rays_from_overlaps(overlaps).to(abi.dev())
    rgb, valid = Guarded((M, 3)), Guarded((M, 1))
    rc = lib.car_ray_tail(abi.ptr(T.arena), T.offs, T.nts, T.n_chunks, abi.ptr(T.bias), abi.ptr(T.scale), T.layers, T.n_layers, abi.ptr(e), ld_ebar, abi.ptr(px), ld_phi,
                          abi.ptr(zin), abi.ptr(rays), b, V, R, rgb.ptr, valid.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return {"rgb": rgb.get("rgb"), "valid": valid.get("valid")[:, 0]}


def run_finalize(lib, rgb_in, ld_in, overlaps):
    b, V, R = overlaps.shape
    src, rays = _padded(rgb_in[:, :3], ld_in, NAN), RC.rays_from_overlaps(overlaps).to(abi.dev())
    rgb, valid = Guarded((b * R, 3)), Guarded((b * R, 1))
    rc = lib.car_finalize(abi.ptr(rays), abi.ptr(src), ld_in, b, V, R, rgb.ptr, valid.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return rgb.get("rgb"), valid.get("valid")[:, 0]


@functools.lru_cache(maxsize=None)
def _tables(which, key="gauss"):
    """The canonical tables (the plan's slots, consumption order, no gaps) of a weight set, built once."""
    params = {"gauss": lambda: RC.gaussian_params(1), "scale0": lambda: RC.case(which + "-scale0")["params"],
              "scale1": lambda: RC.case(which + "-scale1")["params"], "scale2": lambda: RC.case("tail-scale2")["params"], "int": lambda: RC.integer_case()[0]}[key]()
    return RC.ChainTables(abi.lib(), params, which, abi.dev(), stream=abi.stream())


@functools.lru_cache(maxsize=None)
def _reference(tag):
    """The case, its float64 run and its float32 run, computed once and shared."""
    c = RC.case(tag)
    if tag.startswith("mid"):
        return c, RC.mid(c["params"], c["ebar"]), RC.mid(c["params"], c["ebar"], torch.float32)
    args = (c["params"], c["ebar"], c["phi_x"], c["z1"], c["overlaps"], c["V"])
    return c, RC.tail(*args), RC.tail(*args, torch.float32)


def _judge(test, case, got, ref, f32, pairs):
    """Every output finite and held to the float32 restatement's own ratio against the same float64 run and bound."""
    judge(test, case, {k: ((got[k], ref[k], ref[bk]), RC.ratio(f32[k], ref[k], ref[bk])) for k, bk in pairs}, finite=True)


MID_PAIRS = (("z1", "B_z1"), ("uh", "B_uh"))
TAIL_PAIRS = (("rgb", "B_rgb"),)


def _check_tail(test, tag, key="gauss", lds=((RC.C, 20),)):
    c, ref, f32 = _reference(tag)
    for ld_ebar, ld_phi in lds:
        got = run_tail(abi.lib(), _tables("tail", key), c["ebar"], c["phi_x"], c["z1"], c["overlaps"], ld_ebar, ld_phi)
        assert torch.equal(got["valid"].double(), ref["valid"])
        _judge(test, f"{tag} ld_ebar {ld_ebar} ld_phi {ld_phi}", got, ref, f32, TAIL_PAIRS)
    return c, ref, got


def _check_mid(test, tag, key="gauss", lds=(RC.C,)):
    c, ref, f32 = _reference(tag)
    for ld in lds:
        got = run_mid(abi.lib(), _tables("mid", key), c["ebar"], ld)
        _judge(test, f"{tag} ld_ebar {ld}", got, ref, f32, MID_PAIRS)
    return c, ref, got


# ---- 1. Gaussian weights and inputs at every shape ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", RC.MID_M)
def test_ray_mid_matches_fp64(M):
    """One live ray of 32, a full wave, one ray into the next wave / workgroup (the lrow clamp and the row < M store guards), several
    workgroups; ebar rows 576, 580 and 640 apart with inf between them."""
    _check_mid("ray_mid", f"mid-gauss-{M}", lds=RC.LD_EBAR)


@pytest.mark.parametrize("shape", RC.TAIL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ray_tail_matches_fp64(shape):
    """V = 1, 2, 3 (zscale and the mask's views), a scene boundary inside a workgroup, M = 129, three workgroups; every row stride of
    ebar and phi_x, inf / NaN in the padding (and in columns 18, 19 of phi_x)."""
    _check_tail("ray_tail", "tail-gauss-" + "-".join(map(str, shape)), lds=[(a, p) for a in RC.LD_EBAR for p in RC.LD_PHI])


# ---- 2. magnitudes and zero rows ----------------------------------------------------------------------------------------------------
def test_rows_ten_orders_of_magnitude_apart_and_zero_rows():
    """Every wave holds rows from 1e-6 to 1e4 (the per-ray power of two); an all-zero ebar row (m = 0: pow2_scale on its clamp) gives
    z1 == latent_value.bias exactly; rows non-zero only at column 575 / column 0.  z1 lands at 0.9 of the tolerance here (1.7e-6 of
    B_z1 against float32's 1.6e-7) — read from the code, not measured: add_bias runs before layer_global, so on rays around 1e-5 the
    products are added to an accumulator that already holds the bias and round at the bias's ulp (profiles/raychain_parity.md).  The
    headroom is 10 % against the fixed 2^-22 floor: a change of the summation order in layer_global may trip this case.  That is the
    signal it is there to give; the answer is to look at the order, never to raise parity_rule.FACTOR."""
    c, ref, got = _check_mid("magnitudes", "mid-mag", lds=(RC.C, 580))
    s = c["special"]
    assert torch.equal(got["z1"][s["zero"]], c["params"]["latent_value.bias"])
    _check_tail("magnitudes", "tail-mag", lds=((RC.C, 20), (640, 24)))


# ---- 3. layer scales ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ("scale0", "scale1", "scale2"))
def test_layers_with_tiny_large_and_zero_weights(key):
    """encode_latent x 2^-20 and fc_0 of block 1 x 2^10 (the per-layer power of two and its exact undoing); then lin_z.2 all zero (its
    scale on pow2_scale's clamp: the layer contributes its bias); then (scale2, the tail's layers only) lin_z.0 with its first half zero
    and lin_z.1 with its second half x 2^4: the power of two of a layer with W2 must come from max |W + W2|."""
    if key != "scale2":
        _check_mid("layer_scales", f"mid-{key}", key)
    _check_tail("layer_scales", f"tail-{key}", key)


# ---- 4. exact integers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld_ebar,ld_phi", ((RC.C, 20), (580, 24)))
def test_integer_weights_and_inputs_are_reproduced_bit_for_bit(ld_ebar, ld_phi):
    """Weights of +-1 (two per row; lin_z two per half, the halves different), integer biases and inputs, every partial sum below 2^22
    (test_raychain_reference.py asserts it, and that the wide rays' operands have non-zero lo halves): z1, uh and rgb must equal the
    float64 reference bit for bit — the chained and the standard K order of every layer, the hi / lo recombination, the bias offsets
    and the exact undoing of both powers of two; the rays RC.INT_DEAD reach fc_0 of block 0 with nothing positive (m = 0)."""
    params, ebar, z1, phi_x = RC.integer_case()
    M = ebar.shape[0]
    ov = RC.random_overlaps(1, RC.INT_V, M, 3)
    m64 = RC.mid(params, ebar)
    t64 = RC.tail(params, ebar, phi_x, z1, ov, RC.INT_V)
    m = run_mid(abi.lib(), _tables("mid", "int"), ebar, ld_ebar)
    t = run_tail(abi.lib(), _tables("tail", "int"), ebar, phi_x, z1, ov, ld_ebar, ld_phi)
    for k, got, want in (("z1", m["z1"], m64["z1"]), ("uh", m["uh"], m64["uh"]), ("rgb", t["rgb"], t64["rgb"]), ("valid", t["valid"], t64["valid"])):
        wrong = (got.double() != want)
        assert not bool(wrong.any()), (k, int(wrong.sum()), (got.double() - want).abs().max().item())
    live = t64["valid"] > 0
    assert bool((t64["rgb"][live].abs() > 2 ** 12).any()) and bool(live[list(RC.INT_DEAD)].any())


# ---- 5. tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("mid", "tail"))
def test_arena_order_gaps_and_scale_slots_do_not_change_a_bit(which):
    """The same layers with their arena order reversed, with 64-float gaps (NaN) between them, and with other scale slots (the tail on
    the plan's 0, 3, 4 ... 13 and on a shuffled set): only consistent tables, and every arrangement bit-identical to the canonical one."""
    lib, params = abi.lib(), RC.gaussian_params(1)
    c = RC.case("mid-gauss-161" if which == "mid" else "tail-gauss-2-2-80")
    n = 3 if which == "mid" else 12
    shuffled = [int(i) for i in torch.randperm(16, generator=RC.gen(2))[:n]]
    assert shuffled != sorted(shuffled)
    arrangements = {"canonical": dict(slots=range(n)), "reversed": dict(slots=range(n), arena_order=range(n - 1, -1, -1)),
                    "gaps": dict(slots=range(n), gap=64), "plan slots": dict(slots=RC.PLAN_SLOTS[which]), "shuffled slots": dict(slots=shuffled),
                    "all": dict(slots=shuffled, gap=64, arena_order=[int(i) for i in torch.randperm(n, generator=RC.gen(3))])}
    outs = {}
    for name, kw in arrangements.items():
        T = RC.ChainTables(lib, params, which, abi.dev(), stream=abi.stream(), **kw)
        used = torch.zeros(32, dtype=torch.bool)
        used[list(T.slots)] = True
        used[[16 + s for s in T.slots]] = True
        sc = T.scale.cpu()
        assert bool(torch.isfinite(sc[used]).all()) and bool(torch.isnan(sc[~used]).all()), f"{name}: car_chain_pack wrote another slot"
        outs[name] = run_mid(lib, T, c["ebar"]) if which == "mid" else run_tail(lib, T, c["ebar"], c["phi_x"], c["z1"], c["overlaps"])
    for name, o in outs.items():
        for k, v in o.items():
            assert torch.equal(v, outs["canonical"][k]), (name, k)


# ---- 6. valid mask ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (1, 2, 3))
def test_valid_mask_and_white_background_are_exact(V):
    """overlaps in {0, 1}: no view, the first only, the last only, all views, ray by ray.  valid exact; an invalid ray's rgb exactly
    1.0; a valid ray's rgb what an all-valid run gives, bit for bit; valid equal to car_finalize's on the same rays."""
    lib, b, R = abi.lib(), 2, 42
    ebar, z1, phi_x = RC.gaussian_inputs(b * R, 50 + V)
    pat = torch.arange(b * R).reshape(b, R) % 4
    ov = torch.zeros(b, V, R)
    ov[:, 0][(pat == 1) | (pat == 3)] = 1.0
    ov[:, V - 1][(pat == 2) | (pat == 3)] = 1.0
    if V == 3:
        ov[:, 1][pat == 3] = 1.0
    want = (pat != 0).float().reshape(-1)
    T = _tables("tail")
    got = run_tail(lib, T, ebar, phi_x, z1, ov)
    full = run_tail(lib, T, ebar, phi_x, z1, torch.ones(b, V, R))
    assert torch.equal(got["valid"], want) and bool((full["valid"] == 1.0).all())
    assert bool((got["rgb"][want == 0] == 1.0).all())
    assert torch.equal(got["rgb"][want == 1], full["rgb"][want == 1]) and bool((full["rgb"] != 1.0).all())
    rgb_f, valid_f = run_finalize(lib, full["rgb"], 3, ov)
    assert torch.equal(valid_f, got["valid"]) and torch.equal(rgb_f, got["rgb"])


# ---- 7. car_finalize alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld_in", (3, 4, 7))
def test_finalize_matches_the_blend_exactly(ld_in):
    """b R = 666: three 256-thread blocks, the last one partial; NaN in the row padding of rgb_in and around overlaps."""
    b, V, R = 2, 3, 333
    rgb_in = torch.randn(b * R, 3, generator=RC.gen(60)) * 3
    ov = RC.random_overlaps(b, V, R, 61, p=0.25)
    want_rgb, want_valid = RC.finalize(rgb_in, ov)
    assert 0 < want_valid.sum().item() < b * R
    rgb, valid = run_finalize(abi.lib(), rgb_in, ld_in, ov)
    assert torch.equal(valid, want_valid) and torch.equal(rgb, want_rgb)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
# every entry's arguments in the order of its C signature (include/car_hip.h); a call is built from this tuple, name by name
ARGS = {"car_ray_mid": ("arena", "offs", "nts", "n_chunks", "bias", "scale", "layers", "n_layers", "ebar", "ld_ebar", "z1", "uh", "M", "stream"),
        "car_ray_tail": ("arena", "offs", "nts", "n_chunks", "bias", "scale", "layers", "n_layers", "ebar", "ld_ebar", "phi_x", "ld_phi", "z1_in", "rays",
                         "b", "V", "R", "rgb", "valid", "stream"),
        "car_chain_pack": ("W", "ldw", "W2", "K", "N", "chained", "packed", "scale", "slot", "stream"),
        "car_finalize": ("rays", "rgb_in", "ld_in", "b", "V", "R", "rgb", "valid", "stream")}
OUTPUTS = {"car_ray_mid": ("z1", "uh"), "car_ray_tail": ("rgb", "valid"), "car_chain_pack": ("packed", "scale"), "car_finalize": ("rgb", "valid")}
REF_M, REF_B, REF_V, REF_R = 5, 1, 2, 5


def _entry_arguments(entry):
    """The accepted arguments of one entry by name (device pointers as c_void_p), its Guarded outputs, and the substitutes a refusal
    may name: rows of another stride, slot lists and tile counts that are out of range."""
    M, dev = REF_M, abi.dev()
    if entry == "car_chain_pack":
        n = int(abi.lib().car_chain_packed_floats(128, 128))
        outs = {"packed": Guarded((1, n)), "scale": Guarded((1, 32))}
        keep = {"W": torch.zeros(128, 144, device=dev)}
        args = dict(W=abi.ptr(keep["W"]), ldw=144, W2=None, K=128, N=128, chained=1, packed=outs["packed"].ptr, scale=outs["scale"].ptr, slot=0, stream=abi.stream())
        return args, outs, {}, keep
    keep = {"rays": RC.rays_from_overlaps(torch.ones(REF_B, REF_V, REF_R)).to(dev)}
    if entry == "car_finalize":
        outs = {"rgb": Guarded((M, 3)), "valid": Guarded((M, 1))}
        keep["rgb_in"] = torch.zeros(M, 4, device=dev)
        args = dict(rays=abi.ptr(keep["rays"]), rgb_in=abi.ptr(keep["rgb_in"]), ld_in=4, b=REF_B, V=REF_V, R=REF_R, rgb=outs["rgb"].ptr, valid=outs["valid"].ptr,
                    stream=abi.stream())
        return args, outs, {}, keep
    which = "mid" if entry == "car_ray_mid" else "tail"
    T = _tables(which)
    for ld in (572, 576, 578):
        keep[f"e{ld}"] = torch.zeros(M, ld, device=dev)
    for ld in (16, 20, 22):
        keep[f"px{ld}"] = torch.zeros(M, ld, device=dev)
    keep["zin"] = torch.zeros(M, RC.E, device=dev)
    subs = {f"e{ld}": abi.ptr(keep[f"e{ld}"]) for ld in (572, 578)}
    subs.update({f"px{ld}": abi.ptr(keep[f"px{ld}"]) for ld in (16, 22)})
    subs["slot16"] = (ctypes.c_int * T.n_layers)(*([0] * (T.n_layers - 1) + [16]))
    subs["tiles2"] = (ctypes.c_int * T.n_chunks)(*([2] + list(T.nts)[1:]))
    subs["tiles10"] = (ctypes.c_int * T.n_chunks)(*([10] + list(T.nts)[1:]))
    args = dict(arena=abi.ptr(T.arena), offs=T.offs, nts=T.nts, n_chunks=T.n_chunks, bias=abi.ptr(T.bias), scale=abi.ptr(T.scale), layers=T.layers,
                n_layers=T.n_layers, ebar=abi.ptr(keep["e576"]), ld_ebar=576, stream=abi.stream())
    if which == "mid":
        outs = {"z1": Guarded((M, RC.E)), "uh": Guarded((M, RC.D))}
        args.update(z1=outs["z1"].ptr, uh=outs["uh"].ptr, M=M)
    else:
        outs = {"rgb": Guarded((M, 3)), "valid": Guarded((M, 1))}
        args.update(phi_x=abi.ptr(keep["px20"]), ld_phi=20, z1_in=abi.ptr(keep["zin"]), rays=abi.ptr(keep["rays"]), b=REF_B, V=REF_V, R=REF_R, rgb=outs["rgb"].ptr,
                    valid=outs["valid"].ptr)
    return args, outs, subs, keep


def _call(entry, args):
    assert set(args) == set(ARGS[entry])
    return getattr(abi.lib(), entry)(*[args[k] for k in ARGS[entry]])


_CHAIN_BAD = [("n_chunks 0", dict(n_chunks=0)), ("n_chunks 97", dict(n_chunks=97)), ("slot 16", dict(layers="slot16")),
              ("ld_ebar 572", dict(ebar="e572", ld_ebar=572)), ("ld_ebar 578", dict(ebar="e578", ld_ebar=578)), ("2 tiles", dict(nts="tiles2")),
              ("10 tiles", dict(nts="tiles10"))]
REFUSALS = [("car_ray_mid", w, c) for w, c in [("n_layers 12", dict(n_layers=12)), ("n_layers 2", dict(n_layers=2))] + _CHAIN_BAD]
REFUSALS += [("car_ray_mid", f"null {k}", {k: None}) for k in ("arena", "offs", "nts", "bias", "scale", "layers", "ebar", "z1", "uh")]
REFUSALS += [("car_ray_tail", w, c) for w, c in [("n_layers 3", dict(n_layers=3)), ("n_layers 13", dict(n_layers=13))] + _CHAIN_BAD +
             [("ld_phi 16", dict(phi_x="px16", ld_phi=16)), ("ld_phi 22", dict(phi_x="px22", ld_phi=22))]]
REFUSALS += [("car_ray_tail", f"null {k}", {k: None})
             for k in ("arena", "offs", "nts", "bias", "scale", "layers", "ebar", "phi_x", "z1_in", "rays", "rgb", "valid")]
REFUSALS += [("car_chain_pack", w, c) for w, c in (("slot 16", dict(slot=16)), ("slot -1", dict(slot=-1)), ("ldw < K", dict(ldw=127)),
                                                    ("null W", dict(W=None)), ("null packed", dict(packed=None)), ("null scale", dict(scale=None)))]
REFUSALS += [("car_finalize", w, c) for w, c in (("ld_in 2", dict(ld_in=2)), ("null rays", dict(rays=None)), ("null rgb_in", dict(rgb_in=None)),
                                                  ("null rgb", dict(rgb=None)), ("null valid", dict(valid=None)))]


@pytest.mark.parametrize("entry,what,change", REFUSALS, ids=[f"{e}-{w}".replace(" ", "_") for e, w, _ in REFUSALS])
def test_entry_refuses_a_bad_argument_and_writes_nothing(entry, what, change):
    """One argument wrong, every other one as the accepted call has it: CAR_E_ARG, a message, and outputs that are still NaN."""
    lib = abi.lib()
    args, outs, subs, keep = _entry_arguments(entry)
    for k, v in change.items():
        assert k in args
        args[k] = subs[v] if isinstance(v, str) else v
    rc = _call(entry, args)
    assert rc == CAR_E_ARG, (entry, what, rc)
    msg = lib.car_last_error()
    assert msg and entry.replace("car_ray_mid", "car_ray").replace("car_ray_tail", "car_ray").encode() in msg, (entry, what, msg)
    torch.cuda.synchronize()
    for name, o in outs.items():
        assert o.untouched(), f"{entry} {what}: wrote {name}"


@pytest.mark.parametrize("entry", sorted(ARGS))
def test_entry_accepts_the_arguments_the_refusals_start_from(entry):
    """The refusals above are about the one argument each: the unchanged call is accepted and writes all of its outputs."""
    lib = abi.lib()
    args, outs, _, keep = _entry_arguments(entry)
    assert _call(entry, args) == 0, lib.car_last_error()
    torch.cuda.synchronize()
    if entry == "car_chain_pack":
        assert int(lib.car_chain_packed_floats(128, 128)) == 4 * 4 * 1024 and int(lib.car_chain_packed_floats(18, 128)) == 4 * 1024
        assert int(lib.car_chain_packed_floats(128, 3)) == 4 * 1024 and int(lib.car_chain_packed_floats(576, 288)) == 18 * 9 * 1024
        outs["packed"].get("packed")                                                    # all of its tiles and nothing else
        sc = outs["scale"].view.cpu().reshape(32)
        assert bool(torch.isfinite(sc[[0, 16]]).all()) and int(torch.isnan(sc).sum()) == 30 and sc[0].item() * sc[16].item() == 1.0
    else:
        for name, o in outs.items():
            assert bool(torch.isfinite(o.get(name)).all()), name


# ---- 9. the plan's own tables -------------------------------------------------------------------------------------------------------
def test_forward_rgb_and_uh_follow_from_the_workspace_rows():
    """One default-route forward on a synthetic two-view scene; ebar (the second round's rows by then), z1, uh, phi_x and rays read
    back from the workspace: out["rgb"] must agree with tail() on the kernel's own ebar, z1 and phi_x, and uh with
    Wq encode_latent(z1), at the tolerance above — the only test of the offsets, the bias order and the slot lists that car_plan_build
    and car_render_forward assemble."""
    import cases as C
    from cross_attention_renderer_amd import _lib as L, synthetic as S
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    dev = abi.dev()
    H, P, R, b, V = 64, 16, 161, 2, 2
    torch.manual_seed(0)
    m = CrossAttentionRenderer(model="midas_vit", n_view=2, npoints=P, with_encoder=False).eval()
    S.perturb_parameters(m, seed=4)
    m.H = m.W = H
    params = {}
    sd = m.state_dict()
    for name in RC.SHAPES:
        params[name + ".weight"] = sd[name + ".weight"].detach().clone().reshape(RC.SHAPES[name])
        params[name + ".bias"] = sd[name + ".bias"].detach().clone()
    inp = S.stereo_scene(H, b=b, uv=C.select_rays(H, R), seed=7, alpha=0.35)
    z = S.feature_maps(b, 2, H, seed=2)
    with torch.no_grad():
        md = m.to(dev)
        zd = [t.to(dev) for t in z]
        out = md({k: {kk: (vv if kk in ("cam2world", "intrinsics") else vv.to(dev)) for kk, vv in v.items()} for k, v in inp.items()}, z=zd)
    torch.cuda.synchronize()
    eng, lib = md._engine, abi.lib()
    assert eng.last_calls == 1
    d = eng._dims(b, R, zd)

    def ws(name, *shape):
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        L.check(lib.car_workspace_find(ctypes.byref(d), name.encode(), ctypes.byref(off), ctypes.byref(cnt)), "car_workspace_find")
        t = eng._work[off.value:off.value + cnt.value].cpu()
        assert t.numel() == torch.Size(shape).numel(), (name, t.numel(), shape)
        return t.view(*shape)
    ebar, z1, uh = ws("ebar", b * R, RC.C), ws("z1", b * R, RC.E), ws("uh", b * R, RC.D)
    phi = ws("phi_x", b * R, 20)
    rays = ws("rays", b * V, R, 12)
    assert bool((phi[:, 18:] == 0).all()) and bool(torch.isfinite(phi).all())
    ov = rays[:, :, 10].reshape(b, V, R)
    assert bool(((ov == 0) | (ov == 1)).all())
    args = (params, ebar, phi[:, :RC.PHI], z1, ov, V)
    ref, f32 = RC.tail(*args), RC.tail(*args, torch.float32)
    got = {"rgb": out["rgb"].float().cpu().reshape(b * R, 3), "valid": out["valid_mask"].float().cpu().reshape(b * R)}
    assert torch.equal(got["valid"].double(), ref["valid"]) and ref["valid"].sum().item() > 0
    _judge("forward_tables", "rgb from the workspace rows", got, ref, f32, TAIL_PAIRS)

    def uh_of(dtype):
        We, be = params["encode_latent.weight"].to(dtype), params["encode_latent.bias"].to(dtype)
        Wq = params["query_repeat_embed.weight"].to(dtype)[:, :RC.D]
        h = torch.nn.functional.linear(z1.to(dtype), We, be)
        return h, torch.nn.functional.linear(h, Wq)
    h64, uh64 = uh_of(torch.float64)
    refu = {"uh": uh64, "B_uh": h64.abs() @ params["query_repeat_embed.weight"].double()[:, :RC.D].abs().T}
    _judge("forward_tables", "uh from the workspace z1", {"uh": uh}, refu, {"uh": uh_of(torch.float32)[1]}, (("uh", "B_uh"),))
