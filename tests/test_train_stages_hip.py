"""The stages of the training backward on the device (training._decode_backward ... _scatter_to_pyramid, and the dispatch of
_RenderTrain.backward) against tests/train_reference.py at the device's own record, under the parity rule (tests/parity_rule.py).

render_train runs once per case; the autograd node of its result is the backward's ctx.  Each stage function is then called on its own, on a
fresh run record (training._start: the flat gradient buffer starts at zero), with seeded cotangents that no previous stage produced.  The
``Saved`` record is copied to the host once and the reference's closed-form adjoint evaluated AT it: ReLU masks, softmax weights and
weight-gradient operands are the device's, so there is no flip and no budget.  Every entry of every cotangent the stage returns and of
every parameter gradient it wrote counts: error over the composed float64 bound, held to parity_rule.tolerance of the yardstick — the
same adjoint on the same record in the arithmetic each launch is entitled to (float32; the split-fp16 / bf16 emulations of
linear_reference on exactly the launches whose row counts take those routes), never the device.  Parameter gradients the stage must not
write are exactly zero.  The restated stage forwards, in float64 on the record's stage inputs, reproduce the record's stage outputs
under the same rule, so reference and product cannot be consistently wrong about the same forward.  Every comparison prints its
``[parity]`` line (DESIGN.md section 7 holds the table)."""
import dataclasses
import functools
import types

import pytest
import torch

import cases as C
import grad_cases as G
import linear_reference as LR
import parity_rule as PR
import train_reference as T
from hip_harness import build_module, to_device

pytestmark = pytest.mark.gpu

F32 = torch.float32
RATIO = functools.partial(PR.ratio, all_finite=True)
REAL_2V = dict(tier=1, H=64, P=32, b=1, **C.REAL)
# the smallest configurations at which the routes differ: real widths at S = 2048 samples (exactly linear_x3_min_rows and the bf16
# weight-gradient threshold: per-sample layers on the split routes, the 32 per-ray rows on the fp32 pipe) and one ray fewer (S = 1984:
# the layers over S rows on the fp32 pipe too, only the point MLP's S V rows still above the thresholds; ragged everywhere); the
# three-view exchange at real widths; every constructor variant at tiny widths
CASES = {"real_rays32": dict(REAL_2V, rays=32), "real_rays31": dict(REAL_2V, rays=31), "t1_nview3": C.CASES["t1_nview3"],
         **{k: C.CASES[k] for k in ("t0_nview1", "t0_no_latent_concat", "t0_no_repeat", "t0_no_sample", "t0_p5", "t0_default")}}
MODE = {1: "single", 2: "concat2", 3: "concat3"}


def config(name):
    c = dict(C.DEFAULTS)
    c.update(CASES[name], name=name)
    return c


def host(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, (list, tuple)):
        return type(v)(host(x) for x in v)
    return v


def record_of(node) -> dict:
    """The node's staged.Saved record on the host, as the dict train_reference takes."""
    return {f.name: host(getattr(node.saved, f.name)) for f in dataclasses.fields(node.saved)}


@functools.lru_cache(maxsize=None)
def scene(name):
    """One render_train per case: the module, its inputs, the autograd node (the backward's ctx), the record and the parameters on the host."""
    from cross_attention_renderer_amd import synthetic as S
    from cross_attention_renderer_amd.training import render_train
    dev = torch.device("cuda:0")
    c = config(name)
    inp, z = C.build_inputs(c)
    sd = S.seeded_state_dict(C.param_shapes(c), seed=c["w_seed"])
    m = build_module(c, sd, dev).train()
    inp = to_device(inp, dev, cameras_on_host=True)
    zr = [t.to(dev).requires_grad_(True) for t in z]
    out = render_train(m, inp, z=zr)
    node = out["rgb"].grad_fn
    torch.cuda.synchronize()
    mode = "plain" if c["no_latent_concat"] else MODE[c["n_view"]]
    return types.SimpleNamespace(c=c, m=m, inp=inp, z=z, out=out, node=node, dev=dev, mode=mode, repeat=c["repeat_attention"], sv=record_of(node),
                                 par={k: host(v) for k, v in node.params.items()}, eng=m._engine)


def entitled(s) -> T.Arith:
    """The arithmetic the engine's switches, as they stand, entitle each launch to."""
    return T.Arith(F32, s.eng.linear_x3_min_rows, s.eng.wgrad_fp32)


def cot(shape, seed):
    return torch.randn(*shape, generator=PR.gen(seed))


def entries_of(got: dict, ref: dict, yard: dict) -> dict:
    """{name: (device tensor, ...)} against the reference's and the yardstick's pairs of the same names -> judge()'s entries."""
    assert sorted(got) == sorted(ref) == sorted(yard), (sorted(got), sorted(ref))
    out = {}
    for k, t in got.items():
        v64, B = ref[k]
        assert tuple(t.shape) == tuple(v64.shape), (k, t.shape, v64.shape)
        out[k] = ((host(t), v64, B), RATIO(yard[k][0], v64, B))
    return out


def stage_check(s, stage: str, run_device, run_reference, case=None):
    """run_device(r) -> {name: cotangent} on a fresh run record r; run_reference(ar) -> ({name: pair}, Grads)."""
    from cross_attention_renderer_amd import training
    with torch.cuda.device(s.dev):
        r = training._start(s.node)
        assert all(not bool(t.any()) for t in r.grads.values())
        cots = run_device(r)
        torch.cuda.synchronize()
    (ref_c, ref_g), (yard_c, yard_g) = run_reference(T.REF), run_reference(entitled(s))
    ref_g, yard_g = ref_g.shaped(), yard_g.shaped()
    written = {k: r.grads[k] for k in ref_g}
    for k, t in r.grads.items():
        if k not in ref_g:
            assert not bool(t.any()), (stage, k, "written by a stage that does not own it")
    entries = entries_of({**{"d " + k: v for k, v in cots.items()}, **written}, {**{"d " + k: v for k, v in ref_c.items()}, **ref_g},
                         {**{"d " + k: v for k, v in yard_c.items()}, **yard_g})
    PR.judge(f"train_stage.{stage}", case or s.c["name"], entries, what="entitled", ratio=RATIO)


# ---- the cases are the ones they are named for ----------------------------------------------------------------------------------------------------
def test_the_two_real_width_cases_fall_on_different_sides_of_both_thresholds():
    a, b_ = scene("real_rays32"), scene("real_rays31")
    Sa, Sb = T.sizes(a.sv)["S"], T.sizes(b_.sv)["S"]
    rows = a.eng.linear_x3_min_rows
    assert (Sa, Sb) == (2048, 1984) and a.eng.linear_x3 and not a.eng.wgrad_fp32 and not a.eng.scatter_atomics
    Ce = a.sv["Ce"]
    assert Ce == 576 and a.sv["ld_rows"] % 4 == 0
    # the layers over S rows (key_map and its data gradient, key_map_2, the second round's): split routes at 32 rays, the fp32 pipe at 31;
    # the per-ray layers (32 / 31 rows): the fp32 pipe in both; the point MLP runs over S V rows: the split routes in both
    for K, N in ((Ce, 128), (128, Ce), (128, 128)):
        assert T.takes_x3(Sa, K, N, rows) and not T.takes_x3(Sb, K, N, rows), (K, N)
        assert not T.takes_x3(32, K, N, rows)
    for N, K, db in ((128, Ce, True), (128, 128, True), (128, 16, True)):
        assert LR.wgrad_dispatch(Sa, N, K, db) == "bf16" and LR.wgrad_dispatch(Sb, N, K, db) != "bf16", (N, K)
        assert LR.wgrad_dispatch(Sa, N, K, db, LR.WGRAD_FP32) != "bf16" and LR.wgrad_dispatch(32, N, K, db) != "bf16"
    for K, N in ((579, 576), (576, 288)):
        assert T.takes_x3(2 * Sb, K, N, rows) and LR.wgrad_dispatch(2 * Sb, N, K, True) == "bf16"
    # and the tiny cases: S = 2048 samples too at t0_default (b = 2), 185 at t0_p5
    assert T.sizes(scene("t0_p5").sv)["S"] == 2 * 37 * 5


# ---- the restated forward reproduces the record ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_restated_stage_forwards_reproduce_the_record(name):
    s = scene(name)
    sv, par, z = s.sv, s.par, T.sizes(s.sv)
    C_ = T.channels(sv["maps"])

    def run(ar):
        out = {}
        if s.mode != "plain":
            K = C_ + (6 if s.mode == "single" else 3)
            ptcols, rows = sv["enc_rows"][:, C_:K], sv["enc_rows"][:, :K]
            if s.mode == "concat2":
                out["enc_rows"] = T.rows_concat2(sv["maps"], sv["pixel_val"], sv["grid_other"], ptcols, ar.dtype)
                out.update(T.e_concat2(par, rows, ar))
            elif s.mode == "concat3":
                out["enc_rows"] = T.rows_concat3(sv["maps"], sv["pixel_val"], sv["cross"], ptcols, z["b"], ar.dtype)
                out.update(T.e_concat3(par, rows, ar))
            else:
                out["enc_rows"] = T.rows_single(sv["maps"], sv["pixel_val"], ptcols, ar.dtype)
                out.update(T.e_single(par, rows, ar))
        else:
            out.update(T.e_plain(sv["maps"], sv["pixel_val"], ar.dtype))
        out.update(T.keys_and_queries(par, sv["e"], sv["g"], ar))
        at = T.attention_rounds(par, sv, s.repeat, ar, weights=(sv["at_wt"], sv["at_wt2"]))
        out.update({k: v for k, v in at.items() if isinstance(v, tuple)})
        dec = T.decode(par, sv["phi_x"], sv["zrep"], sv["valid"], ar)
        out.update({f"xas.{i}": t for i, t in enumerate(dec["xas"])}, **{f"nets.{i}": t for i, t in enumerate(dec["nets"])}, dec_out=dec["dec_out"], rgb=dec["rgb"])
        return out
    ref, yard = run(T.REF), run(entitled(s))
    K = C_ + (6 if s.mode == "single" else 3)
    got = {}
    for k in ref:
        if k == "rgb":
            got[k] = s.out["rgb"].detach().reshape(z["b"], z["R"], 3)
        elif "." in k:
            got[k] = sv[k.split(".")[0]][int(k.split(".")[1])]
        else:
            got[k] = sv[k][:, :K] if k == "enc_rows" else sv[k]
    PR.judge("train_stage.forward", name, entries_of(got, ref, yard), what="entitled", ratio=RATIO)


# ---- the stages of the backward, one at a time ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_decode_backward(name):
    from cross_attention_renderer_amd import training
    s = scene(name)
    z = T.sizes(s.sv)
    d_rgb = cot((z["b"], 1, z["R"], 3), 101)

    def reference(ar):
        d_z, Gr = T.decode_adjoint(s.sv, s.par, d_rgb, ar)
        return {"z": d_z}, Gr
    stage_check(s, "decode", lambda r: {"z": training._decode_backward(r, d_rgb.to(s.dev))}, reference)


@pytest.mark.parametrize("name", CASES)
def test_attention_rounds_backward(name):
    from cross_attention_renderer_amd import training
    s = scene(name)
    z = T.sizes(s.sv)
    Dl = s.sv["zrep"].shape[1] // z["V"]
    d_z, d_depth = cot((z["bR"], Dl), 102), cot((z["b"], z["R"], 1), 103)

    def device(r):
        d_e, d_key, d_q = training._attention_rounds_backward(r, d_z.to(s.dev), d_depth.to(s.dev))
        return {"e": d_e, "key": d_key, "q": d_q}

    def reference(ar):
        d_e, d_key, d_q, Gr = T.attention_rounds_adjoint(s.sv, s.par, d_z, d_depth.reshape(-1), s.repeat, ar)
        return {"e": d_e, "key": d_key, "q": d_q}, Gr
    stage_check(s, "attention_rounds", device, reference)


@pytest.mark.parametrize("name", CASES)
def test_keys_and_queries_backward(name):
    from cross_attention_renderer_amd import training
    s = scene(name)
    z = T.sizes(s.sv)
    d_e, d_key, d_q = cot((z["S"], s.sv["Ce"]), 104), cot((z["S"], 128), 105), cot((z["S"], 128), 106)

    def device(r):
        de = d_e.to(s.dev)
        training._keys_and_queries_backward(r, de, d_key.to(s.dev), d_q.to(s.dev))
        return {"e": de}

    def reference(ar):
        de, Gr = T.keys_and_queries_adjoint(s.sv, s.par, d_e, d_key, d_q, ar)
        return {"e": de}, Gr
    stage_check(s, "keys_and_queries", device, reference)


@pytest.mark.parametrize("atomics", (False, True), ids=("binned", "atomics"))
@pytest.mark.parametrize("name", CASES)
def test_e_backward_and_the_scatter_to_the_pyramid(name, atomics):
    """The mode's adjoint of e, _scatter_to_pyramid and _level_grads, on both scatters (the three-view route scatters for itself, with
    atomics either way)."""
    from cross_attention_renderer_amd import training
    s = scene(name)
    z = T.sizes(s.sv)
    d_e = cot((z["S"], s.sv["Ce"]), 107)
    stage = {"concat2": training._e_concat2_backward, "concat3": training._encode_three_views_backward, "single": training._e_single_backward,
             "plain": training._e_plain_backward}[s.mode]

    def device(r):
        res = stage(r, d_e.to(s.dev))
        levels = res if s.mode == "concat3" else training._scatter_to_pyramid(r, *res)
        assert all(tuple(t.shape) == tuple(zl.shape) for t, zl in zip(levels, s.z))
        return {f"z.{l}": t for l, t in enumerate(levels)}

    def reference(ar):
        dmaps, Gr = T.E_ADJOINT[s.mode](s.sv, s.par, d_e, True, ar)
        return {f"z.{l}": p for l, p in enumerate(T.level_grads(dmaps, [True] * len(dmaps)))}, Gr
    try:
        s.eng.scatter_atomics = atomics
        stage_check(s, "e_" + s.mode, device, reference, case=f"{name}/{'atomics' if atomics else 'binned'}")
    finally:
        s.eng.scatter_atomics = False


# ---- the whole backward ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("default", "conservative"))
@pytest.mark.parametrize("name", CASES)
def test_the_whole_backward(name, route):
    """loss.backward() with grad_cases' seeded cotangents: every p.grad and z.grad against train_reference.backward at that run's record.
    The levels come in the layouts _level_grads tells apart: NCHW, channels_last, and (where there is a third) one that asks for no
    gradient.  The conservative route (engine.wgrad_fp32 and scatter_atomics) is held to its own yardstick: no bf16 weight gradient.
    A gradient's bound is that of the stage that writes it, from the float64 cotangent that stage receives (train_reference.backward);
    what the earlier stages' rounding adds is in the yardstick, which runs the same chain in the entitled arithmetic."""
    from cross_attention_renderer_amd.training import render_train
    s = scene(name)
    conservative = route == "conservative"
    zr = [t.to(s.dev) for t in s.z]
    zr[1] = zr[1].contiguous(memory_format=torch.channels_last)
    asks = [l < 2 for l in range(len(zr))]
    zr = [t.requires_grad_(a) for t, a in zip(zr, asks)]
    try:
        s.eng.wgrad_fp32, s.eng.scatter_atomics = conservative, conservative
        s.m.zero_grad(set_to_none=True)
        out = render_train(s.m, s.inp, z=zr)
        node = out["rgb"].grad_fn
        c_rgb, c_depth = G.cotangents(out["rgb"].shape, out["depth_ray"].shape)
        ((out["rgb"] * c_rgb.to(s.dev)).sum() + (out["depth_ray"] * c_depth.to(s.dev)).sum()).backward()
        torch.cuda.synchronize()
        ar = entitled(s)
    finally:
        s.eng.wgrad_fp32, s.eng.scatter_atomics = False, False
    assert ar.wgrad_fp32 == conservative
    sv, par = record_of(node), {k: host(v) for k, v in node.params.items()}
    named = dict(s.m.named_parameters())
    got = {k: named[k].grad for k in par if named[k].grad is not None}
    assert all(p.grad is None for k, p in named.items() if k not in par)
    for l, (t, a) in enumerate(zip(zr, asks)):
        assert (t.grad is not None) == a, l
        if a:
            assert t.grad.stride() == t.stride() and t.grad.dtype == t.dtype, l
            got[f"z.{l}"] = t.grad
    s.m.zero_grad(set_to_none=True)

    def reference(a):
        grads, levels = T.backward(sv, par, c_rgb.reshape(-1, 3), c_depth.reshape(-1), s.mode, asks, a)
        assert [lv is not None for lv in levels] == asks
        return {**grads, **{f"z.{l}": lv for l, lv in enumerate(levels) if lv is not None}}
    PR.judge("train_stage.backward", f"{name}/{route}", entries_of(got, reference(T.REF), reference(ar)), what="entitled", ratio=RATIO)
