"""The attention rounds and the row kernels of the backward, each through the C ABI against tests/attention_reference.py (fp64):
car_attend (logits given / dot-product logits, zprev, reps, row padding), car_attend_parts, car_attend_backward, car_scale_rows, car_add,
car_reduce_samples, car_relu_mask, car_add_ray_bias_relu, and the argument refusals.

Tolerance of every fp32-sum comparison: |got - want| <= 2e-5 * bound, entry by entry, `bound` the sum of the absolute values of the terms
(attention_reference.py) — the project's figure for fp32 sums against fp64 (test_wgrad_kernel_matches_torch); a worst-case count of a
plain implementation's roundings (at most 56 sequential terms per lane, a handful of tree steps, |l - M| <= 88 in front of exp) stays
under 1e-5.  Every test prints its worst error / (2e-5 * bound) as a ``[parity]`` line (profiles/attention_parity.md).
Every output lies inside a larger NaN-filled buffer: the margins and the row padding must come back untouched."""
import math

import pytest
import torch

import abi_harness as abi
import attention_reference as A
from abi_harness import CAR_E_ARG, NAN, Guarded
from parity_rule import error_ratio as _ratio

pytestmark = pytest.mark.gpu

TOL = 2e-5
EPS = 2.0 ** -23


def _up(t):
    return None if t is None else t.contiguous().to(abi.dev())


def _poses(inv_q, V):
    """Pose records [b*V, 96], NaN everywhere except inv_q (floats 77:89) of every scene's first view — all these kernels may read."""
    b = inv_q.shape[0]
    p = torch.full((b * V, 96), NAN)
    p[::V, 77:89] = inv_q.reshape(b, 12)
    return p


def _report(test, case, **ratios):
    print(f"[parity] {test} {case}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (test, case, k, v)


def attend(lib, logit, val, V, qb=None, zprev=None, scale=0.0, reps=1, ld_z=None, pt=None, inv_q=None, argmax=True, part=None, tile=0):
    """car_attend, or car_attend_parts when `part` is given.  `logit` is qa ([.., dq]) when qb is given.  Returns host tensors."""
    bV, R, P = logit.shape[:3]
    b = bV // V
    D = (part if part is not None else val).shape[-1]
    ld_z = ld_z or reps * D
    dq = logit.shape[3] if qb is not None else 0
    d = dict(qa=_up(logit), qb=_up(qb), val=_up(part if part is not None else val), zprev=_up(zprev), pt=_up(pt),
             poses=_up(_poses(inv_q, V)) if pt is not None else None)
    w, z = Guarded((bV * R, P)), Guarded((b * R, reps * D), ld_z)
    depth = Guarded((b * R, 1)) if pt is not None else None
    am = Guarded((bV * R, 1), dtype=torch.int32) if (pt is not None and argmax) else None
    if part is not None:
        rc = lib.car_attend_parts(abi.ptr(d["qa"]), abi.ptr(d["val"]), tile, D, b, V, R, P, w.ptr, z.ptr, ld_z, reps, abi.ptr(d["pt"]), abi.ptr(d["poses"]),
                                  depth.ptr if depth else None, am.ptr if am else None, abi.stream())
    else:
        rc = lib.car_attend(abi.ptr(d["qa"]), abi.ptr(d["qb"]), dq, abi.ptr(d["val"]), D, b, V, R, P, abi.ptr(d["zprev"]), scale, w.ptr, z.ptr, ld_z, reps,
                            abi.ptr(d["pt"]), abi.ptr(d["poses"]), depth.ptr if depth else None, am.ptr if am else None, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    out = {"w": w.get("w").view(bV, R, P), "z": z.get("z").view(b, R, reps * D)}
    if depth:
        out["depth"] = depth.get("depth").view(b, R)
    if am:
        out["argmax"] = am.get("argmax").view(bV, R).long()
    return out


def forward_ratios(got, ref, V, wfac=1.0, cls=None, decided=None, winner=None):
    """The checks every forward test shares; `wfac` widens the weights' (and what inherits their error's) tolerance for dot-product logits."""
    w, want = got["w"].double(), ref["w"]
    b = w.shape[0] // V
    r = {"w": _ratio((w - want).abs(), TOL * wfac * want.clamp_min(2.0 ** -100)),
         "wsum": ((A.ray_major(w, b, V).sum(-1) - 1.0).abs() / (TOL * wfac)).max().item(),
         "z": _ratio((got["z"].double() - ref["z"]).abs(), TOL * wfac * ref["Bz"])}
    assert torch.isfinite(got["w"]).all() and torch.isfinite(got["z"]).all()
    if "depth" in got:
        r["depth"] = _ratio((got["depth"].double() - ref["depth"]).abs(), TOL * wfac * ref["Bdepth"])
        if cls is not None:                                                         # a clamped depth is the clamp's own value, exactly
            assert bool((got["depth"][cls == 0] == 0.0).all()) and bool((got["depth"][cls == 2] == 10.0).all())
            inside = got["depth"][cls == 1]
            assert bool(((inside > 0.0) & (inside < 10.0)).all())
    if "argmax" in got and decided is not None:
        assert torch.equal(got["argmax"][decided], winner[decided]), "argmax on a planted ray or a tie"
    return r


def _case_inputs(b, V, R, P, D, spread, seed):
    logit, planted, tie, winner = A.make_logits(b, V, R, P, spread, seed)
    val = torch.randn(b * V, R, P, D, generator=A.gen(seed + 1))
    ref0 = A.forward(logit, val, V)
    pt, inv_q, cls = A.make_depth_inputs(ref0["w"], b, V, seed + 2)
    decided = (planted | tie)[:, None, :].expand(b, V, R).reshape(b * V, R)
    return logit, val, pt, inv_q, cls, decided, winner


FORWARD_SHAPES = ((1, 1, 7, 1, 4), (1, 2, 6, 5, 64), (2, 2, 37, 13, 576), (1, 2, 50, 64, 576), (1, 2, 8, 8, 580), (3, 1, 21, 70, 288),
                  (1, 3, 19, 64, 864), (1, 3, 5, 256, 896), (1, 2, 9, 128, 900), (1, 2, 11, 33, 62))


@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attend_with_given_logits_matches_fp64(shape):
    """Both compiled instances (D <= 576 / D <= 896), the streaming path with a full, a partial and a one-float4 last segment, the scalar
    fallback (D < 64, D > 896, D % 4 != 0), S from 1 to 768, at logit spreads 1, 30 and 1e3."""
    lib = abi.lib()
    b, V, R, P, D = shape
    for spread in (1.0, 30.0, 1e3):
        logit, val, pt, inv_q, cls, decided, winner = _case_inputs(b, V, R, P, D, spread, seed=100 + int(spread))
        ref = A.forward(logit, val, V, pt=pt, inv_q=inv_q)
        assert torch.equal(ref["argmax"][decided], winner[decided])
        got = attend(lib, logit, val, V, pt=pt, inv_q=inv_q)
        _report("attend_logits", f"{shape} spread {spread:g}", **forward_ratios(got, ref, V, cls=cls, decided=decided, winner=winner))


SPECIAL_SHAPES = ((1, 2, 6, 5, 64), (2, 2, 37, 13, 576), (1, 3, 19, 64, 864), (1, 3, 5, 256, 896), (1, 2, 9, 128, 900), (1, 2, 11, 33, 62))


@pytest.mark.parametrize("shape", SPECIAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attend_one_hot_and_constant_logits_are_exact(shape):
    """One logit 1e3 above the rest: w is exactly 1 and 0 and z is the winner's value row bit for bit (as values).  Constant logits:
    every weight is fp32(1) / fp32(S)."""
    lib = abi.lib()
    b, V, R, P, D = shape
    val = torch.randn(b * V, R, P, D, generator=A.gen(7))
    logit, hot = A.one_hot_logits(b, V, R, P, seed=8)
    got = attend(lib, logit, val, V)
    onehot = torch.nn.functional.one_hot(hot, V * P).float()
    assert torch.equal(A.ray_major(got["w"], b, V), onehot)
    rows = A.ray_major(val, b, V).gather(2, hot[:, :, None, None].expand(b, R, 1, D))[:, :, 0]
    assert bool((got["z"] == rows).all())
    const = torch.full((b * V, R, P), 3.25)
    got = attend(lib, const, val, V)
    assert bool((got["w"] == (torch.tensor(1.0) / torch.tensor(float(V * P)))).all())
    ref = A.forward(const, val, V)
    _report("attend_constant", f"{shape}", z=_ratio((got["z"].double() - ref["z"]).abs(), TOL * ref["Bz"]))


@pytest.mark.parametrize("shape", ((2, 2, 37, 13, 576), (1, 3, 19, 64, 864), (1, 2, 11, 33, 62)), ids=("narrow", "wide", "fallback"))
def test_attend_adds_zprev_and_replicates_into_padded_rows(shape):
    """zprev, zprev_scale, reps > 1 and ld_z > reps * D: the header's contract, which no caller in the project uses."""
    lib = abi.lib()
    b, V, R, P, D = shape
    logit, val, pt, inv_q, cls, decided, winner = _case_inputs(b, V, R, P, D, 3.0, seed=40)
    zprev = torch.randn(b, R, D, generator=A.gen(41)) * 3
    for scale in (0.5, 2.0, float(V)):
        for reps in (2, 3):
            ref = A.forward(logit, val, V, zprev=zprev, zprev_scale=scale, reps=reps, pt=pt, inv_q=inv_q)
            got = attend(lib, logit, val, V, zprev=zprev, scale=scale, reps=reps, ld_z=reps * D + 4, pt=pt, inv_q=inv_q)
            for k in range(1, reps):
                assert torch.equal(got["z"][..., :D], got["z"][..., k * D:(k + 1) * D]), "the copies differ"
            _report("attend_zprev", f"{shape} scale {scale:g} reps {reps}", **forward_ratios(got, ref, V, cls=cls, decided=decided, winner=winner))


@pytest.mark.parametrize("shape", ((2, 2, 37, 13, 576), (1, 3, 19, 64, 864), (1, 2, 11, 33, 62)), ids=("narrow", "wide", "fallback"))
def test_attend_optional_outputs_do_not_change_the_others(shape):
    lib = abi.lib()
    b, V, R, P, D = shape
    logit, val, pt, inv_q, _, _, _ = _case_inputs(b, V, R, P, D, 3.0, seed=50)
    full = attend(lib, logit, val, V, pt=pt, inv_q=inv_q)
    no_pt = attend(lib, logit, val, V)
    no_am = attend(lib, logit, val, V, pt=pt, inv_q=inv_q, argmax=False)
    assert torch.equal(full["w"], no_pt["w"]) and torch.equal(full["z"], no_pt["z"])
    assert torch.equal(full["w"], no_am["w"]) and torch.equal(full["z"], no_am["z"]) and torch.equal(full["depth"], no_am["depth"])


@pytest.mark.parametrize("shape", ((1, 2, 6, 5, 64), (2, 2, 37, 13, 576), (1, 3, 19, 64, 864)), ids=lambda s: "x".join(map(str, s)))
def test_attend_with_dot_product_logits_matches_fp64(shape):
    """logit = <qa, qb> / 16 inside the kernel.  An fp32 dot product is off by a few 2^-24 L1 (L1 = sum |qa||qb| / 16), and exp carries an
    absolute error of the logits into a relative one of the weights, on the ray's largest logit and on the sample's own: the weights'
    tolerance is 2e-5 (1 + 2 max_t L1_t) relative, with max L1 <= 8; z and depth inherit the weights' error, so they get the same factor."""
    lib = abi.lib()
    b, V, R, P, D = shape
    _, val, _, _, _, _, _ = _case_inputs(b, V, R, P, D, 1.0, seed=60)
    for dq in (4, 16, 68, 128, 192):
        qa, qb = A.make_dot_inputs(b, V, R, P, dq, seed=61 + dq)
        ref = A.forward((qa, qb), val, V)
        l1 = ref["L1"].max().item()
        assert l1 <= 8.0
        pt, inv_q, cls = A.make_depth_inputs(ref["w"], b, V, seed=62)
        ref = A.forward((qa, qb), val, V, pt=pt, inv_q=inv_q)
        got = attend(lib, qa, val, V, qb=qb, pt=pt, inv_q=inv_q)
        _report("attend_dot", f"{shape} dq {dq}", **forward_ratios(got, ref, V, wfac=1.0 + 2.0 * l1, cls=cls))


@pytest.mark.parametrize("D", (64, 576, 864))
def test_attend_parts_matches_fp64_on_the_raw_rows(D):
    """car_attend_parts fed with fp64-made partial sums, against forward() on the sample rows themselves (not against car_attend): P
    below, at and across the group size, one to three views, a group 200 below its ray's largest logit (its factor underflows to 0) and a
    one-hot ray."""
    lib = abi.lib()
    tile = lib.car_fused_tile_steps()
    R = 7                                                     # rays 0, 3, 6 planted, 1, 4 ties, 2 and 5 free (scene 0)
    for V in (1, 2, 3):
        for P in (5, 8, 13, 64, 70, 256):
            logit, val, pt, inv_q, cls, decided, winner = _case_inputs(1, V, R, P, D, 30.0, seed=70 + V)
            top = A.ray_major(logit, 1, V).amax(-1)
            logit[0, 2, :min(P, tile)] = top[0, 2] - 200.0 - torch.rand(min(P, tile), generator=A.gen(71))
            logit[V - 1, 5, P // 2] = top[0, 5] + 1e3           # ray 5: one-hot
            ref = A.forward(logit, val, V, pt=pt, inv_q=inv_q)
            part = A.parts(logit, val, tile)
            got = attend(lib, logit, None, V, pt=pt, inv_q=inv_q, part=part, tile=tile)
            hot = (V - 1) * P + P // 2
            assert torch.equal(A.ray_major(got["w"], 1, V)[0, 5], torch.nn.functional.one_hot(torch.tensor(hot), V * P).float())
            assert bool((got["z"][0, 5] == val[V - 1, 5, P // 2]).all())
            # ray 2's and 5's depth classes were planted for other weights: the classes are checked on the planted rays only
            keep = torch.ones(1, R, dtype=torch.bool)
            keep[0, 2] = keep[0, 5] = False
            cls_k = torch.where(keep, cls, torch.full_like(cls, -1))
            _report("attend_parts", f"V {V} P {P} D {D}", **forward_ratios(got, ref, V, cls=cls_k, decided=decided, winner=winner))


# ---- car_attend_backward ------------------------------------------------------------------------------------------------------------
def attend_backward(lib, w, val, V, dz, ld_dz, ddepth=None, pt=None, inv_q=None, prior=None):
    bV, R, P = w.shape
    b, D = bV // V, val.shape[-1]
    dzb = torch.full((b * R, ld_dz), NAN)
    dzb[:, :D] = dz.reshape(b * R, D)
    d = dict(w=_up(w), val=_up(val), dz=_up(dzb), dd=_up(ddepth), pt=_up(pt) if ddepth is not None else None,
             poses=_up(_poses(inv_q, V)) if ddepth is not None else None)
    dval = Guarded((bV * R * P, D), init=prior)
    dlogit = Guarded((bV * R, P))
    rc = lib.car_attend_backward(abi.ptr(d["w"]), abi.ptr(d["val"]), D, b, V, R, P, abi.ptr(d["dz"]), ld_dz, abi.ptr(d["dd"]), abi.ptr(d["pt"]), abi.ptr(d["poses"]),
                                 dval.ptr, 0 if prior is None else 1, dlogit.ptr, abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    return dlogit.get("dlogit").view(bV, R, P), dval.get("dval").view(bV, R, P, D)


def backward_ratios(dlogit, ref, V):
    b = dlogit.shape[0] // V
    err = (dlogit.double() - ref["dlogit"]).abs()
    return {"dlogit": _ratio(err, TOL * ref["Bl"]),
            "dlogit_sum": _ratio(A.ray_major(dlogit.double(), b, V).sum(-1).abs(), TOL * A.ray_major(ref["Bl"], b, V).sum(-1))}


@pytest.mark.parametrize("D", (4, 60, 64, 288, 576, 580, 864))
def test_attend_backward_matches_the_closed_form(D):
    """dlogit and dval of one round from given weights (the fp64 softmax rounded to fp32): one sample per ray up to S = 768 (three trips
    of the 256-thread strides), padded dz rows, with and without the depth read-out's term over all three depth classes."""
    lib = abi.lib()
    for V, P in ((1, 1), (2, 5), (2, 64), (3, 64), (3, 256), (1, 70)):
        b, R = (2, 9) if V * P <= 128 else (1, 7)
        logit, val, _, _, _, _, _ = _case_inputs(b, V, R, P, D, 3.0, seed=80 + P)
        w = A.forward(logit, val, V)["w"].float()
        pt, inv_q, cls = A.make_depth_inputs(w, b, V, seed=81)
        g = A.gen(82 + D)
        dz = torch.randn(b, R, D, generator=g)
        ddepth = torch.randn(b, R, generator=g) + 3.0 * torch.sign(torch.randn(b, R, generator=g))      # never near 0
        prior = torch.randn(b * V, R, P, D, generator=g)
        ref0 = A.backward(w, val, dz, V)
        ref1 = A.backward(w, val, dz, V, ddepth=ddepth, pt=pt, inv_q=inv_q)
        wdz = ref0["dval"].abs()
        for ld_dz in (D, D + 8):
            dl0, dv0 = attend_backward(lib, w, val, V, dz, ld_dz)
            dl1, dv1 = attend_backward(lib, w, val, V, dz, ld_dz, ddepth=ddepth, pt=pt, inv_q=inv_q)
            _, dv2 = attend_backward(lib, w, val, V, dz, ld_dz, ddepth=ddepth, pt=pt, inv_q=inv_q, prior=prior)
            r = {k + "_nodepth": v for k, v in backward_ratios(dl0, ref0, V).items()}
            r.update(backward_ratios(dl1, ref1, V))
            # a clamped depth passes no gradient: those rays' dlogit is the one without ddepth, bit for bit; the others' is not
            clamped = (cls != 1)[:, None, :].expand(b, V, R).reshape(b * V, R)
            assert torch.equal(dl1[clamped], dl0[clamped])
            if V * P > 1:
                assert not torch.equal(dl1[~clamped], dl0[~clamped])
            r["dval"] = _ratio((dv0.double() - ref0["dval"]).abs(), EPS * wdz)
            assert torch.equal(dv1, dv0)
            r["dval_acc"] = _ratio((dv2.double() - (prior.double() + ref0["dval"])).abs(), EPS * (prior.double().abs() + wdz))
            _report("attend_backward", f"D {D} V {V} P {P} ld_dz {ld_dz}", **r)


def test_attend_then_backward_matches_fp64_autograd_from_the_logits():
    """The chained case: car_attend's own weights fed to car_attend_backward, against fp64 autograd through the reference forward."""
    lib = abi.lib()
    b, V, R, P, D = 2, 2, 37, 64, 576
    logit, val, pt, inv_q, cls, _, _ = _case_inputs(b, V, R, P, D, 3.0, seed=90)
    g = A.gen(91)
    dz = torch.randn(b, R, D, generator=g)
    ddepth = torch.randn(b, R, generator=g)
    lg = logit.double().requires_grad_(True)
    vl = val.double().requires_grad_(True)
    out = A.forward(lg, vl, V, pt=pt, inv_q=inv_q)
    ((out["z"] * dz.double()).sum() + (out["depth"] * ddepth.double()).sum()).backward()
    got = attend(lib, logit, val, V, pt=pt, inv_q=inv_q)
    dl, dv = attend_backward(lib, got["w"], val, V, dz, D, ddepth=ddepth, pt=pt, inv_q=inv_q)
    ref = A.backward(out["w"].detach(), val, dz, V, ddepth=ddepth, pt=pt, inv_q=inv_q)
    _report("attend_chain", f"{(b, V, R, P, D)}", dlogit=_ratio((dl.double() - lg.grad).abs(), TOL * ref["Bl"]),
            dval=_ratio((dv.double() - vl.grad).abs(), TOL * vl.grad.abs()))


# ---- row kernels -------------------------------------------------------------------------------------------------------------------
def _scale_rows_case(lib, M, N, ldx, ldo, group, scale, accumulate, seed, offset=0):
    """out[m, :] (+)= scale * s[m // group] * x[m, :], compared on the device in fp64 chunk by chunk (the large cases do not fit twice; the
    prior contents of an accumulating call are a pattern of the indices, exact in fp32, so that no copy of them is kept either)."""
    dev = abi.dev()
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, ldx, generator=g, device=dev)
    s = torch.randn((M + group - 1) // group, generator=g, device=dev)
    out = Guarded((M, N), ldo, offset=offset)
    chunk = max(1, (1 << 23) // N)
    cols = torch.arange(N, device=dev)

    def prior_of(m0, m1):
        rows = torch.arange(m0, m1, device=dev)
        return (((rows[:, None] * 31 + cols[None, :] * 17) % 257) - 128).float() / 64.0
    if accumulate:
        for m0 in range(0, M, chunk):
            out.view[m0:min(M, m0 + chunk), :N] = prior_of(m0, min(M, m0 + chunk))
    rc = lib.car_scale_rows(out.ptr, ldo, abi.ptr(x), ldx, abi.ptr(s), group, scale, M, N, int(accumulate), abi.stream())
    assert rc == 0, lib.car_last_error()
    torch.cuda.synchronize()
    worst, exact = 0.0, True
    pow2 = math.frexp(scale)[0] in (0.5, -0.5)
    for m0 in range(0, M, chunk):
        m1 = min(M, m0 + chunk)
        f = torch.tensor(scale, dtype=torch.float32).item() * s[torch.arange(m0, m1, device=dev) // group].double()
        want = f[:, None] * x[m0:m1, :N].double()
        # roundings: the product with x and, accumulating, the sum — 2^-23 of the summed magnitudes; a scale that is no power of two
        # adds the rounding of scale * s itself, another 2^-24 of the product
        bound = want.abs() * (1.0 if pow2 else 1.5)
        if accumulate:
            prior = prior_of(m0, m1).double()
            want, bound = want + prior, bound + prior.abs()
        got = out.view[m0:m1, :N]
        exact = exact and torch.equal(got, want.float())
        worst = max(worst, _ratio((got.double() - want).abs(), EPS * bound))
    assert out.margins_untouched() and bool(torch.isnan(out.view[:, N:]).all())
    return worst, exact


def test_scale_rows_matches_fp64():
    """The decoder's call (N = 3, ldx = 3, ldo = 4: the scalar path), the key / query gradients (N = 128, scale 1 / 16, written and
    accumulated: the float4 path), row groups, an `out` that is 4- but not 16-byte aligned, and both paths beyond the 65 536-block grid cap."""
    lib = abi.lib()
    P = 64
    cases = [("decoder", 2304, 3, 3, 4, 1, 1.0, False, 0), ("key", 4736, 128, 128, 128, 1, 1.0 / 16.0, False, 0),
             ("key_acc", 4736, 128, 128, 128, 1, 1.0 / 16.0, True, 0), ("group7", 1001, 128, 132, 136, 7, 0.3, True, 0),
             ("groupP", 37 * P, 16, 16, 20, P, -1.7, False, 0), ("groupP_scalar", 37 * P, 5, 7, 6, P, 2.5, True, 0),
             ("offset_scalar", 999, 128, 128, 132, 1, 1.0 / 16.0, True, 1),                 # 4 bytes off a 16-byte boundary
             ("cap_scalar", 65536 * 256 // 3 + 12345, 3, 3, 4, 1, 1.0, False, 0),           # M N > 65 536 x 256 threads, about 150 MB
             ("cap_scalar_acc", 65536 * 256 // 3 + 12345, 3, 3, 4, 5, 0.7, True, 0),
             ("cap_float4", 65536 * 256 * 4 // 128 + 4321, 128, 128, 128, 64, 1.0 / 16.0, True, 0)]   # M N / 4 > 65 536 x 256
    for name, M, N, ldx, ldo, group, scale, acc, offset in cases:
        worst, exact = _scale_rows_case(lib, M, N, ldx, ldo, group, scale, acc, seed=len(name), offset=offset)
        if not acc and scale in (1.0, 1.0 / 16.0):                                           # a power of two: one rounding, bit for bit
            assert exact, name
        _report("scale_rows", name, err=worst)


def test_add_matches_fp64():
    """out = alpha a + beta b: b = NULL (one rounding: bit for bit), in place (out == a), b a column-offset view of a wider matrix, three
    different row strides."""
    lib = abi.lib()
    g = A.gen(5)
    M, Dl, V = 777, 288, 2
    zrep = torch.randn(M, V * Dl, generator=g)
    a = torch.randn(M, Dl + 4, generator=g)
    # b = NULL, alpha = V (engine.py / training.py: zrep = V z1)
    out = Guarded((M, Dl), V * Dl)
    ad = _up(a)
    assert lib.car_add(out.ptr, V * Dl, abi.ptr(ad), Dl + 4, float(V), None, 0, 0.0, M, Dl, abi.stream()) == 0, lib.car_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.get("add"), (float(V) * a[:, :Dl].double()).float())
    out = Guarded((M, Dl), Dl + 8)
    assert lib.car_add(out.ptr, Dl + 8, abi.ptr(ad), Dl + 4, -0.37, None, 0, 0.0, M, Dl, abi.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.get("add"), (torch.tensor(-0.37, dtype=torch.float32).double() * a[:, :Dl].double()).float())
    # b a column-offset view (d_zrep[:, Dl:]), all strides different, alpha and beta not 1
    zd = _up(zrep)
    for alpha, beta in ((1.0, 1.0), (0.75, -1.3)):
        out = Guarded((M, Dl), Dl + 12)
        bview = zd[:, Dl:]
        assert lib.car_add(out.ptr, Dl + 12, abi.ptr(ad), Dl + 4, alpha, abi.ptr(bview), V * Dl, beta, M, Dl, abi.stream()) == 0
        torch.cuda.synchronize()
        fa, fb = torch.tensor(alpha, dtype=torch.float32).double(), torch.tensor(beta, dtype=torch.float32).double()
        want = fa * a[:, :Dl].double() + fb * zrep[:, Dl:].double()
        bound = (fa * a[:, :Dl].double()).abs() + (fb * zrep[:, Dl:].double()).abs()
        _report("add", f"view alpha {alpha} beta {beta}", err=_ratio((out.get("add").double() - want).abs(), EPS * bound))
    # in place: out == a (training.py: d_x = d_x + tmp, d_zf = d_zf + d_zrep[:, v Dl:])
    acc = Guarded((M, Dl), Dl + 4, init=a[:, :Dl])
    assert lib.car_add(acc.ptr, Dl + 4, acc.ptr, Dl + 4, 1.0, abi.ptr(zd[:, Dl:]), V * Dl, 1.0, M, Dl, abi.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(acc.get("add in place"), (a[:, :Dl].double() + zrep[:, Dl:].double()).float())


def test_reduce_samples_matches_fp64():
    lib = abi.lib()
    for V in (1, 2, 3):
        for P in (1, 13, 64):
            for C in (4, 128, 300):
                b, R = 2, 11
                d = torch.randn(b * V, R, P, C, generator=A.gen(V * 1000 + P * 10 + C)) + 0.5
                du = Guarded((b * R, C))
                dd = _up(d)
                assert lib.car_reduce_samples(abi.ptr(dd), b, V, R, P, C, du.ptr, abi.stream()) == 0, lib.car_last_error()
                torch.cuda.synchronize()
                dr = A.ray_major(d.double(), b, V)
                _report("reduce_samples", f"V {V} P {P} C {C}",
                        err=_ratio((du.get("du").view(b, R, C).double() - dr.sum(2)).abs(), TOL * dr.abs().sum(2)))


def test_relu_mask_is_exact_on_special_values():
    """grad = act > 0 ? grad : 0 — +0, -0 and NaN activations pass nothing, denormals and +inf do; different row strides."""
    lib = abi.lib()
    g = A.gen(6)
    M, N, ldg, lda = 513, 37, 40, 44
    act = torch.randn(M, lda, generator=g)
    specials = torch.tensor([0.0, -0.0, NAN, 1e-45, -1e-45, 1e-39, -1e-39, float("inf"), float("-inf")])
    flat = act[:, :N].clone().reshape(-1)
    flat[::7] = specials[torch.arange(flat[::7].numel()) % len(specials)]
    act[:, :N] = flat.view(M, N)
    grad = torch.randn(M, N, generator=g)
    gb = Guarded((M, N), ldg, init=grad)
    ad = _up(act)
    assert lib.car_relu_mask(gb.ptr, ldg, abi.ptr(ad), lda, M, N, abi.stream()) == 0, lib.car_last_error()
    torch.cuda.synchronize()
    want = torch.where(act[:, :N].double() > 0, grad, torch.zeros_like(grad))
    got = gb.get("relu_mask")
    assert torch.equal(got, want)
    for v in specials.tolist():
        sel = (act[:, :N] == v) if v == v else torch.isnan(act[:, :N])
        assert sel.any()


def test_add_ray_bias_relu_is_exact():
    """r = relu(r + u[scene, ray]) in place, one rounding: bit for bit; the last size runs beyond the 16 384-block grid cap."""
    lib = abi.lib()
    for b, V, R, P, C in ((1, 1, 5, 3, 4), (2, 2, 37, 13, 128), (3, 3, 10, 7, 16), (1, 2, 1100, 64, 128)):
        assert (b, V, R, P, C) != (1, 2, 1100, 64, 128) or b * V * R * P * C // 4 > 16384 * 256
        g = A.gen(C)
        r = torch.randn(b * V, R, P, C, generator=g)
        u = torch.randn(b, R, C, generator=g)
        rb = Guarded((b * V * R * P, C), init=r)
        ud = _up(u)
        assert lib.car_add_ray_bias_relu(rb.ptr, abi.ptr(ud), b, V, R, P, C, abi.stream()) == 0, lib.car_last_error()
        torch.cuda.synchronize()
        want = (r.double().view(b, V, R, P, C) + u.double()[:, None, :, None, :]).clamp_min(0.0).float().view(-1, C)
        assert torch.equal(rb.get("add_ray_bias_relu"), want), (b, V, R, P, C)


def test_bad_arguments_are_refused_before_anything_is_launched():
    lib = abi.lib()
    b, V, R, P, D = 1, 2, 4, 8, 64
    dev = abi.dev()
    w = torch.rand(b * V, R, P, device=dev)
    val = torch.randn(b * V, R, P, D + 4, device=dev)
    dz = torch.randn(b, R, D + 8, device=dev)
    pt = torch.randn(b * V, R, P, 3, device=dev)
    dd = torch.randn(b, R, device=dev)
    poses = torch.zeros(b * V, 96, device=dev)
    qa = torch.randn(b * V, R, P, 8, device=dev)
    dval, dlogit, z = Guarded((b * V * R * P, D + 4)), Guarded((b * V * R, P)), Guarded((b * R, 2 * D))
    depth, wout = Guarded((b * R, 1)), Guarded((b * V * R, P))

    def bwd(D_=D, ld=D, V_=V, P_=P, ddepth=None, pt_=None):
        return lib.car_attend_backward(abi.ptr(w), abi.ptr(val), D_, b, V_, R, P_, abi.ptr(dz), ld, abi.ptr(ddepth), abi.ptr(pt_), abi.ptr(poses), dval.ptr, 0,
                                       dlogit.ptr, abi.stream())

    def fwd(dq=8, qb=None, ld_z=D, reps=1):
        return lib.car_attend(abi.ptr(qa), abi.ptr(qb), dq, abi.ptr(val), D, b, V, R, P, None, 0.0, wout.ptr, z.ptr, ld_z, reps, None, None, None, None,
                              abi.stream())
    assert bwd(D_=D + 2) == CAR_E_ARG                       # D % 4 != 0
    assert bwd(ld=D - 4) == CAR_E_ARG                       # ld_dz < D
    assert bwd(V_=3, P_=257) == CAR_E_ARG                   # V P > 768
    assert bwd(ddepth=dd) == CAR_E_ARG                      # ddepth without pt
    assert lib.car_last_error()
    assert fwd(ld_z=2 * D - 4, reps=2) == CAR_E_ARG         # ld_z < reps D
    assert fwd(dq=6, qb=qa) == CAR_E_ARG                    # qb given, dq % 4 != 0
    r = Guarded((b * V * R * P, 6))
    assert lib.car_add_ray_bias_relu(r.ptr, abi.ptr(dz), b, V, R, P, 6, abi.stream()) == CAR_E_ARG       # C % 4 != 0
    torch.cuda.synchronize()
    for buf in (dval, dlogit, z, depth, wout, r):
        assert bool(torch.isnan(buf.full).all()), "a refused call wrote something"
    assert bwd() == 0 and fwd(dq=0) == 0                    # and the same buffers with good arguments are accepted
    torch.cuda.synchronize()
