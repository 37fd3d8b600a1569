"""tests/attention_reference.py checked against itself and against the oracle's lines, without a GPU: the closed-form backward against
torch.autograd in fp64 through forward(), forward() against the oracle's ``ray_softmax`` / a14 / a16 lines (oracle/car_oracle.py), the
partial sums of parts() folded back against forward(), and the promises of the input generators."""
import pytest
import torch
import torch.nn.functional as F

import attention_reference as A
from oracle.car_oracle import _apply_4x4

SHAPES = ((1, 2, 50, 64, 576), (1, 3, 19, 64, 864), (1, 1, 5, 768, 896), (2, 2, 40, 5, 64))      # (b, V, R, P, D): S = 128, 192, 768, 10


def _inputs(b, V, R, P, D, seed):
    g = A.gen(seed)
    logit, _, _, _ = A.make_logits(b, V, R, P, 3.0, seed)
    val = torch.randn(b * V, R, P, D, generator=g)
    w = A.forward(logit, val, V)["w"]
    pt, inv_q, cls = A.make_depth_inputs(w, b, V, seed + 1)
    return logit, val, pt, inv_q, cls, g


@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_backward_equals_fp64_autograd_through_the_forward(shape):
    b, V, R, P, D = shape
    logit, val, pt, inv_q, _, g = _inputs(*shape, seed=11)
    dz = torch.randn(b, R, D, generator=g, dtype=A.F64)
    ddepth = torch.randn(b, R, generator=g, dtype=A.F64)
    lg = logit.double().requires_grad_(True)
    vl = val.double().requires_grad_(True)
    out = A.forward(lg, vl, V, pt=pt, inv_q=inv_q)
    ((out["z"] * dz).sum() + (out["depth"] * ddepth).sum()).backward()
    got = A.backward(out["w"].detach(), val, dz, V, ddepth=ddepth, pt=pt, inv_q=inv_q)
    r_l = ((got["dlogit"] - lg.grad).abs() / got["Bl"]).max().item()
    bound_v = (out["w"].detach()[..., None] * A.view_major(dz[:, :, None, :].expand(-1, -1, V * P, -1), b, V)).abs()
    r_v = ((got["dval"] - vl.grad).abs() / bound_v.clamp_min(1e-300)).max().item()
    print(f"{shape}: dlogit {r_l:.1e}, dval {r_v:.1e} of the bound")
    assert r_l <= 1e-12 and r_v <= 1e-12
    # and without the depth term
    lg.grad = None
    (A.forward(lg, vl, V)["z"] * dz).sum().backward()
    got0 = A.backward(out["w"].detach(), val, dz, V)
    assert ((got0["dlogit"] - lg.grad).abs() / got0["Bl"]).max().item() <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_equals_the_oracles_lines(shape):
    """oracle/car_oracle.py: ray_softmax (483-487), a14's value sum over samples then views (496), a16 (511-514) — in fp64 on the same
    tensors: layout, view order, clamp order, the read-out through the query's inverse pose."""
    b, V, R, P, D = shape
    logit, val, pt, inv_q, _, _ = _inputs(*shape, seed=5)
    out = A.forward(logit, val, V, pt=pt, inv_q=inv_q, reps=2)
    lg = logit.double().reshape(b, V, R, P).permute(0, 2, 1, 3).reshape(b, R, V * P)
    at_wt = F.softmax(lg, dim=-1).reshape(b, R, V, P).permute(0, 2, 1, 3).flatten(0, 1)
    assert (out["w"] - at_wt).abs().max().item() <= 1e-15
    zsum = (val.double() * at_wt[..., None]).sum(dim=2).reshape(b, V, R, D).sum(dim=1)
    assert ((out["z"][..., :D] - zsum).abs() / out["Bz"][..., :D]).max().item() <= 1e-13
    assert torch.equal(out["z"][..., :D], out["z"][..., D:])
    pt_mean = (at_wt[..., None] * pt.double().clamp(-100, 100)).sum(dim=-2).reshape(b, V, R, 3).sum(dim=1)
    T = torch.zeros(b, 4, 4, dtype=A.F64)
    T[:, :3, :] = inv_q.double()
    T[:, 3, 3] = 1.0
    depth = _apply_4x4(T[:, None], pt_mean)[..., 2].clamp(0, 10)
    assert ((out["depth"] - depth).abs() / out["Bdepth"]).max().item() <= 1e-13
    unique = (at_wt.amax(-1, keepdim=True) == at_wt).sum(-1) == 1                 # torch.argmax promises nothing on ties: first_argmax's job
    assert unique.any() and torch.equal(out["argmax"][unique], at_wt.argmax(dim=-1)[unique])
    tied = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 0.0, 1.0]])
    assert A.first_argmax(tied).tolist() == [1, 0, 1]
    # dot-product logits: <qa, qb> / 16
    qa, qb = A.make_dot_inputs(b, V, R, min(P, 16), 68, seed=3)
    o2 = A.forward((qa, qb), val[:, :, :min(P, 16)], V)
    assert torch.equal(o2["logit"], (qa.double() * qb.double()).sum(-1) / 16.0)
    assert 7.0 <= o2["L1"].max().item() <= 8.0
    # zprev
    zp = torch.randn(b, R, D, generator=A.gen(9))
    o3 = A.forward(logit, val, V, zprev=zp, zprev_scale=2.0)
    assert (o3["z"] - (zsum + 2.0 * zp.double())).abs().max().item() <= 1e-12


@pytest.mark.parametrize("tile_steps", (4, 8, 16))
@pytest.mark.parametrize("shape", ((1, 2, 9, 13, 64), (2, 3, 7, 70, 288), (1, 1, 4, 256, 576), (1, 2, 6, 5, 64)))
def test_folded_parts_equal_the_forward(shape, tile_steps):
    b, V, R, P, D = shape
    g = A.gen(21)
    logit, _, _, _ = A.make_logits(b, V, R, P, 30.0, 21)
    logit[0, 0, : min(P, tile_steps)] -= 200.0                                    # a group far below the ray's largest logit
    val = torch.randn(b * V, R, P, D, generator=g)
    part = A.parts(logit, val, tile_steps)
    assert part.dtype == torch.float32 and part.shape == (b * V, R, -(-P // tile_steps), D)
    out = A.forward(logit, val, V)
    z = A.fold_parts(logit, part, V, tile_steps)
    assert ((z - out["z"]).abs() / out["Bz"]).max().item() <= 2.0 ** -23            # one fp32 rounding of every part


@pytest.mark.parametrize("spread", (1.0, 30.0, 1e3))
@pytest.mark.parametrize("shape", ((1, 1, 7, 1, 4), (2, 2, 37, 13, 576), (1, 3, 5, 256, 896), (3, 1, 21, 70, 288), (1, 2, 8, 8, 580)))
def test_generators_keep_their_promises(shape, spread):
    b, V, R, P, D = shape
    logit, planted, tie, winner = A.make_logits(b, V, R, P, spread, 31)
    val = torch.zeros(b * V, R, P, 1)
    out = A.forward(logit, val, V)
    w = out["w"]
    pv = planted[:, None, :].expand(b, V, R).reshape(b * V, R)
    tv = tie[:, None, :].expand(b, V, R).reshape(b * V, R)
    assert planted.any() and (P < 2 or R < 2 or tie.any())
    assert ((winner >= 0) == (pv | tv)).all()
    assert torch.equal(out["argmax"][pv | tv], winner[pv | tv])
    if P >= 2:
        top2 = w.topk(2, dim=-1).values
        assert (((top2[..., 0] - top2[..., 1]) > 1e-3 * top2[..., 0]) | ~pv).all()           # every planted margin exceeds 1e-3 of the weight
        assert (top2[..., 0][pv] > 2.0 ** -100).all()
        l2 = logit.topk(2, dim=-1).values
        assert (l2[..., 0] == l2[..., 1])[tv].all() and (l2[..., 0] != l2[..., 1])[pv].all()  # ties are bit-exact in the logits
        assert ((w == w.amax(-1, keepdim=True)).sum(-1)[tv] == 2).all()
    # depth classes
    pt, inv_q, cls = A.make_depth_inputs(w, b, V, 32)
    o = A.forward(logit, val, V, pt=pt, inv_q=inv_q)
    zc = o["zc"]
    assert pt.dtype == torch.float32 and (pt.abs() > 100).any()
    assert (zc[cls == 0] < -1e-3).all() and ((zc[cls == 1] > 1e-3) & (zc[cls == 1] < 10 - 1e-3)).all() and (zc[cls == 2] > 10 + 1e-3).all()
    assert (zc.abs() > 1e-3).all() and ((zc - 10).abs() > 1e-3).all()
    for k in range(3):
        assert (cls == k).double().mean().item() >= 0.1, (k, shape)
    assert torch.equal(o["depth"][cls == 0], torch.zeros_like(zc[cls == 0])) and torch.equal(o["depth"][cls == 2], torch.full_like(zc[cls == 2], 10.0))
    # the same classes hold for the weights rounded to fp32 (what the backward kernel is given)
    zc32 = A.backward(w.float(), val, torch.zeros(b, R, 1), V, ddepth=torch.ones(b, R), pt=pt, inv_q=inv_q)["zc"]
    assert torch.equal(zc32 < 0, zc < 0) and torch.equal(zc32 > 10, zc > 10) and (zc32 - zc).abs().max().item() < 1e-3
    # one-hot rays
    lg, hot = A.one_hot_logits(b, V, R, P, 33)
    wr = A.ray_major(A.forward(lg, val, V)["w"], b, V)
    assert torch.equal(wr, F.one_hot(hot, V * P).double())
