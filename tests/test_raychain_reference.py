"""tests/raychain_reference.py checked against the oracle's lines and against itself, without a GPU: the decoder against
``oracle.car_oracle.resnet_fc``, z1 and z against the oracle's latent_value path through both attention rounds, finalize against the
blend written out, the magnitudes that make the exact-integer case of test_raychain_hip.py a valid bit-for-bit claim, and the
conditioning of every case whose tolerance is derived from the float32 run."""
import pytest
import torch
import torch.nn.functional as F

import raychain_reference as RC
from oracle import car_oracle as O

F64 = torch.float64


def _dbl(params):
    return {k: v.double() for k, v in params.items()}


@pytest.mark.parametrize("shape", ((1, 2, 33), (3, 3, 43), (1, 1, 5)))
def test_fp64_tail_decoder_equals_the_oracles_resnet_fc(shape):
    b, V, R = shape
    params = RC.gaussian_params(3)
    ebar, z1, phi_x = RC.gaussian_inputs(b * R, 4)
    out = RC.tail(params, ebar, phi_x, z1, torch.ones(b, V, R), V)
    z = out["z"]
    want = O.resnet_fc(_dbl(params), torch.cat([z, z, phi_x.double()], dim=-1), d_latent=2 * RC.E)
    assert want.shape == out["raw"].shape == (b * R, 3)
    assert (out["raw"] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert torch.equal(out["rgb"], out["raw"])                                      # every ray valid: the blend changes nothing


@pytest.mark.parametrize("shape", ((1, 2, 9, 7), (2, 3, 5, 4), (2, 1, 6, 3)))
def test_z1_and_z_equal_the_oracles_latent_value_path(shape):
    """models.py:487, 532-565 restated from oracle/car_oracle.py's forward (only its _conv1x1 is a function to call; the oracle has no
    separate entry for this stretch, so this shows the algebra, not agreement with a function of the oracle's): val = latent_value(e) per sample, z_local = the views' sum of sum_s w_s val_s,
    second round z = the views' sum of (sum_s w2_s val_s + z_local).  The softmax weights of a ray sum to 1 over its V P samples, so
    the kernels' order (attention average of e first, then latent_value) is the same numbers."""
    b, V, R, P = shape
    g = RC.gen(6)
    p = _dbl(RC.gaussian_params(5))
    e = torch.randn(b * V, R, P, RC.C, generator=g, dtype=F64)

    def ray_softmax(logit):
        lg = logit.reshape(b, V, R, P).permute(0, 2, 1, 3).reshape(b, R, V * P)
        return F.softmax(lg, dim=-1).reshape(b, R, V, P).permute(0, 2, 1, 3).flatten(0, 1)

    def view_sum(x):
        return x.reshape(b, V, *x.shape[1:]).sum(dim=1, keepdim=True).expand(-1, V, *([-1] * (x.dim() - 1))).flatten(0, 1)
    w1, w2 = (ray_softmax(torch.randn(b * V, R, P, generator=g, dtype=F64) * 3) for _ in range(2))
    val = O._conv1x1(e, p["latent_value.weight"], p["latent_value.bias"])
    z_local = view_sum((val * w1[..., None]).sum(dim=2))
    z_final = view_sum((val * w2[..., None]).sum(dim=2) + z_local)

    def ebar(w):
        return (e * w[..., None]).sum(dim=2).reshape(b, V, R, RC.C).sum(dim=1).reshape(b * R, RC.C)
    m = RC.mid(p, ebar(w1))
    want1 = z_local.reshape(b, V, R, RC.E)[:, 0].reshape(b * R, RC.E)
    assert (m["z1"] - want1).abs().max().item() <= 1e-12 * want1.abs().max().item()
    t = RC.tail(p, ebar(w2), torch.zeros(b * R, RC.PHI, dtype=F64), m["z1"], torch.ones(b, V, R), V)
    want = z_final.reshape(b, V, R, RC.E)[:, 0].reshape(b * R, RC.E)
    assert (t["z"] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    h = O._conv1x1(z_local, p["encode_latent.weight"], p["encode_latent.bias"]).reshape(b, V, R, RC.D)[:, 0].reshape(b * R, RC.D)
    uh = h @ p["query_repeat_embed.weight"][:, :RC.D].T
    assert (m["uh"] - uh).abs().max().item() <= 1e-12 * uh.abs().max().item()


def test_finalize_equals_the_blend_written_out():
    b, V, R = 2, 3, 7
    g = RC.gen(8)
    rgb_in = torch.randn(b * R, 4, generator=g, dtype=F64)
    ov = RC.random_overlaps(b, V, R, 9, p=0.3)
    rgb, valid = RC.finalize(rgb_in, ov)
    assert 0 < valid.sum().item() < b * R
    for s in range(b):
        for r in range(R):
            any_view = any(ov[s, v, r].item() != 0 for v in range(V))
            m = 1.0 if any_view else 0.0
            assert valid[s * R + r].item() == m
            for k in range(3):
                assert rgb[s * R + r, k].item() == rgb_in[s * R + r, k].item() * m + (1.0 - m)
    rays = RC.rays_from_overlaps(ov)
    assert rays.shape == (b * V, R, 12) and torch.equal(rays[:, :, 10].reshape(b, V, R), ov) and bool(torch.isnan(rays[:, :, :10]).all())


def test_exact_integer_case_is_exact_in_22_bit_operands_and_fp32_sums():
    """What makes `z1`, `uh` and `rgb` of the integer case comparable BIT FOR BIT with float64: every input, weight, bias, output and
    every possible partial sum (bounded by sum |W| |x| + |b| + |what the layer adds to|) of every layer is an integer below 2^22 — so a
    22-bit hi + lo operand pair and an fp32 accumulator hold each of them exactly, in any order of summation, and weights of +-1 / +-2
    have no low half whose dropped lo x lo product could matter; some input of every layer is at least 2^12 with an odd value, so its
    lo half is NOT zero; the dead rays' x is non-positive in front of fc_0 of block 0; the two halves of lin_z differ and do not cancel.
    The issue's text asks for inputs in [-8, 8] AND for 2^12 in every layer's input, which no such weights can join: three rays in
    four keep [-8, 8], every fourth is wide."""
    params, ebar, z1, phi_x = RC.integer_case()
    M = ebar.shape[0]
    narrow = torch.arange(M) % 4 != 1
    for t in (ebar, z1, phi_x):
        assert bool((t == t.round()).all()) and t[narrow].abs().max().item() <= 8 and t[~narrow].abs().min().item() > 2 ** 12
    for name, (n, k) in RC.SHAPES.items():
        W, bias = params[name + ".weight"], params[name + ".bias"]
        assert bool((bias == bias.round()).all()) and bias.abs().max().item() <= 4
        if ".lin_z." in name:
            a, c = W[:, :RC.E], W[:, RC.E:]
            assert bool(((a != 0).sum(1) == 2).all()) and bool(((c != 0).sum(1) == 2).all()) and bool((W.abs() <= 1).all())
            assert bool((a != c).any(dim=1).all()) and bool(((a + c) != 0).any(dim=1).all()) and bool(((a + c).abs() == 2).any())
        else:
            Wk = W[:, :RC.D] if name == "query_repeat_embed" else W
            assert bool(((Wk != 0).sum(1) == 2).all()) and bool((Wk.abs() <= 1).all())
    trace = []
    m = RC.mid(params, ebar, trace=trace)
    ov = RC.random_overlaps(1, RC.INT_V, M, 3)
    t = RC.tail(params, ebar, phi_x, z1, ov, RC.INT_V, trace=trace)
    assert len(trace) == 3 + 12
    for name, x, W, bias, res, y in trace:
        bound = x.abs() @ W.abs().T + (bias.abs() if bias is not None else 0) + (res.abs() if res is not None else 0)
        for v in (x, y, bound):
            assert bool((v == v.round()).all()) and v.abs().max().item() < 2 ** 22, name
        big = x[x.abs() >= 2 ** 12]
        assert big.numel() > 0 and bool((big.abs() % 2 == 1).any()), f"{name}: no input whose lo half carries bits"
    dead = list(RC.INT_DEAD)
    fc0 = [tr for tr in trace if tr[0] == "phi.blocks.0.fc_0"][0]
    assert bool((fc0[1][dead] == 0).all()) and torch.equal(fc0[5][dead], params["phi.blocks.0.fc_0.bias"].double().expand(len(dead), -1))
    assert bool((t["z"][dead] == 0).all())
    for out, keys in ((m, ("z1", "uh")), (t, ("rgb",))):                              # and float32 reproduces float64 on them, bit for bit
        f32 = RC.mid(params, ebar, torch.float32) if out is m else RC.tail(params, ebar, phi_x, z1, ov, RC.INT_V, torch.float32)
        for k in keys:
            assert torch.equal(f32[k].double(), out[k]), k


@pytest.mark.parametrize("tag", RC.mid_tags() + RC.tail_tags())
def test_float32_ratio_of_every_tolerance_case_is_finite_and_small(tag):
    """The kernel's tolerance is 8 x max(this ratio, 2^-22): a case whose float32 run is already far from float64 relative to the last
    layer's bound is ill-conditioned and would excuse a wrong kernel."""
    c = RC.case(tag)
    if tag.startswith("mid"):
        ref, f32 = RC.mid(c["params"], c["ebar"]), RC.mid(c["params"], c["ebar"], torch.float32)
        pairs = (("z1", "B_z1"), ("uh", "B_uh"))
    else:
        args = (c["params"], c["ebar"], c["phi_x"], c["z1"], c["overlaps"], c["V"])
        ref, f32 = RC.tail(*args), RC.tail(*args, torch.float32)
        pairs = (("rgb", "B_rgb"),)
        assert torch.equal(ref["valid"], f32["valid"].double())
    for k, bk in pairs:
        r = RC.ratio(f32[k], ref[k], ref[bk])
        print(f"[fp32] {tag} {k}: {r:.3e}")
        assert r == r and r < 1e-5, (tag, k, r)
        assert RC.tolerance(r) >= 8 * 2.0 ** -22


def test_case_promises():
    c = RC.case("mid-mag")
    s = c["special"]
    assert bool((c["ebar"][s["zero"]] == 0).all())
    assert c["ebar"][s["last"], -1] != 0 and bool((c["ebar"][s["last"], :-1] == 0).all())
    assert c["ebar"][s["first"], 0] != 0 and bool((c["ebar"][s["first"], 1:] == 0).all())
    norms = c["ebar"][:32].abs().amax(dim=1)
    assert norms[[0, 1, 2, 4]].max().item() < 1e-4 and norms[31].item() > 1e4                        # both ends inside one wave
    z = RC.mid(c["params"], c["ebar"])["z1"][s["zero"]]
    assert torch.equal(z, c["params"]["latent_value.bias"].double())
    p = RC.case("tail-scale1")["params"]
    assert bool((p["phi.lin_z.2.weight"] == 0).all()) and bool((p["phi.lin_z.2.bias"] != 0).any())
    u, g0 = RC.case("tail-scale2")["params"], RC.gaussian_params(1)
    assert bool((u["phi.lin_z.0.weight"][:, :RC.E] == 0).all()) and torch.equal(u["phi.lin_z.0.weight"][:, RC.E:], g0["phi.lin_z.0.weight"][:, RC.E:])
    w1 = u["phi.lin_z.1.weight"]
    assert torch.equal(w1[:, RC.E:], g0["phi.lin_z.1.weight"][:, RC.E:] * 16) and torch.equal(w1[:, :RC.E], g0["phi.lin_z.1.weight"][:, :RC.E])
    assert (w1[:, :RC.E] + w1[:, RC.E:]).abs().max().item() >= 8 * w1[:, :RC.E].abs().max().item()       # the halves' sum, three binary orders up
    assert len({RC.case(t)["b"] * RC.case(t)["R"] for t in RC.tail_tags()}) >= 5
