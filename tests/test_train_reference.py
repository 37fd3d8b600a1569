"""tests/train_reference.py checked on the CPU: every closed-form stage adjoint, and their composition, against torch.autograd through the
restated stage forwards on a self-consistent float64 record (<= 1e-12 of the composed bound per entry: float64 rounding of it); planted
cases whose results the test states; and the bound's self-test (a float32 run never leaves it)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import attention_reference as AR
import parity_rule as PR
import train_reference as T

F32, F64 = torch.float32, torch.float64
C_LEVELS, DL, HID, BLOCKS = ((6, 5, 8), (3, 4, 8)), 8, 16, 2          # (H, W, C_l) per level: C = 16
TOL64 = 1e-12

# name -> (mode, b, V, R, P, repeat)
CASES = {"concat2": ("concat2", 2, 2, 5, 4, True), "concat2-no-repeat": ("concat2", 2, 2, 5, 4, False), "concat2-ragged": ("concat2", 1, 2, 37, 5, True),
         "concat3": ("concat3", 2, 3, 5, 4, True), "concat3-no-repeat": ("concat3", 1, 3, 7, 3, False), "single": ("single", 2, 1, 5, 4, True),
         "single-no-repeat": ("single", 1, 1, 37, 5, False), "plain-V1": ("plain", 2, 1, 5, 4, True), "plain-V2": ("plain", 1, 2, 37, 5, True),
         "plain-V3": ("plain", 2, 3, 5, 4, False)}


def _up(x, m):
    return (x + m - 1) // m * m


def make_params(mode, V, seed):
    g = PR.gen(seed)
    C = sum(c for _, _, c in C_LEVELS)
    Ce = {"concat2": C, "concat3": 3 * (C // 2), "single": C, "plain": C}[mode]
    shapes = {"latent_value": (DL, Ce, 1), "key_map": (128, Ce, 1, 1), "key_map_2": (128, 128, 1, 1), "query_embed": (128, 16, 1, 1), "query_embed_2": (128, 128),
              "encode_latent": (128, DL), "query_repeat_embed": (128, 144, 1, 1), "query_repeat_embed_2": (128, 128, 1, 1), "phi.lin_in": (HID, 9 * V),
              "phi.lin_out": (3, HID)}
    if mode in ("concat2", "concat3"):
        shapes.update({"query_encode_latent": (C, C + 3, 1, 1), "query_encode_latent_2": (C // 2, C, 1, 1)})
    if mode == "single":
        shapes["update_val_merge"] = (C, C + 6, 1, 1)
    for i in range(BLOCKS):
        shapes.update({f"phi.lin_z.{i}": (HID, V * DL), f"phi.blocks.{i}.fc_0": (HID, HID), f"phi.blocks.{i}.fc_1": (HID, HID)})
    par = {}
    for n, s in shapes.items():
        par[n + ".weight"] = (torch.randn(*s, generator=g, dtype=F64) / s[1] ** 0.5)
        par[n + ".bias"] = 0.1 * torch.randn(s[0], generator=g, dtype=F64)
    return par


def make_geometry(mode, b, V, R, P, seed):
    g = PR.gen(seed + 1000)
    n, S, pts = b * V, b * V * R * P, R * P
    u = lambda *s: torch.rand(*s, generator=g) * 2.4 - 1.2                      # a tenth of the points beyond the maps' edge
    poses = torch.randn(n, 96, generator=g)
    poses[:, 88] = 2.0                                                         # depths on both sides of the clamp at 0 and inside it
    geom = dict(pixel_val=u(n, R, P, 2), g=torch.randn(S, 16, generator=g).double(), pt=3 * torch.randn(n, R, P, 3, generator=g), poses=poses,
                phi_x=torch.zeros(b * R, _up(9 * V, 4), dtype=F64), valid=(torch.rand(b, R, 1, generator=g) < 0.7).double(), grid_other=None, cross=None, ptcols=None)
    geom["phi_x"][:, :9 * V] = torch.randn(b * R, 9 * V, generator=g)
    if mode == "concat2":
        geom.update(grid_other=u(b, V, R, P, 2), ptcols=torch.randn(S * 2, 3, generator=g).tanh().double())
    if mode == "concat3":
        geom.update(cross=[(c, o, k, u(b, pts, 2)) for c in range(3) for k, o in enumerate([o for o in range(3) if o != c], 1)],
                    ptcols=torch.randn(S * 3, 3, generator=g).tanh().double())
    if mode == "single":
        geom["ptcols"] = torch.randn(S, 6, generator=g).tanh().double()
    maps = [torch.randn(n, H, W, Cl, generator=g).double() for H, W, Cl in C_LEVELS]
    return geom, maps


@functools.lru_cache(maxsize=None)
def case(name):
    mode, b, V, R, P, repeat = CASES[name]
    par = make_params(mode, V, seed=sum(map(ord, name)))
    geom, maps = make_geometry(mode, b, V, R, P, seed=sum(map(ord, name)))
    with torch.no_grad():
        rec = T.forward(par, geom, maps, mode, repeat)
    return mode, repeat, par, geom, maps, rec


def cot(shape, seed):
    return torch.randn(*shape, generator=PR.gen(seed)).double()


def leaves(ts):
    return {k: v.detach().clone().requires_grad_(True) for k, v in ts.items()}


def agree(got, want, what, tol=TOL64):
    """`got` a pair from the adjoint, `want` autograd's tensor."""
    v, B = got
    assert v.shape == want.shape, (what, v.shape, want.shape)
    r = PR.ratio(v, want, B)
    assert r <= tol, (what, r)


def check_grads(G, par, autograd, what):
    """G: the adjoint's {name: pair}; autograd: {name: tensor or None}.  Same names, every entry within the bound."""
    assert sorted(G) == sorted(k for k, v in autograd.items() if v is not None), (what, sorted(set(G) ^ {k for k, v in autograd.items() if v is not None}))
    for k, pair in G.items():
        agree(pair, autograd[k], (what, k))


def grads_of(loss, par):
    names = list(par)
    return dict(zip(names, torch.autograd.grad(loss, [par[k] for k in names], allow_unused=True, retain_graph=True)))


# ---- the record is what the issue asks of it ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_no_preactivation_of_the_seeded_records_is_exactly_zero(name):
    mode, repeat, par, geom, maps, rec = case(name)
    pre = {"k1": F.linear(rec["e"], T.weight(par, "key_map"), par["key_map.bias"]),
           "q1": F.linear(rec["g"], T.weight(par, "query_embed"), par["query_embed.bias"]), "dec_out": rec["dec_out"]}
    pre.update({f"xa{i}": t for i, t in enumerate(rec["xas"])})
    pre.update({f"net{i}": t for i, t in enumerate(rec["nets"])})
    if rec["h1"] is not None:
        pre["h1"] = F.linear(rec["enc_rows"], T.weight(par, "query_encode_latent"), par["query_encode_latent.bias"])
    if repeat:
        Wr = T.weight(par, "query_repeat_embed")
        pre["k1r"] = F.linear(rec["g"], Wr[:, 128:], par["query_repeat_embed.bias"]) + (rec["hb"] @ Wr[:, :128].T)[T.ray_of_rows(T.sizes(rec))]
    for k, t in pre.items():
        assert bool((t != 0).all()), k
        assert bool((t > 0).any()) and bool((t < 0).any()), k               # both branches of every ReLU are taken
    for k in ("k1", "q1", "h1", "k1r"):
        if k in pre:
            assert torch.equal(rec[k], F.relu(pre[k])), k
    zc = T.depth_readout(rec["at_wt"], rec["pt"], rec["poses"], T.sizes(rec))[1]
    assert bool(((zc != 0) & (zc != 10)).all())
    if name == "concat2-ragged":
        assert bool((zc < 0).any()) and bool(((zc > 0) & (zc < 10)).any())


# ---- every stage adjoint against autograd through the restated forward -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_decode_adjoint_is_autograds(name):
    mode, repeat, par, geom, maps, rec = case(name)
    z = T.sizes(rec)
    p = leaves(par)
    zl = rec["zrep"][:, :DL].clone().requires_grad_(True)
    out = T.decode(p, rec["phi_x"], zl.repeat(1, z["V"]), rec["valid"])
    assert torch.equal(out["dec_out"][0].detach(), rec["dec_out"])
    d_rgb = cot((z["b"], z["R"], 3), 1)
    loss = (out["rgb"][0] * d_rgb).sum()
    d_z, G = T.decode_adjoint(rec, par, d_rgb)
    agree(d_z, torch.autograd.grad(loss, zl, retain_graph=True)[0], "d_z")
    check_grads(G.shaped(), par, grads_of(loss, p), "decode")
    assert all(k.startswith("phi.") for k in G)


@pytest.mark.parametrize("name", CASES)
def test_attention_rounds_adjoint_is_autograds(name):
    mode, repeat, par, geom, maps, rec = case(name)
    z = T.sizes(rec)
    p = leaves(par)
    x = leaves({k: rec[k] for k in ("e", "q", "key")})
    out = T.attention_rounds(p, dict(rec, **x), repeat)
    assert torch.equal(out["zrep"][0].detach(), rec["zrep"]) and torch.equal(out["at_wt"].detach(), rec["at_wt"])
    d_z, d_depth = cot((z["bR"], DL), 2), cot((z["bR"],), 3)
    loss = (out["zrep"][0][:, :DL] * d_z).sum() + (out["depth"].reshape(-1) * d_depth).sum()
    d_e, d_key, d_q, G = T.attention_rounds_adjoint(rec, par, d_z, d_depth, repeat)
    for pair, k in ((d_e, "e"), (d_key, "key"), (d_q, "q")):
        agree(pair, torch.autograd.grad(loss, x[k], retain_graph=True)[0], "d_" + k)
    check_grads(G.shaped(), par, grads_of(loss, p), "attention_rounds")
    assert sorted({k.rsplit(".", 1)[0] for k in G}) == sorted(["latent_value"] + (["encode_latent", "query_repeat_embed", "query_repeat_embed_2"] if repeat else []))
    # the same adjoint without a depth cotangent: the depth term alone is missing
    loss0 = (out["zrep"][0][:, :DL] * d_z).sum()
    d_e0, _, _, _ = T.attention_rounds_adjoint(rec, par, d_z, None, repeat)
    agree(d_e0, torch.autograd.grad(loss0, x["e"], retain_graph=True)[0], "d_e without depth")


@pytest.mark.parametrize("name", CASES)
def test_attend_adjoint_is_attention_references_backward(name):
    """The dtype-parametrised attention adjoint in float64 is attention_reference.backward, values and bounds."""
    mode, repeat, par, geom, maps, rec = case(name)
    z = T.sizes(rec)
    D = rec["e"].shape[1]
    dz, dd = cot((z["bR"], D), 4), cot((z["bR"],), 5)
    (dl, Bl), (dv, _) = T.attend_adjoint(T.REF, rec["at_wt"], rec["e"], T.given(dz), z, dd, rec["pt"], rec["poses"])
    want = AR.backward(rec["at_wt"], rec["e"].reshape(z["n"], z["R"], z["P"], D), dz.reshape(z["b"], z["R"], D), z["V"], dd.reshape(z["b"], z["R"]), rec["pt"],
                       T.inv_q_of(rec["poses"], z["V"]))
    assert torch.equal(dl, want["dlogit"].reshape(-1)) and torch.equal(Bl, want["Bl"].reshape(-1)) and torch.equal(dv, want["dval"].reshape(-1, D))


@pytest.mark.parametrize("name", CASES)
def test_keys_and_queries_adjoint_is_autograds(name):
    mode, repeat, par, geom, maps, rec = case(name)
    z = T.sizes(rec)
    p = leaves(par)
    e = rec["e"].clone().requires_grad_(True)
    out = T.keys_and_queries(p, e, rec["g"])
    assert torch.equal(out["key"][0].detach(), rec["key"]) and torch.equal(out["q"][0].detach(), rec["q"])
    d_e, d_key, d_q = cot(e.shape, 6), cot((z["S"], 128), 7), cot((z["S"], 128), 8)
    loss = (e * d_e).sum() + (out["key"][0] * d_key).sum() + (out["q"][0] * d_q).sum()
    got, G = T.keys_and_queries_adjoint(rec, par, d_e, d_key, d_q)
    agree(got, torch.autograd.grad(loss, e, retain_graph=True)[0], "d_e")
    check_grads(G.shaped(), par, grads_of(loss, p), "keys_and_queries")


def e_forward(mode, p, geom, maps, b):
    if mode == "concat2":
        return T.e_concat2(p, T.rows_concat2(maps, geom["pixel_val"], geom["grid_other"], geom["ptcols"]))["e"][0]
    if mode == "concat3":
        return T.e_concat3(p, T.rows_concat3(maps, geom["pixel_val"], geom["cross"], geom["ptcols"], b))["e"][0]
    if mode == "single":
        return T.e_single(p, T.rows_single(maps, geom["pixel_val"], geom["ptcols"]))["e"][0]
    return T.e_plain(maps, geom["pixel_val"])["e"][0]


@pytest.mark.parametrize("name", CASES)
def test_e_adjoint_is_autograds(name):
    mode, repeat, par, geom, maps, rec = case(name)
    p = leaves(par)
    mp = [t.clone().requires_grad_(True) for t in maps]
    e = e_forward(mode, p, geom, mp, T.sizes(rec)["b"])
    assert torch.equal(e.detach(), rec["e"])
    d_e = cot(e.shape, 9)
    loss = (e * d_e).sum()
    dmaps, G = T.E_ADJOINT[mode](rec, par, d_e, True)
    for l, (pair, want) in enumerate(zip(dmaps, torch.autograd.grad(loss, mp, retain_graph=True))):
        agree(pair, want, f"level {l}")
        assert bool((want != 0).any())
    check_grads(G.shaped(), par, grads_of(loss, p), "e")
    none, G0 = T.E_ADJOINT[mode](rec, par, d_e, False)
    assert none is None and all(torch.equal(G0[k][0], G[k][0]) for k in G) and sorted(G0) == sorted(G)


@pytest.mark.parametrize("name", CASES)
def test_the_composed_backward_is_autograds(name):
    mode, repeat, par, geom, maps, rec = case(name)
    z = T.sizes(rec)
    p = leaves(par)
    mp = [t.clone().requires_grad_(True) for t in maps]
    out = T.forward(p, geom, mp, mode, repeat)
    d_rgb, d_depth = cot((z["b"], z["R"], 3), 10), cot((z["b"], z["R"]), 11)
    loss = (out["rgb"] * d_rgb).sum() + (out["depth"] * d_depth).sum()
    grads, levels = T.backward(rec, par, d_rgb, d_depth, mode, True)
    check_grads(grads, par, grads_of(loss, p), "backward")
    assert all(v.shape == par[k].shape for k, (v, _) in grads.items())
    for l, (pair, want) in enumerate(zip(levels, torch.autograd.grad(loss, mp))):
        agree(pair, want.permute(0, 3, 1, 2), f"level {l}")
    # the layers the mode does not read get no gradient at all
    assert ("update_val_merge.weight" in grads) == (mode == "single") and ("query_encode_latent.weight" in grads) == (mode in ("concat2", "concat3"))
    assert ("encode_latent.weight" in grads) == repeat
    # one flag per level: a level that asks for none gets None, the others are unchanged
    asks = [l != 0 for l in range(len(maps))]
    grads1, levels1 = T.backward(rec, par, d_rgb, d_depth, mode, asks)
    assert levels1[0] is None and all(torch.equal(a[0], b_[0]) for a, b_ in zip(levels1[1:], levels[1:]))
    assert all(torch.equal(grads1[k][0], grads[k][0]) for k in grads)


# ---- planted cases -------------------------------------------------------------------------------------------------------------------------------
def test_an_activation_that_is_exactly_zero_of_either_sign_gets_no_gradient():
    """!(act > 0) -> 0.  Saved pre-activations (the decoder's): with +0.0 and -0.0 planted the adjoint equals that of a record holding -1
    there.  Saved rectified activations (k1, h1): -0.0 behaves as +0.0.  And the rule itself on one row."""
    mode, repeat, par, geom, maps, rec = case("concat2")
    d_rgb, d_e, d_key, d_q = cot((2, 5, 3), 12), cot(rec["e"].shape, 13), cot(rec["key"].shape, 14), cot(rec["q"].shape, 15)

    row = int(rec["valid"].reshape(-1).nonzero()[0])                        # a ray the image gradient reaches
    live = [rec[k][row, :4] for k in ("dec_out", "k1", "h1")] + [rec["xas"][0][row, :4], rec["nets"][1][row, :4]]
    assert all(bool((t > 0).any()) for t in live)                           # every planted place held a live entry before

    def planted(values, keys):
        r = dict(rec, xas=[t.clone() for t in rec["xas"]], nets=[t.clone() for t in rec["nets"]], **{k: rec[k].clone() for k in ("dec_out", "k1", "h1")})
        for t in [r[k] for k in keys if k in r] + ([r["xas"][0], r["nets"][1]] if "dec_out" in keys else []):
            t[row, :4] = torch.tensor(values, dtype=F64)
        return r

    def same(a, b_):
        (ca, Ga), (cb, Gb) = a, b_
        pairs = list(zip(ca, cb)) if isinstance(ca, list) else [(ca, cb)]
        return all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in pairs) and all(torch.equal(Ga[k][0], Gb[k][0]) for k in Ga)
    dec = lambda r: T.decode_adjoint(r, par, d_rgb)
    assert same(dec(planted([0.0, -0.0, 0.0, -0.0], ("dec_out",))), dec(planted([-1.0] * 4, ("dec_out",))))
    assert not same(dec(planted([0.0, -0.0, 0.0, -0.0], ("dec_out",))), dec(planted([1.0] * 4, ("dec_out",))))
    for run in (lambda r: T.keys_and_queries_adjoint(r, par, d_e, d_key, d_q), lambda r: T.e_concat2_adjoint(r, par, d_e, True)):
        assert same(run(planted([0.0, -0.0, 0.0, -0.0], ("k1", "h1"))), run(planted([0.0] * 4, ("k1", "h1"))))
    d_x = T._dx(T.REF, T.given(cot((1, 3), 16)), torch.ones(3, 4, dtype=F64), act=torch.tensor([[0.0, -0.0, float("nan"), 1e-300]], dtype=F64))
    assert d_x[0][0, :3].tolist() == [0.0, 0.0, 0.0] and d_x[0][0, 3] != 0 and d_x[1][0, :3].tolist() == [0.0, 0.0, 0.0]


def test_a_one_hot_softmax_gives_no_logit_gradient():
    b, V, R, P, D = 2, 2, 5, 4, 6
    logit, hot = AR.one_hot_logits(b, V, R, P, seed=3)
    z = dict(b=b, V=V, R=R, P=P, n=b * V, S=b * V * R * P, bR=b * R, pts=R * P)
    w = AR.view_major(torch.softmax(AR.ray_major(logit, b, V), -1), b, V)
    assert bool(((w == 0) | (w == 1)).all())
    e, dz = cot((z["S"], D), 17), cot((z["bR"], D), 18)
    for ar in (T.REF, T.Arith(F32)):
        (dl, Bl), (dv, _) = T.attend_adjoint(ar, w, e, T.given(dz, ar.dtype), z)
        assert bool((dl == 0).all())
        dvr = T._rays(dv, z)                                              # [b, R, V P, D]: dz on the hot sample, zero elsewhere
        want = torch.zeros_like(dvr).scatter_(2, hot[..., None, None].expand(b, R, 1, D), dz.to(ar.dtype).reshape(b, R, 1, D))
        assert torch.equal(dvr, want)


def test_with_one_view_the_view_sum_is_the_identity():
    mode, repeat, par, geom, maps, rec = case("single")
    p = leaves(par)
    zrep = rec["zrep"].clone().requires_grad_(True)
    d_rgb = cot((2, 5, 3), 19)
    loss = (T.decode(p, rec["phi_x"], zrep, rec["valid"])["rgb"][0] * d_rgb).sum()
    agree(T.decode_adjoint(rec, par, d_rgb)[0], torch.autograd.grad(loss, zrep)[0], "d_z = d_zrep")
    out = T.attention_rounds(par, rec, True)
    want = rec["z1"] + F.linear(rec["ebar2"], T.weight(par, "latent_value"), par["latent_value.bias"])           # V z1 with V = 1
    assert torch.equal(out["zrep"][0], want) and out["zrep"][0].shape == (10, DL)


def test_a_valid_mask_of_zeros_stops_the_image_gradient_but_not_the_depth_gradient():
    mode, repeat, par, geom, maps, rec = case("concat2")
    dead = dict(rec, valid=torch.zeros_like(rec["valid"]))
    d_rgb, d_depth = cot((2, 5, 3), 20), cot((2, 5), 21)
    grads, levels = T.backward(dead, par, d_rgb, d_depth, mode, True)
    rgb_only = {k for k in grads if k.startswith("phi.") or k.split(".")[0] in ("latent_value", "encode_latent", "query_repeat_embed", "query_repeat_embed_2")}
    for k, (v, B) in grads.items():
        assert bool((v == 0).all() and (B == 0).all()) == (k in rgb_only), k
    assert all(bool((lv[0] != 0).any()) for lv in levels)
    want, levels_d = T.backward(rec, par, None, d_depth, mode, True)       # the depth cotangent alone on the live record
    assert all(torch.equal(grads[k][0], want[k][0]) for k in grads if k not in rgb_only)
    assert all(torch.equal(a[0], b_[0]) for a, b_ in zip(levels, levels_d))
    nothing, _ = T.backward(rec, par, d_rgb, None, mode, True)
    assert bool((nothing["phi.lin_out.bias"][0] != 0).any())


@pytest.mark.parametrize("name", ("concat2", "concat3", "single", "plain-V2"))
def test_without_need_dz_there_is_no_level_gradient_and_the_same_parameter_gradients(name):
    mode, repeat, par, geom, maps, rec = case(name)
    d_rgb, d_depth = cot((T.sizes(rec)["bR"], 3), 22), cot((T.sizes(rec)["bR"],), 23)
    g1, l1 = T.backward(rec, par, d_rgb, d_depth, mode, True)
    g0, l0 = T.backward(rec, par, d_rgb, d_depth, mode, False)
    assert l0 == [None] * len(maps) and all(lv is not None for lv in l1)
    assert sorted(g0) == sorted(g1) and all(torch.equal(g0[k][0], g1[k][0]) and torch.equal(g0[k][1], g1[k][1]) for k in g1)


# ---- the bound's self-test ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_a_float32_run_stays_inside_the_bound(name):
    """Per stage and for the composition: the float32 run of the adjoint against the float64 run, entry by entry over the float64 run's bound,
    is finite and below 1 — so the bound is never smaller than a float32 rounding of the value it goes with — and not zero (the two runs
    are different arithmetic)."""
    mode, repeat, par, geom, maps, rec = case(name)
    z = T.sizes(rec)
    f32 = T.Arith(F32)
    d_rgb, d_depth, d_z = cot((z["bR"], 3), 24), cot((z["bR"],), 25), cot((z["bR"], DL), 26)
    d_e, d_key, d_q = cot(rec["e"].shape, 27), cot((z["S"], 128), 28), cot((z["S"], 128), 29)

    def flat(res):
        """Every pair of a stage's result, by name."""
        *cots, G = res
        out = {f"param {k}": v for k, v in (G.shaped() if isinstance(G, T.Grads) else G).items()}
        for i, c in enumerate(cots):
            for j, pair in enumerate(c if isinstance(c, list) else [c]):
                if pair is not None:
                    out[f"cotangent {i}.{j}"] = pair
        return out
    stages = {"decode": lambda ar: T.decode_adjoint(rec, par, d_rgb, ar), "attention_rounds": lambda ar: T.attention_rounds_adjoint(rec, par, d_z, d_depth, repeat, ar),
              "keys_and_queries": lambda ar: T.keys_and_queries_adjoint(rec, par, d_e, d_key, d_q, ar), "e": lambda ar: T.E_ADJOINT[mode](rec, par, d_e, True, ar),
              "backward": lambda ar: tuple(reversed(T.backward(rec, par, d_rgb, d_depth, mode, True, ar)))}
    for stage, run in stages.items():
        r64, r32 = flat(run(T.REF)), flat(run(f32))
        assert sorted(r64) == sorted(r32) and r64
        worst = 0.0
        for k, (v64, B) in r64.items():
            v32, B32 = r32[k]
            assert v32.dtype == F32 and v64.dtype == F64 and B.dtype == F64 and B32.dtype == F64, (stage, k)
            r = PR.ratio(v32, v64, B)
            assert r < 1.0, (stage, k, r)
            assert bool((B >= v64.abs()).all()), (stage, k)                # a sum of magnitudes is never below the magnitude of the sum
            worst = max(worst, r)
        assert 0.0 < worst < 1.0, (stage, worst)


def test_the_entitled_arithmetic_takes_the_split_routes_exactly_where_the_dispatch_says():
    """Arith(F32, min_rows, wgrad_fp32): the emulations on the launches the predicates name, float32 on the others, float32 throughout on the
    conservative route's weight gradients."""
    g = PR.gen(5)
    x, W, b_ = torch.randn(40, 64, generator=g), torch.randn(32, 64, generator=g), torch.randn(32, generator=g)
    ar = T.Arith(F32, 40, False)
    assert T.takes_x3(40, 64, 32, 40) and not T.takes_x3(39, 64, 32, 40) and not T.takes_x3(40, 63, 32, 40) and not T.takes_x3(40, 64, 48, 40)
    import linear_reference as LR
    assert torch.equal(ar.lin(x, W, b_), LR.x3_linear(x, W, b_).float())
    assert torch.equal(ar.lin(x[:39], W, b_), F.linear(x[:39], W, b_))
    assert torch.equal(T.Arith(F32).lin(x, W, b_), F.linear(x, W, b_))
    dy, xx = torch.randn(2048, 32, generator=g), torch.randn(2048, 32, generator=g)
    assert LR.wgrad_dispatch(2048, 32, 32, True) == "bf16" and LR.wgrad_dispatch(2047, 32, 32, True) == "tile22"
    want = LR.wgrad_bf16(dy, xx, True, torch.zeros(32, 32), torch.zeros(32))
    got = ar.wgrad(dy, xx, True, True)
    assert torch.equal(got[0], want[0].float()) and torch.equal(got[1], want[1].float())
    plain = T.Arith(F32, 40, True).wgrad(dy, xx, True, True)
    assert torch.equal(plain[0], dy.T @ F.relu(xx)) and torch.equal(plain[1], dy.sum(0))
    short = ar.wgrad(dy[:2047], xx[:2047], False, False)
    assert torch.equal(short[0], dy[:2047].T @ xx[:2047]) and short[1] is None
