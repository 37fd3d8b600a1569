"""tests/fused_reference.py checked without a GPU: the float32 restatement against the oracle on a tier-0 and a tier-1 fixture (the
lattice built from the fixture's pyramid by the host shim, the first layer applied per texel in torch), the folded logit against the
unfolded one, the exact-integer case's claim, and — so that test_fused_hip.py cannot pass on inputs that miss the edges — the
conditions every input set of the GPU suite must meet.  Sample records come from the host shim (tests/host/car_geom_host.cpp: the
same car_geom.h functions the kernels call)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fused_reference as FR
import pack_reference as PR
from golden_util import load_case, rel_err
from hip_harness import oracle_cfg
from oracle import car_oracle as O
from test_geom_host import _ptr, run_shim, shim  # noqa: F401  (shim: the fixture that compiles the host library)

F64 = torch.float64


def records_of(samples):
    """CarSample records [..., 36] of the shim -> the dict fused_reference wants, flattened over samples."""
    s = torch.as_tensor(samples).reshape(-1, samples.shape[-1])
    assert s.shape[1] == 36
    return {"grid": s[:, 0:2].contiguous(), "pt": s[:, 2:5].contiguous(), "g": s[:, 5:21].contiguous(),
            "pt_in": s[:, 21:30].reshape(-1, 3, 3).contiguous(), "grid_in": s[:, 30:36].reshape(-1, 3, 2).contiguous()}


def host_records(lib, c, rays_edit=FR.patch_rays):
    """The sample records of a case of fused_reference.CASES, made on the host."""
    from cross_attention_renderer_amd.poses import pack_poses
    inp, uv, steps = FR.scene(c)
    b, R, P = c["b"], c["R"], c["P"]
    poses = np.ascontiguousarray(pack_poses(inp, c["H"]).numpy())
    rays = np.zeros((b * 2, R, 12), np.float32)
    lib.host_ray_setup(_ptr(poses), _ptr(np.ascontiguousarray(inp["query"]["uv"].numpy())), b, 2, R, _ptr(rays))
    rays = np.ascontiguousarray(rays_edit(torch.as_tensor(rays)).numpy())
    samples = np.zeros((b * 2, R, P, 36), np.float32)
    fn = lib.host_sample_setup_depth if c["no_sample"] else lib.host_sample_setup
    fn(_ptr(poses), _ptr(rays), _ptr(np.ascontiguousarray(steps.numpy())), b, 2, R, P, c["H"], c["W"], _ptr(samples))
    return records_of(samples)


def lattice_from_pyramid(lib, z, W1):
    """[n_maps][2][lh][lw][C]: every level pushed per texel through its columns of the first layer (torch, float32), then summed on the
    common lattice by the shim's restatement of the merge kernel."""
    Cout = W1.shape[0]
    hm, wm = max(t.shape[2] for t in z), max(t.shape[3] for t in z)
    r = [hm // t.shape[2] for t in z]
    pad = max(r) + 1
    lh, lw = 2 * hm + 2 * pad - 1, 2 * wm + 2 * pad - 1
    n_maps = z[0].shape[0]
    lat = np.zeros((n_maps, 2, lh, lw, Cout), np.float32)
    ia = lambda v: (ctypes.c_int * len(v))(*v)
    c0 = 0
    cols = []
    for t in z:
        cols.append((c0, c0 + t.shape[1]))
        c0 += t.shape[1]
    for n in range(n_maps):
        lv = [np.ascontiguousarray(torch.einsum("chw,oc->hwo", t[n], W1[:, a:b_]).numpy()) for t, (a, b_) in zip(z, cols)]
        ptrs = (ctypes.c_void_p * len(lv))(*[a.ctypes.data for a in lv])
        lib.host_lattice_build(ptrs, ia([t.shape[2] for t in z]), ia([t.shape[3] for t in z]), ia(r), len(z), Cout, lh, lw, pad, _ptr(lat[n]))
    return torch.as_tensor(lat), pad


@pytest.mark.parametrize("name", ["t0_default", "t1_c1"])
def test_float32_restatement_reproduces_the_oracle(shim, name):
    """interp_val and the first round's attention weights (the oracle exposes no logits: softmax of the restatement's logits against
    at_wt1) to the project's 1e-4 contract."""
    from cross_attention_renderer_amd.poses import pack_poses
    c, inp, z, sd, fx = load_case(name)
    b, V, P = c["b"], c["n_view"], c["P"]
    R = inp["query"]["uv"].shape[2]
    with torch.no_grad():
        ora = O.render_forward(sd, inp, z, oracle_cfg(c), debug=True, poses96=pack_poses(inp, c["H"]))
    st = ora["stages"]
    _, _, samples = run_shim(shim, c, inp, host_poses=True)
    rec = records_of(samples)
    Cc = sum(t.shape[1] for t in z)
    W1 = sd["query_encode_latent.weight"].reshape(Cc, -1)
    lat, pad = lattice_from_pyramid(shim, z, W1[:, :Cc].contiguous())
    assert (lat[:, 1, 0] == 0).all() and (lat[:, 1, :, -1] == 0).all()          # the zeros-mode ring, as the kernel's dead taps assume
    out = FR.samples(sd, lat, pad, rec, b * V, V, torch.float32)
    assert rel_err(out["e"].reshape(st["interp_val"].shape), st["interp_val"]) < 1e-4
    lg = out["logit"].reshape(b, V, R, P).permute(0, 2, 1, 3).reshape(b, R, V * P)
    w = F.softmax(lg, dim=-1).reshape(b, R, V, P).permute(0, 2, 1, 3).flatten(0, 1)
    assert rel_err(w, st["at_wt1"]) < 1e-4
    assert 0.05 < out["dead"].float().mean().item() < 0.5                         # the dead rule is exercised, and changes nothing


def test_folded_logit_equals_the_unfolded_one_to_fp32_rounding_of_the_fold(shim):
    """M, v, u, c of pack_reference.bilinear_fold are each rounded once to fp32: the folded form differs from the two closing layers by at
    most 2^-24 of the sum of magnitudes."""
    c = FR.CASES["edge-37-13-2"]
    p = FR.weights("gauss")
    ref = FR.samples(p, FR.case_lattice(c), c["pad"], host_records(shim, c), 2 * c["b"])
    folded = PR.bilinear_fold(p["key_map_2.weight"], p["key_map_2.bias"], p["query_embed_2.weight"], p["query_embed_2.bias"])
    got = FR.folded_logit(p, ref["k1"], ref["x"], folded=folded)
    r = FR.ratio(got, ref["logit"], ref["B_logit"])
    assert 0 < r <= 2.0 ** -24, r
    assert FR.ratio(FR.folded_logit(p, ref["k1"], ref["x"]), ref["logit"], ref["B_logit"]) < 1e-14


def _conditions(c, rec, out):
    """The edges a set must hold; the two-sample set (R = P = 1) can hold none of the statistical ones."""
    Sn = rec["grid"].shape[0]
    n = torch.arange(Sn) // (Sn // (2 * c["b"]))
    cross = torch.stack([(n % 2) != 0, (n % 2) != 1], dim=1)                   # [S, sv]: sv is not the sample's own view
    lh, lw = FR.lattice_dims(c["fh"], c["fw"], c["pad"])
    assert not bool((out["dead"] & ~cross).any())                              # the own view is never dead
    dead = out["dead"][cross].float().mean().item()
    _, ring, _ = FR.lattice_taps(rec["grid"], lw, lh, c["pad"], torch.float32)
    return dead, int(ring.sum()), Sn


@pytest.mark.parametrize("tag", list(FR.CASES))
def test_input_sets_of_the_gpu_suite_meet_their_edges(shim, tag):
    c = FR.CASES[tag]
    rec = host_records(shim, c)
    p, lat = FR.weights(c["wts"]), FR.case_lattice(c)
    ref = FR.samples(p, lat, c["pad"], rec, 2 * c["b"])
    f32 = FR.samples(p, lat, c["pad"], rec, 2 * c["b"], dtype=torch.float32)
    dead, clamped, Sn = _conditions(c, rec, ref)
    print(f"[inputs] {tag}: S {Sn} dead {dead:.3f} clamped in own view {clamped}")
    if c["R"] >= 3:
        assert 0.10 <= dead <= 0.70, dead
        assert clamped > 0
        # non-finite pt scrubbed to 0 (ray 1 of the first set), pt_in saturated by nan_to_num (ray 2 of the last set)
        P = c["P"]
        assert bool((rec["pt"][P:2 * P] == 0).all())
        last = rec["pt_in"][Sn - (c["R"] - 2) * P: Sn - (c["R"] - 3) * P, :2]
        assert bool((last.abs() == FR.FMAX).any())
    assert bool(torch.isfinite(rec["g"]).all()) and bool(torch.isfinite(rec["pt_in"]).all()) and bool(torch.isfinite(rec["grid_in"][:, :2]).all())
    if tag in FR.RAGGED:
        assert 1 <= c["P"] % FR.TILE_STEPS <= 7 and 1 <= c["R"] % FR.TILE_RAYS <= 23
    for k in ("e", "logit"):
        assert bool(torch.isfinite(ref[k]).all()), k
        r = FR.ratio(f32[k], ref[k], ref["B_" + k])
        print(f"[fp32] {tag} {k}: {r:.3e}")
        assert r < 2.0 ** -18, (tag, k, r)
    if c["wts"] == "kbias":
        assert bool((ref["k1"] <= 0).all())
    if c["wts"] == "qbias":
        assert bool((ref["x"] == 0).all())
    if c["wts"] == "w2zero":
        assert torch.equal(ref["e"], p["query_encode_latent_2.bias"].double().repeat(2).expand(Sn, -1))


def test_the_ragged_sets_exist_in_both_directions():
    assert {"edge-23-7-1", "edge-25-9-1", "edge-37-13-2", "edge-49-17-1"} <= set(FR.RAGGED)
    rp = {(FR.CASES[t]["R"] % FR.TILE_RAYS, FR.CASES[t]["P"] % FR.TILE_STEPS) for t in FR.RAGGED}
    assert (23, 7) in rp and (1, 1) in rp                                       # all but one row live, one row live


@pytest.mark.parametrize("tag", list(FR.ROWS_CASES))
def test_rows_sets_meet_their_edges(shim, tag):
    c = FR.ROWS_CASES[tag]
    rec = host_records(shim, c)
    src, grid, pe = FR.rows_lists(c, rec)
    p, lat = FR.weights("gauss"), FR.case_lattice(c)
    ref = FR.rows(p, lat, c["pad"], src, grid, pe)
    f32 = FR.rows(p, lat, c["pad"], src, grid, pe, dtype=torch.float32)
    nc = c["rows_comp"]
    mode = ((src.long() >> 30) & 1).reshape(-1, nc)
    mp = (src.long() & 0x3fffffff).reshape(2 * c["b"], -1, nc)
    assert bool((mp == mp[:, :1]).all()) and len({(int(mp[s, 0, k]), int(mode.reshape(2 * c["b"], -1, nc)[s, 0, k])) for s in range(2 * c["b"]) for k in range(nc)}) \
        == min(2 * c["b"] * nc, 2 * 2 * c["b"])
    assert bool(ref["dead"].any()) and not bool(ref["dead"][mode.reshape(-1) == 0].any())
    assert 0.05 < ref["dead"].float().mean().item() < 0.7
    r = FR.ratio(f32["e"], ref["e"], ref["B_e"])
    print(f"[fp32] {tag} e: {r:.3e}")
    assert r < 2.0 ** -18


def test_exact_integer_case_is_exact_in_fp16_halves_and_fp32_sums(shim):
    """What makes `e` of the integer case comparable BIT FOR BIT: tap weights of exactly 1/4, lattice values multiples of 4, integer
    biases, W2 of two +-1 per row — h and every partial sum of e are integers far below 2^11, so one fp16 half, an fp32 accumulator and
    any power of two hold them exactly in any order; the cross-view half reads an all-zero lattice and a zero point weight."""
    c = FR.INT_CASE
    rec = host_records(shim, c, rays_edit=lambda r: FR.integer_rays(r, c))
    p, lat = FR.weights("int"), FR.integer_lattice(c)
    lh, lw = FR.lattice_dims(c["fh"], c["fw"], c["pad"])
    node, ring, w = FR.lattice_taps(rec["grid"], lw, lh, c["pad"], torch.float32)
    assert bool((w == 0.25).all()) and not bool(ring.any()) and len(set(node.tolist())) >= 30
    assert bool((lat == lat.round()).all()) and bool((lat % 4 == 0).all()) and bool((lat[:, 1] == 0).all()) and lat.abs().max() == 32
    W2 = p["query_encode_latent_2.weight"]
    assert bool(((W2 != 0).sum(1) == 2).all()) and bool((W2.abs() <= 1).all()) and bool((p["query_encode_latent.weight"][:, FR.C:] == 0).all())
    ref = FR.samples(p, lat, c["pad"], rec, 2 * c["b"])
    f32 = FR.samples(p, lat, c["pad"], rec, 2 * c["b"], dtype=torch.float32)
    for k in ("h", "e", "B_h", "B_e"):
        assert bool((ref[k] == ref[k].round()).all()) and ref[k].abs().max().item() < 2 ** 11, k
    assert torch.equal(f32["e"].double(), ref["e"]) and torch.equal(f32["h"].double(), ref["h"])
    assert ref["h"][:, 0].max() > 8 and len(set(ref["e"].reshape(-1).tolist())) > 40
    # the cross-view half is relu(b1) exactly
    Sn = ref["h"].shape[0]
    assert torch.equal(ref["h"][Sn // 2:, 0], F.relu(p["query_encode_latent.bias"].double()).expand(Sn // 2, -1))


def test_fp16_emulation_is_a_usable_yardstick(shim):
    """The fp16 instance is held to 8 x this ratio: it must be finite, above fp32's and far below 1."""
    c = FR.CASES["edge-37-13-2"]
    rec = host_records(shim, c)
    p, lat = FR.weights("gauss"), FR.case_lattice(c)
    ref = FR.samples(p, lat, c["pad"], rec, 2 * c["b"])
    emu = FR.samples(p, lat, c["pad"], rec, 2 * c["b"], dtype=torch.float32, linear=FR.fp16_linear)
    for k in ("e", "logit"):
        r = FR.ratio(emu[k], ref[k], ref["B_" + k])
        print(f"[fp16 emulation] {k}: {r:.3e}")
        assert 2.0 ** -18 < r < 2.0 ** -7, (k, r)


def test_part_restatement_on_a_ragged_group():
    g = FR.gen(3)
    n_sets, R, P = 2, 3, 11
    e = torch.randn(n_sets * R * P, 5, generator=g, dtype=F64)
    lg = torch.randn(n_sets * R * P, generator=g, dtype=F64) * 4
    part, mag = FR.part(e, lg, n_sets, R, P, 8)
    assert part.shape == (n_sets, R, 2, 5)
    ee, ll = e.reshape(n_sets, R, P, 5), lg.reshape(n_sets, R, P)
    for s in range(n_sets):
        for r in range(R):
            for gp, (a, b_) in enumerate(((0, 8), (8, 11))):
                w = torch.exp(ll[s, r, a:b_] - ll[s, r, a:b_].max())
                assert torch.allclose(part[s, r, gp], (w[:, None] * ee[s, r, a:b_]).sum(0), rtol=1e-14, atol=0)
                assert torch.allclose(mag[s, r, gp], (w[:, None] * ee[s, r, a:b_].abs()).sum(0), rtol=1e-14, atol=0)
