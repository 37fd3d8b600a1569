"""``-m gpu``: the matcher's stages (csrc/car_superpoint.hip, csrc/car_superglue.hip) through the C ABI against the restatement
(tests/matcher_reference.py), and ``matching.superpoint`` / ``match_pair`` / ``render_unposed_traj.py --matcher_weights`` on the reference's own
outputs (tests/golden/matcher_expected.npz).  SuperPoint first; SuperGlue's rules stand above its tests further down.

  * arithmetic stages (conv1a, the dense score map, the dense descriptors, the sampled descriptors): parity_rule.judge against the
    float64 restatement, the float32 restatement on the same inputs as the yardstick (FACTOR 8, FLOOR 2^-22); conv1a also bit for bit
    on small integers, where every sum is exact;
  * decision stages (suppression, selection with its order and count): bit-identical to the restated logic on the same fp32 map;
  * every output lies in a NaN-guarded buffer (abi_harness.Guarded): nothing is written outside it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import abi_harness as A  # noqa: E402
import matcher_cases as C  # noqa: E402
import matcher_reference as R  # noqa: E402
import parity_rule as PR  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SHAPES = ((1, 8, 8), (1, 8, 16), (2, 24, 40))        # one feature cell, a 1 x 2 grid, two images of 3 x 5 cells


@pytest.fixture(scope="module")
def state():
    return C.superpoint_state()


@pytest.fixture(scope="module")
def weights(state):
    from cross_attention_renderer_amd import matching as M
    return M.MatcherWeights(state)


@pytest.fixture(scope="module")
def packed(weights):
    return weights.packed(A.dev())


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "golden", "matcher_expected.npz")).items()}


def work_of(nbytes):
    assert nbytes > 0, A.lib().car_last_error()
    return torch.empty(nbytes, dtype=torch.uint8, device=A.dev())


def work_or(work, nbytes):
    """(pointer, bytes) of the caller's own workspace, or of a fresh one of `nbytes`; the third item keeps the fresh one alive."""
    if work is not None:
        return work[0], work[1], None
    buf = work_of(nbytes)
    return A.ptr(buf), nbytes, buf


def images(n, H, W, seed=1):
    return torch.rand(n, H, W, generator=PR.gen(seed))


_dense = {}


def dense_of(state, shape):
    """The restatement's dense stage for one shape, both precisions, computed once."""
    if shape not in _dense:
        im = images(*shape)
        _dense[shape] = (im, R.dense(state, im, F32), R.dense(state, im, F64))
    return _dense[shape]


@pytest.mark.parametrize("shape", SHAPES + ((1, 5, 7), (3, 17, 33)))         # odd sizes, and more than one workgroup (64 pixels each)
def test_conv1a(state, packed, shape):
    n, H, W = shape
    im = images(n, H, W, seed=2) - 0.25
    out = A.Guarded((n, H, W, 64))
    assert A.lib().car_superpoint_conv1a(A.ptr(im.to(A.dev())), n, H, W, A.ptr(packed), out.ptr, A.stream()) == 0, A.lib().car_last_error()
    y64, bound = R.conv1a(state, im, F64)
    y32, _ = R.conv1a(state, im, F32)
    PR.judge("superpoint_conv1a", f"{n}x{H}x{W}", {"": ((out.get("conv1a"), y64, bound), PR.ratio(y32, y64, bound))}, finite=True)


def test_conv1a_small_integers_bit_for_bit():
    """Integer weights, biases and pixels: every product and sum is exact in fp32, so the kernel must give the float64 result's bits."""
    from cross_attention_renderer_amd import matching as M
    g = PR.gen(7)
    st = dict(C.superpoint_state())
    st["conv1a.weight"] = torch.randint(-8, 9, (64, 1, 3, 3), generator=g).float()
    st["conv1a.bias"] = torch.randint(-8, 9, (64,), generator=g).float()
    n, H, W = 2, 9, 13
    im = torch.randint(-16, 17, (n, H, W), generator=g).float()
    out = A.Guarded((n, H, W, 64))
    pk = M.MatcherWeights(st).packed(A.dev())
    assert A.lib().car_superpoint_conv1a(A.ptr(im.to(A.dev())), n, H, W, A.ptr(pk), out.ptr, A.stream()) == 0
    want = R.conv1a(st, im, F64)[0]
    assert float(want.max()) > 0 and torch.equal(out.get("conv1a").double(), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_dense_scores_and_descriptors(state, packed, shape):
    n, H, W = shape
    im, d32, d64 = dense_of(state, shape)
    lib = A.lib()
    nbytes = lib.car_superpoint_workspace_bytes(n, H, W)
    work = work_of(nbytes)
    scores, desc = A.Guarded((n, H, W)), A.Guarded((n, H // 8, W // 8, 256))
    assert lib.car_superpoint_dense(A.ptr(im.to(A.dev())), n, H, W, A.ptr(packed), scores.ptr, desc.ptr, A.ptr(work), nbytes, A.stream()) == 0, lib.car_last_error()
    PR.judge("superpoint_dense", f"{n}x{H}x{W}", {
        "scores": ((scores.get("scores"), d64["scores"], d64["bound_scores"]), PR.ratio(d32["scores"], d64["scores"], d64["bound_scores"])),
        "desc": ((desc.get("desc"), d64["desc"], d64["bound_desc"]), PR.ratio(d32["desc"], d64["desc"], d64["bound_desc"]))}, finite=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_sampled_descriptors(state, shape):
    """The kernel and both restatements read the SAME fp32 dense descriptors; keypoints on the corners, the edges and inside."""
    n, H, W = shape
    _, d32, _ = dense_of(state, shape)
    g = PR.gen(3)
    for i in range(n):
        desc = d32["desc"][i].contiguous()
        k = torch.stack([torch.randint(0, W, (61,), generator=g), torch.randint(0, H, (61,), generator=g)], -1).float()
        k = torch.cat([torch.tensor([[0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0], [W / 2.0, H / 2.0]]), k])       # 66: two workgroups, a ragged one
        out = A.Guarded((len(k), 256))
        assert A.lib().car_superpoint_sample(A.ptr(k.to(A.dev())), len(k), A.ptr(desc.to(A.dev())), H // 8, W // 8, out.ptr, A.stream()) == 0, A.lib().car_last_error()
        zero = torch.zeros_like(desc, dtype=F64)
        s64, bound = R.sample(k, desc.double(), zero, F64)
        s32, _ = R.sample(k, desc, zero, F32)
        PR.judge("superpoint_sample", f"{n}x{H}x{W} image {i}", {"": ((out.get("sample"), s64, bound), PR.ratio(s32, s64, bound))}, finite=True)


def run_nms(maps, r, work=None):
    n, H, W = maps.shape
    lib = A.lib()
    wp, wb, _keep = work_or(work, lib.car_superpoint_nms_workspace_bytes(n, H, W))
    out = A.Guarded((n, H, W))
    assert lib.car_superpoint_nms(A.ptr(maps.to(A.dev())), n, H, W, r, out.ptr, wp, wb, A.stream()) == 0, lib.car_last_error()
    return out.get("nms")


def run_select(kept, thr, border, maxk):
    n, H, W = kept.shape
    lib = A.lib()
    nbytes = lib.car_superpoint_select_workspace_bytes(n, H, W)
    work = work_of(nbytes)
    kp, sc, cnt = A.Guarded((n, maxk, 2)), A.Guarded((n, maxk)), A.Guarded((n,), dtype=I32)
    assert lib.car_superpoint_select(A.ptr(kept.to(A.dev())), n, H, W, ctypes.c_float(thr), border, maxk, kp.ptr, sc.ptr, cnt.ptr, A.ptr(work), nbytes,
                                     A.stream()) == 0, lib.car_last_error()
    return kp.get("kpts"), sc.get("scores"), cnt.get("count")


def check_select(kept, thr, border, maxk, what):
    kp, sc, cnt = run_select(kept, thr, border, maxk)
    counts = []
    for i in range(len(kept)):
        wk, ws = R.select(kept[i], thr, border, maxk)
        N = len(ws)
        assert int(cnt[i]) == N, (what, i, int(cnt[i]), N)
        assert torch.equal(kp[i, :N], wk), (what, i, "keypoints or their order")
        assert torch.equal(A.bits(sc[i, :N]), A.bits(ws)), (what, i, "scores")
        assert bool(torch.isnan(kp[i, N:]).all()) and bool(torch.isnan(sc[i, N:]).all()), (what, i, "wrote behind the count")
        counts.append(N)
    return counts


@pytest.mark.parametrize("r", (0, 1, 4, 8))
def test_nms_is_the_restated_logic_bit_for_bit(r):
    for key, m in C.crafted_maps().items():
        m = torch.from_numpy(m)[None]
        assert torch.equal(A.bits(run_nms(m, r)), A.bits(R.nms(m, r))), (key, r)
    g = PR.gen(r)
    batch = torch.stack([torch.rand(37, 70, generator=g), (torch.randint(0, 5, (37, 70), generator=g) / 4.0)])      # two maps, ragged workgroups
    assert torch.equal(A.bits(run_nms(batch, r)), A.bits(R.nms(batch, r)))


def test_selection_on_the_crafted_maps():
    maps = C.crafted_maps()
    for k, (key, r, thr, border, maxk) in enumerate(C.SELECTIONS):
        check_select(R.nms(torch.from_numpy(maps[key])[None], r), thr, border, maxk, f"selection {k}")
    # plateaus and ties, uncut and cut: equal scores go to the lower row-major index
    for key in ("plateau", "ties", "constant"):
        kept = R.nms(torch.from_numpy(maps[key])[None], 1)
        n_all, = check_select(kept, 0.005, 0, 4096, key)
        assert n_all > 3
        for maxk in (n_all, n_all - 1, n_all + 1, 1, 3):            # exactly the count, one under, one above
            check_select(kept, 0.005, 0, maxk, f"{key} max_keypoints {maxk}")
    # borders that remove everything; everything under the threshold
    assert check_select(torch.from_numpy(maps["distinct"])[None], 0.0, 12, 100, "border 12") == [0]
    assert check_select(torch.from_numpy(maps["distinct"])[None], 0.0, 1000, 100, "border 1000") == [0]
    assert check_select(torch.from_numpy(maps["low"])[None], 0.005, 0, 100, "low") == [0]


def test_selection_at_size():
    """Two 256 x 256 maps without suppression: 49152 candidates on four tied levels, and 65536 distinct ones with negative scores and
    both zeros, each cut to the 4096-keypoint cap and to a ragged 1000."""
    g = PR.gen(4)
    tied = (torch.randint(0, 4, (256, 256), generator=g) / 4.0)
    distinct = (torch.randperm(65536, generator=g).float().reshape(256, 256) - 30000.0) / 65536.0
    distinct[5, 5], distinct[200, 17] = 0.0, -0.0
    both = torch.stack([tied, distinct])
    for maxk in (4096, 1000):
        assert check_select(both, -1.0, 0, maxk, f"at size {maxk}") == [maxk, maxk]
    check_select(both, 0.3, 7, 4096, "at size, threshold 0.3")


@pytest.mark.parametrize("name", sorted(C.PAIRS))
def test_superpoint_end_to_end(state, weights, golden, name):
    from cross_attention_renderer_amd import matching as M
    _, _, _, radius, thr, maxk, border = C.PAIRS[name]
    im = golden[f"{name}.image"]
    got = M.superpoint(im.to(A.dev()), weights, radius, thr, maxk, border)
    again = M.superpoint(im.to(A.dev()), weights, radius, thr, maxk, border)
    res32, _ = R.superpoint(state, im, radius, thr, maxk, border, dtype=F32)
    res64, d64 = R.superpoint(state, im, radius, thr, maxk, border, dtype=F64)
    for i in range(2):
        kp = got["keypoints"][i].cpu()
        assert torch.equal(kp, golden[f"{name}.kpts{i}"]), (name, i, "keypoint set or order")
        pix = kp.long()
        bs = d64["bound_scores"][i][pix[:, 1], pix[:, 0]]
        PR.judge("superpoint", f"{name} image {i}", {
            "scores": ((got["scores"][i].cpu(), res64[i]["scores"], bs), PR.ratio(res32[i]["scores"], res64[i]["scores"], bs)),
            "descriptors": ((got["descriptors"][i].cpu(), res64[i]["descriptors"], res64[i]["bound_descriptors"]),
                            PR.ratio(res32[i]["descriptors"], res64[i]["descriptors"], res64[i]["bound_descriptors"]))}, finite=True)
        for key in ("keypoints", "scores", "descriptors"):
            assert torch.equal(A.bits(got[key][i].cpu()), A.bits(again[key][i].cpu())), (name, i, key, "the same call twice")


def test_superpoint_refusals_on_the_device(weights):
    from cross_attention_renderer_amd import matching as M
    x = torch.zeros(16, 24, device=A.dev())
    with pytest.raises(ValueError, match="weights must come from"):
        M.superpoint(x, None)
    for maxk in (0, -1, 4097):
        with pytest.raises(ValueError, match=r"need 1\.\.4096"):
            M.superpoint(x, weights, max_keypoints=maxk)
    with pytest.raises(ValueError, match="multiples of 8"):
        M.superpoint(torch.zeros(16, 20, device=A.dev()), weights)
    with pytest.raises(ValueError, match=r"need 0\.\.8"):
        M.superpoint(x, weights, nms_radius=9)
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.superpoint(x.cpu(), weights)
    out = M.superpoint(x, weights, keypoint_threshold=2.0)          # nothing passes the threshold: empty sets, no sampling launch
    assert [tuple(t.shape) for t in (out["keypoints"][0], out["scores"][0], out["descriptors"][0])] == [(0, 2), (0,), (0, 256)]


# ==== SuperGlue (csrc/car_superglue.hip) =============================================================================================
# arithmetic stages (attention, the descriptor network's mdesc, the Sinkhorn Z) by parity_rule against the float64 restatement; the match
# rule bit for bit on the same Z; matching.match_pair on the reference's outputs, matches compared where DECIDED (matcher_reference.decided:
# the float64 gaps of the row and of the column exceed twice the tolerance on Z), at most one keypoint in eight undecided.
PAIR_SIZES = ((1, 1), (1, 5), (63, 65), (64, 64), (130, 127))          # wave and tile edges on both sides; (1024, 1024) runs once per stage


@pytest.fixture(scope="module")
def glue():
    return C.superglue_state()


@pytest.fixture(scope="module")
def both(state, glue):
    from cross_attention_renderer_amd import matching as M
    return M.MatcherWeights(state, glue, C.GNN_LAYERS)


@pytest.mark.parametrize("N, M_", PAIR_SIZES + ((1024, 1024),))
def test_attention(N, M_):
    g = PR.gen(N * 2048 + M_)
    q = torch.randn(N, 256, generator=g)
    kv = torch.randn(M_, 768, generator=g)                              # keys and values as columns of one [M, 768] array, as the network holds them
    out = A.Guarded((N, 256), ld=260)
    d = kv.to(A.dev())
    assert A.lib().car_superglue_attention(A.ptr(q.to(A.dev())), 256, ctypes.c_void_p(d.data_ptr() + 256 * 4), 768, ctypes.c_void_p(d.data_ptr() + 512 * 4), 768,
                                           N, M_, out.ptr, 260, A.stream()) == 0, A.lib().car_last_error()
    k, v = kv[:, 256:512].contiguous(), kv[:, 512:].contiguous()
    o64, bound = R.attention_heads(q.double(), k.double(), v.double())
    o32, _ = R.attention_heads(q, k, v)
    PR.judge("superglue_attention", f"{N}x{M_}", {"": ((out.get("attention"), o64, bound), PR.ratio(o32, o64, bound))}, finite=True)


def run_transport(a, b, iters, work=None):
    lib, (m, n) = A.lib(), (len(a), len(b))
    wp, wb, _keep = work_or(work, lib.car_superglue_transport_workspace_bytes(m, n))
    Z = A.Guarded((m + 1, n + 1))
    assert lib.car_superglue_transport(A.ptr(a.to(A.dev())), m, A.ptr(b.to(A.dev())), n, ctypes.c_float(C.BIN_SCORE), iters, Z.ptr, wp, wb,
                                       A.stream()) == 0, lib.car_last_error()
    return Z.get("Z")


@pytest.mark.parametrize("m, n, iters", [(m, n, it) for m, n in PAIR_SIZES for it in (1, 20, 100)] + [(1024, 1024, 20), (7, 9, 0)])
def test_sinkhorn(m, n, iters):
    g = PR.gen(m * 4096 + n * 2 + iters)
    a, b = torch.randn(m, 256, generator=g) * 0.6, torch.randn(n, 256, generator=g) * 0.6
    z64, bound = R.transport(a, b, C.BIN_SCORE, iters, F64)
    z32, _ = R.transport(a, b, C.BIN_SCORE, iters, F32)
    PR.judge("superglue_transport", f"{m}x{n} iterations {iters}", {"": ((run_transport(a, b, iters), z64, bound), PR.ratio(z32, z64, bound))}, finite=True)


_pairs = {}


def pair_of(state, glue, golden, name):
    """The restatement of one fixture pair, both precisions, computed once: SuperPoint's outputs, mdesc and Z."""
    if name not in _pairs:
        H, W, _, radius, thr, maxk, border = C.PAIRS[name]
        out = {}
        for dt in (F32, F64):
            res, d = R.superpoint(state, golden[f"{name}.image"], radius, thr, maxk, border, dtype=dt)
            md = R.match_descriptors(glue, C.GNN_LAYERS, res[0]["keypoints"], res[0]["scores"], res[0]["descriptors"], (H, W), res[1]["keypoints"],
                                     res[1]["scores"], res[1]["descriptors"], (H, W), dt)
            out[dt] = dict(res=res, dense=d, mdesc=md, Z=R.transport(md[0][0], md[1][0], C.BIN_SCORE, C.SINKHORN_ITERATIONS, dt))
        _pairs[name] = out
    return _pairs[name]


@pytest.mark.parametrize("name", ("topk", "unequal", "tiny"))
def test_descriptor_network(state, glue, both, golden, name):
    """car_superglue_descriptors on the float32 restatement's keypoints, scores and descriptors; `tiny`: one keypoint against three."""
    src = pair_of(state, glue, golden, "unequal" if name == "tiny" else name)[F32]["res"]
    H, W = C.PAIRS["unequal" if name == "tiny" else name][:2]
    cut = (1, 3) if name == "tiny" else (None, None)
    k, s, d = ([src[i][key][:cut[i]].float().contiguous() for i in range(2)] for key in ("keypoints", "scores", "descriptors"))
    N0, N1 = len(k[0]), len(k[1])
    lib, packed = A.lib(), both.packed_glue(A.dev())
    nbytes = lib.car_superglue_workspace_bytes(N0, N1)
    work = work_of(nbytes)
    out = A.Guarded((N0 + N1, 256))
    cross = A.ints([int(n == "cross") for n in C.GNN_LAYERS])
    dv = [[t.to(A.dev()) for t in group] for group in (k, s, d)]
    assert lib.car_superglue_descriptors(A.ptr(dv[0][0]), A.ptr(dv[1][0]), A.ptr(dv[2][0]), N0, H, W, A.ptr(dv[0][1]), A.ptr(dv[1][1]), A.ptr(dv[2][1]), N1, H, W,
                                         A.ptr(packed), len(C.GNN_LAYERS), cross, out.ptr, A.ptr(work), nbytes, A.stream()) == 0, lib.car_last_error()
    got = out.get("mdesc")
    m64 = R.match_descriptors(glue, C.GNN_LAYERS, k[0], s[0], d[0], (H, W), k[1], s[1], d[1], (H, W), F64)
    m32 = R.match_descriptors(glue, C.GNN_LAYERS, k[0], s[0], d[0], (H, W), k[1], s[1], d[1], (H, W), F32)
    PR.judge("superglue_descriptors", name, {f"mdesc{i}": ((got[(0, N0)[i]:(N0, N0 + N1)[i]], m64[i][0], m64[i][1]), PR.ratio(m32[i][0], m64[i][0], m64[i][1]))
                                             for i in range(2)}, finite=True)


def run_matches(Z, thr, work=None):
    lib, (m, n) = A.lib(), (Z.shape[0] - 1, Z.shape[1] - 1)
    wp, wb, _keep = work_or(work, lib.car_superglue_matches_workspace_bytes(m, n))
    m0, m1, s0, s1 = A.Guarded((m,), dtype=I32), A.Guarded((n,), dtype=I32), A.Guarded((m,)), A.Guarded((n,))
    assert lib.car_superglue_matches(A.ptr(Z.to(A.dev())), m, n, ctypes.c_float(thr), m0.ptr, m1.ptr, s0.ptr, s1.ptr, wp, wb, A.stream()) == 0, lib.car_last_error()
    return m0.get("matches0"), m1.get("matches1"), s0.get("scores0"), s1.get("scores1")


@pytest.mark.parametrize("m, n", PAIR_SIZES + ((5, 3), (1024, 1000)))
def test_match_rule_bit_for_bit(m, n):
    """Crafted Z: a few tied levels (ties go to the lowest index), values around log(0.2) so that the threshold decides both ways.  The
    indices are the restated rule's on the same fp32 Z; the scores are exp(max) formed in float64 and rounded once."""
    g = PR.gen(m * 2048 + n)
    for Z in (torch.randint(-12, 1, (m + 1, n + 1), generator=g).float() / 4.0, torch.randn(m + 1, n + 1, generator=g) - 1.6, torch.zeros(m + 1, n + 1)):
        got = run_matches(Z, C.MATCH_THRESHOLD)
        w0, w1, _, _ = R.matches(Z, C.MATCH_THRESHOLD)
        _, _, s0, s1 = R.matches(Z.double(), 0.0)
        assert torch.equal(got[0].long(), w0) and torch.equal(got[1].long(), w1), (m, n, "matches")
        assert torch.equal(A.bits(got[2]), A.bits(s0.float())) and torch.equal(A.bits(got[3]), A.bits(s1.float())), (m, n, "scores")


@pytest.mark.parametrize("name", sorted(C.PAIRS))
def test_match_pair_end_to_end(state, glue, both, golden, name):
    from cross_attention_renderer_amd import matching as M
    _, _, _, radius, thr, maxk, border = C.PAIRS[name]
    im = golden[f"{name}.image"].to(A.dev())
    args = (both, radius, thr, maxk, border, C.SINKHORN_ITERATIONS, C.MATCH_THRESHOLD)
    got, again = M.match_pair(im[0], im[1], *args), M.match_pair(im[0], im[1], *args)
    assert sorted(got) == sorted(f"{k}{i}" for k in ("keypoints", "scores", "descriptors", "matches", "matching_scores") for i in (0, 1))
    for key in got:
        assert torch.equal(got[key].cpu().view(I32), again[key].cpu().view(I32)), (name, key, "the same call twice")
    ref = pair_of(state, glue, golden, name)
    for i in range(2):
        assert torch.equal(got[f"keypoints{i}"].cpu(), golden[f"{name}.kpts{i}"]), (name, i, "keypoint set or order")
    (z32, _), (z64, bound) = ref[F32]["Z"], ref[F64]["Z"]
    tol = PR.tolerance(PR.ratio(z32, z64, bound)) * bound
    decided = R.decided(z64, tol)
    undecided = sum(int((~d).sum()) for d in decided)
    total = sum(len(d) for d in decided)
    print(f"[decided] {name}: {undecided} of {total} keypoints undecided")
    assert undecided * 8 <= total, (name, undecided, total)
    w32, w64 = R.matches(z32, C.MATCH_THRESHOLD), R.matches(z64, C.MATCH_THRESHOLD)
    entries = {}
    for i in range(2):
        d = decided[i]
        assert torch.equal(got[f"matches{i}"].cpu().long()[d], w64[i][d]), (name, i, "a decided match differs from the float64 restatement's")
        assert torch.equal(golden[f"{name}.matches{i}"].long()[d], w64[i][d]), (name, i, "the fixture itself")
        # |d exp(Z)| = exp(Z) |dZ|: the bound on Z at the arg-max, scaled by the score
        zi = z64[:-1, :-1] if i == 0 else z64[:-1, :-1].t()
        bi = bound[:-1, :-1] if i == 0 else bound[:-1, :-1].t()
        at = zi.argmax(1)
        sb = w64[2 + i].double() * bi[torch.arange(len(at)), at]
        entries[f"scores{i}"] = ((got[f"matching_scores{i}"].cpu(), w64[2 + i], sb, d), PR.ratio(w32[2 + i], w64[2 + i], sb, d))
    PR.judge("match_pair", name, entries, finite=True)


# ---- every workspace-taking entry over a workspace of exactly its size entry's bytes, NaN all around it, then over one twice as large:
# nothing is written outside either and the outputs are the same bytes (abi_harness.exact_then_twice).  The smallest shapes that
# populate every piece of each layout.
def test_dense_fits_its_workspace_exactly(packed):
    """One 16 x 16 image: 2 x 2 cells, both maps of the workspace and the heads' two pieces inside the second."""
    n, H, W = 1, 16, 16
    lib, im = A.lib(), images(n, H, W, seed=5).to(A.dev())

    def run(work, wb):
        scores, desc = A.Guarded((n, H, W)), A.Guarded((n, H // 8, W // 8, 256))
        assert lib.car_superpoint_dense(A.ptr(im), n, H, W, A.ptr(packed), scores.ptr, desc.ptr, work.ptr, wb, A.stream()) == 0, lib.car_last_error()
        return scores.get("scores"), desc.get("desc")

    scores, desc = A.exact_then_twice(lib.car_superpoint_workspace_bytes(n, H, W), run, "car_superpoint_dense")
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(desc).all())


def test_nms_fits_its_workspace_exactly():
    maps = torch.rand(2, 8, 8, generator=PR.gen(11))
    kept, = A.exact_then_twice(A.lib().car_superpoint_nms_workspace_bytes(2, 8, 8), lambda w, wb: (run_nms(maps, 2, work=(w.ptr, wb)),), "car_superpoint_nms")
    assert torch.equal(A.bits(kept), A.bits(R.nms(maps, 2)))


def test_glue_stages_fit_their_workspaces_exactly(glue):
    """N0 = 3 against N1 = 5 keypoints through the three stages, each over its own exact workspace: the descriptor network with two layers
    (self, cross), two Sinkhorn iterations, the match rule on the couplings they give."""
    from cross_attention_renderer_amd import matching as M
    lib, g, (N0, N1), (H, W) = A.lib(), PR.gen(13), (3, 5), (48, 64)
    layers = ("self", "cross")
    packed = M.MatcherWeights(C.superpoint_state(), C.superglue_state(len(layers)), layers).packed_glue(A.dev())
    k = [(torch.rand(N, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to(A.dev()) for N in (N0, N1)]
    sc = [torch.rand(N, generator=g).to(A.dev()) for N in (N0, N1)]
    d = [torch.nn.functional.normalize(torch.randn(N, 256, generator=g), dim=1).to(A.dev()) for N in (N0, N1)]

    def descriptors(work, wb):
        out = A.Guarded((N0 + N1, 256))
        assert lib.car_superglue_descriptors(A.ptr(k[0]), A.ptr(sc[0]), A.ptr(d[0]), N0, H, W, A.ptr(k[1]), A.ptr(sc[1]), A.ptr(d[1]), N1, H, W, A.ptr(packed),
                                             len(layers), A.ints([0, 1]), out.ptr, work.ptr, wb, A.stream()) == 0, lib.car_last_error()
        return (out.get("mdesc"),)

    mdesc, = A.exact_then_twice(lib.car_superglue_workspace_bytes(N0, N1), descriptors, "car_superglue_descriptors")
    assert bool(torch.isfinite(mdesc).all())
    Z, = A.exact_then_twice(lib.car_superglue_transport_workspace_bytes(N0, N1), lambda w, wb: (run_transport(mdesc[:N0], mdesc[N0:], 2, work=(w.ptr, wb)),),
                            "car_superglue_transport")
    assert bool(torch.isfinite(Z).all())
    got = A.exact_then_twice(lib.car_superglue_matches_workspace_bytes(N0, N1), lambda w, wb: run_matches(Z, C.MATCH_THRESHOLD, work=(w.ptr, wb)), "car_superglue_matches")
    w0, w1, _, _ = R.matches(Z, C.MATCH_THRESHOLD)
    assert torch.equal(got[0].long(), w0) and torch.equal(got[1].long(), w1)


def test_superglue_refusals(both, weights):
    from cross_attention_renderer_amd import matching as M
    lib, dev = A.lib(), A.dev()
    one = ctypes.c_void_p(16)
    err = lambda: lib.car_last_error().decode()
    k, s, d = torch.zeros(3, 2, device=dev), torch.zeros(3, device=dev), torch.zeros(3, 256, device=dev)
    e = (torch.zeros(0, 2, device=dev), torch.zeros(0, device=dev), torch.zeros(0, 256, device=dev))
    out = M.superglue(*e, k, s, d, (16, 16), both)                      # an empty side: all -1 and zeros, nothing launched
    assert out["matches0"].numel() == 0 and out["matches1"].tolist() == [-1, -1, -1] and out["matching_scores1"].tolist() == [0.0, 0.0, 0.0]
    big = (torch.zeros(1025, 2, device=dev), torch.zeros(1025, device=dev), torch.zeros(1025, 256, device=dev))
    with pytest.raises(ValueError, match="at most 1024"):
        M.superglue(*big, k, s, d, (16, 16), both)
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.superglue(k.cpu(), s.cpu(), d.cpu(), k.cpu(), s.cpu(), d.cpu(), (16, 16), both)
    with pytest.raises(ValueError, match="hold no SuperGlue"):
        M.superglue(k, s, d, k, s, d, (16, 16), weights)
    with pytest.raises(ValueError, match="at most 1024"):
        M.match_pair(torch.zeros(16, 16, device=dev), torch.zeros(16, 16, device=dev), both, max_keypoints=2048)
    for n0, n1 in ((0, 4), (4, 0), (1025, 4), (4, 1025)):
        assert lib.car_superglue_workspace_bytes(n0, n1) == 0 and "need 1..1024" in err()
        assert lib.car_superglue_transport(one, n0, one, n1, ctypes.c_float(1.0), 20, one, one, 1 << 30, None) == -1 and "need 1..1024" in err()
        assert lib.car_superglue_matches(one, n0, n1, ctypes.c_float(0.2), one, one, one, one, one, 1 << 30, None) == -1 and "need 1..1024" in err()
        assert lib.car_superglue_attention(one, 256, one, 256, one, 256, n0, n1, one, 256, None) == -1 and "need 1..1024" in err()
    assert lib.car_superglue_packed_floats(0) == 0 and "need 1..64" in err()
    assert lib.car_superglue_pack(one, 28, 0, one, None) == -1 and "need 1..64" in err()
    assert lib.car_superglue_pack(one, 91, 4, one, None) == -1 and "4 layers need 92" in err()
    assert lib.car_superglue_pack(None, 92, 4, one, None) == -1 and "null pointer" in err()
    cross = A.ints([0, 1, 0, 1])
    assert lib.car_superglue_descriptors(one, one, one, 4, 16, 16, one, one, one, 4, 16, 16, one, 0, cross, one, one, 1 << 30, None) == -1 and "need 1..64" in err()
    assert lib.car_superglue_descriptors(one, one, one, 4, 16, 16, one, one, one, 4, 16, 16, one, 4, cross, one, one, lib.car_superglue_workspace_bytes(4, 4) - 1,
                                         None) == -1 and "workspace holds" in err()
    assert lib.car_superglue_descriptors(one, one, None, 4, 16, 16, one, one, one, 4, 16, 16, one, 4, cross, one, one, 1 << 30, None) == -1 and "null pointer" in err()
    assert lib.car_superglue_transport(one, 4, one, 4, ctypes.c_float(1.0), 20, one, one, lib.car_superglue_transport_workspace_bytes(4, 4) - 1, None) == -1
    assert "workspace holds" in err()
    assert lib.car_superglue_transport(one, 4, one, 4, ctypes.c_float(1.0), 20, None, one, 1 << 30, None) == -1 and "null pointer" in err()
    assert lib.car_superglue_matches(one, 4, 4, ctypes.c_float(0.2), one, one, one, one, one, 63, None) == -1 and "workspace holds" in err()
    assert lib.car_superglue_matches(None, 4, 4, ctypes.c_float(0.2), one, one, one, one, one, 64, None) == -1 and "null pointer" in err()
    assert lib.car_superglue_attention(one, 255, one, 256, one, 256, 4, 4, one, 256, None) == -1 and "row strides" in err()


def test_script_matches_the_pair_and_saves_the_matches(state, glue, both, tmp_path):
    """render_unposed_traj.py --matcher_weights ... --save_matches on the synthetic pair with the seeded weights, in a fresh child process:
    the .npz reads back (trajectory.read_matches) to what match_pair gives here on the same images, and the script either reaches the
    pose estimate or stops with its message for fewer than five matches."""
    import subprocess
    from cross_attention_renderer_amd import matching as M, trajectory
    torch.save(state, tmp_path / "sp.pth")
    torch.save(glue, tmp_path / "sg.pth")
    root = os.path.dirname(HERE)
    out = tmp_path / "pair_matches.npz"
    cmd = [sys.executable, os.path.join(root, "experiment_scripts", "render_unposed_traj.py"), "--experiment_name", "t", "--views", "2", "--synthetic",
           "--matcher_weights", str(tmp_path / "sp.pth"), str(tmp_path / "sg.pth"), "--save_matches", str(out), "--pose_hypotheses", "256", "--n_frames", "1",
           "--out_dir", str(tmp_path), "--logging_root", str(tmp_path)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert "matched " in run.stdout, run.stdout + run.stderr
    assert (run.returncode == 0 and "inliers" in run.stdout) or "at least five good ones are needed" in run.stderr, run.stdout + run.stderr
    g = np.random.default_rng(0)
    ims = [g.random((256, 256, 3)) for _ in range(2)]
    gray = [torch.from_numpy(0.2125 * im[..., 0] + 0.7154 * im[..., 1] + 0.0721 * im[..., 2]).to(A.dev(), F32) for im in ims]
    want = {k: v.cpu().numpy() for k, v in M.match_pair(gray[0], gray[1], M.load_matcher_weights(str(tmp_path / "sp.pth"), str(tmp_path / "sg.pth"))).items()}
    with np.load(out) as f:
        assert sorted(f.files) == ["keypoints0", "keypoints1", "match_confidence", "matches"]
        for key, mine in (("keypoints0", "keypoints0"), ("keypoints1", "keypoints1"), ("matches", "matches0"), ("match_confidence", "matching_scores0")):
            assert np.array_equal(f[key], want[mine]), key
    m0, m1, conf = trajectory.read_matches(str(out))
    valid = want["matches0"] > -1
    assert np.array_equal(m0, want["keypoints0"][valid]) and np.array_equal(m1, want["keypoints1"][want["matches0"][valid]])
    assert np.array_equal(conf, want["matching_scores0"][valid]) and 0 < len(want["keypoints0"]) <= 1024
